"""The tolerance of the cell-sharded FunctionEstimator tests (tests/test_gpu_function_sharded.py),
measured on the CPU with the oracle's landmark conditional; the sharded code is never imported.

What differs between a fit on one rank and on N is the order of the two sums over cells, A A^T and A (y - mu), amplified
by the conditioning of A A^T / sigma^2 + I.  The oracle's `landmarks_conditional` is therefore run in two steps: the
sums are formed (a) once over all rows and (b) shard by shard in rank order for 2, 3 and 4 contiguous shards (the
bounds of distributed.shard_bounds, restated here), and the same m x m solve turns each pair of sums into weights.
Reported: the largest change of the predictions -- at the training cells and at the held-out points -- relative to
the largest absolute prediction, per data seed and over 5 seeds.  tol = 16 x that value, the factor for the device's
different blocking inside each partial sum.

    python tools/function_shard_tol.py
"""
import os
import sys

# one thread: scikit-learn's k-means (the workload's landmarks) and a threaded BLAS add their partial sums in an order
# that changes from run to run, and the figure below would change in its second digit with them
for _var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_var] = "1"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import mellon_oracle as mo                    # noqa: E402
from function_shard_workload import SIGMA, make_workload  # noqa: E402

SEEDS = (3, 4, 5, 6, 7)
SHARDS = (2, 3, 4)
FACTOR = 16


def shard_bounds(n, world, rank):
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def weights_from_sums(Lp, AAt, Ar, sigma):
    """Second step of landmarks_conditional (conditional.py:57-66 with A_l = A / sigma^2, r_l = r / sigma^2)."""
    s2 = sigma ** 2
    L_B = mo._sp_cholesky(mo.stabilize(AAt / s2, 1.0), lower=True, check_finite=False)
    c = mo._sp_trsolve(L_B, Ar / s2, lower=True)
    return mo._sp_trsolve(Lp.T, mo._sp_trsolve(L_B.T, c, lower=False), lower=False)


def measure(seed):
    x, y, xu, x_new = make_workload(seed)
    ls = mo.compute_ls(mo.validate_nn_distances(mo.exact_nn_distances(x)))
    cov = mo.compute_cov_func(mo.Matern52, ls)
    mu = 0.0
    Lp = mo._get_L(xu, cov)
    A = mo._sp_trsolve(Lp, cov(xu, x), lower=True)          # first step: A, then the two sums over cells
    r = y - mu
    K_eval = cov(np.concatenate([x, x_new]), xu)
    one = mu + K_eval @ weights_from_sums(Lp, A @ A.T, A @ r, SIGMA)
    # the two-step form is the oracle's conditional (which scales A by 1 / sigma^2 BEFORE the product: a re-association
    # of its own, so the two agree to rounding times conditioning, not bit for bit)
    ref = mo.landmarks_conditional(x, xu, y, mu, cov, sigma=SIGMA)
    assert np.abs(one - ref(np.concatenate([x, x_new]))).max() <= 1e-10 * np.abs(one).max()
    worst = 0.0
    for world in SHARDS:
        AAt, Ar = np.zeros((A.shape[0],) * 2), np.zeros((A.shape[0], r.shape[1]))
        for rank in range(world):
            lo, hi = shard_bounds(x.shape[0], world, rank)
            AAt = AAt + A[:, lo:hi] @ A[:, lo:hi].T
            Ar = Ar + A[:, lo:hi] @ r[lo:hi]
        sharded = mu + K_eval @ weights_from_sums(Lp, AAt, Ar, SIGMA)
        worst = max(worst, float(np.abs(sharded - one).max() / np.abs(one).max()))
    return worst


def measure_leverage(seed):
    """The same re-association applied to B^T B of the landmark leverage h = diag(B M^-1 B^T), M = sigma^2 K_uu + B^T B
    + jitter I (conditional.py:660-685, the oracle's _landmarks_leverage_one): the largest change of h, relative to the
    largest h.  Not part of tol: M is far worse conditioned than A A^T / sigma^2 + I, and this figure says by how much
    everything downstream of the leverage (HC3 residuals, variance weights) moves with the order of that sum."""
    x, y, xu, _ = make_workload(seed)
    ls = mo.compute_ls(mo.validate_nn_distances(mo.exact_nn_distances(x)))
    cov = mo.compute_cov_func(mo.Matern52, ls)
    Lp = mo._get_L(xu, cov)
    B, K_uu = cov(x, xu), Lp @ Lp.T

    def leverage(S):
        M = mo.stabilize(SIGMA ** 2 * K_uu + S, mo.DEFAULT_JITTER)
        return np.sum((B @ np.linalg.inv(M)) * B, axis=1), np.linalg.cond(M)

    one, cond = leverage(B.T @ B)
    assert np.abs(one - mo._landmarks_leverage_one(B, K_uu, SIGMA, mo.DEFAULT_JITTER)).max() == 0.0
    worst = 0.0
    for world in SHARDS:
        S = np.zeros_like(K_uu)
        for rank in range(world):
            lo, hi = shard_bounds(x.shape[0], world, rank)
            S = S + B[lo:hi].T @ B[lo:hi]
        worst = max(worst, float(np.abs(leverage(S)[0] - one).max() / np.abs(one).max()))
    return worst, cond


if __name__ == "__main__":
    per_seed = [measure(s) for s in SEEDS]
    for s, v in zip(SEEDS, per_seed):
        print(f"seed {s}: {v:.6e}")
    print(f"largest relative change: {max(per_seed):.6e}   tol = {FACTOR} x = {FACTOR * max(per_seed):.6e}")
    for s in SEEDS:
        v, cond = measure_leverage(s)
        print(f"seed {s}: leverage changes by {v:.6e} (cond M = {cond:.3e})")
