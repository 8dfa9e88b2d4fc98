"""The importance tail of the MAP solve on a real MI355X (-m gpu): after the preconditioner rebuild the solve finishes on
the first-order-corrected objective of an importance-sampled row LIST, the full fp64 objective anchoring and verifying.

* the objective kernel over a row list (csrc/objective.hip): a list that is an arithmetic progression gives the bits of the
  strided launch; a random sorted list with weights against a NumPy restatement with long-double accumulation;
* the path: same optimum with the tail on and off, fewer full passes with it on, sharded = unsharded, bit-reproducible,
  and a hard workload (tools/hard_cases.py's tree) on which the phase must not cost the optimum.
"""
import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu


def rel_max(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def rel_std(a, b):
    return np.std(a - b) / np.std(b)


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


# ---- kernel ---------------------------------------------------------------------------------------------------------
# m = 300: the row-per-lane (VEC) variants, leading dimension 304 (4 pad columns); m = 3200: the wide variants (four column
# pairs per thread), leading dimension 3200; m = 3210: the same with pad columns (3216).  The leading dimension is the
# library's pad16(m), so the pad columns of the wide path need an m of their own.
KERNEL_M = [300, 3200, 3210]
N_ROWS = 1000


@pytest.fixture(scope="module", params=KERNEL_M)
def kernel_problem(request, ctx):
    from mellon_amd import _lib
    m = request.param
    rng = np.random.default_rng(m)
    L = rng.normal(size=(N_ROWS, m)) * (0.5 / np.sqrt(m))
    nn = rng.uniform(0.2, 1.0, size=N_ROWS)
    V, Vdr = mo.nn_likelihood_constants(nn, 5)
    fit = _lib.Fit.from_L(ctx, L)
    fit.set_likelihood(V, Vdr, -3.0)
    z = rng.normal(size=m) * 0.3
    yield fit, L, V, Vdr, -3.0, z
    fit.close()


@pytest.mark.parametrize("count,first,stride", [(1, 7, 3), (255, 2, 3), (700, 1, 1), (143, 0, 7)])
def test_a_progression_list_equals_the_strided_launch(kernel_problem, count, first, stride):
    """1 row, 255 rows (fewer than the 256 workgroups), 700 rows (ragged last workgroup), and a stride that ends on the
    buffer's last row: loss, gradient and the rows' f of the list launch are the bits of the strided launch."""
    fit, L, V, Vdr, mu, z = kernel_problem
    assert first + (count - 1) * stride < N_ROWS
    rows = first + stride * np.arange(count, dtype=np.int64)
    for scale in (0.0, float(stride)):
        ls, gs, fs = fit.objective_rows(z, count=count, first=first, stride=stride, out_scale=scale)
        ll, gl, fl = fit.objective_rows(z, rows=rows, out_scale=scale)
        assert ll == ls, (ll, ls)
        assert np.array_equal(gl, gs)
        assert np.array_equal(fl, fs)
    # ... and the strided launch is what it says (so that equal bits are the right bits)
    assert rel_max(fs, L[rows] @ z + mu) < 1e-12


def _restatement(L, V, Vdr, mu, z, rows, w):
    """Likelihood sum and its gradient over the listed rows, the weight on each row's exponential (csrc/objective.hip, row
    list), long-double accumulation (inference.py:83-92)."""
    Lr = L[rows].astype(np.longdouble)
    f = Lr @ z.astype(np.longdouble) + np.longdouble(mu)
    a = np.exp(f + V[rows].astype(np.longdouble))
    wl = w.astype(np.longdouble)
    loss = (wl * a - (f + Vdr[rows].astype(np.longdouble))).sum()
    grad = Lr.T @ (wl * a - 1.0)
    return float(loss), np.asarray(grad, dtype=np.float64), np.asarray(f, dtype=np.float64)


@pytest.mark.parametrize("count", [1, 255, 700])
def test_a_weighted_random_list_against_numpy(kernel_problem, count):
    """Random sorted list, weights in [1, 1e4].  Tolerances: those of the objective-kernel tests of tests/test_gpu_ops.py at
    these sizes -- loss 1e-12 and gradient 1e-10 (test_fit_pipeline_sparse, m <= 1000), gradient 1e-11 beyond
    (test_objective_wide_landmark_counts) -- f 1e-12 (both)."""
    fit, L, V, Vdr, mu, z = kernel_problem
    rng = np.random.default_rng(1000 + count)
    rows = np.sort(rng.choice(N_ROWS, size=count, replace=False)).astype(np.int64)
    w = np.exp(rng.uniform(0.0, np.log(1e4), size=count))
    loss, grad, f = fit.objective_rows(z, rows=rows, weights=w)
    loss_ref, grad_ref, f_ref = _restatement(L, V, Vdr, mu, z, rows, w)
    print(f"m={L.shape[1]} count={count}: loss rel {abs(loss - loss_ref) / abs(loss_ref):.2e}, grad rel {rel_max(grad, grad_ref):.2e}, "
          f"f rel {rel_max(f, f_ref):.2e}")
    assert abs(loss - loss_ref) < 1e-12 * abs(loss_ref)
    assert rel_max(grad, grad_ref) < (1e-10 if L.shape[1] <= 1000 else 1e-11)
    assert rel_max(f, f_ref) < 1e-12
    # weights of exactly one: the unweighted list
    l1, g1, _ = fit.objective_rows(z, rows=rows, weights=np.ones(count))
    l0, g0, _ = fit.objective_rows(z, rows=rows)
    assert l1 == l0 and np.array_equal(g1, g0)


# ---- path -----------------------------------------------------------------------------------------------------------
PATH_ENV = {"MELLON_AMD_REBUILD": "1", "MELLON_AMD_SUBSAMPLE": "1", "MELLON_AMD_MIXED": "0"}


def _fit_path(mellon, monkeypatch, x, nn, lm, tail):
    for k, v in PATH_ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MELLON_AMD_IMPORTANCE_TAIL", tail)
    est = mellon.DensityEstimator(landmarks=lm, nn_distances=nn, check_rank=False)
    dens = est.fit_predict(x)
    st = est._fit.stage_times()
    return dens, st, est.opt_state


@pytest.fixture(scope="module")
def path_workload():
    """The shape of tests/test_gpu_round3.py's path_workload."""
    from sklearn.cluster import k_means
    n, d, m = 40_000, 10, 300
    x = mo.gaussian_mixture(n, d, seed=13)
    nn = mo.exact_nn_distances(x)
    lm = np.ascontiguousarray(k_means(x[:8000], m, n_init=1, random_state=42)[0])
    ref = mo.density_fit(x, landmarks=lm, nn_distances=nn, lbfgsb_options=mo.LBFGSB_TIGHT)
    return x, nn, lm, ref


def test_tail_on_and_off_reach_the_oracles_optimum(mellon, path_workload, monkeypatch):
    x, nn, lm, ref = path_workload
    on, st_on, _ = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    off, st_off, _ = _fit_path(mellon, monkeypatch, x, nn, lm, "0")
    print("tail on :", {k: st_on[k] for k in ("objective_launches", "objective_tail_launches", "objective_tail_rows",
                                               "objective_pass_equivalents", "objective_tail_guard", "precond_rebuilds")})
    print("tail off:", {k: st_off[k] for k in ("objective_launches", "objective_tail_launches", "objective_pass_equivalents",
                                               "precond_rebuilds")})
    print(f"on vs oracle {rel_max(on, ref.log_density_x):.2e}, off vs oracle {rel_max(off, ref.log_density_x):.2e}, "
          f"on vs off {rel_max(on, off):.2e}")
    assert st_on["objective_tail_launches"] > 0 and st_on["objective_tail_rows"] > 0, st_on
    assert st_off["objective_tail_launches"] == 0, st_off
    assert st_on["precond_rebuilds"] == 1.0 and st_off["precond_rebuilds"] == 1.0
    for dens in (on, off):
        assert rel_max(dens, ref.log_density_x) < 1e-5 and rel_std(dens, ref.log_density_x) < 1e-5
    assert rel_max(on, off) < 2e-6
    assert st_on["objective_launches"] <= st_off["objective_launches"], (st_on, st_off)


def test_tail_sharded_equals_unsharded(mellon, path_workload, monkeypatch):
    """3 uneven thread-rank shards: the list is drawn by a hash of the GLOBAL cell index from all-reduced sums."""
    from mellon_amd import distributed
    x, nn, lm, _ = path_workload
    x, nn = x[:-7], nn[:-7]
    dens1, st1, _ = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    assert st1["objective_tail_launches"] > 0

    def body(comm):
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        est = mellon.DensityEstimator(landmarks=lm, nn_distances=nn[lo:hi], check_rank=False)
        dens = est.fit_predict(np.ascontiguousarray(x[lo:hi]))
        st = est._fit.stage_times()
        return dens, st["objective_tail_launches"], st["precond_rebuilds"]

    res = distributed.run_loopback(3, body)
    assert all(r[1] > 0 and r[2] == 1.0 for r in res), [r[1:] for r in res]
    dens = np.concatenate([r[0] for r in res])
    print(f"sharded vs unsharded {rel_max(dens, dens1):.2e}")
    assert rel_max(dens, dens1) < 1e-6


def test_two_tail_fits_are_the_same_bits(mellon, path_workload, monkeypatch):
    x, nn, lm, _ = path_workload
    a, st_a, _ = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    b, st_b, _ = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    assert st_a["objective_tail_launches"] > 0
    assert np.array_equal(a, b)
    for k in ("objective_launches", "objective_tail_launches", "objective_tail_rows", "objective_sub_launches"):
        assert st_a[k] == st_b[k], k


def _tree_cells(n, d, rng, branches=6):
    """tools/hard_cases.py `trajectories`: cells along a branching tree in a 3-D latent space, embedded in d dimensions."""
    t = rng.beta(0.7, 1.3, size=n)
    b = rng.integers(0, branches, size=n)
    dirs = rng.normal(size=(branches, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    bend = rng.normal(size=(branches, 3)) * 0.5
    z = t[:, None] * dirs[b] + (t ** 2)[:, None] * bend[b] + 0.02 * (1 + 3 * t)[:, None] * rng.normal(size=(n, 3))
    W1 = rng.normal(size=(3, d)); W2 = rng.normal(size=(3, d))
    x = np.tanh(z @ W1) + 0.3 * np.sin(2.0 * z @ W2)
    return np.ascontiguousarray(x * (0.8 ** np.arange(d))[None, :])


def test_tail_on_a_hard_workload(mellon, ctx, monkeypatch):
    """The tree of tools/hard_cases.py (d = 20) cut to 40 000 cells, 300 landmarks: with the tail the fit lands where it
    lands without, and does not run into the iteration limit; a guard that fired is on the record."""
    n, d, m = 40_000, 20, 300
    x = _tree_cells(n, d, np.random.default_rng(11))
    xd = ctx.to_device(x)
    nn = ctx.nn_distances(xd, xd)
    xd.free()
    lm = np.ascontiguousarray(x[np.sort(np.random.default_rng(42).choice(n, m, replace=False))])
    on, st_on, state_on = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    off, st_off, state_off = _fit_path(mellon, monkeypatch, x, nn, lm, "0")
    print("tail on :", {k: st_on[k] for k in ("objective_launches", "objective_tail_launches", "objective_pass_equivalents",
                                               "objective_tail_guard", "precond_rebuilds", "precond_rebuilds_declined")}, state_on.nit)
    print("tail off:", {k: st_off[k] for k in ("objective_launches", "objective_pass_equivalents", "precond_rebuilds",
                                               "precond_rebuilds_declined")}, state_off.nit)
    print(f"on vs off {np.abs(on - off).max() / np.abs(off).max():.2e}")
    assert state_on.success and state_on.status == 0 and state_on.nit < 5000, state_on
    assert np.isfinite(on).all()
    assert np.abs(on - off).max() <= 1e-5 * np.abs(off).max()
    assert st_off["objective_tail_launches"] == 0 and st_off["objective_tail_guard"] == 0
    assert st_on["objective_tail_guard"] in (0.0, 1.0)          # at most once per solve, and counted
    assert st_on["objective_tail_launches"] > 0 and st_on["precond_rebuilds"] >= 1.0, st_on


def test_a_preconditioner_that_fails_its_trial_inside_the_tail(mellon, path_workload, monkeypatch):
    """The rebuilt preconditioner's trial (solver.h: revert_after) counts the tail's iterations: with a trial of one
    iteration it fails while the solve is on the row list -- back to the tail's anchor, first preconditioner restored,
    the rest on full passes, same optimum."""
    x, nn, lm, ref = path_workload
    monkeypatch.setenv("MELLON_AMD_REVERT_AFTER", "1")
    monkeypatch.setenv("MELLON_AMD_MAX_REBUILDS", "1")
    dens, st, state = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    print({k: st[k] for k in ("objective_launches", "objective_tail_launches", "precond_rebuilds", "precond_reverts", "objective_tail_guard")})
    assert st["objective_tail_launches"] > 0 and int(st["precond_reverts"]) == 1 and st["precond_rebuilds"] == 1.0, st
    assert state.success
    assert rel_max(dens, ref.log_density_x) < 1e-5 and rel_std(dens, ref.log_density_x) < 1e-5


def test_the_guard_returns_to_the_anchor(mellon, path_workload, monkeypatch):
    """A deliberately poor list (MELLON_AMD_TAIL_POOR_LIST=1: weights of at most 1 where 1 / p_i belongs, a surrogate with far
    too little curvature): the point it leads to is worse on the full objective than the anchor, the verification pass says so,
    the solve goes back to the anchor and finishes on full passes -- same optimum, and the counter says what happened."""
    x, nn, lm, ref = path_workload
    monkeypatch.setenv("MELLON_AMD_TAIL_POOR_LIST", "1")
    dens, st, state = _fit_path(mellon, monkeypatch, x, nn, lm, "1")
    print({k: st[k] for k in ("objective_launches", "objective_tail_launches", "objective_tail_guard", "precond_rebuilds")}, state.nit)
    assert st["objective_tail_launches"] > 0 and st["objective_tail_guard"] == 1.0, st
    assert state.success and state.nit < 5000
    assert rel_max(dens, ref.log_density_x) < 1e-5 and rel_std(dens, ref.log_density_x) < 1e-5
