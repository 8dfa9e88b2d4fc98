"""One rank of the multi-PROCESS DimensionalityEstimator test (tests/test_gpu_dimensionality_sharded.py): a sharded fit
under the launcher's environment (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*), results to <out_dir>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_dir):
    import mellon_amd
    from mellon_amd import distributed
    comm = distributed.init_from_env()
    n, d, m = 3000, 5, 150
    x = np.random.default_rng(33).normal(size=(n, d))                 # identical on every rank
    cuts = [0] + [int(round(0.37 * n)) + (n - int(round(0.37 * n))) * r // (comm.world_size - 1)
                  for r in range(comm.world_size - 1)] + [n]          # rank 0 holds 37 %, the others share the rest
    lo, hi = cuts[comm.rank], cuts[comm.rank + 1]
    est = mellon_amd.DimensionalityEstimator(n_landmarks=m, predictor_with_uncertainty=True)
    dim = est.fit_predict(np.ascontiguousarray(x[lo:hi]))
    q = x[::37] + 0.01
    np.savez(os.path.join(out_dir, f"rank{comm.rank}.npz"), dim=dim, dens=est.log_density_x, z=est.pre_transformation,
             std=est.pre_transformation_std, L=np.asarray(est.L), distances=est.distances, d=est.d, nn=est.nn_distances,
             mu_dim=est.mu_dim, mu_dens=est.mu_dens, landmarks=np.asarray(est.landmarks), pred=est.predict(q),
             pred_dens=est.predict_density(q), n_eval=est.loss_func.n_eval, lo=lo, hi=hi, backend=str(comm.backend),
             self_test_ok=bool(comm.self_test_report.get("ok")))
    comm.barrier()


if __name__ == "__main__":
    main(sys.argv[1])
