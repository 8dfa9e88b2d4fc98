"""One rank of the multi-PROCESS FunctionEstimator test (tests/test_gpu_function_sharded.py): a cell-sharded fit with one
scalar sigma under the launcher's environment (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*); the inputs come from
<out_dir>/workload.npz (x, y, landmarks, x_new: what the parent test holds), results go to <out_dir>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_dir):
    import mellon_amd
    from mellon_amd import distributed
    comm = distributed.init_from_env()
    with np.load(os.path.join(out_dir, "workload.npz")) as data:
        x, y, lm, x_new = data["x"], data["y"], data["landmarks"], data["x_new"]
    lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
    est = mellon_amd.FunctionEstimator(landmarks=lm, sigma=0.3)
    train = est.fit_predict(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(y[lo:hi]))
    np.savez(os.path.join(out_dir, f"rank{comm.rank}.npz"), train=train, new=est.predict(x_new), weights=est.predict.weights,
             n_obs=est.predict.n_obs, ls=est.ls, lo=lo, hi=hi, backend=str(comm.backend))
    comm.barrier()


if __name__ == "__main__":
    main(sys.argv[1])
