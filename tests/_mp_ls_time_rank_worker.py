"""One rank of the two-process test of the automatic `ls_time` (tests/test_gpu_ls_time_sharded.py): the default
TimeSensitiveDensityEstimator call on this rank's contiguous shard under the launcher's environment, results to
<out_dir>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out_dir):
    import mellon_amd
    from mellon_amd import distributed
    from test_gpu_ls_time_sharded import N_LANDMARKS, time_series      # (the shared synthetic input)
    comm = distributed.init_from_env()
    x, times = time_series()
    lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
    est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=N_LANDMARKS)
    est.fit(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(times[lo:hi]))
    np.savez(os.path.join(out_dir, f"rank{comm.rank}.npz"), ls_time=est.ls_time, dens=np.asarray(est.log_density_x),
             landmarks=np.asarray(est.landmarks), z=np.asarray(est.pre_transformation), backend=str(comm.backend))
    comm.barrier()


if __name__ == "__main__":
    main(sys.argv[1])
