"""The synthetic regression workload of the cell-sharded FunctionEstimator tests (tests/test_gpu_function_sharded.py,
tests/_mp_function_rank_worker.py) and of the script that measures their tolerance (tools/function_shard_tol.py):
NumPy and the oracle only, nothing of the code under test."""
import numpy as np

N_CELLS, N_DIMS, N_OUTPUTS, N_LANDMARKS, N_HELD_OUT, SIGMA = 2399, 5, 3, 150, 64, 0.3


def make_workload(seed=3, n=N_CELLS, d=N_DIMS, p=N_OUTPUTS, m=N_LANDMARKS, held_out=N_HELD_OUT, noise=SIGMA):
    """(x (n, d), y (n, p), landmarks (m, d), held-out points (held_out, d)): cells of a 10-component Gaussian mixture
    (n odd, so shards are uneven), p smooth functions of them plus Gaussian noise, m k-means centroids as the given
    landmarks (m = 0: none), and further draws from the same mixture that are not trained on."""
    from oracle import mellon_oracle as mo
    cells = mo.gaussian_mixture(n + held_out, d, seed=seed)
    x, x_new = np.ascontiguousarray(cells[:n]), np.ascontiguousarray(cells[n:])
    rng = np.random.default_rng(1000 + seed)
    directions = rng.normal(size=(d, p)) / np.sqrt(d)
    phase = rng.uniform(0, 2 * np.pi, size=p)
    y = np.sin(0.5 * (x @ directions) + phase) + 0.25 * np.cos(0.3 * x[:, :1] * x[:, 1:2]) + noise * rng.normal(size=(n, p))
    landmarks = None
    if m:
        from sklearn.cluster import k_means
        landmarks = np.ascontiguousarray(k_means(x, m, n_init=1, random_state=42)[0])
    return x, np.ascontiguousarray(y), landmarks, x_new
