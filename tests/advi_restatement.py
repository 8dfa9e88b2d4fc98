"""NumPy restatement of the reference's mean-field ADVI (mellon/inference.py:768-876) on top of the oracle's loss and
gradient, written from reading it.  Test infrastructure only: the product never imports it.

The reference differentiates  objective(params, t) = -mean_s[ -loss(z_s) - log q(z_s) ],  z_s = mean + exp(log_std) eps_s,
with jax.value_and_grad; the gradients below are that derivative in closed form.  The draws are the project's own stream
(mellon_amd.inference.advi_draws: NumPy's generator keyed by the step), not JAX's."""
import numpy as np

from oracle import mellon_oracle as mo

LOG_2PI = np.log(2 * np.pi)


def advi_draws(t, nsamples, m):
    return np.random.default_rng(int(t)).standard_normal((int(nsamples), int(m)))


def elbo_value_and_grad(mean, log_std, eps, L, mu, V, Vdr):
    """(-ELBO estimate, d / d mean, d / d log_std) over the draws eps (S x m)."""
    std = np.exp(log_std)
    value, g_mean, g_ls = 0.0, np.zeros_like(mean), np.zeros_like(mean)
    S = eps.shape[0]
    for s in range(S):
        loss, grad = mo.loss_and_grad(mean + std * eps[s], L, mu, V, Vdr)
        logq = np.sum(-0.5 * eps[s] ** 2 - log_std - 0.5 * LOG_2PI)       # norm.logpdf(z, mean, std) summed
        value += loss + logq
        g_mean += grad
        g_ls += grad * eps[s]
    return value / S, g_mean / S, std * g_ls / S - 1.0


def run_advi(z0, L, mu, V, Vdr, n_iter=100, init_learn_rate=0.1, nsamples=40, draws=advi_draws):
    """inference.py:821-876 with jax.example_libraries.optimizers.adam restated (b1 0.9, b2 0.999, eps 1e-8, bias-corrected,
    rate exp(-0.01 t) init_learn_rate) on the two leaves (mean, log_std); log_std starts at 0."""
    params = [np.array(z0, dtype=np.float64), np.zeros(len(z0))]
    m1 = [np.zeros_like(p) for p in params]
    m2 = [np.zeros_like(p) for p in params]
    losses = []
    for t in range(n_iter):
        value, gm, gs = elbo_value_and_grad(params[0], params[1], draws(t, nsamples, len(z0)), L, mu, V, Vdr)
        losses.append(value)
        for j, g in enumerate((gm, gs)):
            m1[j] = 0.1 * g + 0.9 * m1[j]
            m2[j] = 0.001 * g * g + 0.999 * m2[j]
            mhat, vhat = m1[j] / (1 - 0.9 ** (t + 1)), m2[j] / (1 - 0.999 ** (t + 1))
            params[j] = params[j] - np.exp(-1e-2 * t) * init_learn_rate * mhat / (np.sqrt(vhat) + 1e-8)
    return params[0], np.exp(params[1]), np.asarray(losses)


def two_blobs(n, d, seed=42):
    """Two Gaussian blobs of n / 2 cells each at +1 and -1, std 0.5 (the reference's tests/test_laplace.py:170-176)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n // 2, d)) * 0.5 + 1
    b = rng.standard_normal((n - n // 2, d)) * 0.5 - 1
    return np.ascontiguousarray(np.concatenate([a, b]))
