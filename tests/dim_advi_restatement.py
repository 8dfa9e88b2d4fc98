"""NumPy restatement of the reference's mean-field ADVI (mellon/inference.py:768-876) for the dimensionality loss, on top of
dim_restatement's loss and gradient.  Test infrastructure only: the product never imports it.

The parameters are the (2, m) pair (log-dimensionality row, log-density row); the reference flattens them for the draws
(2 m per sample) and restores the shape of the two gradient leaves.  As in advi_restatement.py, the draws are the
project's own stream (NumPy's generator keyed by the step) and the gradients are jax.value_and_grad's in closed form:
  value = mean_s[loss(z_s) + log q(z_s)],  d / d mean = mean_s grad loss(z_s),
  d / d log_std = exp(log_std) mean_s(grad loss(z_s) eps_s) - 1,  z_s = mean + exp(log_std) eps_s."""
import numpy as np

import dim_restatement as dr

LOG_2PI = np.log(2 * np.pi)
GRAD_NOISE = 1e-8          # relative to each sample's largest gradient entry: the device's gradient tolerance


def advi_draws(t, nsamples, m):
    return np.random.default_rng(int(t)).standard_normal((int(nsamples), int(m)))


def losses_and_grads(Z, L, ell, mu_dim, mu_dens):
    """(loss[S], grad[S, 2 m]) of dim_restatement at the S flat points of Z."""
    loss = np.array([dr.dim_loss(z, L, ell, mu_dim, mu_dens) for z in Z])
    grad = np.stack([dr.dim_grad_hess(z, L, ell, mu_dim, mu_dens)[0].ravel() for z in Z])
    return loss, grad


def elbo_value_and_grad(mean, log_std, eps, L, ell, mu_dim, mu_dens, noise=None, batch=None):
    """(-ELBO estimate, d / d mean, d / d log_std) over the draws eps (S x 2 m); mean and log_std flat or (2, m), the
    gradients in their shape.  `noise` (a Generator): every sample's gradient is perturbed by GRAD_NOISE of its largest
    entry.  `batch(Z) -> (loss, grad)` replaces the restatement's loss (the device's, teacher-forced)."""
    shape = np.shape(mean)
    mean, log_std = np.ravel(mean), np.ravel(log_std)
    std = np.exp(log_std)
    Z = mean[None, :] + std[None, :] * eps
    loss, g = losses_and_grads(Z, L, ell, mu_dim, mu_dens) if batch is None else batch(Z)
    if noise is not None:
        g = g + GRAD_NOISE * np.abs(g).max(axis=1, keepdims=True) * noise.standard_normal(g.shape)
    logq = np.sum(-0.5 * np.square(eps) - log_std[None, :] - 0.5 * LOG_2PI, axis=1)     # norm.logpdf(z, mean, std) summed
    return (float(np.mean(loss + logq)), np.mean(g, axis=0).reshape(shape),
            (std * np.mean(g * eps, axis=0) - 1.0).reshape(shape))


def run_advi(z0, L, ell, mu_dim, mu_dens, n_iter=100, init_learn_rate=0.1, nsamples=40, draws=advi_draws, noise=None,
             history=None):
    """inference.py:821-876 with jax.example_libraries.optimizers.adam restated (b1 0.9, b2 0.999, eps 1e-8, bias-corrected,
    rate exp(-0.01 t) init_learn_rate) on the two leaves (mean, log_std), each (2, m); log_std starts at 0.  `history`
    (a list) receives (mean, log_std) after every step.  Returns (mean, std, losses)."""
    b1, b2 = 0.9, 0.999
    params = [np.array(z0, dtype=np.float64), np.zeros(np.shape(z0))]
    m1 = [np.zeros_like(p) for p in params]
    m2 = [np.zeros_like(p) for p in params]
    losses = []
    for t in range(n_iter):
        value, gm, gs = elbo_value_and_grad(params[0], params[1], draws(t, nsamples, params[0].size), L, ell, mu_dim,
                                            mu_dens, noise=noise)
        losses.append(value)
        rate = np.exp(-1e-2 * t) * init_learn_rate
        for j, g in enumerate((gm, gs)):
            m1[j] = (1 - b1) * g + b1 * m1[j]
            m2[j] = (1 - b2) * np.square(g) + b2 * m2[j]
            mhat, vhat = m1[j] / (1 - b1 ** (t + 1)), m2[j] / (1 - b2 ** (t + 1))
            params[j] = params[j] - rate * mhat / (np.sqrt(vhat) + 1e-8)
        if history is not None:
            history.append((params[0].copy(), params[1].copy()))
    return params[0], np.exp(params[1]), np.asarray(losses)


def synthetic(n, m, k, seed):
    """A factor, sorted distances and means on which the restatement is finite everywhere near z = 0 (the inputs of
    test_gpu_dimensionality.py::test_dim_objective_against_restatement)."""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, m)) * (0.5 / np.sqrt(m))
    ell = dr.ell_of(np.abs(rng.normal(size=(n, k))) + 0.05)
    return L, ell, 0.3, 1.1


def knn_distances(x, k):
    """The k nearest other cells of every cell, ascending (brute force, difference form)."""
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return np.sqrt(np.sort(d2, axis=1)[:, :k])
