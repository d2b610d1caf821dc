"""The float64 definition of observable.msd for the tests, as vectorised CPU torch (one slice per lag over all origins and atoms):

    M_p[tau] = 1 / (|O_tau| sum_i w_i)  sum_{t0 in O_tau} sum_i w_i |x_i(t0 + tau) - x_i(t0)|^p ,   O_tau = {0, s, 2 s, ... : t0 + tau < T}

msd64 takes the float32 positions the kernels see, cast to float64, and returns (M2, M4, gx, gabs): gx = d(sum g2 M2 + sum g4 M4)/dx
from float64 autograd, gabs the same gather with every term replaced by its absolute value,

    gabs_i(t) = sum_tau c_tau w_i [ (t - tau in O_tau) |f|(x_t - x_{t-tau}) + (t in O_tau, t + tau < T) |f|(x_{t+tau} - x_t) ]
    |f|(d)    = |2 g2_tau d| + |4 g4_tau |d|^2 d|   per component,      c_tau = 1 / (|O_tau| sum w)

the scale a float32 sum of those terms is allowed to err by."""
import numpy as np
import torch


def origins(T, tau, stride):
    return torch.arange(0, T - tau, stride)


def msd64(x, n_lags, stride=1, weights=None, g2=None, g4=None):
    """x [T, N, 3] (one replica).  Returns numpy float64 (M2 [L], M4 [L], gx [T, N, 3], gabs [T, N, 3]); the gradients are of
    sum(g2 * M2) + sum(g4 * M4), g2 defaulting to ones and g4 to zeros."""
    x32 = np.asarray(x, dtype=np.float32)
    T, N = x32.shape[0], x32.shape[1]
    q = torch.tensor(x32, dtype=torch.float64, requires_grad=True)
    w = torch.ones(N, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32)).double()
    c2 = torch.ones(n_lags, dtype=torch.float64) if g2 is None else torch.as_tensor(np.asarray(g2, dtype=np.float32)).double()
    c4 = torch.zeros(n_lags, dtype=torch.float64) if g4 is None else torch.as_tensor(np.asarray(g4, dtype=np.float32)).double()
    sw = w.sum()
    M2, M4 = [], []
    gabs = torch.zeros(T, N, 3, dtype=torch.float64)
    for tau in range(n_lags):
        t0 = origins(T, tau, stride)
        d = q[t0 + tau] - q[t0]                               # [n_origins, N, 3]
        d2 = d.pow(2).sum(-1)
        c = 1.0 / (len(t0) * sw)
        M2.append((w * d2).sum() * c)
        M4.append((w * d2 * d2).sum() * c)
        with torch.no_grad():
            term = c * w[None, :, None] * ((2 * c2[tau] * d).abs() + (4 * c4[tau] * d2[..., None] * d).abs())
            gabs.index_add_(0, t0 + tau, term)
            gabs.index_add_(0, t0, term)
    M2, M4 = torch.stack(M2), torch.stack(M4)
    (gx,) = torch.autograd.grad((c2 * M2).sum() + (c4 * M4).sum(), q)
    return M2.detach().numpy(), M4.detach().numpy(), gx.numpy(), gabs.numpy()


def random_walk(T, N, seed, step=1.0, drift=50.0):
    """float32 [T, N, 3]: a Gaussian random walk of step length `step` per component, started at positions spread over
    +-drift -- many cell lengths from the origin, as the unwrapped positions of a long fused trajectory are."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-drift, drift, (1, N, 3))
    steps = rng.normal(0.0, step, (T, N, 3))
    steps[0] = 0.0
    return (x0 + np.cumsum(steps, 0)).astype(np.float32)
