"""The float64 definition of the static structure factor that the S(k) tests and tests/golden/make_sk_goldens.py share
(vectorised torch on the CPU), and the tests' error measure.  Inputs are the float32 positions and cell lengths the kernels
see, cast to float64; k = 2 pi n / L in float64.

    rho_f(k) = sum_i w_i exp(i k.x_fi)     S_f(k) = |rho_f(k)|^2 / sum_i w_i^2     S_f[b] = mean of S_f(k) over the bin's vectors
"""
import numpy as np
import torch


def sk64(xyz32, cell32, n, seg, weights=None, gS=None):
    """(S [F, B], S per vector [F, M], d sum(gS * S) / dx [F, N, 3] by float64 autograd or None) as float64 numpy arrays.
    n [M, 3] integer vectors sorted by bin, seg [B + 1] the bins' offsets in n."""
    x = torch.as_tensor(np.asarray(xyz32, dtype=np.float32)).double()
    x = (x[None] if x.dim() == 2 else x).clone().requires_grad_(gS is not None)
    L = torch.as_tensor(np.asarray(cell32, dtype=np.float32)).double().reshape(3)
    n = np.asarray(n, dtype=np.int64).reshape(-1, 3)
    seg = np.asarray(seg, dtype=np.int64)
    k = 2 * np.pi * torch.as_tensor(n).double() / L                               # [M, 3]
    w = torch.ones(x.shape[1], dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32)).double()
    Sk = []
    for f in range(x.shape[0]):                                                    # (a frame at a time: [N, M] phases)
        ph = x[f] @ k.t()
        re, im = (w[:, None] * ph.cos()).sum(0), (w[:, None] * ph.sin()).sum(0)
        Sk.append((re * re + im * im) / w.pow(2).sum())
    Sk = torch.stack(Sk)
    cnt = np.diff(seg)
    A = torch.zeros(len(n), len(cnt), dtype=torch.float64)                         # the bins' means as a matrix
    b = np.repeat(np.arange(len(cnt)), cnt)
    A[torch.arange(len(n)), torch.as_tensor(b)] = torch.as_tensor(1.0 / cnt[b])
    S = Sk @ A
    g = None
    if gS is not None:
        (g,) = torch.autograd.grad((S * torch.as_tensor(np.asarray(gS)).double()).sum(), x)
        g = g.numpy()
    return S.detach().numpy(), Sk.detach().numpy(), g


def n_eff(weights, n_atoms):
    if weights is None:
        return float(n_atoms)
    w = np.asarray(weights, dtype=np.float64)
    return float(w.sum() ** 2 / (w * w).sum())


def err_measure(S, S64, neff):
    """e = |S - S64| / (sqrt(N_eff S64) + 1): a per-atom phase error eps moves |rho|^2 by at most 2 |rho| N eps, so e is an
    eps-scale at Bragg peaks (S ~ N) and in the troughs alike."""
    S, S64 = np.asarray(S, dtype=np.float64), np.asarray(S64, dtype=np.float64)
    return np.abs(S - S64) / (np.sqrt(neff * np.abs(S64)) + 1.0)
