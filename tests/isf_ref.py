"""The float64 definition of observable.intermediate_scattering for the tests, as vectorised CPU torch, from the float32
positions and cell lengths the kernels see cast to float64, k = 2 pi n / L in float64:

    rho(k, t)   = sum_i w_i exp(i k.x_i(t))                 W2 = sum_i w_i^2
    F(k, tau)   = 1 / (|O_tau| W2)  sum_{t0 in O_tau} Re[ rho(k, t0 + tau) conj rho(k, t0) ]
    F_s(k, tau) = 1 / (|O_tau| W2)  sum_{t0 in O_tau} sum_i w_i^2 cos( k.(x_i(t0 + tau) - x_i(t0)) )
    O_tau = {0, s, 2 s, ... : t0 + tau < T}       F[b, tau], F_s[b, tau] = mean over the vectors of bin b (empty bin: 0)

isf64 returns F and F_s per bin and per vector, the gradients of sum(G * F) and sum(G * F_s) by float64 autograd, and for the
self part gabs: the gather of the gradient with every term replaced by |coefficient| |k_d|, NOT multiplied by |sin| (the
kernel's error in a sine is absolute, so the bound must not vanish where the sine does):

    gabs_i(t)[d] = w_i^2 sum_k |k_d| sum_{tau >= 1} |G[b(k), tau]| / (cnt_b |O_tau| W2) [ (t - tau in O_tau) + (t in O_tau, t + tau < T) ]

(lag 0 differentiates cos 0: no term)."""
import numpy as np
import torch


def origins(T, tau, stride):
    return torch.arange(0, T - tau, stride)


def bin_matrix(n_vecs, seg):
    """[M, B]: the bins' means as a matrix; an empty bin's column is zero."""
    cnt = np.diff(np.asarray(seg, dtype=np.int64))
    A = torch.zeros(n_vecs, len(cnt), dtype=torch.float64)
    b = np.repeat(np.arange(len(cnt)), cnt)
    A[torch.arange(n_vecs), torch.as_tensor(b)] = torch.as_tensor(1.0 / cnt[b])
    return A, b


def isf64(x, cell32, n, seg, n_lags, stride=1, weights=None, G=None, coherent=True, self_part=True):
    """x [T, N, 3] (one replica), n [M, 3] integer vectors sorted by bin, seg [B + 1].  Returns a dict of float64 numpy arrays:
    F, Fs [B, L]; Fk, Fsk [M, L] (per vector); g, gs [T, N, 3] = d sum(G * F) / dx, d sum(G * Fs) / dx (G [B, L], ones when
    None); gabs [T, N, 3].  Parts not asked for are None."""
    x32 = np.asarray(x, dtype=np.float32)
    T, N = x32.shape[0], x32.shape[1]
    q = torch.tensor(x32, dtype=torch.float64, requires_grad=True)
    Lc = torch.as_tensor(np.asarray(cell32, dtype=np.float32)).double().reshape(3)
    n = np.asarray(n, dtype=np.int64).reshape(-1, 3)
    M, B = len(n), len(seg) - 1
    k = 2 * np.pi * torch.as_tensor(n).double() / Lc                               # [M, 3]
    w = torch.ones(N, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights, dtype=np.float32)).double()
    w2, W2 = w * w, (w * w).sum()
    A, b_of = bin_matrix(M, seg)
    Gt = torch.ones(B, n_lags, dtype=torch.float64) if G is None else torch.as_tensor(np.asarray(G, dtype=np.float32)).double()
    ph = q @ k.t()                                                                 # [T, N, M]
    c, s = ph.cos(), ph.sin()
    out = dict(F=None, Fs=None, Fk=None, Fsk=None, g=None, gs=None, gabs=None)
    if coherent:
        re, im = (w[None, :, None] * c).sum(1), (w[None, :, None] * s).sum(1)     # [T, M]
        Fk = []
        for tau in range(n_lags):
            t0 = origins(T, tau, stride)
            Fk.append((re[t0 + tau] * re[t0] + im[t0 + tau] * im[t0]).sum(0) / (len(t0) * W2))
        Fk = torch.stack(Fk, 1)                                                    # [M, L]
        F = A.t() @ Fk
        (g,) = torch.autograd.grad((Gt * F).sum(), q, retain_graph=self_part)
        out.update(F=F.detach().numpy(), Fk=Fk.detach().numpy(), g=g.numpy())
    if self_part:
        Fsk = []
        gabs = torch.zeros(T, N, 3, dtype=torch.float64)
        cnt = np.diff(np.asarray(seg, dtype=np.int64))
        for tau in range(n_lags):
            t0 = origins(T, tau, stride)
            cosd = c[t0 + tau] * c[t0] + s[t0 + tau] * s[t0]                       # [n_o, N, M]
            Fsk.append((w2[None, :, None] * cosd).sum((0, 1)) / (len(t0) * W2))
            if tau >= 1:
                with torch.no_grad():
                    coef = Gt[torch.as_tensor(b_of), tau].abs() / (torch.as_tensor(cnt[b_of]).double() * len(t0) * W2)   # [M]
                    term = (w2[:, None] * (coef[:, None] * k.abs()).sum(0)[None, :])[None].expand(len(t0), N, 3)
                    gabs.index_add_(0, t0 + tau, term)
                    gabs.index_add_(0, t0, term)
        Fsk = torch.stack(Fsk, 1)
        Fs = A.t() @ Fsk
        (gs,) = torch.autograd.grad((Gt * Fs).sum(), q)
        out.update(Fs=Fs.detach().numpy(), Fsk=Fsk.detach().numpy(), gs=gs.numpy(), gabs=gabs.numpy())
    return out


def random_walk(T, N, seed, step=1.0, spread=50.0):
    """float32 [T, N, 3]: a Gaussian random walk of step length `step` per component, started at positions spread over
    +-spread: many cell lengths from the origin, as the unwrapped positions of a long fused trajectory are."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-spread, spread, (1, N, 3))
    steps = rng.normal(0.0, step, (T, N, 3))
    steps[0] = 0.0
    return (x0 + np.cumsum(steps, 0)).astype(np.float32)
