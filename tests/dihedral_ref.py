"""The float64 definitions behind the dihedral tests, as CPU torch (differentiable; pass float64 tensors).

Quadruple (i, j, k, l):  b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k,  n1 = b1 x b2, n2 = b2 x b3

    cos phi = n1.n2 / sqrt(|n1|^2 |n2|^2)            phi = atan2(|b2| b1.n2, n1.n2)   in (-pi, pi]  (IUPAC sign)
    U       = sum_m A[type, m] cos^m phi ,  m = 0 .. 4
    raw[b]  = sum exp(-1/2 (wrap(phi - mu_b) / width)^2) ,  mu_b = -pi + (b + 1/2) 2 pi / nbins,  wrap onto [-pi, pi)

With cell lengths L every bond vector is re-imaged with topology.get_offsets (-[b >= L/2] + [b < -L/2]).  A term with
|n1|^2 <= eps^2 |b1|^2 |b2|^2 or |n2|^2 <= eps^2 |b2|^2 |b3|^2, eps = 2^-20, is skipped: phi = cos phi = 0 with zero gradient,
no energy, no histogram weight."""
import math

import numpy as np
import torch

EPS = 2.0 ** -20


def _image(b, L):
    if L is None:
        return b
    L = torch.as_tensor(np.asarray(L, dtype=np.float32)).to(b)
    return b + (-(b >= 0.5 * L).to(b) + (b < -0.5 * L).to(b)) * L


def geometry(x, top, L=None):
    """x [..., N, 3], top [n, 4] -> (cos phi, phi, valid), each [..., n]."""
    top = torch.as_tensor(np.asarray(top), dtype=torch.long).reshape(-1, 4)
    i, j, k, l = top.unbind(1)
    b1 = _image(x[..., j, :] - x[..., i, :], L)
    b2 = _image(x[..., k, :] - x[..., j, :], L)
    b3 = _image(x[..., l, :] - x[..., k, :], L)
    n1 = torch.cross(b1, b2, dim=-1)
    n2 = torch.cross(b2, b3, dim=-1)
    N1, N2 = n1.pow(2).sum(-1), n2.pow(2).sum(-1)
    B1, B2, B3 = b1.pow(2).sum(-1), b2.pow(2).sum(-1), b3.pow(2).sum(-1)
    valid = (N1 > EPS * EPS * B1 * B2) & (N2 > EPS * EPS * B2 * B3)
    one = torch.ones_like(N1)
    dot = (n1 * n2).sum(-1)
    cos = torch.where(valid, dot / torch.where(valid, N1 * N2, one).sqrt(), torch.zeros_like(dot))
    y = torch.where(valid, B2, one).sqrt() * (b1 * n2).sum(-1)
    phi = torch.where(valid, torch.atan2(torch.where(valid, y, torch.zeros_like(y)), torch.where(valid, dot, one)),
                      torch.zeros_like(dot))
    return cos, phi, valid


def cos_phi(x, top, L=None):
    return geometry(x, top, L)[0]


def phi(x, top, L=None):
    return geometry(x, top, L)[1]


def energy(x, top, coeffs, types=None, L=None):
    """sum over the valid terms of sum_m A[type, m] cos^m phi; coeffs [5] or [n_types, 5]."""
    c, _, valid = geometry(x, top, L)
    A = coeffs.reshape(-1, 5)
    ty = torch.zeros(c.shape[-1], dtype=torch.long) if types is None else torch.as_tensor(np.asarray(types), dtype=torch.long)
    a = A[ty]
    u = a[:, 0] + c * (a[:, 1] + c * (a[:, 2] + c * (a[:, 3] + c * a[:, 4])))
    return torch.where(valid, u, torch.zeros_like(u)).sum()


def centres(nbins):
    d = 2.0 * math.pi / nbins
    return -math.pi + (torch.arange(nbins, dtype=torch.float64) + 0.5) * d


def histogram(ph, valid, nbins, width=None):
    """raw [nbins] of the angles ph [...] (nearest image of every centre), skipped terms left out."""
    width = 2.0 * math.pi / nbins if width is None else float(width)
    mu = centres(nbins).to(ph.dtype)
    d = ph.reshape(-1, 1) - mu[None, :]
    d = d - 2.0 * math.pi * torch.floor((d + math.pi) / (2.0 * math.pi))           # wrap onto [-pi, pi)
    e = torch.exp(-0.5 * (d / width).pow(2)) * valid.reshape(-1, 1).to(ph.dtype)
    return e.sum(0)


def distribution(x, top, nbins, width=None, L=None):
    _, ph, valid = geometry(x, top, L)
    raw = histogram(ph, valid, nbins, width)
    return raw / raw.sum(), ph


class DihedralTerm:
    """The torsion term with the oracle's term protocol (n_theta, reset, energy, force, force_vjp by autograd, like
    oracle._BondedTerm), with the coefficients as its parameters: force_vjp's third output is d(w.F)/dcoeffs, flattened."""

    def __init__(self, top, coeffs, cell, types=None):
        self.top = np.asarray(top)
        self.theta = torch.as_tensor(np.asarray(coeffs, dtype=np.float32)).reshape(-1)
        self.types = types
        c = torch.as_tensor(np.asarray(cell, dtype=np.float32))
        self.cell_len = (torch.diag(c) if c.dim() == 2 else c).numpy()

    @property
    def n_theta(self):
        return self.theta.numel()

    def reset(self, q):
        pass

    def energy(self, q, theta=None):
        th = self.theta.to(q) if theta is None else theta
        return energy(q, self.top, th, self.types, self.cell_len)

    def force(self, q):
        with torch.enable_grad():
            x = q.detach().requires_grad_(True)
            (g,) = torch.autograd.grad(self.energy(x), x)
        return -g

    def force_vjp(self, q, w):
        with torch.enable_grad():
            x = q.detach().requires_grad_(True)
            th = self.theta.to(q).detach().requires_grad_(True)
            (g,) = torch.autograd.grad(self.energy(x, th), x, create_graph=True)
            dq, dth = torch.autograd.grad((w.detach() * (-g)).sum(), (x, th))
        return (-g).detach(), dq.detach(), dth.detach()


def random_chain(n, seed, step=1.1, min_sin=0.35, start=(2.5, 2.5, 2.5)):
    """float64 [n, 3]: a random walk of fixed step whose consecutive bonds make an angle with sine >= min_sin, so that every
    chain dihedral is regular (unwrapped)."""
    rng = np.random.default_rng(seed)
    x = [np.asarray(start, dtype=np.float64)]
    prev = None
    while len(x) < n:
        s = rng.normal(0, 1, 3)
        s *= step / np.linalg.norm(s)
        if prev is not None and np.linalg.norm(np.cross(prev, s)) < min_sin * step * step:
            continue
        x.append(x[-1] + s)
        prev = s
    return np.array(x)
