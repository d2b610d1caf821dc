"""Reference of trajectory reweighting (mdgrad_amd/reweight.py) in float64 numpy, CPU only: the weights, the effective sample
size, the weighted average and the covariance-identity gradient, from per-frame energies and per-frame observables.

    w_f      = exp(-(U_f - Uref_f) / kT) / sum_g exp(-(U_g - Uref_g) / kT)
    n_eff    = exp(-sum_f w_f ln w_f)
    <O>      = sum_f w_f O_f
    d<O>/dtheta = -(sum_f w_f O_f dU_f/dtheta - <O> sum_f w_f dU_f/dtheta) / kT         (O_f does not depend on theta)

Used by tests/test_reweight_host.py and tests/test_gpu_reweight.py."""
import numpy as np


def weights(U, U_ref, kT):
    a = -(np.asarray(U, np.float64) - np.asarray(U_ref, np.float64)).reshape(-1) / float(kT)
    e = np.exp(a - a.max())
    return e / e.sum()


def n_eff(w):
    w = np.asarray(w, np.float64).reshape(-1)
    nz = w[w > 0]
    return float(np.exp(-(nz * np.log(nz)).sum()))


def average(w, values):
    """sum_f w_f values[f] for values [F.., ...] (leading dimensions of product F, any trailing shape)"""
    v = np.asarray(values, np.float64)
    w = np.asarray(w, np.float64).reshape(-1)
    return (w @ v.reshape(w.size, -1)).reshape(v.shape[_lead(v, w.size):])


def _lead(v, F):
    """number of leading dimensions of v whose product is F"""
    n, k = 1, 0
    while n < F:
        n *= v.shape[k]
        k += 1
    assert n == F, (v.shape, F)
    return k


def gradient(w, values, dU_dtheta, kT):
    """d<O>/dtheta [..., K] for values [F, ...] and dU_dtheta [F, K] at the weights w (the covariance identity)."""
    w = np.asarray(w, np.float64).reshape(-1)
    O = np.asarray(values, np.float64).reshape(w.size, -1)
    G = np.asarray(dU_dtheta, np.float64).reshape(w.size, -1)
    mO, mG = w @ O, w @ G
    cov = (w[:, None, None] * O[:, :, None] * G[:, None, :]).sum(0) - mO[:, None] * mG[None, :]
    return (-cov / float(kT)).reshape(np.asarray(values).shape[_lead(np.asarray(values), w.size):] + (G.shape[1],))
