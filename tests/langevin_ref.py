"""Float64 numpy reference of the Langevin (BAOAB) integrator, independent of the package: Philox4x32-10 and the mapping of
its words to normals, the BAOAB loop and its hand-written reverse sweep for a model given as callables, and a restatement of
both with every operation rounded to float32 -- the floor the GPU tests measure their tolerances from.

A model is a triple of callables on float64 arrays:  F(q) -> [N, 3],  Hw(q, w) -> H(q) w = d(w.F)/dq  [N, 3],
Pw(q, w) -> d(w.F)/dtheta  [P]  (P may be 0)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Random123's Philox4x32-10.  counter: four, key: two arrays (or ints) of 32-bit words; returns four uint64 arrays
    holding the 32-bit output words."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
    return c


def words(seed, step, n):
    """The four output words of atoms 0..n-1 at (seed, step): key = seed's words, counter = (atom, step lo, step hi, 0)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10((np.arange(n), step & 0xFFFFFFFF, step >> 32, 0), (seed & 0xFFFFFFFF, seed >> 32))


def normals(seed, step, n, dtype=np.float64):
    """xi [n, 3]: u_j = ((x_j >> 9) + 1/2) 2^-23, r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2),
    xi = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3).  dtype float32: every operation rounded to float32."""
    f = dtype
    u = [((x >> np.uint64(9)).astype(f) + f(0.5)) * f(2.0 ** -23) for x in words(seed, step, n)]
    r0, r1 = np.sqrt(f(-2.0) * np.log(u[0])), np.sqrt(f(-2.0) * np.log(u[2]))
    two_pi = f(2.0 * np.pi)
    return np.stack((r0 * np.cos(two_pi * u[1]), r0 * np.sin(two_pi * u[1]), r1 * np.cos(two_pi * u[3])), 1).astype(f)


def coefficients(gamma, h, dtype=np.float64):
    f = dtype
    return np.exp(-f(gamma) * f(h)).astype(f), np.sqrt(-np.expm1(f(-2.0) * f(gamma) * f(h))).astype(f)


def forward(F, v0, q0, t, mass, T, gamma, seed, step0=0, dtype=np.float64, xi=None):
    """Frames (v_t, q_t) [len(t), N, 3] of BAOAB.  `xi` (optional): the noise per step, [len(t) - 1, N, 3]."""
    f = dtype
    v, q = np.asarray(v0, f), np.asarray(q0, f)
    m = np.asarray(mass, f)[:, None]
    t = np.asarray(t, f)
    vs, qs = [v], [q]
    Fq = np.asarray(F(q), f)
    for k in range(len(t) - 1):
        h = f(t[k + 1] - t[k])
        hh = f(0.5) * h
        c1, c2 = coefficients(gamma, h, f)
        x = normals(seed, step0 + k, v.shape[0], f) if xi is None else np.asarray(xi[k], f)
        v = v + hh * Fq / m
        q = q + hh * v
        v = c1 * v + c2 * np.sqrt(f(T) / m) * x
        q = q + hh * v
        Fq = np.asarray(F(q), f)
        v = v + hh * Fq / m
        vs.append(v), qs.append(q)
    return np.stack(vs).astype(f), np.stack(qs).astype(f)


def adjoint(F, Hw, Pw, v_t, q_t, g_v, g_q, t, mass, T, gamma, seed, step0=0, dtype=np.float64, xi=None):
    """Reverse sweep over the saved frames: (dL/dv0, dL/dq0, dL/dtheta, dL/dgamma, A_gamma) for L with frame cotangents g_v,
    g_q.  Written operation by operation (two B+ per interval, unmerged) -- the package merges the two that meet at a frame.
    A_gamma is the sum of the absolute values of the (atom, component, step) terms that dL/dgamma adds up: the scale its
    float32 error is measured on (the terms cancel; a sum is judged by what was added up, as in pair_forms_ref)."""
    f = dtype
    m = np.asarray(mass, f)[:, None]
    t = np.asarray(t, f)
    n = len(t)
    lv, lq = np.asarray(g_v[-1], f).copy(), np.asarray(g_q[-1], f).copy()
    th, gb, ga = None, f(0.0), 0.0

    def B_adj(q, lv, lq, hh, th):
        w = hh * lv / m
        p = np.asarray(Pw(q, w), f)
        return lq + np.asarray(Hw(q, w), f), (p if th is None else th + p)

    for i in range(n - 1, 0, -1):
        h = f(t[i] - t[i - 1])
        hh = f(0.5) * h
        c1, c2 = coefficients(gamma, h, f)
        x = normals(seed, step0 + i - 1, m.shape[0], f) if xi is None else np.asarray(xi[i - 1], f)
        qi, vi = np.asarray(q_t[i], f), np.asarray(v_t[i], f)
        lq, th = B_adj(qi, lv, lq, hh, th)                       # closing B of the step
        v2 = vi - hh * np.asarray(F(qi), f) / m                  # the velocity after O
        lv = lv + hh * lq                                        # A
        if c2 != 0:
            terms = lv * (h * (np.sqrt(f(T) / m) * x / c2 - v2))     # O: d v2 / d gamma
            gb = gb + np.sum(terms, dtype=f)
            ga = ga + float(np.abs(terms.astype(np.float64)).sum())
        lv = c1 * lv
        lv = lv + hh * lq                                        # A
        lq, th = B_adj(np.asarray(q_t[i - 1], f), lv, lq, hh, th)   # opening B of the step
        lv = lv + np.asarray(g_v[i - 1], f)
        lq = lq + np.asarray(g_q[i - 1], f)
    return lv, lq, (np.zeros(0, f) if th is None else th), gb, ga


# ---- a toy model with closed-form derivatives:  U = sum_a 1/2 k0 |q_a|^2 + 1/4 k1 |q_a|^4 + 1/2 k2 sum_a |q_a - q_{a+1}|^2 (ring)
def toy_model(theta):
    k0, k1, k2 = (float(x) for x in theta)

    def F(q):
        r2 = (q * q).sum(1, keepdims=True)
        return -k0 * q - k1 * r2 * q - k2 * (2 * q - np.roll(q, 1, 0) - np.roll(q, -1, 0))

    def Hw(q, w):
        r2 = (q * q).sum(1, keepdims=True)
        qw = (q * w).sum(1, keepdims=True)
        return -k0 * w - k1 * (r2 * w + 2 * qw * q) - k2 * (2 * w - np.roll(w, 1, 0) - np.roll(w, -1, 0))

    def Pw(q, w):
        r2 = (q * q).sum(1, keepdims=True)
        return np.array([-(w * q).sum(), -(w * r2 * q).sum(), -(w * (2 * q - np.roll(q, 1, 0) - np.roll(q, -1, 0))).sum()])

    return F, Hw, Pw
