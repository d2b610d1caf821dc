"""Reference of the soft-histogram RDF (csrc/rdf.hip, csrc/rdf_cell.hip) in numpy, CPU only, from exactly what a kernel
receives: float32 frames [F, N, 3], the cell (three lengths or a 3x3 matrix, float32 values), the float32 centres mu as given
(the float32 linspace values are the definition), coeff, the cutoff, an optional pair mask or index_tuple, and upstream
gradients g_raw.

    raw[k] = sum_frames sum_{i<j, 0<d<cutoff} exp(coeff (d - mu_k)^2)
    g_xyz  = d(sum_k g_raw[k] raw[k]) / d xyz,   D = x_j - x_i,
    minimum image of topology.py:59-64 (csrc/common.hpp): s = D . inv, shift by -1 where s > 0.5 and by +1 where s < -0.5.

`dtype` selects float64 or float32 for every operation on those inputs (the float32 evaluation is the rounding floor of the
formula itself).  `model` restates, in that dtype, the documented approximation of a kernel variant:

    None               the exact sum (terms below 1e-46 of a peak term are skipped)
    ("reach", R)       only the 2R+1 bins around the nearest centre kc = rint((d - mu0) / dmu), -R <= kc <= nbins-1+R
                       (rdf_fwd_lane_kernel, rdf_fwd_half_kernel, rdf_bwd_kernel<., R>)
    ("hermite", R, sub)   backward only: dL/dd from the cubic Hermite interpolant of (S, h S') on `sub` nodes per centre
                       spacing (the library's: mdg_rdf_fine_grid) from mu0 - (R+1) dmu, each node summed over the 2R+3
                       centres around it (fine_grid, rdf_node_sum, rdf_bwd_table_kernel, rdf_bwd_fine_kernel)
    ("fine", h, reach, bins)   forward only: every pair is moved to the centre of its bin of the grid of `bins` bins of
                       width h from mu0 - reach, a centre sums the bins within `reach` of it (rdf_fwd_fine_kernel,
                       rdf_fwd_ell_kernel, the cell sweep, rdf_fine_finish_kernel); `bins` None: mdg_rdf_fine_plan's count
    ("utable", nodes)  backward only: phi'(r) / r from the cubic Hermite table over u = r^2 that ops._rdf_pair_table builds
                       for the cell sweep and the list route (pair_eval, MDG_PAIR_TABLE)
    {"fwd": m, "bwd": m}   one model per direction.

Pinned by tests/test_rdf_ref_host.py; used by tests/test_gpu_rdf_ref.py."""
import collections
import math

import numpy as np

TINY = 1e-46                     # terms below this fraction of a peak term are skipped by the exact sum: under half the
#                                  smallest float32 denormal, so what the reference skips is an exact zero in float32 too
HALF_EPS, CUT_EPS = 1e-6, 1e-5   # a pair is fragile within these of a half cell (fractional) / of the cutoff
Result = collections.namedtuple("Result", "raw g_xyz A fragile")


def pair_mask(n_atoms, mask=None, index_tuple=None):
    """bool [N, N] of the selected pairs (symmetric) or None: `mask` as given, or a-b pairs of index_tuple = (a, b)."""
    if mask is not None:
        return np.asarray(mask).astype(bool)
    if index_tuple is None:
        return None
    sel = np.zeros((n_atoms, n_atoms), bool)
    sel[np.asarray(index_tuple[0])[:, None], np.asarray(index_tuple[1])[None, :]] = True
    return sel | sel.T


def _cell(cell, dt):
    h = np.asarray(cell, np.float32).astype(dt)
    if h.ndim == 1:
        h = np.diag(h)
    return h, np.linalg.inv(h).astype(dt), bool((h == np.diag(np.diag(h))).all())


def _pairs(n_atoms, sel):
    iu, ju = np.triu_indices(n_atoms, 1)
    if sel is not None:
        keep = sel[iu, ju]
        iu, ju = iu[keep], ju[keep]
    return iu, ju


def _images(x, h, inv, diag, iu, ju):
    """D = x_j - x_i with the minimum image of topology.py:59-64, the fractional coordinates s and the shifts o."""
    D = x[:, ju] - x[:, iu]
    s = D * np.diag(inv) if diag else D @ inv
    o = (s < -0.5).astype(x.dtype) - (s > 0.5).astype(x.dtype)
    return (D + o * np.diag(h) if diag else D + o @ h), s, o


def _frame_chunks(F, per_frame, budget=1 << 21):
    step = max(1, budget // max(per_frame, 1))
    return [(a, min(F, a + step)) for a in range(0, F, step)]


def fragile_pairs(frames, cell, mu, coeff, cutoff, mask=None, index_tuple=None):
    """Rows (frame, i, j) of the pairs about which float32 and float64 may disagree while one of the two candidate distances
    lies within reach of the centres (a term of at least 1e-46 of a peak term) and inside the cutoff: a fractional
    coordinate within 1e-6 of +-0.5, or a distance within 1e-5 of the cutoff.  float64 throughout."""
    x = np.asarray(frames, np.float32).astype(np.float64)
    x = x.reshape(-1, x.shape[-2], 3)
    h, inv, diag = _cell(cell, np.float64)
    mu = np.asarray(mu, np.float32).astype(np.float64)
    xr = math.sqrt(math.log(TINY) / float(np.float32(coeff)))
    cut = float(np.float32(cutoff))
    iu, ju = _pairs(x.shape[1], pair_mask(x.shape[1], mask, index_tuple))

    def in_reach(d):
        return (d > mu[0] - xr) & (d < mu[-1] + xr) & (d < cut + CUT_EPS) & (d > 0)

    rows = []
    for a, b in _frame_chunks(x.shape[0], iu.size):
        D, s, o = _images(x[a:b], h, inv, diag, iu, ju)
        d = np.sqrt((D * D).sum(-1))
        hit = (np.abs(d - cut) < CUT_EPS) & in_reach(d)
        for c in range(3):
            f, p = np.nonzero(np.abs(np.abs(s[..., c]) - 0.5) < HALF_EPS)
            if f.size:
                sgn = np.sign(s[f, p, c])
                alt = D[f, p] - (sgn * (1.0 + 2.0 * o[f, p, c] * sgn))[:, None] * h[c][None, :]     # the other decision
                hit[f, p] |= in_reach(d[f, p]) | in_reach(np.sqrt((alt * alt).sum(-1)))
        f, p = np.nonzero(hit)
        rows.append(np.stack([f + a, iu[p], ju[p]], 1))
    return np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)


def fine_bins(nbins, dmu, h, reach):
    """mdg_rdf_fine_plan: ceil(((nbins - 1) spacing + 2 reach) / h) + 1."""
    return int(math.ceil(((nbins - 1) * float(dmu) + 2.0 * float(reach)) / float(h))) + 1


def _direction(model, which):
    if isinstance(model, dict):
        return model.get(which)
    if model is None or model[0] == "reach":
        return model
    return model if {"hermite": "bwd", "utable": "bwd", "fine": "fwd"}[model[0]] == which else None


def _slices(m, ds, mu, coeff, dt):
    """Per bin k the slice of the sorted distances that contributes to it."""
    B = mu.size
    if m is None:
        xr = dt(math.sqrt(math.log(TINY) / float(coeff)))
        return np.searchsorted(ds, mu - xr, "right"), np.searchsorted(ds, mu + xr, "left")
    R = int(m[1])
    dmu = (mu[-1] - mu[0]) / dt(B - 1)
    kc = np.rint((ds - mu[0]) * (dt(1) / dmu)).astype(np.int64)            # monotone in d: sorted
    k = np.arange(B)
    return np.searchsorted(kc, k - R, "left"), np.searchsorted(kc, k + R, "right")


def _hermite_eval(nodes_v, nodes_s, t, last_cell):
    """Cubic Hermite interpolant of the node values and (cell width x slope) at the grid coordinate t."""
    g = np.minimum(np.floor(t).astype(np.int64), last_cell)
    f = t - g.astype(t.dtype)
    a0, a1, b0, b1 = nodes_v[..., g], nodes_s[..., g], nodes_v[..., g + 1], nodes_s[..., g + 1]
    c2 = 3 * (b0 - a0) - 2 * a1 - b1
    c3 = 2 * (a0 - b0) + a1 + b1
    return a0 + f * (a1 + f * (c2 + f * c3))


def _dldd_hermite(R, sub, d, mu, coeff, g, dt):
    B = mu.size
    dmu = (mu[-1] - mu[0]) / dt(B - 1)
    xlo, hf = mu[0] - dt(R + 1) * dmu, dmu / dt(sub)
    nn = (B - 1 + 2 * (R + 1)) * sub + 1
    r = np.arange(nn).astype(dt) * hf + xlo
    ks = np.rint((r - mu[0]) / dmu).astype(np.int64)[:, None] + np.arange(-R - 1, R + 2)[None, :]
    ok = (ks >= 0) & (ks < B)
    ks = np.clip(ks, 0, B - 1)
    x = r[:, None] - mu[ks]
    e = np.where(ok, np.exp(coeff * x * x), dt(0))
    two = dt(2) * coeff
    S = (g[:, ks] * (two * x * e)[None]).sum(-1, dtype=dt)                                # [G, nn]
    dS = (g[:, ks] * (two * (dt(1) + two * x * x) * e)[None]).sum(-1, dtype=dt) * hf
    t = (d - xlo) * (dt(sub) / dmu)
    ok = (t >= 0) & (t < nn - 1)
    return np.where(ok, _hermite_eval(S, dS, np.where(ok, t, dt(0)), nn - 2), dt(0))


def _dldd_utable(nodes, d, mu, coeff, cutoff, g, dt):
    lo = max(float(mu[0]) - 6.0 / math.sqrt(-2.0 * float(coeff)), 0.05)
    u0, u1 = dt(lo * lo), dt(float(cutoff) ** 2)
    du = (u1 - u0) / dt(nodes - 1)
    r = np.sqrt(u0 + du * np.arange(nodes).astype(dt))
    x = r[:, None] - mu[None, :]
    e = np.exp(coeff * x * x)
    two = dt(2) * coeff
    p1 = ((two * x * e)[None] * g[:, None, :]).sum(-1, dtype=dt)                          # phi'   [G, nodes]
    p2 = (((two + (two * x) ** 2) * e)[None] * g[:, None, :]).sum(-1, dtype=dt)           # phi''
    c1 = p1 / r
    dc1 = (p2 / r - p1 / (r * r)) / (dt(2) * r) * du
    t = np.clip((d * d - u0) / du, dt(0), dt(nodes - 1))
    return _hermite_eval(c1, dc1, t, nodes - 2) * d


def _raw_fine(m, d, mu, coeff, dt):
    h, reach = dt(np.float32(m[1])), dt(np.float32(m[2]))
    B = mu.size
    nfine = m[3] if len(m) > 3 and m[3] else fine_bins(B, (mu[-1] - mu[0]) / dt(B - 1), h, reach)
    lo = mu[0] - reach
    inv_h = dt(1) / h
    t = d * inv_h + (-lo * inv_h)
    t = t[(t >= 0) & (t < nfine)]
    H = np.bincount(np.floor(t).astype(np.int64), minlength=nfine).astype(dt)
    xm = lo + (np.arange(nfine).astype(dt) + dt(0.5)) * h
    raw = np.zeros(B, dt)
    for k in range(B):
        m0 = max(0, int(np.floor((mu[k] - reach - lo) / h)))
        m1 = min(nfine, int(np.ceil((mu[k] + reach - lo) / h)))
        x = xm[m0:m1] - mu[k]
        raw[k] = (H[m0:m1] * np.exp(coeff * x * x)).sum(dtype=dt)
    return raw


def _to_atoms(vals, fi, pi, F, iu, ju, N, sign, dt):
    """sum over the pairs of an atom: + vals at atom j, sign * vals at atom i.  vals [M, C] of the pairs (fi, pi)."""
    C = vals.shape[1]
    out = np.zeros((F, N, C), dt)
    for a, b in _frame_chunks(F, N * N * C):
        lo, hi = np.searchsorted(fi, a, "left"), np.searchsorted(fi, b, "left")
        W = np.zeros((b - a, N, N, C), dt)
        W[fi[lo:hi] - a, iu[pi[lo:hi]], ju[pi[lo:hi]]] = vals[lo:hi]
        out[a:b] = W.sum(1, dtype=dt) + dt(sign) * W.sum(2, dtype=dt)
    return out


def rdf_reference(frames, cell, mu, coeff, cutoff, g_raw=None, mask=None, index_tuple=None, dtype=np.float64, model=None):
    """Result(raw [B], g_xyz, A, fragile).  g_raw [B] or [G, B] -> g_xyz [F, N, 3] or [G, F, N, 3], likewise the per-(frame,
    atom) scale A = sum over the pairs of the atom of |dL/dd| ([F, N] or [G, F, N]); None without g_raw.  fragile: the rows
    of fragile_pairs for the exact float64 evaluation, None otherwise."""
    dt = np.dtype(dtype).type
    x = np.asarray(frames)
    assert x.dtype == np.float32, "the frames are the float32 values a kernel receives"
    x = x.reshape(-1, x.shape[-2], 3).astype(dt)
    F, N = x.shape[:2]
    h, inv, diag = _cell(cell, dt)
    mu = np.asarray(mu, np.float32).astype(dt)
    B = mu.size
    coeff = dt(np.float32(coeff))
    cut = dt(np.float32(cutoff))
    iu, ju = _pairs(N, pair_mask(N, mask, index_tuple))
    fi, pi, dist, vec = [], [], [], []
    for a, b in _frame_chunks(F, iu.size):
        D = _images(x[a:b], h, inv, diag, iu, ju)[0]
        d2 = (D * D).sum(-1, dtype=dt)
        f, p = np.nonzero((d2 < cut * cut) & (d2 != 0))
        fi.append(f + a), pi.append(p), dist.append(np.sqrt(d2[f, p])), vec.append(D[f, p])
    fi, pi, d, vec = (np.concatenate(v) for v in (fi, pi, dist, vec))
    order = np.argsort(d, kind="stable")
    ds = d[order]
    mf, mb = _direction(model, "fwd"), _direction(model, "bwd")
    assert mf is None or mf[0] in ("reach", "fine"), mf
    assert mb is None or mb[0] in ("reach", "hermite", "utable"), mb
    g = None if g_raw is None else np.atleast_2d(np.asarray(g_raw, np.float32)).astype(dt)
    sums_b = g is not None and (mb is None or mb[0] == "reach")
    raw = _raw_fine(mf, ds, mu, coeff, dt) if mf is not None and mf[0] == "fine" else None
    dl = np.zeros((g.shape[0], ds.size), dt) if g is not None else None
    passes = []
    if raw is None:
        passes.append((mf, True, sums_b and mb == mf))
    if sums_b and not (raw is None and mb == mf):
        passes.append((mb, False, True))
    if raw is None:
        raw = np.zeros(B, dt)
    for m, fwd, bwd in passes:
        lo, hi = _slices(m, ds, mu, coeff, dt)
        for k in range(B):
            if hi[k] <= lo[k]:
                continue
            xx = ds[lo[k]:hi[k]] - mu[k]
            e = np.exp(coeff * xx * xx)
            if fwd:
                raw[k] = e.sum(dtype=dt)
            if bwd:
                dl[:, lo[k]:hi[k]] += g[:, k, None] * (dt(2) * coeff * xx * e)[None, :]
    if g is not None and mb is not None and mb[0] == "hermite":
        dl = _dldd_hermite(int(mb[1]), int(mb[2]), ds, mu, coeff, g, dt)
    if g is not None and mb is not None and mb[0] == "utable":
        dl = _dldd_utable(int(mb[1]), ds, mu, coeff, cut, g, dt)
    g_xyz = A = None
    if g is not None:
        un = np.empty_like(dl)
        un[:, order] = dl
        g_xyz = np.stack([_to_atoms((row / d)[:, None] * vec, fi, pi, F, iu, ju, N, -1, dt) for row in un])
        A = np.stack([_to_atoms(np.abs(row)[:, None], fi, pi, F, iu, ju, N, 1, dt)[..., 0] for row in un])
        if np.ndim(g_raw) == 1:
            g_xyz, A = g_xyz[0], A[0]
    fragile = None
    if dt is np.float64 and model is None:
        fragile = fragile_pairs(frames, cell, mu, coeff, cutoff, mask, index_tuple)
    return Result(raw, g_xyz, A, fragile)


# ----------------------------------------------------------------------------------------------- error measure
ULP = 2.0 ** -24


def forward_error(raw, ref):
    """max_k |raw_k - ref_k| / max_k ref, ref the exact float64 Result."""
    return float(np.abs(np.asarray(raw, np.float64) - ref.raw).max() / ref.raw.max())


def scale_floor(g_row, coeff):
    """One float32 unit roundoff of a single unit contribution: 2^-24 max|g_k| x the largest |d/dd exp(coeff x^2)| =
    sqrt(2 |coeff|) exp(-1/2).  The per-atom scale A is not taken below it: with a one-hot upstream gradient most atoms see
    only the far tails of that one Gaussian, A down to 1e-40 of a unit contribution, where every variant's documented
    truncation (2^-21.6 .. 2^-28 of a peak term) and the float32 / float64 ties of its nearest-centre rint are of order A
    itself and the measure would report 0.9 for the model, the floor and the kernel alike."""
    return ULP * float(np.abs(g_row).max()) * math.sqrt(2.0 * abs(coeff)) * math.exp(-0.5)


def backward_error(g, ref, form, a_min, want=None):
    """max over frames, atoms and components of |g - want| / (A + a_min), A the atom's scale in the exact float64 Result
    `ref` for upstream gradient number `form`, a_min = scale_floor(...), want = ref's gradient unless given; an atom with
    A = 0 must hold exact zeros and everything must be finite (inf otherwise)."""
    want, A = (ref.g_xyz[form] if want is None else want), ref.A[form]
    got = np.asarray(g, np.float64).reshape(want.shape)
    if (got[A == 0] != 0).any() or not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - want) / (A + a_min)[..., None]).max())


# ----------------------------------------------------------------------------------------------- inputs
def draw_frames(base, box, n_frames, seed, check, sigma=0.05, post=None):
    """n_frames float32 frames np.mod(base + normal(0, sigma), box) from default_rng(seed), as the sibling tests draw them
    (`post`: applied to every frame afterwards, e.g. a translation); a frame for which check(frames) names a fragile pair is
    redrawn with the next random numbers until it has none.  Returns (frames, number of frames that were redrawn)."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, np.float32)
    post = post or (lambda fr: fr)

    def one():
        return post(np.mod(base + rng.normal(0, sigma, base.shape), box).astype(np.float32))

    frames = np.stack([one() for _ in range(n_frames)])
    todo = np.unique(check(frames)[:, 0])
    redrawn = set(todo.tolist())
    while todo.size:
        for f in todo:
            frames[f] = one()
        todo = todo[np.unique(check(frames[todo])[:, 0])]
    return frames, len(redrawn)


# ----------------------------------------------------------------------------------------------- the cases of the GPU tests
TRI_CELL = [[4.8, 0, 0], [0.7, 4.8, 0], [-0.5, 0.4, 4.8]]
FORMS = ("linspace", "first", "last")          # upstream gradients: linspace(-1, 1), one-hot on the first / last bin


class Case:
    """One input of tests/test_gpu_rdf_ref.py: what the kernel receives, what it must run, and the model of that variant.
    expect = (route, forward variant, backward variant, forward (R, waves, 128-column rows) or None, backward R or None)."""

    def __init__(self, name, n_frames, n_atoms, width, expect, nbins=100, r_range=(0.75, 2.5), tri=False, masked=False,
                 uniform=True, jitter_mu=False, one_hot=False, post=None, liquid=None):
        self.name, self.n_frames, self.n_atoms, self.width, self.expect = name, n_frames, n_atoms, width, expect
        self.nbins, self.r_range, self.tri, self.masked, self.uniform = nbins, r_range, tri, masked, uniform
        self.jitter_mu, self.post, self.liquid = jitter_mu, post, liquid
        self.forms = FORMS if one_hot else FORMS[:1]
        self._refs = {}

    # ---- what the kernel receives
    def centres(self):
        import torch
        mu = torch.linspace(self.r_range[0], self.r_range[1], self.nbins).numpy().copy()
        if self.jitter_mu:                      # not a linspace: every centre moved by up to a quarter spacing
            mu[1:-1] += (np.random.default_rng(5).uniform(-0.25, 0.25, self.nbins - 2) * (mu[1] - mu[0])).astype(np.float32)
        return mu

    def spacing(self):
        mu = self.centres()
        return float(mu[1] - mu[0]) if self.uniform else 0.0

    def coeff(self):
        import torch
        lin = torch.linspace(self.r_range[0], self.r_range[1], self.nbins)
        return float(-0.5 / (self.width * float(lin[1] - lin[0])) ** 2)

    def mu_last(self):
        return float(self.r_range[1]) if self.liquid else None

    def box(self):
        if self.liquid:
            return _liquid(*self.liquid)[1]
        return np.full(3, 4.8, np.float32)

    def cell(self):
        return np.array(TRI_CELL, np.float32) if self.tri else self.box()

    def cutoff(self):
        """The cutoff RdfRawFn hands to its kernels (the list routes trim it: ops._rdf_list_cutoff)."""
        if self.liquid:
            return min(self.r_range[1] + 0.5, self.r_range[1] + 1.02 * 5.3 / math.sqrt(-self.coeff() * 1.4426950408889634) + 1e-6)
        return 2.3 if self.tri else 3.0

    def index_tuple(self):
        n = self.n_atoms
        return (list(range(0, (5 * n) // 12)), list(range((5 * n) // 12, n))) if self.masked else None

    def upstream(self):
        g = np.zeros((len(self.forms), self.nbins), np.float32)
        g[0] = np.linspace(-1, 1, self.nbins, dtype=np.float32)
        if len(self.forms) > 1:
            g[1, 0] = g[2, -1] = 1.0
        return g

    def check(self, frames):
        return fragile_pairs(frames, self.cell(), self.centres(), self.coeff(), self.cutoff(), index_tuple=self.index_tuple())

    def frames(self):
        """(float32 frames, frames redrawn for a fragile pair); built once."""
        if "frames" not in self._refs:
            if self.liquid:
                # liquid(n_side, seed) of tests/test_gpu_parity.py is frame 0; further frames and redraws continue its generator
                frames, rng, drawn = [], np.random.default_rng(self.liquid[1]), 0
                while len(frames) < self.n_frames:
                    fr = _liquid(self.liquid[0], rng)[0]
                    drawn += 1
                    if not len(self.check(fr[None])):
                        frames.append(fr)
                self._refs["frames"] = (np.stack(frames), drawn - self.n_frames)
            else:
                from conftest import load_golden
                base = load_golden("rdf")["xyz"][0][:self.n_atoms]
                self._refs["frames"] = draw_frames(base, self.box(), self.n_frames, 13, self.check, post=self.post)
        return self._refs["frames"]

    # ---- the references (cached for the session)
    def reference(self, dtype=np.float64, model=None):
        key = (np.dtype(dtype).name, repr(model))
        if key not in self._refs:
            self._refs[key] = rdf_reference(self.frames()[0], self.cell(), self.centres(), self.coeff(), self.cutoff(),
                                            self.upstream(), index_tuple=self.index_tuple(), dtype=dtype, model=model)
        return self._refs[key]

    def a_min(self, k):
        return scale_floor(self.upstream()[k], self.coeff())

    def allowances(self, model):
        """{quantity: (floor, model_gap)} for "raw" and every form of self.forms, in the error measure above: floor =
        distance of the float32 model from the float64 model (at least 2^-24), model_gap = distance of the float64 model
        from the exact float64 sum."""
        ref, m64, m32 = self.reference(), self.reference(model=model), self.reference(np.float32, model)
        out = {"raw": (max(float(np.abs(m32.raw.astype(np.float64) - m64.raw).max() / ref.raw.max()), ULP), forward_error(m64.raw, ref))}
        for k, form in enumerate(self.forms):
            scale = (ref.A[k] + self.a_min(k))[..., None]
            out[form] = (max(float((np.abs(m32.g_xyz[k].astype(np.float64) - m64.g_xyz[k]) / scale).max()), ULP),
                         float((np.abs(m64.g_xyz[k] - ref.g_xyz[k]) / scale).max()))
        return out


def _liquid(n_side, seed, rho=0.845, jitter=0.08):
    """tests/test_gpu_parity.py: liquid(); `seed` may be a generator to continue."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    L = (n_side ** 3 / rho) ** (1 / 3)
    a = L / n_side
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3) * a
    pos = np.mod(g + rng.uniform(-jitter, jitter, g.shape) * a, L).astype(np.float32)
    return pos, np.array([L, L, L], dtype=np.float32)


def _translated(fr):
    return fr + np.float32(0.3) * np.full(3, 4.8, np.float32)


def _unwrapped(fr):
    fr = fr.copy()
    for a in range(fr.shape[0] // 4):           # a quarter of the atoms, one cell further along x, y or z in turn
        fr[a, a % 3] += np.float32(4.8)
    return fr


def _coincident(fr):
    fr = fr.copy()
    fr[17] = fr[3]
    return fr


HALF, TAB6 = (5, 8, 1), 6
CASES = [
    Case("3 frames, arbitrary centres", 3, 48, 1.0, ("frames", "direct", "atom", None, 0), uniform=False),
    Case("8 frames", 8, 48, 1.0, ("frames", "block8", "atom", None, 0)),
    Case("8 frames, centres not a linspace", 8, 48, 1.0, ("frames", "direct", "atom", None, 0), uniform=False, jitter_mu=True),
    Case("half/table R=6", 1024, 48, 1.0, ("frames", "half", "table", HALF, 6), one_hot=True),
    Case("half/table R=6 triclinic", 1024, 48, 1.0, ("frames", "half", "table", (5, 8, 0), 6), tri=True, one_hot=True),
    Case("half/table R=6 masked", 1024, 48, 1.0, ("frames", "half", "table", (5, 8, 0), 6), masked=True, one_hot=True),
    Case("lane/table R=11", 1024, 48, 1.6, ("frames", "lane", "table", (11, 4, 1), 11), one_hot=True),
    Case("lane/table R=11 triclinic", 1024, 48, 1.6, ("frames", "lane", "table", (11, 4, 0), 11), tri=True, one_hot=True),
    Case("lane/frame R=6 width 0.4", 1024, 48, 0.4, ("frames", "lane", "frame", (5, 4, 1), 6), one_hot=True),
    Case("lane/frame R=11 500 centres", 1024, 48, 1.6, ("frames", "lane", "frame", (11, 1, 1), 11), nbins=500, one_hot=True),
    Case("direct/frame R=0", 1024, 48, 1.0, ("frames", "direct", "frame", None, 0), uniform=False),
    Case("fine/table 64 atoms", 1024, 64, 1.0, ("frames", "fine", "table", (0, 16, 0), 6), one_hot=True),
    Case("fine/table 65 atoms", 1024, 65, 1.0, ("frames", "fine", "table", (0, 16, 0), 6), one_hot=True),
    Case("fine/table 65 atoms masked", 1024, 65, 1.0, ("frames", "fine", "table", (0, 16, 0), 6), masked=True, one_hot=True),
    Case("tail workgroup, 1025 frames", 1025, 48, 1.0, ("frames", "half", "table", HALF, 6)),
    Case("low and high edge", 1024, 48, 1.0, ("frames", "half", "table", HALF, 6), nbins=60, r_range=(1.2, 2.2), one_hot=True),
    Case("tiny, 2 atoms", 1024, 2, 1.0, ("frames", "half", "table", HALF, 6)),
    Case("tiny, 7 atoms", 1024, 7, 1.0, ("frames", "half", "table", HALF, 6)),
    Case("translated by 0.3 cell", 1024, 48, 1.0, ("frames", "half", "table", HALF, 6), post=_translated),
    Case("a quarter of the atoms unwrapped", 1024, 48, 1.0, ("frames", "half", "table", HALF, 6), post=_unwrapped),
    Case("coincident atoms", 8, 48, 1.0, ("frames", "block8", "atom", None, 0), post=_coincident),
    Case("cell sweep", 2, 512, 1.0, ("cell", None, None, None, None), liquid=(8, 61)),
    Case("list", 2, 512, 1.0, ("list", None, None, None, None), liquid=(8, 61)),
]
BY_NAME = {c.name: c for c in CASES}


def plan_of(case, list_atoms=256, cell_direct=None):
    """(route, forward plan, backward plan, model) of a case from the library's own queries (ops.rdf_route, ops.rdf_plan: no
    GPU needed): the model restates what the planned variants approximate, with R, h and reach as the plan reports them.
    The two liquid cases lower ops.RDF_LIST_ATOMS to `list_atoms` for the query (restored) as their GPU test does."""
    from mdgrad_amd import _lib, ops
    cs = _lib.make_cell(case.cell())
    mask = None if case.index_tuple() is None else pair_mask(case.n_atoms, index_tuple=case.index_tuple())
    shape = (case.n_frames, case.n_atoms, case.nbins, case.spacing(), case.coeff())
    saved = ops.RDF_LIST_ATOMS, ops.RDF_CELL_DIRECT
    try:
        if case.liquid:
            ops.RDF_LIST_ATOMS = list_atoms
            ops.RDF_CELL_DIRECT = case.expect[0] == "cell" if cell_direct is None else cell_direct
        route = ops.rdf_route(*shape, case.cutoff(), cs, mask)
    finally:
        ops.RDF_LIST_ATOMS, ops.RDF_CELL_DIRECT = saved
    fwd, bwd = ops.rdf_plan("fwd", *shape, cs, mask), ops.rdf_plan("bwd", *shape, cs, mask)
    fine = ("fine", fwd["fine_h"], fwd["fine_reach"], fwd["fine_bins"])
    if route[0] != "frames":
        return route, fwd, bwd, {"fwd": fine, "bwd": ("utable", 4096)}
    model = {"fwd": fine if route[1] == "fine" else ("reach", fwd["R"]) if route[1] in ("lane", "half") else None,
             "bwd": ("hermite", bwd["R"], bwd["table_sub"]) if route[2] == "table" else ("reach", bwd["R"]) if bwd["R"] else None}
    return route, fwd, bwd, (None if model == {"fwd": None, "bwd": None} else model)
