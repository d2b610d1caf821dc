"""Observables with the reference's interface (torchmd/observable.py): generate_vol_bins
:10-21, Observable :24-31, rdf :33-76, vacf :153-163.  The pair search + Gaussian smearing +
histogram of rdf.forward is one HIP op (ops.RdfRawFn, csrc/rdf.hip), and rdf.per_frame keeps the frames' rows of it
(ops.RdfFramesFn, csrc/rdf_frames.hip; rdf.normalise is forward's tail); vacf is one fused reduction over the
velocity trajectory (ops.VacfFn, csrc/observe.hip).  angle_distribution :120-151 (with Angles :89-118 and
compute_angle :166-179): the triplet search + Gaussian smearing + histogram and its gradient are one HIP op
(ops.AdfRawFn, csrc/adf.hip); the per-triplet angles are torch ops over the device-built angle list.  structure_factor has no
counterpart in the reference: the static structure factor S(k) over the cell's own wave vectors (ops.SkFn, csrc/sk.hip).  Nor
has msd: the mean-squared displacement over all lags and time origins with its fourth moment (ops.MsdFn, csrc/msd.hip), and
diffusion_coefficient, the Einstein slope of it; nor intermediate_scattering: the coherent and self intermediate scattering
functions F(k,t), F_s(k,t) over the wave vectors of structure_factor and the lags of msd (ops.IsfFn, csrc/isf.hip), with
relaxation and relaxation_time; nor bond_order and bond_order_distribution: the Steinhardt order parameters q_l, Q_l over a
smooth neighbour shell and the histogram of q_l (ops.BondOrderFn, csrc/bond_order.hip)."""
import math
import warnings

import numpy as np
import torch

from . import _lib, ops, topology
from .nn.layers import GaussianSmearing
from .system import check_system
from .topology import generate_angle_list, get_offsets


def generate_vol_bins(start, end, nbins, dim):
    """(volume of the ball of radius `end`, volumes of the nbins shells between the equally spaced edges, the edges):
    the ideal-gas normalisation of g(r) (torchmd/observable.py:10-21).  Same constants in the same association as
    the reference, so the float32 results agree to the last bit."""
    if dim not in (2, 3):
        raise ValueError("generate_vol_bins: dim must be 2 or 3")
    edges = torch.linspace(start, end, nbins + 1)
    shell_coef, ball = (4 * np.pi / 3, (4 / 3) * np.pi * end ** 3) if dim == 3 else (np.pi, np.pi * end ** 2)
    shells = shell_coef * (edges[1:] ** dim - edges[:-1] ** dim)
    return ball, torch.Tensor(shells), edges


class Observable(torch.nn.Module):
    def __init__(self, system):
        super().__init__()
        check_system(system)
        self.device = system.device
        self.volume = system.get_volume()
        self.cell = torch.Tensor(system.get_cell()).diag().to(self.device)
        # replica-stacked systems: observables are per replica (frames = time x replica)
        self.n_rep = getattr(system, "n_replicas", 1)
        self.natoms = getattr(system, "group_size", system.get_number_of_atoms())


class rdf(Observable):
    def __init__(self, system, nbins, r_range, index_tuple=None, width=None):
        super().__init__(system)
        start, end = r_range[0], r_range[1]
        V, vol_bins, bins = generate_vol_bins(start, end, nbins, dim=system.dim)
        self.V = V
        self.vol_bins = vol_bins.to(self.device)
        self.r_axis = np.linspace(start, end, nbins)
        self.bins = bins
        # GaussianSmearing(start, stop=bins[-1], n_gaussians=nbins, width)   nff/nn/layers.py:54-61
        offsets = torch.linspace(start, float(bins[-1]), nbins)
        w = (offsets[1] - offsets[0]) if width is None else torch.tensor(float(width))
        self.register_buffer("offsets", offsets.to(self.device))
        self.spacing = float(offsets[1] - offsets[0]) if nbins > 1 else 0.0     # linspace: equally spaced
        self.width = float(w)
        self.coeff = float(-0.5 / torch.pow(w.to(torch.float32), 2))
        self.nbins = nbins
        self.cutoff_boundary = end + 5e-1
        self.index_tuple = index_tuple
        self._cell_struct = _lib.make_cell(self.cell)      # diagonal of the cell, as the reference
        self._mask = ops.build_mask(self.natoms, index_tuple, None, self.device)
        self._warned_fused = False
        self.last_path = None           # "kernel" | "fused-trajectory": which path produced the last forward's histogram

    def _fused_raw(self, xyz):
        """The raw histogram of `xyz` if a fused trajectory launch already produced it (ops.fused_traj); otherwise
        None -- after registering this observable and the frame selection with the integrator, so that the NEXT
        launch produces it.  `xyz` must be the trajectory tensor itself or a slice of it along time that runs to
        the last frame (q_t, q_t[::k], q_t[s:], q_t[s::k])."""
        base = xyz if hasattr(xyz, "_mdg_traj") else getattr(xyz, "_base", None)
        tag = getattr(base, "_mdg_traj", None) if base is not None else None
        if tag is None or self._mask is not None or self.nbins < 2:
            return None
        spec, td, hint, raw = tag
        start, stride = 0, 1
        if xyz is not base:
            if (xyz.dim() != base.dim() or base.stride(td) == 0 or
                    any(xyz.shape[d] != base.shape[d] or xyz.stride(d) != base.stride(d) for d in range(base.dim()) if d != td)):
                return None
            off, bs = xyz.storage_offset() - base.storage_offset(), base.stride(td)
            if off < 0 or off % bs or xyz.stride(td) % bs or xyz.shape[td] < 1:
                return None
            start, stride = off // bs, max(1, xyz.stride(td) // bs)
            if start >= base.shape[td] or xyz.shape[td] != (base.shape[td] - start + stride - 1) // stride:
                return None
        if hint is not None and raw is not None and hint.matches(self, start, stride):
            if not self._warned_fused:
                self._warned_fused = True
                warnings.warn("mdgrad_amd.rdf: the histogram of this trajectory was produced inside the fused trajectory "
                              "launch; its dependence on the frames is routed through the adjoint launch (raw -> FusedTrajFn), "
                              "not through q_t in the autograd graph (autograd.grad(loss, q_t) / hooks on q_t do not see the "
                              "RDF term), and it is the fine-grid histogram (<= 2e-5 per bin from the exact kernel).  "
                              "(opted into with integrator.fuse_observables = True; rdf.last_path tells which path ran).",
                              stacklevel=3)
            return raw
        # OPT-IN (integrator.fuse_observables = True, or integrator.attach_observable): the fused histogram is an output of
        # the trajectory launch, not a function of q_t in the autograd graph -- a reference caller that differentiates
        # w.r.t. q_t or hooks it would lose the RDF term, so nothing is fused unless asked for
        integ = getattr(spec, "_integrator", None)
        if integ is not None and getattr(integ, "fuse_observables", False):
            new = ops.RdfFuse(self, start, stride)
            spec.rdf_hint = new
            integ._rdf_hint = new
        return None

    def forward(self, xyz):
        count = self._fused_raw(xyz)
        self.last_path = "fused-trajectory" if count is not None else "kernel"
        if count is None:
            if self.n_rep > 1 and xyz.shape[-2] == self.n_rep * self.natoms:
                xyz = xyz.reshape(xyz.shape[:-2] + (self.n_rep, self.natoms, 3))
            count = ops.RdfRawFn.apply(xyz, self.offsets, self.coeff, self.cutoff_boundary,
                                       self._cell_struct, self._mask, self.spacing, float(self.r_axis[-1]))
        norm = count.sum()
        count = count / norm
        rdf = count / (self.vol_bins / self.V)
        return count, self.bins, rdf

    # -- the rows of the sum above: what a weighted average over frames needs (reweight.Reweighting) --------------------
    PER_FRAME_MAX_ATOMS = ops.RDF_FRAMES_MAX_ATOMS
    PER_FRAME_MAX_BINS = ops.RDF_FRAMES_MAX_BINS

    def per_frame(self, xyz):
        """raw[..., k] = sum_{i<j, 0<d<cutoff_boundary} exp(coeff (d - mu_k)^2), the smeared pair count of every frame of xyz
        ([N, 3], [T, N, 3], [R, T, N, 3] or replica-stacked [..., k N, 3] giving a trailing k before the bins), with the
        observable's index_tuple selection.  `forward`'s histogram is the sum of these rows; `normalise` turns a row, a sum or
        a weighted average of rows into an RDF.  float32 device positions run one HIP launch (ops.RdfFramesFn,
        csrc/rdf_frames.hip); host or float64 positions take the torch restatement with the exact sum.  Differentiable once
        with respect to xyz.  At most 1024 atoms, a diagonal cell, 2 <= nbins <= 1024."""
        n = xyz.shape[-2] if xyz.dim() >= 2 else 0
        if n == 0 or xyz.shape[-1] != 3 or n % self.natoms:
            raise ValueError("rdf.per_frame: xyz must be [..., k * %d, 3], got %s" % (self.natoms, tuple(xyz.shape)))
        if self.natoms > self.PER_FRAME_MAX_ATOMS:
            raise ValueError("rdf.per_frame: at most %d atoms per frame, got %d" % (self.PER_FRAME_MAX_ATOMS, self.natoms))
        if not 2 <= self.nbins <= self.PER_FRAME_MAX_BINS:
            raise ValueError("rdf.per_frame: nbins must be in [2, %d], got %d" % (self.PER_FRAME_MAX_BINS, self.nbins))
        if not self._cell_struct.diag:
            raise ValueError("rdf.per_frame: the cell must be diagonal")
        k = n // self.natoms
        lead = tuple(xyz.shape[:-2]) + ((k,) if k > 1 else ())
        x = xyz.reshape(-1, self.natoms, 3)
        if x.is_cuda and x.dtype == torch.float32:
            raw = ops.RdfFramesFn.apply(x, self.offsets, self.spacing, self.coeff, self.cutoff_boundary, self._cell_struct,
                                        self._mask)
        else:
            raw = self._torch_per_frame(x)
        return raw.reshape(lead + (self.nbins,))

    def _torch_per_frame(self, x, budget=1 << 16):
        """The same rows by torch ops in x's dtype on x's device: all pairs, every centre (no reach), chunked over frames."""
        F, N = x.shape[0], x.shape[1]
        iu = torch.triu_indices(N, N, offset=1, device=x.device)
        if self._mask is not None:
            iu = iu[:, self._mask.to(x.device).bool()[iu[0], iu[1]]]
        L, mu = self.cell.detach().to(x), self.offsets.detach().to(x)
        out = []
        step = max(1, budget // max(1, iu.shape[1]))
        for a in range(0, F, step):
            xa = x[a:a + step]
            D = xa[:, iu[1]] - xa[:, iu[0]]
            s = D.detach() * (1.0 / L)
            D = D + (-(s > 0.5).to(x) + (s < -0.5).to(x)) * L
            d2 = D.pow(2).sum(-1)
            keep = (d2.detach() < self.cutoff_boundary ** 2) & (d2.detach() != 0)
            fi, pi = torch.nonzero(keep, as_tuple=True)
            e = torch.exp(self.coeff * (d2[fi, pi].sqrt()[:, None] - mu[None, :]).pow(2))
            out.append(x.new_zeros(xa.shape[0], self.nbins).index_add(0, fi, e))
        return torch.cat(out)

    def normalise(self, raw):
        """(count, bins, g) of a smeared pair count raw[..., k] -- a row of `per_frame`, their sum or a weighted average of
        them -- by the tail of `forward`: count = raw / raw.sum(-1), g = count / (vol_bins / V)."""
        count = raw / raw.sum(-1, keepdim=True)
        return count, self.bins, count / (self.vol_bins.to(raw) / self.V)


def compute_angle(xyz, angle_list, cell, N):
    """torchmd/observable.py:166-179: cos of the angle at atom j between x_i - x_j and x_k - x_j for rows (frame, i, j, k),
    each bond vector re-imaged with topology.get_offsets on the diagonal `cell`."""
    frames = xyz.reshape(-1, N, 3)
    f, i, j, k = angle_list.to(frames.device).unbind(1)
    centre = frames[f, j]
    u = frames[f, i] - centre
    v = frames[f, k] - centre
    u = u + get_offsets(u, cell, frames.device) * cell
    v = v + get_offsets(v, cell, frames.device) * cell
    return (u * v).sum(-1) / (u.pow(2).sum(-1) * v.pow(2).sum(-1)).sqrt()


class Angles(Observable):
    """torchmd/observable.py:89-118: forward(xyz) -> cos of every triplet angle, in the reference's list order."""

    def __init__(self, system, nbins, angle_range, cutoff=3.0, index_tuple=None, width=None):
        super().__init__(system)
        start, end = angle_range[0], angle_range[1]
        self.bins = torch.linspace(start, end, nbins + 1).to(self.device)
        self.smear = GaussianSmearing(start=start, stop=self.bins[-1], n_gaussians=nbins, width=width,
                                      trainable=False).to(self.device)
        self.width = self.smear.width[0].item()
        self.cutoff = cutoff
        self.index_tuple = index_tuple
        self.nbins = nbins
        self._cell_struct = _lib.make_cell(self.cell)      # diagonal of the cell, as the reference
        self._mask = ops.build_mask(self.natoms, index_tuple, None, self.device)

    def _angle_cos(self, frames):
        """cos of every triplet angle of `frames` [F, N, 3] in the reference's order (compute_angle over the angle list).  The
        half lists are built in the frame chunks of ops.AdfRawFn, the size of the triplet list is checked before it is
        built, and an allocation failure anywhere on the way is the same ValueError, naming keep_angles=False."""
        F, N = frames.shape[0], self.natoms
        fc = ops._adf_chunk_frames(F, N, self._cell_struct, self.cutoff)
        x = frames.detach()
        try:
            halves, n_cand = [], 0
            for f0 in range(0, F, fc):
                ell = ops.build_ell(x[f0:f0 + fc].reshape(-1, 3), self._cell_struct, self.cutoff, self._mask, group=N)
                c = ell.cnt.to(torch.int64)
                n_cand += int((c * c).sum())          # the candidate rows of generate_angle_list: sum over centres cnt^2
                if 4 * n_cand > topology.ANGLE_LIST_MAX:
                    raise ValueError("%s: more than %d candidate triplets exceed the list limit of %d entries; use "
                                     "angle_distribution(..., keep_angles=False) for the histogram alone"
                                     % (type(self).__name__, n_cand, topology.ANGLE_LIST_MAX))
                nbr = ell.half_list()[0]
                del ell
                f = torch.div(nbr[:, :1], N, rounding_mode="floor")
                halves.append(torch.cat([f + f0, nbr - f * N], 1))
            return compute_angle(frames, generate_angle_list(torch.cat(halves, 0)), self.cell, N=N)
        except torch.cuda.OutOfMemoryError as e:
            raise ValueError("%s: the triplet list does not fit in device memory (%s); use angle_distribution(..., "
                             "keep_angles=False) for the histogram alone" % (type(self).__name__, e)) from None

    def forward(self, xyz):
        return self._angle_cos(xyz.reshape(-1, self.natoms, 3))


class angle_distribution(Angles):
    """torchmd/observable.py:120-151: forward(xyz) -> (bins, count, angles).  count is the normalised Gaussian-smeared
    histogram of every ordered triplet angle (ops.AdfRawFn: HIP histogram and gradient).  angles are the per-triplet angles in
    the reference's order (torch ops, differentiable); keep_angles=False returns None there and never builds the list."""

    def __init__(self, system, nbins, angle_range, cutoff=3.0, index_tuple=None, width=None, keep_angles=True):
        super().__init__(system, nbins, angle_range, cutoff=cutoff, index_tuple=index_tuple, width=width)
        offsets = self.smear.offsets
        self.spacing = float(offsets[1] - offsets[0]) if nbins > 1 else 0.0      # linspace: equally spaced
        self.coeff = float(-0.5 / torch.pow(self.smear.width[0].detach().cpu().to(torch.float32), 2))
        if not (self.width != 0 and math.isfinite(self.coeff)):        # (a descending range gives a negative width)
            raise ValueError("angle_distribution: width must be nonzero, got %r" % self.width)
        self.keep_angles = keep_angles

    def forward(self, xyz):
        frames = xyz.reshape(-1, self.natoms, 3)
        count = ops.AdfRawFn.apply(frames, self.smear.offsets, self.coeff, self.cutoff, self._cell_struct, self._mask,
                                   self.spacing)
        count = count / count.sum()
        angles = None
        if self.keep_angles:
            angles = self._angle_cos(frames).acos()
        return self.bins, count, angles

    # -- the rows of the sum above: what a weighted average over frames needs (reweight.Reweighting) --------------------
    def per_frame(self, xyz):
        """raw[..., b] = sum over the ordered triplets of ONE frame of exp(coeff (theta - mu_b)^2): the un-normalised histogram
        of every frame of xyz ([N, 3], [T, N, 3], [R, T, N, 3] or replica-stacked [..., k N, 3] giving a trailing k before the
        bins), with the observable's cutoff and index_tuple selection.  `forward`'s histogram before its normalisation is the
        sum of these rows; `normalise` turns a row, a sum or a weighted average of rows into the distribution.  float32
        device positions run the HIP kernels of `forward` frame by frame (ops.AdfFramesFn, csrc/adf.hip: a workgroup per
        frame, no global atomics); host or float64 positions take the torch restatement `_torch_per_frame` with the exact
        sum.  In the kernels a non-finite angle makes the row of its frame NaN and no other (an atom with a non-finite
        coordinate has no listed neighbour, as in `forward`).  Differentiable once with respect to xyz."""
        n = xyz.shape[-2] if xyz.dim() >= 2 else 0
        if n == 0 or xyz.shape[-1] != 3 or n % self.natoms:
            raise ValueError("angle_distribution.per_frame: xyz must be [..., k * %d, 3], got %s" % (self.natoms, tuple(xyz.shape)))
        k = n // self.natoms
        lead = tuple(xyz.shape[:-2]) + ((k,) if k > 1 else ())
        x = xyz.reshape(-1, self.natoms, 3)
        if x.is_cuda and x.dtype == torch.float32:
            raw = ops.AdfFramesFn.apply(x, self.smear.offsets, self.coeff, self.cutoff, self._cell_struct, self._mask, self.spacing)
        else:
            raw = self._torch_per_frame(x)
        return raw.reshape(lead + (self.nbins,))

    def _torch_per_frame(self, x, budget=1 << 18):
        """The same rows by torch ops in x's dtype on x's device: all pairs of a frame (the neighbour test of the list
        builders: strict minimum image, 0 < d^2 < cutoff^2, the selection), every unordered pair of neighbours of every
        centre with weight 2, bond vectors re-imaged with topology.get_offsets, theta = atan2(|u x v|, u.v), every centre (no
        reach); chunked over frames.  A triplet with |u x v| <= 2^-20 |u| |v| has no gradient, as in the kernels."""
        F, N = x.shape[0], x.shape[1]
        L, mu = self.cell.detach().to(x), self.smear.offsets.detach().to(x)
        sel = None if self._mask is None else self._mask.to(x.device).bool()
        eps2 = (2.0 ** -20) ** 2
        out = []
        for f in range(F):
            xf = x[f]
            with torch.no_grad():
                D = xf[None, :, :] - xf[:, None, :]
                s = D * (1.0 / L)
                D = D + (-(s > 0.5).to(x) + (s < -0.5).to(x)) * L
                d2 = D.pow(2).sum(-1)
                adj = (d2 < self.cutoff ** 2) & (d2 != 0)
                if sel is not None:
                    adj = adj & sel
                c, e = torch.nonzero(adj, as_tuple=True)                     # (centre, end), sorted by centre then end
                cnt = torch.bincount(c, minlength=N)
                start = torch.cumsum(cnt, 0) - cnt
                # every unordered pair (p < q) of entries of one centre's row
                K = int(cnt.max()) if c.numel() else 0
                tp, tq = torch.triu_indices(K, K, offset=1, device=x.device) if K > 1 else (c[:0], c[:0])
                ok = tq[None, :] < cnt[:, None]
                ci, ti = torch.nonzero(ok, as_tuple=True)
                ia, ib = e[start[ci] + tp[ti]], e[start[ci] + tq[ti]]
            row = x.new_zeros(self.nbins)
            for a in range(0, ci.numel(), budget):
                cc, aa, bb = ci[a:a + budget], ia[a:a + budget], ib[a:a + budget]
                u, v = xf[aa] - xf[cc], xf[bb] - xf[cc]
                u = u + get_offsets(u.detach(), L, x.device).to(x) * L
                v = v + get_offsets(v.detach(), L, x.device).to(x) * L
                w = torch.cross(u, v, dim=-1)
                w2, dot = w.pow(2).sum(-1), (u * v).sum(-1)
                deg = w2.detach() <= eps2 * (u.pow(2).sum(-1) * v.pow(2).sum(-1)).detach()
                th = torch.where(deg, torch.atan2(torch.zeros_like(dot), dot).detach(),
                                 torch.atan2(torch.where(deg, torch.ones_like(w2), w2).sqrt(), dot))
                row = row + 2.0 * torch.exp(self.coeff * (th[:, None] - mu[None, :]).pow(2)).sum(0)
            out.append(row)
        return torch.stack(out)

    def normalise(self, raw):
        """The distribution of an un-normalised histogram raw[..., b] -- a row of `per_frame`, their sum or a weighted average
        of them -- by the tail of `forward`: raw / raw.sum(-1)."""
        return raw / raw.sum(-1, keepdim=True)


def compute_dihe(xyz, dihes):
    """torchmd/observable.py:181-197: cos of the dihedral angle of every row (i, j, k, l) of `dihes` in every frame of xyz
    [F, N, 3] -> [F, n].  No periodic imaging, as in the reference (Dihedrals images the bond vectors).  Torch ops with the
    cross products taken along the last axis explicitly: the reference's torch.cross without `dim` picks the first axis of
    size 3, so it is wrong for three frames or three rows."""
    assert len(xyz.shape) == 3
    d = torch.as_tensor(dihes).to(xyz.device).to(torch.long).reshape(-1, 4)
    xi, xj, xk, xl = (xyz[:, d[:, a]] for a in range(4))
    cross1 = torch.cross(xj - xi, xj - xk, dim=-1)
    cross2 = torch.cross(xk - xj, xk - xl, dim=-1)
    norm = (cross1.pow(2).sum(-1) * cross2.pow(2).sum(-1)).sqrt()
    return (cross1 * cross2).sum(-1) / norm


DIHEDRAL_MAX_BINS, DIHEDRAL_MAX_WIDTH = 4096, 0.5                      # csrc/dihedral.hip


class Dihedrals(Observable):
    """Signed dihedral angles over a static table `top` [n_terms, 4] of quadruples (i, j, k, l).

    With b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k, each re-imaged with topology.get_offsets on the diagonal of the cell
    (so wrapped frames, as Simulations returns them, are fine), n1 = b1 x b2 and n2 = b2 x b3:

        phi = atan2(|b2| b1.n2, n1.n2)  in (-pi, pi]        cos phi = n1.n2 / sqrt(|n1|^2 |n2|^2)

    This is the IUPAC sign.  cos phi is the reference's compute_dihe (torchmd/observable.py:181-197) wherever every bond vector
    is shorter than half the box; the signed dihedral d_i of the polymer demo's compute_intcoord (demo/fold.py:57-72) is -phi
    wherever that function does not clamp.  A term with three collinear atoms (|n1|^2 <= eps^2 |b1|^2 |b2|^2 or
    |n2|^2 <= eps^2 |b2|^2 |b3|^2, eps = 2^-20) is skipped: phi = cos phi = 0 with zero gradient.

    forward(xyz) -> phi [F, n_terms] and cos(xyz) -> cos phi [F, n_terms], with xyz reshaped to (-1, natoms, 3) like the other
    observables: replica-stacked trajectories [T, R N, 3] give T R frames with a `top` over one replica's atoms; a `top` that
    names atoms of the whole stacked system keeps them as T frames of R N atoms.  HIP kernels forward and backward
    (ops.DihedralPhiFn, csrc/dihedral.hip); the gradient of phi has no 1 / sin phi and is finite at phi = 0 and +-pi.
    Differentiable once."""

    def __init__(self, system, top):
        super().__init__(system)
        self.top = torch.as_tensor(top).to(torch.long).reshape(-1, 4)
        total = system.get_number_of_atoms()
        if self.top.numel() and int(self.top.max()) >= self.natoms and total > self.natoms:
            self.natoms = total                            # the table indexes the stacked system
        self._table = ops.DihedralTable(self.top, self.natoms, self.cell.detach().cpu().tolist(), self.device)
        self.n_terms = self._table.n_terms

    def _phi_cos(self, xyz):
        return ops.DihedralPhiFn.apply(xyz.reshape(-1, self.natoms, 3), self._table)

    def cos(self, xyz):
        return self._phi_cos(xyz)[1]

    def forward(self, xyz):
        return self._phi_cos(xyz)[0]


class dihedral_distribution(Dihedrals):
    """Periodic Gaussian-smeared histogram of the signed dihedral angles of Dihedrals, in the shape of angle_distribution:
    forward(xyz) -> (bins, count, phi).

        bins = linspace(-pi, pi, nbins + 1),   centres mu_b = -pi + (b + 1/2) 2 pi / nbins,   width default 2 pi / nbins
        raw[b] = sum over frames and terms of exp(-1/2 (wrap(phi - mu_b) / width)^2),        count = raw / raw.sum()

    wrap maps onto [-pi, pi): an angle near pi also feeds the bins near -pi.  Only the nearest image of a centre counts, so
    width > 0.5 is refused (beyond it the neglected second image exceeds exp(-pi^2 / (2 0.25)) ~ 3e-9 of a peak term);
    centres farther than 5.3 width sqrt(2 ln 2) from an angle are dropped (below 2^-28 of a peak term, the reach of
    angle_distribution).  Skipped (degenerate) terms carry no weight.  phi [F, n_terms] is None with keep_angles=False.
    HIP kernels forward and backward (ops.DihedralHistFn, ops.DihedralPhiFn), bitwise reproducible, differentiable once."""

    def __init__(self, system, top, nbins, width=None, keep_angles=True):
        super().__init__(system, top)
        if not (isinstance(nbins, (int, np.integer)) and 1 <= int(nbins) <= DIHEDRAL_MAX_BINS):
            raise ValueError("dihedral_distribution: nbins must be an integer in 1..%d, got %r" % (DIHEDRAL_MAX_BINS, nbins))
        self.nbins = int(nbins)
        self.spacing = 2.0 * math.pi / self.nbins
        self.width = self.spacing if width is None else float(width)
        if not (0.0 < self.width <= DIHEDRAL_MAX_WIDTH):
            raise ValueError("dihedral_distribution: width must be in (0, %g] (nearest image only), got %r%s"
                             % (DIHEDRAL_MAX_WIDTH, self.width, "; give a width with fewer than 13 bins" if width is None else ""))
        self.coeff = -0.5 / self.width ** 2
        self.bins = torch.linspace(-math.pi, math.pi, self.nbins + 1).to(self.device)
        self.offsets = (-math.pi + (torch.arange(self.nbins, dtype=torch.float64) + 0.5) * self.spacing).to(torch.float32).to(self.device)
        self.keep_angles = keep_angles

    def forward(self, xyz):
        phi, cos = self._phi_cos(xyz)
        raw = ops.DihedralHistFn.apply(phi, cos, self.nbins, self.width)
        return self.bins, raw / raw.sum(), (phi if self.keep_angles else None)


SK_MAX_VECTORS, SK_MAX_BINS, SK_MAX_INDEX = 65536, 1024, 1024          # csrc/sk.hip


def sk_vectors(lengths, nbins, k_range, dim=3, max_per_bin=None):
    """The wave vectors of structure_factor, on the host in float64: (n int64 [M, 3] sorted by bin, then by (|n|^2, nx, ny,
    nz) inside a bin; seg int64 [nbins + 1], the bins' segment offsets in n; |k| float64 [M]; edges float64 [nbins + 1]).
    Half space only: nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and nz > 0; dim = 2 keeps nz = 0."""
    L = np.asarray(lengths, dtype=np.float64)
    k0, k1 = float(k_range[0]), float(k_range[1])
    edges = torch.linspace(k0, k1, nbins + 1, dtype=torch.float64).numpy()
    nmax = np.floor(k1 * L / (2 * np.pi)).astype(np.int64)
    if dim == 2:
        nmax[2] = 0
    if int(nmax.max()) > SK_MAX_INDEX:
        raise ValueError("structure_factor: k_range[1] = %g reaches wave-vector indices beyond %d in this cell" % (k1, SK_MAX_INDEX))
    ax = [np.arange(0, nmax[0] + 1), np.arange(-nmax[1], nmax[1] + 1), np.arange(-nmax[2], nmax[2] + 1)]
    n = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))
    n = n[half]
    kabs = np.sqrt(((2 * np.pi * n / L) ** 2).sum(1))
    b = np.searchsorted(edges, kabs, side="right") - 1              # edges[b] <= |k| < edges[b + 1]
    keep = (b >= 0) & (b < nbins)
    n, kabs, b = n[keep], kabs[keep], b[keep]
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], (n * n).sum(1), b))
    n, kabs, b = n[order], kabs[order], b[order]
    seg = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=nbins))]).astype(np.int64)
    if max_per_bin is not None:
        first = (np.arange(len(n)) - seg[b]) < int(max_per_bin)
        n, kabs, b = n[first], kabs[first], b[first]
        seg = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=nbins))]).astype(np.int64)
    return n, seg, kabs, edges


class structure_factor(Observable):
    """Static structure factor over the wave vectors the periodic cell allows (no counterpart in the reference).

    For a diagonal cell of lengths L the vectors are k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz), integer n != 0; k and -k give
    the same value, so the half space nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and nz > 0 is used (nz = 0 only for
    system.dim == 2).  With real per-atom weights w (default 1), for frame f

        rho_f(k) = sum_i w_i exp(i k.x_fi)        S_f(k) = |rho_f(k)|^2 / sum_i w_i^2
        S_f[b]   = mean of S_f(k) over the selected vectors with bins[b] <= |k| < bins[b + 1]

    bins = linspace(k_range[0], k_range[1], nbins + 1); |k| is taken in float64 on the host; inside a bin the vectors are
    ordered by (|n|^2, nx, ny, nz) and max_per_bin=m keeps the first m of each bin (large boxes: a 4 096-atom LJ box has
    ~1.3e5 half-space vectors below k = 15).  An empty bin gives S = 0 and n_vectors = 0 there: mask it.  The vectors do not
    depend on the positions, so the hard bins are exactly differentiable in x; S is periodic in every coordinate and the
    phases are reduced in turns per axis before sine and cosine, so unwrapped positions many cells away cost no accuracy.

    forward(xyz) -> (k [nbins], S [nbins]): the mean |k| of each bin's vectors (the bin centre for an empty bin) and the mean
    of S_f[b] over all frames.  per_frame(xyz) -> S_f with the leading shape of xyz ([N, 3] -> [nbins], [T, N, 3] ->
    [T, nbins], [R, T, N, 3] -> [R, T, nbins], replica-stacked [..., k N, 3] -> [..., k, nbins]).  Attributes: bins (the edges),
    n_vectors [nbins], kvecs [M, 3] (the integer vectors, bin by bin).  HIP kernels forward and backward (ops.SkFn,
    csrc/sk.hip), differentiable once with respect to the positions; the weights are constants.

    Partials: 0/1 weights give the partial S_AA of the selected atoms.  The cross partial takes three calls, since
    |rho_A + rho_B|^2 = |rho_A|^2 + |rho_B|^2 + 2 Re rho_A rho_B*: with N_X = sum w_X^2,
    Re rho_A rho_B* = (N_AB S_AB - N_A S_AA - N_B S_BB) / 2 for w_AB = w_A + w_B."""

    def __init__(self, system, nbins, k_range, weights=None, max_per_bin=None):
        super().__init__(system)
        full = np.asarray(system.get_cell(), dtype=np.float64)
        if full.shape == (3, 3) and np.any(full - np.diag(np.diag(full)) != 0.0):
            raise ValueError("structure_factor: the cell must be diagonal (triclinic cells are not supported)")
        if not (int(nbins) >= 1 and int(nbins) <= SK_MAX_BINS):
            raise ValueError("structure_factor: nbins must be 1..%d, got %r" % (SK_MAX_BINS, nbins))
        if not (len(k_range) == 2 and 0 < float(k_range[0]) < float(k_range[1])):
            raise ValueError("structure_factor: k_range must be (k_min, k_max) with 0 < k_min < k_max, got %r" % (k_range,))
        if max_per_bin is not None and int(max_per_bin) < 1:
            raise ValueError("structure_factor: max_per_bin must be a positive integer, got %r" % (max_per_bin,))
        self.nbins, self.dim = int(nbins), getattr(system, "dim", 3)
        lengths = self.cell.detach().cpu().to(torch.float64).numpy()          # the float32 lengths the kernels see
        n, seg, kabs, edges = sk_vectors(lengths, self.nbins, k_range, self.dim, max_per_bin)
        if len(n) == 0:
            raise ValueError("structure_factor: no wave vector of this cell lies in k_range = %r" % (tuple(k_range),))
        if len(n) > SK_MAX_VECTORS:
            raise ValueError("structure_factor: %d wave vectors exceed the limit of %d; thin them with max_per_bin"
                             % (len(n), SK_MAX_VECTORS))
        self.bins = torch.as_tensor(edges)
        counts = np.diff(seg)
        sums = np.bincount(np.repeat(np.arange(self.nbins), counts), weights=kabs, minlength=self.nbins)
        centre = 0.5 * (edges[1:] + edges[:-1])
        self.n_vectors = torch.as_tensor(counts)
        self.kvecs = torch.as_tensor(n)
        self.k = torch.as_tensor(np.where(counts > 0, sums / np.maximum(counts, 1), centre), dtype=torch.float32).to(self.device)
        self._seg_host = [int(x) for x in seg]
        self._kvec = torch.as_tensor(n, dtype=torch.int32).contiguous().to(self.device)
        self._seg = torch.as_tensor(seg, dtype=torch.int32).to(self.device)
        if weights is None:
            self.weights, self._norm = None, float(self.natoms)
        else:
            w = torch.as_tensor(weights, dtype=torch.float32).detach().reshape(-1).cpu()
            if w.numel() != self.natoms:
                raise ValueError("structure_factor: weights must hold one entry per atom (%d), got %d" % (self.natoms, w.numel()))
            self._norm = float(w.double().pow(2).sum())
            if not (self._norm > 0 and np.isfinite(self._norm)):
                raise ValueError("structure_factor: the weights must be finite and not all zero")
            self.weights = w.contiguous().to(self.device)
        self._cell_struct = _lib.make_cell(self.cell)

    def _frames(self, x):
        n = x.shape[-2] if x.dim() >= 2 else 0
        if n == 0 or x.shape[-1] != 3 or n % self.natoms:
            raise ValueError("structure_factor: xyz must be [..., k * %d, 3], got %s" % (self.natoms, tuple(x.shape)))
        k = n // self.natoms                             # replica-stacked state [..., k N, 3]: one row per replica
        lead = tuple(x.shape[:-2]) + ((k,) if k > 1 else ())
        return x.reshape(-1, self.natoms, 3), lead

    def per_frame(self, xyz):
        """S_f[b] of every frame of xyz ([N, 3], [T, N, 3], [R, T, N, 3] or replica-stacked [..., k N, 3])."""
        x, lead = self._frames(xyz)
        S = ops.SkFn.apply(x, self._cell_struct, self.weights, self._norm, self._kvec, self._seg)
        return S.reshape(lead + (self.nbins,))

    def forward(self, xyz):
        return self.k, self.per_frame(xyz).reshape(-1, self.nbins).mean(0)


MSD_MAX_LAGS = 1024                                                    # csrc/msd.hip


class msd(Observable):
    """Mean-squared displacement over all lags and time origins, optionally with the fourth moment (no counterpart in the
    reference).

    For one replica of T frames, real per-atom weights w_i >= 0 (default 1), s = origin_stride and the time origins
    O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T}, the moments of order p = 2 and 4 are

        M_p[tau] = 1 / (|O_tau| sum_i w_i)  sum_{t0 in O_tau} sum_i w_i |x_i(t0 + tau) - x_i(t0)|^p ,   tau = 0 .. t_range - 1

    (the lag convention of vacf: t_range lags, the first is 0, and M_p[0] is exactly 0).  The positions are taken as given:
    all three components are used and nothing is re-imaged, so q_t has to be ONE continuous, unwrapped trajectory -- what a
    single simulate / odeint_adjoint call returns (the fused trajectories do not wrap inside a call), not frames concatenated
    across epochs, between which Simulations.simulate wraps the positions into the cell.

    index_tuple selects atoms: a list of atom indices, or the pair form of the other observables (two lists), meaning their
    union; it is shorthand for 0/1 weights, so a per-species MSD is one call.  weights and index_tuple multiply.  The weights
    are constants (no gradient).

    forward(q_t) -> M_2 [t_range], the mean over the replicas.  per_replica(q_t) keeps them: [T, N, 3] -> [t_range],
    [R, T, N, 3] -> [R, t_range] (time is dim -3), replica-stacked [T, k N, 3] -> [k, t_range] and [R, T, k N, 3] ->
    [R, k, t_range].  With fourth_moment=True: moments(q_t) -> (M_2, M_4), moments_per_replica(q_t) likewise, and
    non_gaussian(q_t) -> alpha_2 = d M_4 / ((d + 2) M_2^2) - 1 with d = system.dim, 0 where M_2 is 0 (lag 0).
    diffusion_coefficient(m, dt) turns M_2 into the Einstein estimate of D.

    HIP kernels forward and backward (ops.MsdFn, csrc/msd.hip): every position is read once, whatever t_range is.
    Differentiable once with respect to the positions; t_range <= 1024."""

    def __init__(self, system, t_range, index_tuple=None, weights=None, origin_stride=1, fourth_moment=False):
        super().__init__(system)
        if not (isinstance(t_range, (int, np.integer)) and 1 <= int(t_range) <= MSD_MAX_LAGS):
            raise ValueError("msd: t_range must be an integer in 1..%d, got %r" % (MSD_MAX_LAGS, t_range))
        if not (isinstance(origin_stride, (int, np.integer)) and int(origin_stride) >= 1):
            raise ValueError("msd: origin_stride must be an integer >= 1, got %r" % (origin_stride,))
        self.t_range, self.origin_stride, self.fourth_moment = int(t_range), int(origin_stride), bool(fourth_moment)
        self.dim = getattr(system, "dim", 3)
        self.index_tuple = index_tuple
        w = None
        if weights is not None:
            w = torch.as_tensor(weights, dtype=torch.float32).detach().reshape(-1).cpu()
            if w.numel() != self.natoms:
                raise ValueError("msd: weights must hold one entry per atom (%d), got %d" % (self.natoms, w.numel()))
            if not (bool(torch.isfinite(w).all()) and bool((w >= 0).all())):
                raise ValueError("msd: weights must be finite and non-negative")
        if index_tuple is not None:
            idx = list(index_tuple)
            if len(idx) and not isinstance(idx[0], (int, np.integer)):            # the pair form: the union of both lists
                idx = [i for part in idx for i in list(part)]
            sel = torch.as_tensor(np.asarray(idx, dtype=np.int64)).reshape(-1)
            if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= self.natoms:
                raise ValueError("msd: index_tuple must name atoms in 0..%d, got %r" % (self.natoms - 1, index_tuple))
            mask = torch.zeros(self.natoms)
            mask[sel] = 1.0
            w = mask if w is None else w * mask
        if w is not None and not float(w.double().sum()) > 0:
            raise ValueError("msd: the weights%s must not all be zero" % (" (with index_tuple applied)" if index_tuple is not None else ""))
        self.weights = None if w is None else w.contiguous().to(self.device)

    def _batch(self, x):
        if x.dim() not in (3, 4) or x.shape[-1] != 3 or x.shape[-2] == 0 or x.shape[-2] % self.natoms:
            raise ValueError("msd: q_t must be [T, k * %d, 3] or [R, T, k * %d, 3], got %s" % (self.natoms, self.natoms, tuple(x.shape)))
        if self.t_range > x.shape[-3]:
            raise ValueError("msd: t_range = %d exceeds the %d frames of q_t" % (self.t_range, x.shape[-3]))
        k = x.shape[-2] // self.natoms
        lead = (tuple(x.shape[:-3]) + ((k,) if k > 1 else ()))
        return (x if x.dim() == 4 else x.unsqueeze(0)), lead

    def moments_per_replica(self, q_t):
        """(M_2, M_4) of every replica (M_4 is None without fourth_moment), shaped as per_replica."""
        x, lead = self._batch(q_t)
        m2, m4 = ops.MsdFn.apply(x, self.natoms, self.weights, self.t_range, self.origin_stride, self.fourth_moment)
        return m2.reshape(lead + (self.t_range,)), (m4.reshape(lead + (self.t_range,)) if m4 is not None else None)

    def per_replica(self, q_t):
        """M_2 of every replica: [t_range], [R, t_range], [k, t_range] or [R, k, t_range]."""
        return self.moments_per_replica(q_t)[0]

    def moments(self, q_t):
        """(M_2, M_4), each [t_range], averaged over the replicas; needs fourth_moment=True."""
        if not self.fourth_moment:
            raise ValueError("msd: moments / non_gaussian need fourth_moment=True")
        m2, m4 = self.moments_per_replica(q_t)
        return m2.reshape(-1, self.t_range).mean(0), m4.reshape(-1, self.t_range).mean(0)

    def non_gaussian(self, q_t):
        """alpha_2[tau] = d M_4 / ((d + 2) M_2^2) - 1 from the replica-averaged moments; 0 where M_2 = 0 (lag 0)."""
        m2, m4 = self.moments(q_t)
        ok = m2 > 0
        safe = torch.where(ok, m2, torch.ones_like(m2))
        return torch.where(ok, self.dim * m4 / ((self.dim + 2) * safe * safe) - 1.0, torch.zeros_like(m2))

    def forward(self, q_t):
        return self.per_replica(q_t).reshape(-1, self.t_range).mean(0)


def diffusion_coefficient(m, dt, fit_range=None, dim=3):
    """Einstein estimate D = slope / (2 dim): the least-squares slope of m[..., a:b] against tau * dt over the lags
    tau = a .. b - 1 of fit_range = (a, b) (default: every lag), in closed form,

        slope = sum_tau (tau - mean tau) m[tau] / (dt sum_tau (tau - mean tau)^2)

    so it is differentiable in m and works on any leading batch shape.  m [..., L] is what msd returns (lag tau at index tau)."""
    L = m.shape[-1]
    a, b, _ = slice(*(fit_range if fit_range is not None else (0, L))).indices(L)
    if b - a < 2:
        raise ValueError("diffusion_coefficient: fit_range = %r selects %d of the %d lags; a slope needs two"
                         % (fit_range, max(b - a, 0), L))
    tau = torch.arange(a, b, device=m.device, dtype=m.dtype)
    c = tau - tau.mean()
    return (m[..., a:b] * (c / (c.pow(2).sum() * dt))).sum(-1) / (2 * dim)


def isf_max_lags():
    """The largest t_range of intermediate_scattering: what the LDS ring of csrc/isf.hip holds (mdg_isf_max_lags)."""
    return int(_lib.load().mdg_isf_max_lags())


class intermediate_scattering(Observable):
    """Intermediate scattering function over all lags and time origins, coherent or self (no counterpart in the reference).

    The cell is diagonal with lengths L; the wave vectors k(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz) are selected, ordered and
    binned exactly as structure_factor does (sk_vectors: half space, hard bins on |k| taken in float64, max_per_bin,
    system.dim == 2 keeping nz = 0).  For one replica of T frames, real per-atom weights w_i (default 1), s = origin_stride,
    the time origins O_tau = {t0 = 0, s, 2 s, ... : t0 + tau < T} and the lags tau = 0 .. t_range - 1 (the lag convention of
    vacf and msd)

        rho(k, t)   = sum_i w_i exp(i k.x_i(t))                 W2 = sum_i w_i^2
        F(k, tau)   = 1 / (|O_tau| W2)  sum_{t0 in O_tau} Re[ rho(k, t0 + tau) conj rho(k, t0) ]                  kind="coherent"
        F_s(k, tau) = 1 / (|O_tau| W2)  sum_{t0 in O_tau} sum_i w_i^2 cos( k.(x_i(t0 + tau) - x_i(t0)) )          kind="self"
        F[b, tau], F_s[b, tau] = mean over the selected vectors of bin b      (empty bin: 0, n_vectors[b] = 0: mask it)

    F_s is exactly the i = j part of F, so the distinct part is F - F_s; with 0/1 weights both are the partial functions of
    the selected atoms.  F[b, 0] with origin_stride = 1 is the frame mean of structure_factor's S[b]; F_s[b, 0] = 1; for one
    atom F = F_s.  The small-k limit of F_s is exp(-k^2 MSD / 6).  Both are periodic in every coordinate of every frame:
    positions wrapped into the cell and unwrapped positions give the same value, unlike msd.  The frames still have to be
    consecutive in time, but wrapping between epochs (Simulations.simulate) does no harm.

    index_tuple selects atoms as in msd: a list of atom indices, or the pair form of the other observables (two lists),
    meaning their union; it is shorthand for 0/1 weights and multiplies into weights.  Weights and vectors are constants.

    forward(q_t) -> (k [nbins], F [nbins, t_range]): the mean |k| of each bin's vectors (the bin centre for an empty bin) and
    the mean over the replicas.  per_replica(q_t) keeps them: [T, N, 3] -> [nbins, t_range], [R, T, N, 3] ->
    [R, nbins, t_range] (time is dim -3), replica-stacked [T, k N, 3] -> [k, nbins, t_range] and [R, T, k N, 3] ->
    [R, k, nbins, t_range].  Attributes: bins (the edges), n_vectors [nbins], kvecs [M, 3], k [nbins].  relaxation(F)
    normalises by the lag-0 value, relaxation_time(phi, dt) gives the time at which it has fallen to 1 / e.

    HIP kernels forward and backward (ops.IsfFn, csrc/isf.hip): the self part costs one sine / cosine pair per (frame, atom,
    vector), not per (origin, lag, atom, vector).  Differentiable once with respect to the positions; t_range <= isf_max_lags()."""

    KINDS = {"coherent": 0, "self": 1}

    def __init__(self, system, nbins, k_range, t_range, kind="coherent", weights=None, index_tuple=None, max_per_bin=None,
                 origin_stride=1):
        super().__init__(system)
        name = "intermediate_scattering"
        full = np.asarray(system.get_cell(), dtype=np.float64)
        if full.shape == (3, 3) and np.any(full - np.diag(np.diag(full)) != 0.0):
            raise ValueError("%s: the cell must be diagonal (triclinic cells are not supported)" % name)
        if kind not in self.KINDS:
            raise ValueError("%s: kind must be 'coherent' or 'self', got %r" % (name, kind))
        if not (isinstance(nbins, (int, np.integer)) and 1 <= int(nbins) <= SK_MAX_BINS):
            raise ValueError("%s: nbins must be 1..%d, got %r" % (name, SK_MAX_BINS, nbins))
        if not (len(k_range) == 2 and 0 < float(k_range[0]) < float(k_range[1])):
            raise ValueError("%s: k_range must be (k_min, k_max) with 0 < k_min < k_max, got %r" % (name, k_range))
        if max_per_bin is not None and int(max_per_bin) < 1:
            raise ValueError("%s: max_per_bin must be a positive integer, got %r" % (name, max_per_bin))
        if not (isinstance(t_range, (int, np.integer)) and 1 <= int(t_range) <= isf_max_lags()):
            raise ValueError("%s: t_range must be an integer in 1..%d, got %r" % (name, isf_max_lags(), t_range))
        if not (isinstance(origin_stride, (int, np.integer)) and int(origin_stride) >= 1):
            raise ValueError("%s: origin_stride must be an integer >= 1, got %r" % (name, origin_stride))
        self.kind, self.nbins, self.dim = kind, int(nbins), getattr(system, "dim", 3)
        self.t_range, self.origin_stride, self.index_tuple = int(t_range), int(origin_stride), index_tuple
        lengths = self.cell.detach().cpu().to(torch.float64).numpy()          # the float32 lengths the kernels see
        try:
            n, seg, kabs, edges = sk_vectors(lengths, self.nbins, k_range, self.dim, max_per_bin)
        except ValueError as e:
            raise ValueError(str(e).replace("structure_factor", name)) from None
        if len(n) == 0:
            raise ValueError("%s: no wave vector of this cell lies in k_range = %r" % (name, tuple(k_range)))
        if len(n) > SK_MAX_VECTORS:
            raise ValueError("%s: %d wave vectors exceed the limit of %d; thin them with max_per_bin" % (name, len(n), SK_MAX_VECTORS))
        self.bins = torch.as_tensor(edges)
        counts = np.diff(seg)
        sums = np.bincount(np.repeat(np.arange(self.nbins), counts), weights=kabs, minlength=self.nbins)
        centre = 0.5 * (edges[1:] + edges[:-1])
        self.n_vectors = torch.as_tensor(counts)
        self.kvecs = torch.as_tensor(n)
        self.k = torch.as_tensor(np.where(counts > 0, sums / np.maximum(counts, 1), centre), dtype=torch.float32).to(self.device)
        self._seg_host = [int(x) for x in seg]
        self._kvec = torch.as_tensor(n, dtype=torch.int32).contiguous().to(self.device)
        self._seg = torch.as_tensor(seg, dtype=torch.int32).to(self.device)
        w = None
        if weights is not None:
            w = torch.as_tensor(weights, dtype=torch.float32).detach().reshape(-1).cpu()
            if w.numel() != self.natoms:
                raise ValueError("%s: weights must hold one entry per atom (%d), got %d" % (name, self.natoms, w.numel()))
            if not bool(torch.isfinite(w).all()):
                raise ValueError("%s: the weights must be finite and not all zero" % name)
        if index_tuple is not None:
            idx = list(index_tuple)
            if len(idx) and not isinstance(idx[0], (int, np.integer)):            # the pair form: the union of both lists
                idx = [i for part in idx for i in list(part)]
            sel = torch.as_tensor(np.asarray(idx, dtype=np.int64)).reshape(-1)
            if sel.numel() == 0 or int(sel.min()) < 0 or int(sel.max()) >= self.natoms:
                raise ValueError("%s: index_tuple must name atoms in 0..%d, got %r" % (name, self.natoms - 1, index_tuple))
            mask = torch.zeros(self.natoms)
            mask[sel] = 1.0
            w = mask if w is None else w * mask
        self._norm = float(self.natoms) if w is None else float(w.double().pow(2).sum())
        if not (self._norm > 0 and np.isfinite(self._norm)):
            raise ValueError("%s: the weights%s must be finite and not all zero"
                             % (name, " (with index_tuple applied)" if index_tuple is not None else ""))
        self.weights = None if w is None else w.contiguous().to(self.device)
        self._cell_struct = _lib.make_cell(self.cell)

    def _batch(self, x):
        if x.dim() not in (3, 4) or x.shape[-1] != 3 or x.shape[-2] == 0 or x.shape[-2] % self.natoms:
            raise ValueError("intermediate_scattering: q_t must be [T, k * %d, 3] or [R, T, k * %d, 3], got %s"
                             % (self.natoms, self.natoms, tuple(x.shape)))
        if self.t_range > x.shape[-3]:
            raise ValueError("intermediate_scattering: t_range = %d exceeds the %d frames of q_t" % (self.t_range, x.shape[-3]))
        k = x.shape[-2] // self.natoms
        lead = (tuple(x.shape[:-3]) + ((k,) if k > 1 else ()))
        return (x if x.dim() == 4 else x.unsqueeze(0)), lead

    def per_replica(self, q_t):
        """F (or F_s) of every replica: [nbins, t_range], [R, ...], [k, ...] or [R, k, nbins, t_range]."""
        x, lead = self._batch(q_t)
        F = ops.IsfFn.apply(x, self.KINDS[self.kind], self.natoms, self._cell_struct, self.weights, self._norm, self._kvec,
                            self._seg, self._seg_host, self.t_range, self.origin_stride)
        return F.reshape(lead + (self.nbins, self.t_range))

    def forward(self, q_t):
        return self.k, self.per_replica(q_t).reshape(-1, self.nbins, self.t_range).mean(0)


def relaxation(F):
    """phi = F / F[..., :1], the intermediate scattering function normalised by its lag-0 value (S(k) for the coherent one, 1
    for the self one); 0 where F[..., 0] is 0 (empty bins)."""
    f0 = F[..., :1]
    ok = f0 != 0
    return torch.where(ok, F / torch.where(ok, f0, torch.ones_like(f0)), torch.zeros_like(F))


def relaxation_time(phi, dt, level=math.exp(-1.0)):
    """The time at which phi [..., L] (lag tau at index tau, spacing dt) first falls to `level`, per leading row: with a the
    last lag before the first lag b = a + 1 at which phi <= level,

        t = dt (a + (phi[a] - level) / (phi[a] - phi[b]))

    the linear interpolation between the two, in closed form and differentiable in phi[a] and phi[b].  A row whose lag 0 is
    already at or below the level gives 0; a row that never falls to it gives inf, with no gradient."""
    L = phi.shape[-1]
    below = phi <= level
    hit = below.any(-1)
    b = below.to(torch.int64).argmax(-1)                                   # the first lag at or below the level
    a = (b - 1).clamp(min=0)
    pa, pb = phi.gather(-1, a.unsqueeze(-1)).squeeze(-1), phi.gather(-1, b.unsqueeze(-1)).squeeze(-1)
    inner = hit & (b > 0)
    den = torch.where(inner, pa - pb, torch.ones_like(pa))
    t = dt * (a.to(phi.dtype) + (pa - level) / den)
    out = torch.where(inner, t, torch.zeros_like(t))
    return torch.where(hit, out, torch.full_like(out, float("inf")))


class vacf(Observable):
    def __init__(self, system, t_range):
        super().__init__(system)
        self.t_window = [i for i in range(1, t_range, 1)]

    def forward(self, vel):
        """Lags 0 .. t_range-1 of the velocity autocorrelation of vel [T, N, 3] (mean over frames, atoms and
        components per lag, torchmd/observable.py:158-163) from one fused HIP reduction (ops.VacfFn)."""
        return ops.VacfFn.apply(vel, len(self.t_window) + 1)


BOND_ORDER_MAX_L, BOND_ORDER_MAX_NL = 12, 4                            # csrc/bond_order.hip
BOND_ORDER_Q_FLOOR = 2.0e-3


def _floored_ratio(num2, den):
    """sqrt(num2) / den with the floor rule of bond_order: 0 where den = 0, and a constant (zero gradient) wherever the value
    is at or below BOND_ORDER_Q_FLOOR -- sqrt has no derivative at 0."""
    with torch.no_grad():
        none = den == 0                                  # (a NaN count is not "no neighbours": it stays NaN)
        val = torch.where(none, torch.zeros_like(num2), num2.clamp_min(0).sqrt() / torch.where(none, torch.ones_like(den), den))
        live = val > BOND_ORDER_Q_FLOOR
    return torch.where(live, torch.where(live, num2, torch.ones_like(num2)).sqrt() / torch.where(live, den, torch.ones_like(den)), val)


class bond_order(Observable):
    """Steinhardt bond-orientational order parameters q_l (per atom) and Q_l (per frame) with a smooth neighbour weight
    (Steinhardt, Nelson, Ronchetti, Phys. Rev. B 28, 784 (1983); no counterpart in the reference).

    The bonds of atom i in one frame are the atoms j != i of the same replica (and of index_tuple's pairs) with
    r = |u| < cutoff, u = x_j - x_i re-imaged on the diagonal cell, s = u / r.  With

        w(r)    = 1                                                   r <= r_in
                = 1/2 [1 + cos(pi (r - r_in) / (cutoff - r_in))]      r_in < r < cutoff         (C^1; default r_in = 0.85 cutoff)
                = 0                                                   r >= cutoff
        A_lm(i) = sum_j w(r_ij) Y_lm(s_ij)        n_i = sum_j w(r_ij)             (Y_lm: real orthonormal harmonics, m = -l .. l)
        q_l(i)  = sqrt(4 pi / (2l+1) sum_m A_lm(i)^2) / n_i                       (0 where n_i = 0)
        Q_l     = sqrt(4 pi / (2l+1) sum_m (sum_i A_lm(i))^2) / sum_i n_i         per frame and replica (0 where sum n = 0)

    the smooth w replaces the textbook's hard neighbour count, so everything is differentiable in the positions; with r_in
    and cutoff between two neighbour shells it IS the textbook definition (fcc: q_4 = 0.19094, q_6 = 0.57452; bcc, 8 bonds:
    0.50918, 0.62854; hcp: 0.09722, 0.48476; tetrahedral: q_3 = 0.74536).

    Floor rule: sqrt has no derivative at 0, and q_l is exactly 0 for odd l in a centrosymmetric environment.  Wherever
    q_l(i) <= BOND_ORDER_Q_FLOOR = 2e-3 its gradient is defined as zero (the value is kept), and likewise for Q_l.  The floor
    is at least 16 times the float32 error bound of q_l, 2^-24 (kappa_l + sqrt(l (l+1)) (D + r) / r + 2 row length + 2l + 10):
    1.1e-4 for l = 12 (kappa_12 = 576, the measured rounding constant of the harmonic recurrences times 4), rows of 64 bonds
    and a raw coordinate difference D of 80 bond lengths r -- below the floor the direction of the gradient is rounding noise.
    Q_l of a disordered sample falls as 1 / sqrt(atoms x bonds): under the floor beyond ~2.5e5 bonds per frame.  Q_l of an
    odd l is identically 0, in any configuration: every bond is counted from both of its ends and Y_lm(-s) = -Y_lm(s).

    ls: 1 to 4 distinct l in 1 .. 12.  cutoff must be below half the shortest cell length (one image per pair), the cell
    diagonal; positions may be wrapped or unwrapped as long as two atoms are never more than 1.5 cell lengths apart in a
    coordinate (the list builder's image search) -- what one simulate call returns.  Two atoms at the same point give NaN.

    per_atom(q_t) -> q [F, N, n_l] ([F, k, N, n_l] replica-stacked); per_frame(q_t) -> Q [F, n_l] ([F, k, n_l]);
    forward(q_t) -> Q [n_l], the mean over frames and replicas; moments(q_t) -> (A [F, (k,) N, K], n [F, (k,) N]) for other
    invariants, K = sum (2l+1).  Component order of A: the l of `ls` in the given order, inside one l the 2l+1 entries
    m = -l .. l with Y_l,-m = c_lm Q_l^m(s_z) Im (s_x + i s_y)^m, Y_l0 = N_l0 P_l(s_z), Y_l,+m = c_lm Q_l^m(s_z) Re (s_x + i s_y)^m,
    Q_l^m = d^m P_l / dz^m (no Condon-Shortley phase), c_lm = sqrt(2 (2l+1) / (4 pi) (l-m)! / (l+m)!).

    HIP kernels forward and backward (ops.BondOrderFn, csrc/bond_order.hip), bitwise reproducible, differentiable once."""

    def __init__(self, system, ls=(4, 6), cutoff=None, r_in=None, index_tuple=None):
        super().__init__(system)
        name = type(self).__name__
        full = np.asarray(system.get_cell(), dtype=np.float64)
        if full.shape == (3, 3) and np.any(full - np.diag(np.diag(full)) != 0.0):
            raise ValueError("%s: the cell must be diagonal (triclinic cells are not supported)" % name)
        try:
            ls = [l for l in ls]
        except TypeError:
            ls = [ls]
        if not (1 <= len(ls) <= BOND_ORDER_MAX_NL) or any(not isinstance(l, (int, np.integer)) or not 1 <= l <= BOND_ORDER_MAX_L
                                                          for l in ls) or len(set(ls)) != len(ls):
            raise ValueError("%s: ls must be 1 to %d distinct integers in 1..%d, got %r" % (name, BOND_ORDER_MAX_NL, BOND_ORDER_MAX_L, ls))
        if cutoff is None or not (float(cutoff) > 0 and math.isfinite(float(cutoff))):
            raise ValueError("%s: cutoff must be a positive number, got %r" % (name, cutoff))
        shortest = float(self.cell.min())
        if not float(cutoff) < 0.5 * shortest:
            raise ValueError("%s: cutoff = %g must be below half the shortest cell length (%g): one image per pair"
                             % (name, float(cutoff), shortest))
        r_in = 0.85 * float(cutoff) if r_in is None else float(r_in)
        if not 0.0 < r_in < float(cutoff):
            raise ValueError("%s: r_in must lie in (0, cutoff = %g), got %g" % (name, float(cutoff), r_in))
        self.ls = tuple(int(l) for l in ls)
        self.offsets_l = tuple(int(o) for o in np.cumsum([0] + [2 * l + 1 for l in self.ls]))
        self.n_components = self.offsets_l[-1]
        self.cutoff, self.r_in = float(cutoff), r_in
        self.index_tuple = index_tuple
        self._cell_struct = _lib.make_cell(self.cell)
        self._mask = ops.build_mask(self.natoms, index_tuple, None, self.device)

    def _frames(self, x):
        n = x.shape[-2] if x.dim() >= 2 else 0
        if n == 0 or x.shape[-1] != 3 or n % self.natoms:
            raise ValueError("%s: q_t must be [..., k * %d, 3], got %s" % (type(self).__name__, self.natoms, tuple(x.shape)))
        k = n // self.natoms
        lead = tuple(x.shape[:-2]) + ((k,) if k > 1 else ())
        return x.reshape(-1, self.natoms, 3), lead

    def moments(self, q_t):
        x, lead = self._frames(q_t)
        A, n = ops.BondOrderFn.apply(x, self.ls, self.cutoff, self.r_in, self._cell_struct, self._mask)
        return A.reshape(lead + (self.natoms, self.n_components)), n.reshape(lead + (self.natoms,))

    def _invariants(self, A, n):
        """sqrt(4 pi / (2l+1) sum_m A_lm^2) / n for every l of ls, on the last axes of A [..., K] and n [...]."""
        out = []
        for k, l in enumerate(self.ls):
            a = A[..., self.offsets_l[k]:self.offsets_l[k + 1]]
            out.append(_floored_ratio(4.0 * math.pi / (2 * l + 1) * a.pow(2).sum(-1), n))
        return torch.stack(out, -1)

    def per_atom(self, q_t):
        return self._invariants(*self.moments(q_t))

    def per_frame(self, q_t):
        A, n = self.moments(q_t)
        return self._invariants(A.sum(-2), n.sum(-1))

    def forward(self, q_t):
        return self.per_frame(q_t).reshape(-1, len(self.ls)).mean(0)


class bond_order_distribution(bond_order):
    """Gaussian-smeared histogram of the per-atom q_l of bond_order, in the shape of angle_distribution:
    forward(q_t) -> (bins, count, q).  bins = linspace(q_range[0], q_range[1], nbins + 1); the centres and the width follow
    GaussianSmearing(start, stop, nbins, width) as in Angles (width: the centre spacing unless given);
    count[b] = sum over frames, replicas and atoms with n_i > 0 of exp(-1/2 ((q_l(i) - mu_b) / width)^2), normalised to sum 1.
    Atoms without a neighbour (n_i = 0) are left out.  q [F, (k,) N] is None with keep_values=False.  The moments come from the
    HIP kernels of bond_order; the histogram is per-atom torch work."""

    def __init__(self, system, l, nbins, q_range, cutoff, r_in=None, index_tuple=None, width=None, keep_values=True):
        super().__init__(system, ls=(l,), cutoff=cutoff, r_in=r_in, index_tuple=index_tuple)
        if not (isinstance(nbins, (int, np.integer)) and int(nbins) >= 1):
            raise ValueError("bond_order_distribution: nbins must be a positive integer, got %r" % (nbins,))
        start, end = float(q_range[0]), float(q_range[1])
        if width is not None and not (float(width) != 0 and math.isfinite(float(width))):
            raise ValueError("bond_order_distribution: width must be nonzero, got %r" % (width,))
        if width is None and (nbins < 2 or start == end):
            raise ValueError("bond_order_distribution: give a width with one bin or an empty q_range")
        self.nbins = int(nbins)
        self.bins = torch.linspace(start, end, self.nbins + 1).to(self.device)
        self.smear = GaussianSmearing(start=start, stop=self.bins[-1], n_gaussians=self.nbins, width=width, trainable=False).to(self.device)
        self.width = self.smear.width[0].item()
        self.coeff = float(-0.5 / torch.pow(self.smear.width[0].detach().cpu().to(torch.float32), 2))
        self.keep_values = keep_values

    def forward(self, q_t):
        A, n = self.moments(q_t)
        q = self._invariants(A, n)[..., 0]
        keep = (n > 0).to(q.dtype).reshape(-1, 1)
        raw = (keep * torch.exp(self.coeff * (q.reshape(-1, 1) - self.smear.offsets[None, :]).pow(2))).sum(0)
        return self.bins, raw / raw.sum(), (q if self.keep_values else None)
