"""Device ops: thin Python over the C ABI (include/mdgrad_hip.h) plus the
torch.autograd.Function wrappers that own the differentiation contract

    PairEnergyFn -> PairGradFn -> (Hessian-vector product)     pair potentials, any order <= 2
    FusedTrajFn                                                 whole NH-Verlet/Verlet trajectory + adjoint
    RdfRawFn                                                    soft histogram
    AdfRawFn                                                    soft histogram of bond angles
    AdfFramesFn                                                 soft histogram of bond angles of every frame
    VirialFn                                                    pair virial of every frame (pressure)
    EnergyFramesFn                                              pair potential energy of every frame (reweighting)
    EnergyTableFn                                               tabulated pair energy of every frame (learned pair modules)
    SWFramesFn                                                  Stillinger-Weber energy of every frame (reweighting)
    EAMTableFramesFn, EAMFramesFn                               embedded-atom energy of every frame (reweighting)
    RdfFramesFn                                                 soft histogram of every frame
    SkFn                                                        static structure factor of every frame
    MsdFn                                                       mean-squared displacement over all lags (+ fourth moment)
    IsfFn                                                       intermediate scattering functions F(k,t), F_s(k,t)
    BondOrderFn                                                 Steinhardt moments A_lm(i), n_i over the per-atom list
    TermEnergyFn -> TermGradFn                                  every other term with parameters, order <= 2 in x, 1 in the
                                                                parameters; what differs per kernel family is a small `term` object:
      DihedralTerm                                              torsion term, parameters: its coefficients
      CoulombTerm, EwaldTerm, EwaldExclTerm                     the point-charge terms (damped shifted-force sum, Ewald reciprocal
                                                                sum, erf correction of excluded pairs) on _ChargeTerm, parameters:
                                                                the charges; `pot_scale` says which factor their kernel leaves out
      SWTerm                                                    Stillinger-Weber term, parameters: (epsilon, sigma, lam)
      SWMultiTerm                                               the same for up to four species: (epsilon [S,S], sigma [S,S], lam [S,S,S])
      EAMTerm                                                   Sutton-Chen term, parameters: (epsilon, a, c)
      EAMTableTerm                                              tabulated embedded-atom term, parameters: the trainable node tables
      TersoffTerm                                               Tersoff bond-order term, parameters: (A, B, h)
      TersoffMultiTerm                                          the same for up to four species: (A [S,S], B [S,S], h [S])
    DihedralPhiFn, DihedralHistFn                               signed dihedral angles of every frame, their periodic histogram

Everything here requires HIP tensors; there is no CPU path.
"""
import ctypes as C
import math
import weakref

import numpy as np
import torch
from array import array as _array

from . import _lib
from . import _torch_ops
from ._lib import MdgPairTerm, MdgTerms, MdgTrajParams, check, ptr, stream_ptr, require_gpu


# ----------------------------------------------------------------------------- neighbour lists
def build_mask(n_atoms, index_tuple=None, ex_pairs=None, device=None):
    """[N,N] uint8 selection equivalent to the reference's multiplicative masks
    (torchmd/topology.py:15-27 index_tuple product, :44-53 ex_pairs).  None when unrestricted."""
    if index_tuple is None and ex_pairs is None:
        return None
    keep = torch.ones(n_atoms, n_atoms, dtype=torch.bool)
    if index_tuple is not None:
        a = torch.as_tensor(list(index_tuple[0]), dtype=torch.long)
        b = torch.as_tensor(list(index_tuple[1]), dtype=torch.long)
        sel = torch.zeros(n_atoms, n_atoms, dtype=torch.bool)
        sel[a[:, None], b[None, :]] = True
        keep &= sel | sel.t()
    if ex_pairs is not None:
        ex = torch.as_tensor(ex_pairs, dtype=torch.long).reshape(-1, 2).cpu()
        keep[ex[:, 0], ex[:, 1]] = False
        keep[ex[:, 1], ex[:, 0]] = False
    return keep.to(torch.uint8).contiguous().to(device)


def estimate_max_nbr(n_atoms, cell_struct, cutoff):
    h = cell_struct.h
    vol = abs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6])
              + h[2] * (h[3] * h[7] - h[4] * h[6]))
    est = n_atoms / max(vol, 1e-30) * 4.0 / 3.0 * math.pi * cutoff ** 3
    cap = int(est * 1.5) + 16
    cap = (cap + 7) // 8 * 8
    return max(8, min(max(n_atoms - 1, 1), cap))


class EllList:
    """Immutable device snapshot of one neighbour list (layout: include/mdgrad_hip.h K1)."""

    def __init__(self, n_atoms, max_nbr, col, shift, cnt, cell_struct, cutoff, mask):
        self.n_atoms, self.max_nbr = n_atoms, max_nbr
        self.col, self.shift, self.cnt = col, shift, cnt
        self.cell_struct, self.cutoff, self.mask = cell_struct, cutoff, mask
        self._half = None

    def half_list(self, with_edge_id=False):
        """(nbr int64 [P,2], offsets f32 [P,3][, edge_id int32 [N,max_nbr]]) in the reference's
        lexicographic i<j order (torchmd/topology.py:68-73).  One host sync (P)."""
        if self._half is None or (with_edge_id and self._half[2] is None):
            lib = _lib.load()
            dev = self.col.device
            row_base = torch.empty(self.n_atoms + 1, dtype=torch.int32, device=dev)
            st = stream_ptr(dev)
            check(lib.mdg_nbr_half_count(ptr(self.col), ptr(self.cnt), self.n_atoms, self.max_nbr,
                                         ptr(row_base), st), "mdg_nbr_half_count")
            P = int(row_base[-1].item())
            nbr = torch.empty(P, 2, dtype=torch.int64, device=dev)
            off = torch.empty(P, 3, dtype=torch.float32, device=dev)
            eid = (torch.zeros(self.n_atoms, self.max_nbr, dtype=torch.int32, device=dev)
                   if with_edge_id else None)
            check(lib.mdg_nbr_half_fill(ptr(self.col), ptr(self.shift), ptr(self.cnt), ptr(row_base),
                                        self.n_atoms, self.max_nbr, ptr(nbr), ptr(off), ptr(eid), st),
                  "mdg_nbr_half_fill")
            self._half = (nbr, off, eid)
        return self._half if with_edge_id else self._half[:2]

    def half_list_padded(self, capacity, pad_offset, need):
        """Fixed-capacity half list for HIP-graph capture (no host sync): (nbr [capacity,2] with (-1,-1)
        padding rows, offsets [capacity,3] with (pad_offset,0,0) there, edge_id, n_valid int32[1]).
        need: persistent int32 buffer, need[1] <- max(need[1], pairs) when the capacity is exceeded."""
        lib = _lib.load()
        dev = self.col.device
        row_base = torch.empty(self.n_atoms + 1, dtype=torch.int32, device=dev)
        st = stream_ptr(dev)
        check(lib.mdg_nbr_half_count(ptr(self.col), ptr(self.cnt), self.n_atoms, self.max_nbr, ptr(row_base), st),
              "mdg_nbr_half_count")
        nbr = torch.empty(capacity, 2, dtype=torch.int64, device=dev)
        off = torch.empty(capacity, 3, dtype=torch.float32, device=dev)
        eid = torch.zeros(self.n_atoms, self.max_nbr, dtype=torch.int32, device=dev)
        n_valid = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.mdg_nbr_half_fill_padded(ptr(self.col), ptr(self.shift), ptr(self.cnt), ptr(row_base),
                                           self.n_atoms, self.max_nbr, int(capacity), float(pad_offset), ptr(nbr),
                                           ptr(off), ptr(eid), ptr(n_valid), C.c_void_p(need.data_ptr() + 4), st),
              "mdg_nbr_half_fill_padded")
        return nbr, off, eid, n_valid


def _use_cell_list(n_atoms, cs, cutoff):
    """The cell list pays from 512 atoms, in an orthorhombic box of at least three bins per side -- bins as the
    builder counts them (csrc/nbr.hip make_bins: wider than the cutoff by a margin)."""
    if not cs.diag or n_atoms < 512:
        return False
    return bool(_lib.load().mdg_nbr_cell_bins(C.byref(cs), float(cutoff), None))


def build_ell(xyz, cell_struct, cutoff, mask=None, max_nbr=None, method="auto", group=None, need=None):
    """Neighbour list of one frame xyz[N,3] (replaces generate_nbr_list).  method: auto|dense|cell.
    group: atoms per independent replica when xyz stacks several replicas of one system (pairs stay
    inside a group; mask is [group, group]).
    need: persistent int32[2] buffer => fixed-capacity mode for HIP-graph capture: one pass with the
    given max_nbr, no host sync; need[0] <- max(need[0], longest row) when a row does not fit."""
    require_gpu(xyz, "xyz")
    lib = _lib.load()
    xyz = xyz.detach().contiguous()
    N, dev = xyz.shape[0], xyz.device
    cutoff = float(cutoff)
    grouped = group is not None and group != N
    Ng = group if grouped else N
    cap = estimate_max_nbr(Ng, cell_struct, cutoff) if max_nbr is None else int(max_nbr)
    use_cell = method == "cell" or (method == "auto" and _use_cell_list(Ng, cell_struct, cutoff))
    st = stream_ptr(dev)
    while True:
        if need is not None and max_nbr is None:
            raise ValueError("build_ell: fixed-capacity mode needs max_nbr")
        col = torch.empty(N, cap, dtype=torch.int32, device=dev)
        shift = torch.empty(N, cap, dtype=torch.int32, device=dev)
        cnt = torch.empty(N, dtype=torch.int32, device=dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev) if need is None else need
        if use_cell and cap <= 512:                 # (the cell-list kernel sorts rows of up to 512 entries in LDS)
            ns = lib.mdg_nbr_cell_scratch_groups(N, Ng, C.byref(cell_struct), cutoff)
            scratch = torch.empty(int(ns), dtype=torch.int32, device=dev)
            check(lib.mdg_nbr_build_cell_groups(ptr(xyz), N, Ng, C.byref(cell_struct), cutoff, ptr(mask), ptr(col),
                                                ptr(shift), ptr(cnt), cap, ptr(overflow), ptr(scratch), st),
                  "mdg_nbr_build_cell")
        else:
            check(lib.mdg_nbr_build_dense_groups(ptr(xyz), N, Ng, C.byref(cell_struct), cutoff, ptr(mask), ptr(col),
                                                 ptr(shift), ptr(cnt), cap, ptr(overflow), st),
                  "mdg_nbr_build_dense")
        if cap >= Ng - 1 or need is not None:
            break                                   # cannot overflow / checked later by the caller
        longest = int(overflow.item())              # longest row the builder met (one host sync)
        if longest <= cap:
            break
        cap = min(Ng - 1, (longest + 15) // 8 * 8)  # grow to fit and rebuild
    return EllList(N, cap, col, shift, cnt, cell_struct, cutoff, mask)


# ----------------------------------------------------------------------------- pair potentials
MDG_PAIR_TABLE = 4


def make_term(desc, cutoff, theta_off=0, n_theta=0, mask=None):
    t = MdgPairTerm()
    t.kind = desc["kind"]
    t.p, t.q, t.c = desc.get("p", 0), desc.get("q", 0), desc.get("c", 0.0)
    t.a, t.phi = desc.get("a", 0.0), desc.get("phi", 0.0)
    t.cutoff = float(cutoff)
    t.theta_off, t.n_theta = theta_off, n_theta
    t.mask = mask.data_ptr() if mask is not None else None
    return t


def pair_eval(ell, xyz, term, theta, w=None, energy=True, grad=True, into=None, scale=1.0, theta_grads=True):
    """One launch of mdg_pair_eval_ell.  Returns dict with the requested outputs.  `into` = (grad_buffer, hw_buffer or
    None): the per-atom outputs are ADDED onto those buffers, times `scale` (F += -dU/dx of a Stack member without extra
    launches); without `into`, `scale` multiplies the fresh outputs.  theta_grads=False: dU/dtheta and d(w.dU/dx)/dtheta are
    not wanted (a force-only evaluation then skips the scalar reduction launch)."""
    lib = _lib.load()
    require_gpu(xyz, "xyz")
    if theta is not None and theta.numel():
        require_gpu(theta, "theta")
    if w is not None:
        require_gpu(w, "w")
    if xyz.shape != (ell.n_atoms, 3):
        raise ValueError("mdgrad_amd: xyz must be [%d, 3] (got %s)" % (ell.n_atoms, tuple(xyz.shape)))
    dev = xyz.device
    N, K = ell.n_atoms, term.n_theta
    out = {}
    e = torch.empty(1, device=dev) if energy else None
    acc = into is not None
    g = (into[0] if acc else torch.empty(N, 3, device=dev)) if grad else None
    gth = torch.empty(K, device=dev) if (grad and K and theta_grads) else None
    hw = (into[1] if acc else torch.empty(N, 3, device=dev)) if w is not None else None
    gthw = torch.empty(K, device=dev) if (w is not None and K and theta_grads) else None
    partial = torch.empty(int(lib.mdg_pair_partial_size(N)), device=dev)
    recheck = bool(getattr(ell, "verlet", False))        # a list searched with a skin: exact cutoff test per pair
    if acc or scale != 1.0 or recheck:
        check(lib.mdg_pair_eval_ell_into(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift),
                                         ptr(ell.cnt), ell.max_nbr, C.byref(term), ptr(theta), ptr(w), ptr(e),
                                         ptr(g), ptr(gth), ptr(hw), ptr(gthw), ptr(partial), float(scale),
                                         int(acc) | (2 if recheck else 0), stream_ptr(dev)), "mdg_pair_eval_ell_into")
    else:
        check(lib.mdg_pair_eval_ell(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift),
                                    ptr(ell.cnt), ell.max_nbr, C.byref(term), ptr(theta), ptr(w), ptr(e),
                                    ptr(g), ptr(gth), ptr(hw), ptr(gthw), ptr(partial), stream_ptr(dev)),
              "mdg_pair_eval_ell")
    out.update(energy=e, grad=g, gtheta=gth, hw=hw, gtheta_w=gthw)
    return out


class PairGradFn(torch.autograd.Function):
    """(dU/dx, dU/dtheta) as a differentiable op; backward = Hessian-vector product and the
    mixed theta-derivative (the second autograd pass of torchmd/sovlers.py:229-233).
    Second derivatives w.r.t. theta alone (a cotangent on dU/dtheta) are not supported."""

    @staticmethod
    def forward(ctx, xyz, theta, ell, term, cache):
        ctx.ell, ctx.term = ell, term
        ctx.save_for_backward(xyz, theta)
        ctx.set_materialize_grads(False)        # an unused dU/dtheta output arrives as None, not as zeros: no device read
        if cache is not None:
            g, gth = cache
        else:
            o = pair_eval(ell, xyz, term, theta, energy=False, grad=True)
            g, gth = o["grad"], o["gtheta"]
        if gth is None:
            gth = xyz.new_zeros(0)
        return g, gth

    @staticmethod
    def backward(ctx, wg, wgth):
        xyz, theta = ctx.saved_tensors
        if wgth is not None and wgth.numel():
            raise NotImplementedError("mdgrad_amd: second derivatives of a pair energy w.r.t. its parameters alone "
                                      "(a cotangent on dU/dtheta) are not provided by the HIP pair kernels")
        if wg is None:
            return None, None, None, None, None
        w = wg.detach().contiguous()
        o = pair_eval(ctx.ell, xyz, ctx.term, theta, w=w, energy=False, grad=False)
        gthw = o["gtheta_w"] if o["gtheta_w"] is not None else None
        return o["hw"], gthw, None, None, None


class PairEnergyFn(torch.autograd.Function):
    """U(x, theta) = sum_pairs phi(r)  (torchmd/interface.py:298-300), differentiable twice."""

    @staticmethod
    def forward(ctx, xyz, theta, ell, term):
        o = pair_eval(ell, xyz, term, theta, energy=True, grad=True)
        ctx.ell, ctx.term = ell, term
        ctx.cache = (o["grad"], o["gtheta"])
        ctx.save_for_backward(xyz, theta)
        return o["energy"].reshape(())

    @staticmethod
    def backward(ctx, gU):
        xyz, theta = ctx.saved_tensors
        g, gth = PairGradFn.apply(xyz, theta, ctx.ell, ctx.term, ctx.cache)
        gtheta = gU * gth if theta.numel() else None
        return gU * g, gtheta, None, None


# ----------------------------------------------------------------------------- bonded terms (f4)
class BondedTable:
    """Static topology table of a bonded term for mdg_bonded_eval (csrc/bonded.hip): `top` [n_terms, 2 | 3] atom indices
    (torchmd/interface.py:406-510) as int32 on the device, plus the incidence list of every atom -- entries
    4 * term + role, ascending per atom -- built once on the host.  Negative indices count from the end; indices outside
    [0, n_atoms) and rows that name an atom twice (a bond i == j, a repeated atom in an angle) are refused; duplicate rows are
    kept, each a term of its own."""

    def __init__(self, kind, top, n_atoms, cell_len, k, x0, device):
        import numpy as np
        width = 2 if kind == _lib.BONDED_BOND else 3
        t = torch.as_tensor(top).detach().cpu().numpy().astype(np.int64).reshape(-1, width)
        t = np.where(t < 0, t + n_atoms, t)                      # (the reference's xyz[top] accepts negative indices)
        if t.size and (t.min() < 0 or t.max() >= n_atoms):
            raise ValueError("mdgrad_amd: bonded topology refers to atoms outside [0, %d)" % n_atoms)
        s = np.sort(t, axis=1)
        if t.size and bool((s[:, 1:] == s[:, :-1]).any()):
            raise ValueError("mdgrad_amd: a bonded row names the same atom twice")
        self.kind, self.n_atoms, self.n_terms = int(kind), int(n_atoms), int(t.shape[0])
        atoms = t.reshape(-1)
        codes = (4 * np.repeat(np.arange(self.n_terms), width) + np.tile(np.arange(width), self.n_terms)).astype(np.int64)
        order = np.lexsort((codes, atoms))                       # by atom, then by (term, role)
        ptr_ = np.zeros(n_atoms + 1, dtype=np.int64)
        np.add.at(ptr_, atoms + 1, 1)
        i32 = dict(dtype=torch.int32, device=device)
        self.top = torch.as_tensor(t.astype(np.int32).copy(), **i32).contiguous()
        self.inc_ptr = torch.as_tensor(np.cumsum(ptr_).astype(np.int32), **i32)
        self.inc = torch.as_tensor(codes[order].astype(np.int32), **i32)
        self.cell_len = (C.c_float * 3)(*[float(x) for x in cell_len])
        self.k, self.x0 = float(k), float(x0)


def bonded_eval(tab, xyz, w=None, energy=False, grad=True, into=None, scale=1.0):
    """One launch of mdg_bonded_eval -> dict(e_atom, grad, hw).  `into` = (grad buffer, hw buffer or None): the per-atom
    outputs are ADDED onto them, times `scale` (a Stack member's force without extra launches)."""
    lib = _lib.load()
    require_gpu(xyz, "xyz")
    if xyz.shape != (tab.n_atoms, 3):
        raise ValueError("mdgrad_amd: xyz must be [%d, 3] (got %s)" % (tab.n_atoms, tuple(xyz.shape)))
    xyz = xyz.contiguous()
    dev, N = xyz.device, tab.n_atoms
    acc = into is not None
    e = torch.empty(N, device=dev) if energy else None
    g = (into[0] if acc else torch.empty(N, 3, device=dev)) if grad else None
    hw = None
    if w is not None:
        require_gpu(w, "w")
        if w.shape != (N, 3):
            raise ValueError("mdgrad_amd: w must be [%d, 3] (got %s)" % (N, tuple(w.shape)))
        w = w.contiguous()
        hw = into[1] if acc else torch.empty(N, 3, device=dev)
    check(lib.mdg_bonded_eval(ptr(xyz), N, tab.cell_len, tab.kind, ptr(tab.top), tab.n_terms, tab.k, tab.x0, ptr(tab.inc_ptr),
                              ptr(tab.inc), ptr(w), ptr(e), ptr(g), ptr(hw), float(scale), int(acc), stream_ptr(dev)),
          "mdg_bonded_eval")
    return dict(e_atom=e, grad=g, hw=hw)


class BondedGradFn(torch.autograd.Function):
    """dU/dx of a bonded term as a differentiable op; backward = the Hessian-vector product (the second autograd pass of
    torchmd/sovlers.py:229-233)."""

    @staticmethod
    def forward(ctx, xyz, tab, cache):
        ctx.tab = tab
        ctx.save_for_backward(xyz)
        return cache if cache is not None else bonded_eval(tab, xyz)["grad"]

    @staticmethod
    def backward(ctx, wg):
        (xyz,) = ctx.saved_tensors
        return bonded_eval(ctx.tab, xyz, w=wg.detach().contiguous(), grad=False)["hw"], None, None


class BondedEnergyFn(torch.autograd.Function):
    """U(x) of a bonded term (torchmd/interface.py:447-455, 496-508), differentiable twice."""

    @staticmethod
    def forward(ctx, xyz, tab):
        o = bonded_eval(tab, xyz, energy=True, grad=True)
        ctx.tab, ctx.cache = tab, o["grad"]
        ctx.save_for_backward(xyz)
        return o["e_atom"].sum()

    @staticmethod
    def backward(ctx, gU):
        (xyz,) = ctx.saved_tensors
        return gU * BondedGradFn.apply(xyz, ctx.tab, ctx.cache), None


# ----------------------------------------------------------------------------- terms with parameters: one autograd pair
# Every term below (dihedral, Coulomb, Ewald, Ewald exclusions, Stillinger-Weber, Sutton-Chen, Tersoff) differentiates through this
# pair.  PairGradFn / PairEnergyFn stay on their own (the empty-theta case, two C entry points), and so do BondedGradFn /
# BondedEnergyFn (no parameters, ten lines).  A `term` holds what the two evaluations of its kernel family need and has
#     first_order(xyz, energy) -> (U or None, dU/dx, packed)    packed: the flat dU/dparams, in the order of `params`
#     second_order(xyz, w)     -> (H w, packed_w)               packed_w: the flat d(w.dU/dx)/dparams
#     noun                                                      what the NotImplementedError below calls the parameter gradient
def _split(packed, params):
    """The flat `packed` as one tensor per parameter, in the parameter's shape."""
    out, pos = [], 0
    for p in params:
        out.append(packed[pos:pos + p.numel()].reshape(p.shape))
        pos += p.numel()
    return out


class TermGradFn(torch.autograd.Function):
    """(dU/dx, packed dU/dparams) of a term as a differentiable op; backward = the Hessian-vector product and the mixed
    derivative d(w.dU/dx)/dparams (the second autograd pass of torchmd/sovlers.py:229-233).  A cotangent on the parameter
    gradient (second derivatives with respect to the parameters alone, or dU/dparams differentiated in x) is not provided."""

    @staticmethod
    def forward(ctx, xyz, term, cache, *params):
        ctx.term = term
        ctx.save_for_backward(xyz, *params)
        ctx.set_materialize_grads(False)        # an unused output arrives as None, not as zeros: no device read
        if cache is None:
            cache = term.first_order(xyz, energy=False)[1:]
        return cache

    @staticmethod
    def backward(ctx, wg, wpacked):
        xyz, *params = ctx.saved_tensors
        if wpacked is not None:
            raise NotImplementedError("mdgrad_amd: derivatives of %s (a cotangent on it) are not provided by the HIP kernels"
                                      % ctx.term.noun)
        if wg is None:
            return (None,) * (3 + len(params))
        hw, packed_w = ctx.term.second_order(xyz, wg.detach().contiguous())
        return (hw, None, None) + tuple(_split(packed_w, params))


class TermEnergyFn(torch.autograd.Function):
    """U(x, *params) of a term, differentiable twice in x and once in the parameters."""

    @staticmethod
    def forward(ctx, xyz, term, *params):
        e, g, packed = term.first_order(xyz, energy=True)
        ctx.term, ctx.cache = term, (g, packed)
        ctx.save_for_backward(xyz, *params)
        return e.reshape(())

    @staticmethod
    def backward(ctx, gU):
        xyz, *params = ctx.saved_tensors
        g, packed = TermGradFn.apply(xyz, ctx.term, ctx.cache, *params)
        return (gU * g, None) + tuple(gU * t for t in _split(packed, params))


def _eval_prologue(N, xyz, w, energy, grad, into, want_aux, aux_shape, q_atom=None):
    """The common opening of coulomb_eval, sw_eval, eam_eval, tersoff_eval, ewald_eval and ewald_excl_eval: the device and shape checks
    and the outputs -- energy [1], grad / hw [N, 3] (the buffers of `into` when given) and the auxiliary per-atom output of
    `aux_shape` when wanted: without `w` the first-order one, with `w` its directional derivative.  Returns
    (xyz, w, e, g, hw, aux, aux_w, acc).  (bonded_eval and dihedral_eval have per-atom energies and no per-atom auxiliary
    output; they keep their own few lines.)"""
    require_gpu(xyz, "xyz")
    if q_atom is not None:
        require_gpu(q_atom, "q_atom")
    if xyz.shape != (N, 3):
        raise ValueError("mdgrad_amd: xyz must be [%d, 3] (got %s)" % (N, tuple(xyz.shape)))
    if q_atom is not None and q_atom.shape != (N,):
        raise ValueError("mdgrad_amd: q_atom must be [%d] (got %s)" % (N, tuple(q_atom.shape)))
    xyz = xyz.contiguous()
    dev = xyz.device
    acc = into is not None
    e = torch.empty(1, device=dev) if energy else None
    g = (into[0] if acc else torch.empty(N, 3, device=dev)) if grad else None
    hw = aux = aux_w = None
    if w is not None:
        require_gpu(w, "w")
        if w.shape != (N, 3):
            raise ValueError("mdgrad_amd: w must be [%d, 3] (got %s)" % (N, tuple(w.shape)))
        w = w.contiguous()
        hw = into[1] if acc else torch.empty(N, 3, device=dev)
        aux_w = torch.empty(aux_shape, device=dev) if want_aux else None
    elif want_aux:
        aux = torch.empty(aux_shape, device=dev)
    return xyz, w, e, g, hw, aux, aux_w, acc


def _check_theta(theta):
    """`theta`, when given, is the contiguous device float [3] the SW / EAM / Tersoff kernels read their three parameters from."""
    if theta is not None:
        require_gpu(theta, "theta")
        if theta.shape != (3,) or not theta.is_contiguous():
            raise ValueError("mdgrad_amd: theta must be a contiguous [3] tensor (got %s)" % (tuple(theta.shape),))


def _list_flags(acc, ell):
    """The flags word of the list kernels: 1 = add onto the output buffers, 2 = the list was searched with a skin
    (ops.VerletList), so the kernel applies the exact cutoff test per pair."""
    return int(acc) | (2 if getattr(ell, "verlet", False) else 0)


# ----------------------------------------------------------------------------- dihedral terms (K19)
class DihedralTable:
    """Static table of dihedral quadruples for the kernels of csrc/dihedral.hip: `top` [n_terms, 4] rows (i, j, k, l) as
    int32 on the device, the optional per-term `types` in [0, n_types), and the incidence list of every atom -- entries
    4 * term + role, ascending per atom -- built once on the host.  Indices outside [0, n_atoms) and rows that name an atom
    twice are refused."""

    def __init__(self, top, n_atoms, cell_len, device, types=None, n_types=1):
        import numpy as np
        t = torch.as_tensor(top).detach().cpu().numpy().astype(np.int64).reshape(-1, 4)
        if t.size and (t.min() < 0 or t.max() >= n_atoms):
            raise ValueError("mdgrad_amd: dihedral topology refers to atoms outside [0, %d)" % n_atoms)
        s = np.sort(t, axis=1)
        if t.size and bool((s[:, 1:] == s[:, :-1]).any()):
            raise ValueError("mdgrad_amd: a dihedral row names the same atom twice")
        self.n_atoms, self.n_terms, self.n_types = int(n_atoms), int(t.shape[0]), int(n_types)
        if self.n_types < 1:
            raise ValueError("mdgrad_amd: a dihedral table needs at least one type")
        atoms = t.reshape(-1)
        codes = (4 * np.repeat(np.arange(self.n_terms), 4) + np.tile(np.arange(4), self.n_terms)).astype(np.int64)
        order = np.lexsort((codes, atoms))                       # by atom, then by (term, role)
        ptr_ = np.zeros(n_atoms + 1, dtype=np.int64)
        np.add.at(ptr_, atoms + 1, 1)
        i32 = dict(dtype=torch.int32, device=device)
        self.top = torch.as_tensor(t.astype(np.int32).copy(), **i32).contiguous()
        self.inc_ptr = torch.as_tensor(np.cumsum(ptr_).astype(np.int32), **i32)
        self.inc = torch.as_tensor(codes[order].astype(np.int32), **i32)
        self.types = None
        if types is not None:
            ty = torch.as_tensor(types).detach().cpu().numpy().astype(np.int64).reshape(-1)
            if ty.shape[0] != self.n_terms:
                raise ValueError("mdgrad_amd: dihedral types must hold one entry per term (%d), got %d" % (self.n_terms, ty.shape[0]))
            if ty.size and (ty.min() < 0 or ty.max() >= self.n_types):
                raise ValueError("mdgrad_amd: dihedral types must lie in [0, %d)" % self.n_types)
            self.types = torch.as_tensor(ty.astype(np.int32), **i32)
        self.cell_len = (C.c_float * 3)(*[float(x) for x in cell_len])


def _dihedral_coeff(tab, coeff):
    require_gpu(coeff, "coeffs")
    if coeff.numel() != 5 * tab.n_types:
        raise ValueError("mdgrad_amd: coeffs must be [%d, 5] (got %s)" % (tab.n_types, tuple(coeff.shape)))
    return coeff.detach().contiguous()


def dihedral_eval(tab, xyz, coeff, w=None, energy=False, grad=True, into=None, scale=1.0, terms=False):
    """One launch of mdg_dihedral_eval -> dict(e_atom, grad, hw, c_term, cd_term).  `into` = (grad buffer, hw buffer or
    None): the per-atom outputs are ADDED onto them, times `scale`.  terms=True also returns cos phi of every term and, with
    `w`, its directional derivative (what dihedral_coeff_grad reduces to the parameter gradients)."""
    lib = _lib.load()
    require_gpu(xyz, "xyz")
    if xyz.shape != (tab.n_atoms, 3):
        raise ValueError("mdgrad_amd: xyz must be [%d, 3] (got %s)" % (tab.n_atoms, tuple(xyz.shape)))
    xyz = xyz.contiguous()
    coeff = _dihedral_coeff(tab, coeff)
    dev, N = xyz.device, tab.n_atoms
    acc = into is not None
    e = torch.empty(N, device=dev) if energy else None
    g = (into[0] if acc else torch.empty(N, 3, device=dev)) if grad else None
    hw = None
    if w is not None:
        require_gpu(w, "w")
        w = w.contiguous()
        hw = into[1] if acc else torch.empty(N, 3, device=dev)
    ct = torch.empty(tab.n_terms, device=dev) if terms else None
    cd = torch.empty(tab.n_terms, device=dev) if (terms and w is not None) else None
    check(lib.mdg_dihedral_eval(ptr(xyz), N, tab.cell_len, ptr(tab.top), tab.n_terms, ptr(coeff), ptr(tab.types), tab.n_types,
                                ptr(tab.inc_ptr), ptr(tab.inc), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(ct), ptr(cd), float(scale),
                                int(acc), stream_ptr(dev)), "mdg_dihedral_eval")
    return dict(e_atom=e, grad=g, hw=hw, c_term=ct, cd_term=cd)


def dihedral_coeff_grad(tab, c_term, cd_term=None, want_u=True):
    """(dU/dcoeffs, d(w.dU/dx)/dcoeffs), each [n_types, 5] or None, from the per-term outputs of dihedral_eval: one launch,
    fixed summation order."""
    lib = _lib.load()
    dev = c_term.device
    gu = torch.empty(tab.n_types, 5, device=dev) if want_u else None
    gw = torch.empty(tab.n_types, 5, device=dev) if cd_term is not None else None
    check(lib.mdg_dihedral_coeff_grad(ptr(c_term), ptr(cd_term), ptr(tab.types), tab.n_terms, tab.n_types, ptr(gu), ptr(gw),
                                      stream_ptr(dev)), "mdg_dihedral_coeff_grad")
    return gu, gw


class DihedralTerm:
    """The torsion term for TermEnergyFn: U(x, coeffs) = sum_terms sum_m coeffs[type, m] cos^m phi (csrc/dihedral.hip) on a
    DihedralTable."""

    noun = "dU/dcoeffs of the torsion term"

    def __init__(self, tab, coeff):
        self.tab, self.coeff = tab, coeff

    def first_order(self, xyz, energy):
        o = dihedral_eval(self.tab, xyz, self.coeff, energy=energy, grad=True, terms=True)
        return (o["e_atom"].sum() if energy else None), o["grad"], dihedral_coeff_grad(self.tab, o["c_term"])[0].reshape(-1)

    def second_order(self, xyz, w):
        o = dihedral_eval(self.tab, xyz, self.coeff, w=w, grad=False, terms=True)
        return o["hw"], dihedral_coeff_grad(self.tab, o["c_term"], o["cd_term"], want_u=False)[1].reshape(-1)


class DihedralPhiFn(torch.autograd.Function):
    """(phi, cos phi) [F, n_terms] of every term of a DihedralTable in every frame of xyz [F, N, 3] (mdg_dihedral_phi_fwd /
    _bwd), differentiable once.  Skipped (degenerate) terms give 0 in both with zero gradient."""

    @staticmethod
    def forward(ctx, xyz, tab):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        if xyz.dim() != 3 or tuple(xyz.shape[1:]) != (tab.n_atoms, 3):
            raise ValueError("mdgrad_amd: xyz must be [F, %d, 3] (got %s)" % (tab.n_atoms, tuple(xyz.shape)))
        x3 = xyz.detach().contiguous()
        F, dev = x3.shape[0], x3.device
        phi, cos = torch.empty(F, tab.n_terms, device=dev), torch.empty(F, tab.n_terms, device=dev)
        if F:
            check(lib.mdg_dihedral_phi_fwd(ptr(x3), F, tab.n_atoms, tab.cell_len, ptr(tab.top), tab.n_terms, ptr(phi), ptr(cos),
                                           stream_ptr(dev)), "mdg_dihedral_phi_fwd")
        ctx.tab = tab
        ctx.save_for_backward(x3)
        ctx.set_materialize_grads(False)
        return phi, cos

    @staticmethod
    def backward(ctx, g_phi, g_cos):
        (x3,) = ctx.saved_tensors
        tab = ctx.tab
        if (g_phi is None and g_cos is None) or x3.shape[0] == 0:
            return torch.zeros_like(x3), None
        gp = None if g_phi is None else g_phi.detach().to(torch.float32).contiguous()
        gc = None if g_cos is None else g_cos.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x3)
        check(_lib.load().mdg_dihedral_phi_bwd(ptr(x3), x3.shape[0], tab.n_atoms, tab.cell_len, ptr(tab.top), tab.n_terms,
                                               ptr(tab.inc_ptr), ptr(tab.inc), ptr(gp), ptr(gc), ptr(gx), stream_ptr(x3.device)),
              "mdg_dihedral_phi_bwd")
        return gx, None


class DihedralHistFn(torch.autograd.Function):
    """raw[b] = sum exp(-1/2 (wrap(phi - mu_b) / width)^2) over all entries of phi, mu_b = -pi + (b + 1/2) 2 pi / nbins
    (mdg_dihedral_hist_fwd / _bwd).  `cos` (the cosines that came with phi) only marks the skipped terms; the gradient goes
    to phi."""

    @staticmethod
    def forward(ctx, phi, cos, nbins, width):
        lib = _lib.load()
        require_gpu(phi, "phi")
        p = phi.detach().contiguous()
        c = None if cos is None else cos.detach().contiguous()
        dev, n = p.device, p.numel()
        raw = torch.empty(int(nbins), device=dev)
        scratch = torch.empty(int(lib.mdg_dihedral_hist_scratch(n, int(nbins))), dtype=torch.int64, device=dev)
        check(lib.mdg_dihedral_hist_fwd(ptr(p), ptr(c), n, int(nbins), float(width), ptr(raw), ptr(scratch), stream_ptr(dev)),
              "mdg_dihedral_hist_fwd")
        ctx.args = (int(nbins), float(width), c is not None)
        ctx.save_for_backward(*((p, c) if c is not None else (p,)))
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        nbins, width, has_cos = ctx.args
        p = ctx.saved_tensors[0]
        c = ctx.saved_tensors[1] if has_cos else None
        gr = g_raw.detach().to(torch.float32).contiguous()
        gp = torch.empty_like(p)
        check(_lib.load().mdg_dihedral_hist_bwd(ptr(p), ptr(c), p.numel(), nbins, width, ptr(gr), ptr(gp), stream_ptr(p.device)),
              "mdg_dihedral_hist_bwd")
        return gp, None, None, None


# ----------------------------------------------------------------------------- Coulomb sum with per-atom charges (K20)
COULOMB_SHIFTS = ("none", "potential", "force")


def coulomb_consts(cutoff, alpha=0.0, shift="force", conversion=1.0, self_energy=True):
    """MdgCoulombConsts of the damped shifted-force sum, in double: c0, c1 make psi ("potential", "force") and psi' ("force")
    vanish at the cutoff; self_s = c0 / 2 + alpha / sqrt(pi) is the self term (0 with self_energy=False)."""
    if shift not in COULOMB_SHIFTS:
        raise ValueError("mdgrad_amd: shift must be one of %s (got %r)" % (COULOMB_SHIFTS, shift))
    alpha, rc = float(alpha), float(cutoff)
    if not alpha >= 0.0:
        raise ValueError("mdgrad_amd: alpha must be >= 0 (got %r)" % alpha)
    if not rc > 0.0:
        raise ValueError("mdgrad_amd: the cutoff must be positive (got %r)" % rc)
    k = _lib.MdgCoulombConsts()
    k.alpha, k.rc, k.alpha2, k.conversion = alpha, rc, alpha * alpha, float(conversion)
    k.g0 = 2.0 * alpha / math.sqrt(math.pi)
    E, G = math.erfc(alpha * rc), k.g0 * math.exp(-alpha * alpha * rc * rc)
    k.c0 = E / rc if shift != "none" else 0.0
    k.c1 = E / (rc * rc) + G / rc if shift == "force" else 0.0
    k.self_s = 0.5 * k.c0 + alpha / math.sqrt(math.pi) if self_energy else 0.0
    return k


def coulomb_eval(ell, xyz, q_atom, consts, w=None, energy=True, grad=True, into=None, scale=1.0, want_pot=False):
    """One launch of mdg_coulomb_eval -> dict(energy, grad, hw, pot, potw).  `into` = (grad buffer, hw buffer or None): the
    per-atom outputs are ADDED onto them, times `scale`, as in pair_eval.  want_pot: without `w` the per-atom potential
    pot_i = sum_j q_j psi(r_ij), with `w` potw_i = sum_j q_j psi'(r_ij) rhat_ij.(w_i - w_j) -- what coulomb_charge_grad reduces
    to the charge gradients.  A list searched with a skin (ops.VerletList) gets the exact cutoff test per pair."""
    lib = _lib.load()
    N = ell.n_atoms
    xyz, w, e, g, hw, pot, potw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_pot, (N,), q_atom)
    partial = torch.empty(int(lib.mdg_coulomb_partial_size(N)), device=xyz.device) if energy else None
    check(lib.mdg_coulomb_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                               ptr(q_atom), C.byref(consts), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pot), ptr(potw), ptr(partial),
                               float(scale), _list_flags(acc, ell), stream_ptr(xyz.device)), "mdg_coulomb_eval")
    return dict(energy=e, grad=g, hw=hw, pot=pot, potw=potw)


def coulomb_charge_grad(pot, slot, n_slots):
    """[n_slots] sums of the per-atom values `pot` [N] over the atoms of every charge slot, one launch in a fixed order:
    `slot` = int32 [group] types of one replica's atoms (slot(i) = slot[i % group]) or None (slot(i) = i % n_slots)."""
    lib = _lib.load()
    require_gpu(pot, "pot")
    pot = pot.contiguous()
    group = int(slot.numel()) if slot is not None else int(n_slots)
    out = torch.empty(int(n_slots), device=pot.device)
    check(lib.mdg_coulomb_charge_reduce(ptr(pot), ptr(slot), pot.numel(), group, int(n_slots), ptr(out), stream_ptr(pot.device)),
          "mdg_coulomb_charge_reduce")
    return out


class _ChargeTerm:
    """A point-charge term for TermEnergyFn: the per-atom charge buffer `q_atom` (charges[types] tiled over the replicas, kept
    current by CoulombPotentials) and the charge slots, around the term's one evaluation `_eval(xyz, **kw)` -- called like
    SWTerm._eval, returning the dict of coulomb_eval.  `pot_scale` is the factor that `pot` / `potw` of the term's kernel still
    owe (docs/KERNELS.md, "What the charge kernels' outputs carry"): the conversion where the kernel leaves it out, 1.0
    where its table holds it.  Nowhere else is that written.  What is a term's own -- a self term, a background term --
    it adds in `_own`."""

    pot_scale = 1.0

    def __init__(self, q_atom, slot, n_slots):
        self.q_atom, self.slot, self.n_slots = q_atom, slot, int(n_slots)

    def _eval(self, xyz, **kw):
        raise NotImplementedError

    def charge_grad(self, per_atom):
        """coulomb_charge_grad over the term's slots: nothing is scaled (force_vjp hands -pot_scale to its reduction)."""
        return coulomb_charge_grad(per_atom, self.slot, self.n_slots)

    def charge_grad_w(self, potw):
        """The per-atom `potw` (or `pot`) of `_eval` -> the [n_slots] charge gradient: reduced first, then times the owed
        scale (no multiplication where nothing is owed)."""
        gw = self.charge_grad(potw)
        return gw if self.pot_scale == 1.0 else gw * self.pot_scale

    def _own(self, e, pot):
        """(U, dU/dcharges [n_slots]) from the kernel's energy (None when not asked for) and per-atom `pot`."""
        return e, self.charge_grad_w(pot)

    def first_order(self, xyz, energy):
        o = self._eval(xyz, energy=energy, grad=True, want_pot=True)
        e, gq = self._own(o["energy"], o["pot"])
        return e, o["grad"], gq

    def second_order(self, xyz, w):
        o = self._eval(xyz, w=w, energy=False, grad=False, want_pot=True)
        return o["hw"], self.charge_grad_w(o["potw"])


class CoulombTerm(_ChargeTerm):
    """The damped shifted-force Coulomb sum (csrc/coulomb.hip): the list and the constants beside what _ChargeTerm holds."""

    noun = "dU/dcharges of the Coulomb term"

    def __init__(self, ell, consts, q_atom, slot, n_slots):
        super().__init__(q_atom, slot, n_slots)
        self.ell, self.consts, self.pot_scale = ell, consts, float(consts.conversion)

    def _eval(self, xyz, **kw):
        return coulomb_eval(self.ell, xyz, self.q_atom, self.consts, **kw)

    def _own(self, e, pot):
        """The self term -(2 self_s) q_i stands inside the conversion, which is applied per atom, before the reduction."""
        dq_atom = self.pot_scale * (pot - (2.0 * float(self.consts.self_s)) * self.q_atom)           # dU/dq_i
        return e, self.charge_grad(dq_atom)


# ----------------------------------------------------------------------------- Stillinger-Weber term (K23)
def sw_consts(epsilon, sigma, lam=21.0, a=1.80, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584, p=4, q=0):
    """MdgSWConsts: the fixed constants of the Stillinger-Weber form and host copies of (epsilon, sigma, lam) -- the kernel
    reads those three from a device buffer instead when sw_eval is given one."""
    epsilon, sigma, lam, a, gamma = float(epsilon), float(sigma), float(lam), float(a), float(gamma)
    if not epsilon > 0.0:
        raise ValueError("mdgrad_amd: epsilon must be positive (got %r)" % epsilon)
    if not sigma > 0.0:
        raise ValueError("mdgrad_amd: sigma must be positive (got %r)" % sigma)
    if not lam >= 0.0:
        raise ValueError("mdgrad_amd: lam must be >= 0 (got %r)" % lam)
    if not (a > 0.0 and gamma >= 0.0):
        raise ValueError("mdgrad_amd: a must be positive and gamma >= 0 (got %r, %r)" % (a, gamma))
    if int(p) != p or int(q) != q or not 0 <= int(q) < int(p) <= 12:
        raise ValueError("mdgrad_amd: the exponents must be integers with 0 <= q < p <= 12 (got p = %r, q = %r)" % (p, q))
    k = _lib.MdgSWConsts()
    k.epsilon, k.sigma, k.lam, k.a, k.gamma, k.cos0, k.A, k.B = epsilon, sigma, lam, a, gamma, float(cos0), float(A), float(B)
    k.p, k.q = int(p), int(q)
    return k


def sw_eval(ell, xyz, consts, theta=None, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False):
    """One launch of mdg_sw_eval -> dict(energy, grad, hw, pth, pthw).  `theta`: device float [3] = (epsilon, sigma, lam) that
    the kernel reads in place of the host copies in `consts`.  `into` = (grad buffer, hw buffer or None): the per-atom outputs
    are ADDED onto them, times `scale`, as in pair_eval.  want_theta: without `w` the per-atom parameter terms pth [N, 3] =
    d u_i / d(epsilon, sigma, lam), with `w` their directional derivatives pthw [N, 3] -- what sw_theta_sum reduces.  The list
    may have been searched with any radius >= a sigma (a skin, a kept cutoff): the kernel applies r < a sigma per pair."""
    lib = _lib.load()
    N = ell.n_atoms
    _check_theta(theta)
    xyz, w, e, g, hw, pth, pthw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (N, 3))
    partial = torch.empty(int(lib.mdg_sw_partial_size(N)), device=xyz.device) if energy else None
    check(lib.mdg_sw_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                          C.byref(consts), ptr(theta), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pth), ptr(pthw), ptr(partial),
                          float(scale), _list_flags(acc, ell), stream_ptr(xyz.device)), "mdg_sw_eval")
    return dict(energy=e, grad=g, hw=hw, pth=pth, pthw=pthw)


class _FlatOut:
    """A bare output buffer with ThetaAccum's fields, for GradJobs.run."""

    def __init__(self, n, device):
        self.flat, self.t, self.idx = torch.empty(n, device=device, dtype=torch.float32), None, None


def theta_sum(per_atom, alpha=1.0):
    """[P] = alpha * the sums over the atoms of the per-atom parameter terms [N, P] of sw_eval, eam_eval, tersoff_eval (P = 3)
    or tersoff_multi_eval (P = 2 S S + S, in (A, B, h) order) or sw_multi_eval (P = 2 S S + S S S, in (epsilon, sigma, lam)
    order), in the fixed order of mdg_grad_jobs."""
    out = _FlatOut(per_atom.shape[1], per_atom.device)
    jobs = GradJobs()
    jobs.colsum(0, per_atom)
    jobs.run(out, alpha=alpha, accumulate=False)
    return out.flat


sw_theta_sum = eam_theta_sum = tersoff_multi_theta_sum = theta_sum          # the names the terms were introduced with


class SWTerm:
    """The Stillinger-Weber term (csrc/sw.hip) for TermEnergyFn: the list, the constants and the device buffer
    (epsilon, sigma, lam), kept current by StillingerWeber."""

    noun = "dU/d(epsilon, sigma, lam) of the Stillinger-Weber term"

    def __init__(self, ell, consts, theta):
        self.ell, self.consts, self.theta = ell, consts, theta

    def _eval(self, xyz, **kw):
        return sw_eval(self.ell, xyz, self.consts, self.theta, **kw)

    def first_order(self, xyz, energy):
        o = self._eval(xyz, energy=energy, grad=True, want_theta=True)
        return o["energy"], o["grad"], theta_sum(o["pth"])

    def second_order(self, xyz, w):
        o = self._eval(xyz, w=w, energy=False, grad=False, want_theta=True)
        return o["hw"], theta_sum(o["pthw"])


# ----------------------------------------------------------------------------- Sutton-Chen embedded-atom term (K24)
EAM_SHIFTS = {"none": 0, "force": 1}


def eam_consts(epsilon, a, c, n, m, cutoff, shift="force"):
    """MdgEAMConsts: the constants (rc, n, m, shift) of the Sutton-Chen form and host copies of (epsilon, a, c) -- the kernels
    read those three from a device buffer instead when eam_eval is given one."""
    epsilon, a, c, cutoff = float(epsilon), float(a), float(c), float(cutoff)
    if not epsilon > 0.0:
        raise ValueError("mdgrad_amd: epsilon must be positive (got %r)" % epsilon)
    if not a > 0.0:
        raise ValueError("mdgrad_amd: the length a must be positive (got %r)" % a)
    if not c >= 0.0:
        raise ValueError("mdgrad_amd: c must be >= 0 (got %r)" % c)
    if int(n) != n or int(m) != m or not 1 <= int(m) < int(n) <= 16:
        raise ValueError("mdgrad_amd: the exponents must be integers with 1 <= m < n <= 16 (got n = %r, m = %r)" % (n, m))
    if not cutoff > 0.0:
        raise ValueError("mdgrad_amd: cutoff must be positive (got %r)" % cutoff)
    if shift not in EAM_SHIFTS:
        raise ValueError("mdgrad_amd: shift must be 'force' or 'none' (got %r)" % (shift,))
    k = _lib.MdgEAMConsts()
    k.epsilon, k.a, k.c, k.rc = epsilon, a, c, cutoff
    k.n, k.m, k.shift, k.pad_ = int(n), int(m), EAM_SHIFTS[shift], 0
    return k


def eam_eval(ell, xyz, consts, theta=None, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False, work=None):
    """One call of mdg_eam_eval (density pass, force pass) -> dict(energy, grad, hw, pth, pthw), argument for argument sw_eval
    with theta = device float [3] = (epsilon, a, c).  `work`: the [N, 4] float scratch of the density pass (a persistent buffer
    of the caller, so that a captured graph sees a fixed address); allocated here when None.  The list may have been searched
    with any radius >= rc (a skin): the kernels apply r < rc per pair."""
    lib = _lib.load()
    N, dev = ell.n_atoms, xyz.device
    _check_theta(theta)
    if work is None:
        work = torch.empty(N, 4, device=dev)
    else:
        require_gpu(work, "work")
        if work.shape != (N, 4) or not work.is_contiguous():
            raise ValueError("mdgrad_amd: work must be a contiguous [%d, 4] tensor (got %s)" % (N, tuple(work.shape)))
    xyz, w, e, g, hw, pth, pthw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (N, 3))
    partial = torch.empty(int(lib.mdg_eam_partial_size(N)), device=dev) if energy else None
    check(lib.mdg_eam_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                           C.byref(consts), ptr(theta), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pth), ptr(pthw), ptr(partial),
                           ptr(work), float(scale), _list_flags(acc, ell), stream_ptr(dev)), "mdg_eam_eval")
    return dict(energy=e, grad=g, hw=hw, pth=pth, pthw=pthw)


class EAMTerm(SWTerm):
    """The Sutton-Chen term (csrc/eam.hip) for TermEnergyFn: the list, the constants, the device buffer (epsilon, a, c) and
    the scratch of the density pass, kept current by SuttonChen; the two evaluations are SWTerm's."""

    noun = "dU/d(epsilon, a, c) of the Sutton-Chen term"

    def __init__(self, ell, consts, theta, work=None):
        self.ell, self.consts, self.theta, self.work = ell, consts, theta, work

    def _eval(self, xyz, **kw):
        return eam_eval(self.ell, xyz, self.consts, self.theta, work=self.work, **kw)


# ----------------------------------------------------------------------------- tabulated embedded-atom term (K27)
EAM_TABLE_MAX_SPECIES = 4
EAM_TABLE_NODES = (4, 4096)


def eam_table_consts(n_species, n_r, n_rho, r_min, cutoff, rho_min, rho_max, pin_cutoff=True):
    """MdgEAMTableConsts: the grids of the tabulated embedded-atom term -- n_r nodes on [r_min, cutoff] for phi and f, n_rho nodes
    on [rho_min, rho_max] for F."""
    S, n_r, n_rho = int(n_species), int(n_r), int(n_rho)
    r_min, cutoff, rho_min, rho_max = float(r_min), float(cutoff), float(rho_min), float(rho_max)
    if not 1 <= S <= EAM_TABLE_MAX_SPECIES:
        raise ValueError("mdgrad_amd: the number of species must lie in [1, %d] (got %d)" % (EAM_TABLE_MAX_SPECIES, S))
    lo, hi = EAM_TABLE_NODES
    if not (lo <= n_r <= hi and lo <= n_rho <= hi):
        raise ValueError("mdgrad_amd: the node counts must lie in [%d, %d] (got n_r = %d, n_rho = %d)" % (lo, hi, n_r, n_rho))
    if not (r_min >= 0.0 and cutoff > r_min):
        raise ValueError("mdgrad_amd: the r grid needs 0 <= r_min < cutoff (got %r, %r)" % (r_min, cutoff))
    if not rho_max > rho_min:
        raise ValueError("mdgrad_amd: the rho grid needs rho_min < rho_max (got %r, %r)" % (rho_min, rho_max))
    k = _lib.MdgEAMTableConsts()
    k.r_min, k.h_r, k.rc, k.rho_min, k.h_rho = r_min, (cutoff - r_min) / (n_r - 1), cutoff, rho_min, (rho_max - rho_min) / (n_rho - 1)
    k.n_species, k.n_r, k.n_rho, k.pin_cutoff = S, n_r, n_rho, int(bool(pin_cutoff))
    return k


def eam_table_size(consts):
    """The number of floats of the flat table image (pair, density, embed) on the grids of `consts`."""
    return int(_lib.load().mdg_eam_table_size(consts.n_species, consts.n_r, consts.n_rho))


def eam_table_fx_size(consts):
    """The number of int64 words of the fixed-point scratch of the table gradient on the grids of `consts`."""
    return int(_lib.load().mdg_eam_table_fx_size(consts.n_species, consts.n_r, consts.n_rho))


def eam_table_eval(ell, xyz, types, consts, tables, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False,
                   work=None, fx=None):
    """One call of mdg_eam_table_eval (density pass, force pass, and for the table gradient its prologue and finish kernels)
    -> dict(energy, grad, hw, gtab, gtabw), argument for argument eam_eval with `types` (device int32 [N], values in
    [0, n_species): not read here), `consts` (eam_table_consts) and `tables` (device float32, the flat node image in the order
    pair, density, embed) in place of the constants and theta.  want_theta: without `w` gtab = dU/dtables, with `w` gtabw =
    d(w.dU/dx)/dtables, flat in the layout of `tables`.  `work` [N, 4] and `fx` (int64 [eam_table_fx_size]): the scratch of the
    density pass and of the fixed-point scatter, persistent buffers of the caller (a captured graph sees fixed addresses);
    allocated here when None.  The list may have been searched with any radius >= cutoff (a skin)."""
    lib = _lib.load()
    N, dev = ell.n_atoms, xyz.device
    n_tab = eam_table_size(consts)
    require_gpu(types, "types", dtype=None)
    if types.shape != (N,) or types.dtype != torch.int32 or not types.is_contiguous():
        raise ValueError("mdgrad_amd: types must be a contiguous int32 [%d] tensor (got %s %s)" % (N, types.dtype, tuple(types.shape)))
    require_gpu(tables, "tables")
    if tables.shape != (n_tab,) or tables.dtype != torch.float32 or not tables.is_contiguous():
        raise ValueError("mdgrad_amd: tables must be a contiguous float32 [%d] tensor (got %s)" % (n_tab, tuple(tables.shape)))
    if work is None:
        work = torch.empty(N, 4, device=dev)
    else:
        require_gpu(work, "work")
        if work.shape != (N, 4) or not work.is_contiguous():
            raise ValueError("mdgrad_amd: work must be a contiguous [%d, 4] tensor (got %s)" % (N, tuple(work.shape)))
    if want_theta:
        if fx is None:
            fx = torch.empty(eam_table_fx_size(consts), dtype=torch.int64, device=dev)
        else:
            require_gpu(fx, "fx", dtype=None)
            if fx.shape != (eam_table_fx_size(consts),) or fx.dtype != torch.int64 or not fx.is_contiguous():
                raise ValueError("mdgrad_amd: fx must be a contiguous int64 [%d] tensor (got %s %s)"
                                 % (eam_table_fx_size(consts), fx.dtype, tuple(fx.shape)))
    xyz, w, e, g, hw, gtab, gtabw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (n_tab,))
    partial = torch.empty(int(lib.mdg_eam_table_partial_size(N)), device=dev) if energy else None
    check(lib.mdg_eam_table_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                                 ptr(types), C.byref(consts), ptr(tables), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(gtab), ptr(gtabw),
                                 ptr(partial), ptr(work), ptr(fx) if want_theta else None, float(scale), _list_flags(acc, ell),
                                 stream_ptr(dev)), "mdg_eam_table_eval")
    return dict(energy=e, grad=g, hw=hw, gtab=gtab, gtabw=gtabw)


class EAMTableTerm:
    """The tabulated embedded-atom term (csrc/eam_table.hip) for TermEnergyFn: the list, the species of the atoms, the grids,
    the device tables and the two scratch buffers, kept current by interface.EAM.  The parameter gradient comes back reduced
    (flat, in the layout of the tables); `select` = the (start, stop) ranges of it that belong to the trainable tensors, in
    their order, is what first_order / second_order return as "packed"."""

    noun = "dU/dnodes of the tabulated embedded-atom term"

    def __init__(self, ell, types, consts, tables, work=None, fx=None, select=()):
        self.ell, self.types, self.consts, self.tables, self.work, self.fx = ell, types, consts, tables, work, fx
        self.select = tuple(select)

    def _eval(self, xyz, **kw):
        return eam_table_eval(self.ell, xyz, self.types, self.consts, self.tables, work=self.work, fx=self.fx, **kw)

    def _packed(self, flat):
        if len(self.select) == 1:
            return flat[self.select[0][0]:self.select[0][1]]
        return torch.cat([flat[a:b] for a, b in self.select]) if self.select else flat[:0]

    def first_order(self, xyz, energy):
        o = self._eval(xyz, energy=energy, grad=True, want_theta=bool(self.select))
        return o["energy"], o["grad"], self._packed(o["gtab"]) if self.select else xyz.new_zeros(0)

    def second_order(self, xyz, w):
        o = self._eval(xyz, w=w, energy=False, grad=False, want_theta=bool(self.select))
        return o["hw"], self._packed(o["gtabw"]) if self.select else xyz.new_zeros(0)


# ----------------------------------------------------------------------------- Tersoff bond-order term (K25)
def tersoff_consts(A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3=0.0, m=3, gamma=1.0):
    """MdgTersoffConsts: the constants of the Tersoff form and host copies of (A, B, h) -- the kernels read those three from a
    device buffer instead when tersoff_eval is given one."""
    A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma = (float(v) for v in (A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma))
    if not (A > 0.0 and B > 0.0):
        raise ValueError("mdgrad_amd: A and B must be positive (got %r, %r)" % (A, B))
    if not (lam1 > 0.0 and lam2 > 0.0):
        raise ValueError("mdgrad_amd: lam1 and lam2 must be positive (got %r, %r)" % (lam1, lam2))
    if not (D > 0.0 and R > D):
        raise ValueError("mdgrad_amd: the cutoff needs D > 0 and R > D (got R = %r, D = %r)" % (R, D))
    if int(m) != m or int(m) not in (1, 3):
        raise ValueError("mdgrad_amd: m must be 1 or 3 (got %r)" % (m,))
    if not (n > 0.0 and beta >= 0.0):
        raise ValueError("mdgrad_amd: n must be positive and beta >= 0 (got %r, %r)" % (n, beta))
    if d == 0.0:
        raise ValueError("mdgrad_amd: d must not be 0")
    k = _lib.MdgTersoffConsts()
    k.A, k.B, k.lam1, k.lam2, k.beta, k.n, k.c, k.d, k.h, k.R, k.D, k.lam3, k.gamma = A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, gamma
    k.m, k.pad_ = int(m), 0
    return k


def tersoff_work_size(ell):
    """The number of floats of the bond-pass scratch for the list `ell` (4 per list slot)."""
    return int(_lib.load().mdg_tersoff_work_size(ell.n_atoms, ell.max_nbr))


def _bond_work(work, need, device):
    """The flat float32 scratch of a bond pass, at least `need` long: `work` validated, or a fresh buffer when it is None."""
    if work is None:
        return torch.empty(need, device=device)
    require_gpu(work, "work")
    if work.dim() != 1 or work.numel() < need or work.dtype != torch.float32 or not work.is_contiguous():
        raise ValueError("mdgrad_amd: work must be a contiguous flat float32 tensor of at least %d elements (got %s)"
                         % (need, tuple(work.shape)))
    return work


def tersoff_eval(ell, xyz, consts, theta=None, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False, work=None):
    """One call of mdg_tersoff_eval (bond pass, force pass) -> dict(energy, grad, hw, pth, pthw), argument for argument sw_eval
    with theta = device float [3] = (A, B, h).  `work`: the flat float scratch of the bond pass, at least tersoff_work_size(ell)
    long (a persistent buffer of the caller, so that a captured graph sees a fixed address); allocated here when None.  The
    list may have been searched with any radius >= R + D (a skin): the kernels apply r < R + D per pair."""
    lib = _lib.load()
    N, dev = ell.n_atoms, xyz.device
    _check_theta(theta)
    work = _bond_work(work, tersoff_work_size(ell), dev)
    xyz, w, e, g, hw, pth, pthw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (N, 3))
    partial = torch.empty(int(lib.mdg_tersoff_partial_size(N)), device=dev) if energy else None
    check(lib.mdg_tersoff_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                               C.byref(consts), ptr(theta), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pth), ptr(pthw), ptr(partial),
                               ptr(work), float(scale), _list_flags(acc, ell), stream_ptr(dev)), "mdg_tersoff_eval")
    return dict(energy=e, grad=g, hw=hw, pth=pth, pthw=pthw)


class TersoffTerm(EAMTerm):
    """The Tersoff term (csrc/tersoff.hip) for TermEnergyFn: the list, the constants, the device buffer (A, B, h) and the
    scratch of the bond pass, kept current by Tersoff; the two evaluations are SWTerm's."""

    noun = "dU/d(A, B, h) of the Tersoff term"

    def _eval(self, xyz, **kw):
        return tersoff_eval(self.ell, xyz, self.consts, self.theta, work=self.work, **kw)


# ----------------------------------------------------------------------------- multi-species Tersoff term (K26)
TERSOFF_MULTI_MAX_SPECIES = 4
TERSOFF_MULTI_PAIR = ("A", "B", "lam1", "lam2", "R", "D")
TERSOFF_MULTI_CENTRE = ("beta", "n", "c", "d", "h", "gamma")


def tersoff_multi_tables(pair, centre):
    """The table image mdg_tersoff_multi_eval reads, as a host float32 array of 8 S (S + 1) derived constants, from
    pair = dict of [S, S] arrays A, B, lam1, lam2, R, D (row = centre species, column = end species) and centre = dict of [S]
    arrays beta, n, c, d, h, gamma:
        pair entry   out[8 (a S + b) ...] = A, B, lam1, lam2, R, R - D, R + D, pi / (2 D)
        centre entry out[8 S S + 8 a ...] = h, beta, n, -1/(2n), d^2, gamma, gamma (c/d)^2, 2 gamma (c/d)^2 d^2
    Every entry is validated: A, B, lam1, lam2 > 0; D > 0; R > D; n > 0; beta >= 0; d != 0."""
    cen = {k: np.asarray(centre[k], dtype=np.float64).reshape(-1) for k in TERSOFF_MULTI_CENTRE}
    S = cen["h"].shape[0]
    if not 1 <= S <= TERSOFF_MULTI_MAX_SPECIES:
        raise ValueError("mdgrad_amd: the number of species must lie in [1, %d] (got %d)" % (TERSOFF_MULTI_MAX_SPECIES, S))
    for k, v in cen.items():
        if v.shape != (S,):
            raise ValueError("mdgrad_amd: centre[%r] must hold %d entries (got %s)" % (k, S, v.shape))
    pr = {}
    for k in TERSOFF_MULTI_PAIR:
        pr[k] = np.asarray(pair[k], dtype=np.float64)
        if pr[k].shape != (S, S):
            raise ValueError("mdgrad_amd: pair[%r] must be [%d, %d] (got %s)" % (k, S, S, pr[k].shape))
    for k in ("A", "B", "lam1", "lam2"):
        if not (pr[k] > 0.0).all():
            raise ValueError("mdgrad_amd: every entry of %s must be positive (got %r)" % (k, pr[k].tolist()))
    if not ((pr["D"] > 0.0) & (pr["R"] > pr["D"])).all():
        raise ValueError("mdgrad_amd: the cutoffs need D > 0 and R > D for every pair (got R = %r, D = %r)"
                         % (pr["R"].tolist(), pr["D"].tolist()))
    if not ((cen["n"] > 0.0) & (cen["beta"] >= 0.0)).all():
        raise ValueError("mdgrad_amd: n must be positive and beta >= 0 for every species (got %r, %r)"
                         % (cen["n"].tolist(), cen["beta"].tolist()))
    if (cen["d"] == 0.0).any():
        raise ValueError("mdgrad_amd: d must not be 0")
    out = np.empty(8 * S * (S + 1), dtype=np.float32)
    P = out[:8 * S * S].reshape(S, S, 8)
    for c, v in enumerate((pr["A"], pr["B"], pr["lam1"], pr["lam2"], pr["R"], pr["R"] - pr["D"], pr["R"] + pr["D"],
                           0.5 * np.pi / pr["D"])):
        P[:, :, c] = v
    Cn = out[8 * S * S:].reshape(S, 8)
    cd2 = (cen["c"] / cen["d"]) ** 2
    for c, v in enumerate((cen["h"], cen["beta"], cen["n"], -0.5 / cen["n"], cen["d"] ** 2, cen["gamma"], cen["gamma"] * cd2,
                           2.0 * cen["gamma"] * cd2 * cen["d"] ** 2)):
        Cn[:, c] = v
    return out


def tersoff_multi_work_size(ell):
    """The number of floats of the bond-pass scratch for the list `ell` (4 per list slot)."""
    return int(_lib.load().mdg_tersoff_multi_work_size(ell.n_atoms, ell.max_nbr))


def tersoff_multi_eval(ell, xyz, types, n_species, tables, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False,
                       work=None):
    """One call of mdg_tersoff_multi_eval (bond pass, force pass) -> dict(energy, grad, hw, pth, pthw), argument for argument
    tersoff_eval with `types` (device int32 [N], values in [0, n_species): not read here) and `tables` (device float32, the
    image of tersoff_multi_tables) in place of the constants and theta.  pth / pthw are [N, 2 S S + S]: row i holds
    d u_i / d(A [S, S], B [S, S], h [S]) flattened in that order, zero outside A[t_i, :], B[t_i, :], h[t_i] -- what
    tersoff_multi_theta_sum reduces.  The list may have been searched with any radius >= max (R + D)."""
    lib = _lib.load()
    N, dev, S = ell.n_atoms, xyz.device, int(n_species)
    if not 1 <= S <= TERSOFF_MULTI_MAX_SPECIES:
        raise ValueError("mdgrad_amd: n_species must lie in [1, %d] (got %r)" % (TERSOFF_MULTI_MAX_SPECIES, n_species))
    require_gpu(types, "types", dtype=None)
    if types.shape != (N,) or types.dtype != torch.int32 or not types.is_contiguous():
        raise ValueError("mdgrad_amd: types must be a contiguous int32 [%d] tensor (got %s %s)" % (N, types.dtype, tuple(types.shape)))
    require_gpu(tables, "tables")
    if tables.shape != (8 * S * (S + 1),) or tables.dtype != torch.float32 or not tables.is_contiguous():
        raise ValueError("mdgrad_amd: tables must be a contiguous float32 [%d] tensor (got %s)" % (8 * S * (S + 1), tuple(tables.shape)))
    work = _bond_work(work, tersoff_multi_work_size(ell), dev)
    xyz, w, e, g, hw, pth, pthw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (N, 2 * S * S + S))
    partial = torch.empty(int(lib.mdg_tersoff_multi_partial_size(N)), device=dev) if energy else None
    check(lib.mdg_tersoff_multi_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt),
                                     ell.max_nbr, ptr(types), S, ptr(tables), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pth),
                                     ptr(pthw), ptr(partial), ptr(work), float(scale), _list_flags(acc, ell), stream_ptr(dev)),
          "mdg_tersoff_multi_eval")
    return dict(energy=e, grad=g, hw=hw, pth=pth, pthw=pthw)


class TersoffMultiTerm(SWTerm):
    """The multi-species Tersoff term (csrc/tersoff_multi.hip) for TermEnergyFn: the list, the species of the atoms, the device
    table and the scratch of the bond pass, kept current by TersoffMulti; the two evaluations are SWTerm's."""

    noun = "dU/d(A, B, h) of the multi-species Tersoff term"

    def __init__(self, ell, types, n_species, tables, work=None):
        self.ell, self.types, self.n_species, self.tables, self.work = ell, types, n_species, tables, work

    def _eval(self, xyz, **kw):
        return tersoff_multi_eval(self.ell, xyz, self.types, self.n_species, self.tables, work=self.work, **kw)


# ----------------------------------------------------------------------------- multi-species Stillinger-Weber term (K28)
SW_MULTI_MAX_SPECIES = 4
SW_MULTI_PAIR = ("epsilon", "sigma", "a", "gamma", "A", "B", "p", "q")
SW_MULTI_TRIPLET = ("lam", "epsilon3", "cos0")
SW_MULTI_PAIR_FLOATS, SW_MULTI_TRIPLET_FLOATS = 12, 4


def sw_multi_tables(pair, triplet):
    """The table image mdg_sw_multi_eval reads, as a host float32 array of 12 S S + 4 S S S derived constants, from
    pair = dict of [S, S] arrays epsilon, sigma, a, gamma, A, B, p, q (row = centre species, column = end species) and
    triplet = dict of [S, S, S] arrays lam, epsilon3, cos0 (centre, end, end):
        pair entry    out[12 (a S + b) ...]                 = epsilon, sigma, a sigma, gamma sigma, gamma, A, B, p, q, a, A epsilon, 0
        triplet entry out[12 S S + 4 ((a S + b) S + c) ...] = K_a{bc}, cos0_abc, w_abc, 0
    with K_a{bc} = (lam_abc epsilon3_abc + lam_acb epsilon3_acb) / 2 and w_abc = epsilon3_abc / 2 (epsilon3_abb for b = c),
    the weight of lam_abc in K_a{bc}.  Every entry is validated: epsilon, sigma, a, A > 0; gamma, lam, epsilon3 >= 0; p, q
    integers with 0 <= q < p <= 12; cos0 symmetric in its two ends."""
    pr = {k: np.asarray(pair[k], dtype=np.float64) for k in SW_MULTI_PAIR}
    S = pr["epsilon"].shape[0] if pr["epsilon"].ndim == 2 else -1
    if not 1 <= S <= SW_MULTI_MAX_SPECIES:
        raise ValueError("mdgrad_amd: the number of species must lie in [1, %d] (got epsilon of shape %s)"
                         % (SW_MULTI_MAX_SPECIES, pr["epsilon"].shape))
    for k, v in pr.items():
        if v.shape != (S, S):
            raise ValueError("mdgrad_amd: pair[%r] must be [%d, %d] (got %s)" % (k, S, S, v.shape))
    tr = {k: np.asarray(triplet[k], dtype=np.float64) for k in SW_MULTI_TRIPLET}
    for k, v in tr.items():
        if v.shape != (S, S, S):
            raise ValueError("mdgrad_amd: triplet[%r] must be [%d, %d, %d] (got %s)" % (k, S, S, S, v.shape))
    for k in ("epsilon", "sigma", "a", "A"):
        if not (pr[k] > 0.0).all():
            raise ValueError("mdgrad_amd: every entry of %s must be positive (got %r)" % (k, pr[k].tolist()))
    if not (pr["gamma"] >= 0.0).all():
        raise ValueError("mdgrad_amd: every entry of gamma must be >= 0 (got %r)" % pr["gamma"].tolist())
    for k in ("lam", "epsilon3"):
        if not (tr[k] >= 0.0).all():
            raise ValueError("mdgrad_amd: every entry of %s must be >= 0 (got %r)" % (k, tr[k].tolist()))
    p, q = pr["p"], pr["q"]
    if not ((np.rint(p) == p) & (np.rint(q) == q) & (0 <= q) & (q < p) & (p <= 12)).all():
        raise ValueError("mdgrad_amd: the exponents must be integers with 0 <= q < p <= 12 for every pair (got p = %r, q = %r)"
                         % (p.tolist(), q.tolist()))
    if not np.isfinite(tr["cos0"]).all() or not np.array_equal(tr["cos0"], tr["cos0"].transpose(0, 2, 1)):
        raise ValueError("mdgrad_amd: cos0[a, b, c] must equal cos0[a, c, b]: the two ends of a triplet are unordered (got %r)"
                         % tr["cos0"].tolist())
    out = np.zeros(SW_MULTI_PAIR_FLOATS * S * S + SW_MULTI_TRIPLET_FLOATS * S ** 3, dtype=np.float32)
    P = out[:SW_MULTI_PAIR_FLOATS * S * S].reshape(S, S, SW_MULTI_PAIR_FLOATS)
    eps, sig, gam = (pr[k].astype(np.float32) for k in ("epsilon", "sigma", "gamma"))
    a32, A32 = pr["a"].astype(np.float32), pr["A"].astype(np.float32)
    for c, v in enumerate((eps, sig, a32 * sig, gam * sig, gam, A32, pr["B"], p, q, a32, A32 * eps)):
        P[:, :, c] = v                                # (the derived entries in float32, as the module's device pack forms them)
    T = out[SW_MULTI_PAIR_FLOATS * S * S:].reshape(S, S, S, SW_MULTI_TRIPLET_FLOATS)
    le = tr["lam"].astype(np.float32) * tr["epsilon3"].astype(np.float32)
    T[..., 0] = np.float32(0.5) * (le + le.transpose(0, 2, 1))
    T[..., 1] = tr["cos0"]
    T[..., 2] = sw_multi_lam_weight(tr["epsilon3"])
    return out


def sw_multi_lam_weight(epsilon3):
    """w_abc = d K_a{bc} / d lam_abc: epsilon3_abc / 2, and epsilon3_abb for b = c (float32 [S, S, S])."""
    e3 = np.asarray(epsilon3, dtype=np.float32)
    S = e3.shape[0]
    same = np.eye(S, dtype=bool)[None, :, :]
    return np.where(same, e3, np.float32(0.5) * e3).astype(np.float32)


def sw_multi_eval(ell, xyz, types, n_species, tables, w=None, energy=True, grad=True, into=None, scale=1.0, want_theta=False):
    """One launch of mdg_sw_multi_eval -> dict(energy, grad, hw, pth, pthw), argument for argument sw_eval with `types` (device
    int32 [N], values in [0, n_species): not read here) and `tables` (device float32, the image of sw_multi_tables) in place of
    the constants and theta.  Layout of pth / pthw [N, 2 S S + S S S]: row i holds d u_i / d(epsilon [S, S], sigma [S, S],
    lam [S, S, S]) flattened in that order, for u_i = 1/2 sum_j phi2 + the triplets centred on i.  With a = types[i] it is zero
    outside epsilon[a, :], sigma[a, :], lam[a, :, :]; the words lam[a, b, c] and lam[a, c, b] hold w_abc and w_acb times the
    sum T_a{bc} of (cos theta - cos0)^2 g g over the triplets of the unordered class {b, c} centred on i, i.e. each ordering
    receives half of the class's derivative times its own epsilon3 (both halves for b = c).  The column sums over the atoms
    (theta_sum) are therefore dU/d(epsilon, sigma, lam) in the parameters' shapes, with no index map.  The list may have been
    searched with any radius >= max a sigma: the kernel applies r < a_ab sigma_ab per entry."""
    lib = _lib.load()
    N, dev, S = ell.n_atoms, xyz.device, int(n_species)
    if not 1 <= S <= SW_MULTI_MAX_SPECIES:
        raise ValueError("mdgrad_amd: n_species must lie in [1, %d] (got %r)" % (SW_MULTI_MAX_SPECIES, n_species))
    require_gpu(types, "types", dtype=None)
    if types.shape != (N,) or types.dtype != torch.int32 or not types.is_contiguous():
        raise ValueError("mdgrad_amd: types must be a contiguous int32 [%d] tensor (got %s %s)" % (N, types.dtype, tuple(types.shape)))
    require_gpu(tables, "tables")
    size = SW_MULTI_PAIR_FLOATS * S * S + SW_MULTI_TRIPLET_FLOATS * S ** 3
    if tables.shape != (size,) or tables.dtype != torch.float32 or not tables.is_contiguous():
        raise ValueError("mdgrad_amd: tables must be a contiguous float32 [%d] tensor (got %s)" % (size, tuple(tables.shape)))
    xyz, w, e, g, hw, pth, pthw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_theta, (N, 2 * S * S + S ** 3))
    partial = torch.empty(int(lib.mdg_sw_multi_partial_size(N)), device=dev) if energy else None
    check(lib.mdg_sw_multi_eval(ptr(xyz), N, C.byref(ell.cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt), ell.max_nbr,
                                ptr(types), S, ptr(tables), ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pth), ptr(pthw), ptr(partial),
                                float(scale), _list_flags(acc, ell), stream_ptr(dev)), "mdg_sw_multi_eval")
    return dict(energy=e, grad=g, hw=hw, pth=pth, pthw=pthw)


class SWMultiTerm(SWTerm):
    """The multi-species Stillinger-Weber term (csrc/sw_multi.hip) for TermEnergyFn: the list, the species of the atoms and the
    device table, kept current by StillingerWeberMulti; the two evaluations are SWTerm's."""

    noun = "dU/d(epsilon, sigma, lam) of the multi-species Stillinger-Weber term"

    def __init__(self, ell, types, n_species, tables):
        self.ell, self.types, self.n_species, self.tables = ell, types, n_species, tables

    def _eval(self, xyz, **kw):
        return sw_multi_eval(self.ell, xyz, self.types, self.n_species, self.tables, **kw)


# ----------------------------------------------------------------------------- Ewald reciprocal-space sum (K21)
EWALD_MAX_INDEX = 1024
EWALD_MAX_VECS = 65536


def ewald_vectors(lengths, k_cutoff):
    """The wave vectors of the reciprocal sum on a diagonal cell, on the host in float64: (n int32 [M, 3], |k|^2 float64 [M])
    with k(n) = 2 pi n / L, n != 0, |k| <= k_cutoff, of the half space of observable.sk_vectors (nx > 0, or nx = 0 and ny > 0,
    or nx = ny = 0 and nz > 0), sorted by |k|^2 and then by (nx, ny, nz)."""
    L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    if L.shape != (3,) or not (L > 0).all():
        raise ValueError("mdgrad_amd: ewald_vectors needs three positive cell lengths (got %r)" % (lengths,))
    kc = float(k_cutoff)
    if not kc > 0.0:
        raise ValueError("mdgrad_amd: k_cutoff must be positive (got %r)" % (k_cutoff,))
    nmax = np.floor(kc * L / (2 * np.pi)).astype(np.int64)
    if int(nmax.max()) > EWALD_MAX_INDEX:
        raise ValueError("mdgrad_amd: k_cutoff = %g reaches wave-vector indices beyond %d in this cell" % (kc, EWALD_MAX_INDEX))
    ax = [np.arange(0, nmax[0] + 1), np.arange(-nmax[1], nmax[1] + 1), np.arange(-nmax[2], nmax[2] + 1)]
    n = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))
    n = n[half]
    k2 = ((2 * np.pi * n / L) ** 2).sum(1)
    keep = k2 <= kc * kc
    n, k2 = n[keep], k2[keep]
    if len(n) == 0:
        raise ValueError("mdgrad_amd: no wave vector below k_cutoff = %g (the smallest is 2 pi / L_max = %g)"
                         % (kc, 2 * np.pi / L.max()))
    if len(n) > EWALD_MAX_VECS:
        raise ValueError("mdgrad_amd: %d wave vectors below k_cutoff = %g, at most %d (lower the accuracy or k_cutoff)"
                         % (len(n), kc, EWALD_MAX_VECS))
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], k2))
    return torch.from_numpy(n[order].astype(np.int32)), torch.from_numpy(k2[order])


def ewald_coef(k2, volume, alpha):
    """c(k) = (4 pi / V) exp(-k^2 / (4 alpha^2)) / k^2 in float64."""
    k2 = torch.as_tensor(k2, dtype=torch.float64)
    alpha = float(alpha)
    if not alpha > 0.0:
        raise ValueError("mdgrad_amd: the Ewald splitting parameter alpha must be positive (got %r)" % alpha)
    return (4.0 * math.pi / float(volume)) * torch.exp(-k2 / (4.0 * alpha * alpha)) / k2


class EwaldTable:
    """What the reciprocal sum needs beside positions and charges, built once: the integer wave vectors and the table
    conversion * c(k) as persistent device buffers (no torch op for them inside a graph capture), the cell, the replica
    layout and the background constant  conversion * pi / (V alpha^2)."""

    def __init__(self, cell_struct, lengths, alpha, k_cutoff, conversion, n_rep, n_atoms, device):
        self.cell_struct, self.n_rep, self.n_atoms = cell_struct, int(n_rep), int(n_atoms)
        self.alpha, self.k_cutoff, self.conversion = float(alpha), float(k_cutoff), float(conversion)
        L = np.asarray(lengths, dtype=np.float64).reshape(3)
        self.lengths, self.volume = L, float(np.prod(L))
        self.n_host, self.k2_host = ewald_vectors(L, k_cutoff)
        self.coef_host = ewald_coef(self.k2_host, self.volume, self.alpha)                # (without the conversion)
        self.n_vecs = int(self.n_host.shape[0])
        self.kvec = self.n_host.to(device).contiguous()
        self.coef = (self.conversion * self.coef_host).to(torch.float32).to(device).contiguous()
        self.background = self.conversion * math.pi / (self.volume * self.alpha * self.alpha)


def ewald_eval(table, xyz, q_atom, w=None, energy=True, grad=True, into=None, scale=1.0, want_pot=False):
    """One mdg_ewald_eval -> dict(energy, grad, hw, pot, potw), shaped like coulomb_eval; everything carries the table's
    conversion, nothing the background term: energy = conversion sum_k c |rho|^2 over all replicas, grad = scale dU/dx, with
    `w` hw = scale H w; want_pot: pot_i = conversion sum_k 2 c (A c_i + B s_i) without `w`, potw_i = d(w.dU/dx)/dq_i with it.
    `into` = (grad buffer, hw buffer or None): grad / hw are ADDED onto them."""
    lib = _lib.load()
    N = table.n_rep * table.n_atoms
    xyz, w, e, g, hw, pot, potw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_pot, (N,), q_atom)
    dev = xyz.device
    ws = torch.empty(int(lib.mdg_ewald_workspace(table.n_rep, table.n_atoms, table.n_vecs)), device=dev)
    check(lib.mdg_ewald_eval(ptr(xyz), table.n_rep, table.n_atoms, C.byref(table.cell_struct), ptr(q_atom), ptr(table.kvec),
                             ptr(table.coef), table.n_vecs, ptr(w), ptr(e), ptr(g), ptr(hw), ptr(pot), ptr(potw), ptr(ws),
                             float(scale), int(acc), stream_ptr(dev)), "mdg_ewald_eval")
    return dict(energy=e, grad=g, hw=hw, pot=pot, potw=potw)


class EwaldTerm(_ChargeTerm):
    """The Ewald reciprocal sum with its neutralising background (csrc/ewald.hip): the table beside what _ChargeTerm holds (the
    charge slots are those of the real-space CoulombPotentials the term belongs to).  Nothing is owed: the table's `coef`
    and `background` hold the conversion."""

    noun = "dU/dcharges of the Ewald reciprocal term"

    def __init__(self, table, q_atom, slot, n_slots):
        super().__init__(q_atom, slot, n_slots)
        self.table = table

    def _eval(self, xyz, **kw):
        return ewald_eval(self.table, xyz, self.q_atom, **kw)

    def _own(self, e, pot):
        """The background term, in the energy and in dU/dq_i."""
        t = self.table
        Q = self.q_atom.reshape(t.n_rep, t.n_atoms).sum(1)                                   # net charge of every replica
        dq_atom = pot - t.background * Q.repeat_interleave(t.n_atoms)                        # dU/dq_i
        return None if e is None else e - (0.5 * t.background) * Q.pow(2).sum(), self.charge_grad_w(dq_atom)


# ----------------------------------------------------------------------------- Ewald correction for excluded pairs (K22)
class EwaldExclTable:
    """What the erf correction of excluded / scaled pairs needs beside positions and charges, built once on the host: the
    pairs of ONE replica as int64 [P, 2] with i < j (`pairs`), their scales float64 [P] (`scale`), and the CSR incidence list
    the kernel walks -- row(a) = the partners of atom a in ascending order with the pair's scale, every pair once per end --
    as persistent device buffers (no torch op for them inside a graph capture).  ValueError on a pair with i == j, an index
    outside [0, n_atoms), a pair listed twice in either orientation (this sum would subtract it twice) or a scale outside
    [0, 1]."""

    def __init__(self, pairs, scale, n_atoms, n_rep, lengths, alpha, conversion, device):
        n = int(n_atoms)
        p = np.asarray(torch.as_tensor(pairs).detach().cpu().numpy(), dtype=np.int64).reshape(-1, 2)
        if p.shape[0] == 0:
            raise ValueError("mdgrad_amd: the list of excluded pairs is empty")
        if p.min() < 0 or p.max() >= n:
            raise ValueError("mdgrad_amd: an excluded pair refers to an index outside the replica [0, %d)" % n)
        if bool((p[:, 0] == p[:, 1]).any()):
            raise ValueError("mdgrad_amd: an excluded pair has i == j (%d)" % int(p[p[:, 0] == p[:, 1]][0, 0]))
        p = np.stack([p.min(1), p.max(1)], 1)
        key = p[:, 0] * n + p[:, 1]
        if len(np.unique(key)) != len(key):
            u, c = np.unique(key, return_counts=True)
            d = int(u[c > 1][0])
            raise ValueError("mdgrad_amd: the excluded pair (%d, %d) is listed twice (in either orientation): the correction "
                             "would be applied twice" % (d // n, d % n))
        if scale is None:
            s = np.zeros(len(p), dtype=np.float64)
        else:
            s = np.asarray(torch.as_tensor(scale).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
            if s.size == 1:
                s = np.full(len(p), float(s[0]))
            if s.shape != (len(p),):
                raise ValueError("mdgrad_amd: scale must be None, one number or one number per excluded pair (%d), got %d"
                                 % (len(p), s.size))
        if s.size and not bool(((s >= 0.0) & (s <= 1.0)).all()):
            raise ValueError("mdgrad_amd: the scale of an excluded pair must lie in [0, 1]")
        alpha = float(alpha)
        if not alpha > 0.0:
            raise ValueError("mdgrad_amd: the Ewald splitting parameter alpha must be positive (got %r)" % alpha)
        L = np.asarray(lengths, dtype=np.float64).reshape(-1)
        if L.shape != (3,) or not (L > 0).all():
            raise ValueError("mdgrad_amd: EwaldExclTable needs three positive cell lengths (got %r)" % (lengths,))
        self.pairs, self.scale = torch.from_numpy(p.copy()), torch.from_numpy(s.copy())
        self.n_atoms, self.n_rep, self.n_pairs = n, int(n_rep), int(len(p))
        self.alpha, self.conversion, self.lengths = alpha, float(conversion), L
        self.cell_len = (C.c_float * 3)(*[float(x) for x in L])
        atom = np.concatenate([p[:, 0], p[:, 1]])
        other = np.concatenate([p[:, 1], p[:, 0]])
        order = np.lexsort((other, atom))                          # by atom, then by partner
        cnt = np.zeros(n + 1, dtype=np.int64)
        np.add.at(cnt, atom + 1, 1)
        self.row_ptr_host = np.cumsum(cnt).astype(np.int32)
        self.col_host = other[order].astype(np.int32)
        self.scl_host = np.concatenate([s, s])[order].astype(np.float32)
        self.device = device
        if torch.device(device).type == "cuda":
            self.row_ptr = torch.as_tensor(self.row_ptr_host, device=device).contiguous()
            self.col = torch.as_tensor(self.col_host, device=device).contiguous()
            self.scl = torch.as_tensor(self.scl_host, device=device).contiguous()
        else:
            self.row_ptr = self.col = self.scl = None


def ewald_excl_eval(table, xyz, q_atom, w=None, energy=True, grad=True, into=None, scale=1.0, want_pot=False):
    """One launch of mdg_ewald_excl_eval (plus the finish for the energy) -> dict(energy, grad, hw, pot, potw), shaped like
    coulomb_eval: energy and grad carry the table's conversion, pot_i = sum_j q_j chi(r_ij) and potw_i = sum_j q_j chi'(r_ij)
    rhat_ij.(w_i - w_j) do not (dU/dq_i = conversion pot_i).  `into` = (grad buffer, hw buffer or None): grad / hw are ADDED
    onto them, times `scale`; atoms without an excluded pair leave them untouched."""
    lib = _lib.load()
    N = table.n_rep * table.n_atoms
    xyz, w, e, g, hw, pot, potw, acc = _eval_prologue(N, xyz, w, energy, grad, into, want_pot, (N,), q_atom)
    dev = xyz.device
    partial = None
    if energy:
        partial = torch.empty(int(lib.mdg_ewald_excl_partial_size(table.n_rep, table.n_atoms)), device=dev, dtype=torch.float64)
    check(lib.mdg_ewald_excl_eval(ptr(xyz), table.n_rep, table.n_atoms, table.cell_len, ptr(table.row_ptr), ptr(table.col),
                                  ptr(table.scl), ptr(q_atom), table.alpha, table.conversion, ptr(w), ptr(e), ptr(g), ptr(hw),
                                  ptr(pot), ptr(potw), ptr(partial), float(scale), int(acc), stream_ptr(dev)),
          "mdg_ewald_excl_eval")
    return dict(energy=e, grad=g, hw=hw, pot=pot, potw=potw)


class EwaldExclTerm(_ChargeTerm):
    """The erf correction of excluded / scaled pairs (csrc/ewald_excl.hip): an EwaldExclTable beside what _ChargeTerm holds.
    No self term, no background term: dU/dq_i = conversion pot_i."""

    noun = "dU/dcharges of the Ewald exclusion term"

    def __init__(self, table, q_atom, slot, n_slots):
        super().__init__(q_atom, slot, n_slots)
        self.table, self.pot_scale = table, table.conversion

    def _eval(self, xyz, **kw):
        return ewald_excl_eval(self.table, xyz, self.q_atom, **kw)


# ----------------------------------------------------------------------------- fused trajectories
class FusedSpec:
    """Host-side descriptor of a fusable integrator (NoseHooverChain / NVE over built-in pair
    terms, topology_update_freq == 1)."""

    def __init__(self, ensemble, n_atoms, mass, cell_struct, terms, n_theta_total, masks,
                 T=0.0, n_dof=0.0, Q=(), block=0, large=False):
        self.large = large
        self.ensemble, self.n_atoms, self.mass = ensemble, n_atoms, mass
        self.cell_struct, self.terms, self.n_theta_total, self.masks = cell_struct, terms, n_theta_total, masks
        self.T, self.n_dof, self.Q, self.block = float(T), float(n_dof), list(Q), block
        # what the trajectory code reads beyond the constructor's arguments (assigned by md.fused_spec, the observable
        # and FusedTrajFn): tabulated pair model, topology_update_freq > 1, the fused observable, stacked replicas
        self.table, self.stale_freq, self.rdf_hint, self.n_rep = False, 0, None, 1
        self._integrator, self._last_large = None, None

    def params(self, n_rep, n_frames):
        p = MdgTrajParams()
        p.n_rep, p.n_atoms, p.n_frames = n_rep, self.n_atoms, n_frames
        p.n_chains, p.ensemble, p.block = len(self.Q), self.ensemble, self.block
        p.T, p.n_dof = self.T, self.n_dof
        for k, q in enumerate(self.Q):
            p.Q[k] = q
        return p


def make_terms(term_list, n_theta_total):
    ts = MdgTerms()
    ts.n_terms, ts.n_theta_total = len(term_list), n_theta_total
    for k, t in enumerate(term_list):
        ts.t[k] = t
    return ts


# diagnostics of the multi-launch (large-N) trajectory path: how often the adjoint could not use the stored candidate
# lists of the forward pass (tests read these)
LARGE_STATS = {"lists_incomplete": 0, "adjoint_redone_with_searches": 0}
# the RDF of large systems searches and counts in one sweep over the cell bins (False: through a neighbour list)
RDF_CELL_DIRECT = True


def large_list_builds(spec):
    """After a forward pass of the multi-launch (large-N) kernels on `spec` (and before its workspace is released by the
    backward pass): int32 [R, T], entry (r, f) = the frame whose neighbour search produced the candidate list that
    served frame f (Verlet reuse, csrc/traj_large.hip); None when the lists were not kept.  Diagnostics:
    `len(set(row))` searches ran for that replica."""
    last = spec._last_large
    if last is None:
        raise RuntimeError("mdgrad_amd: no trajectory of the multi-launch (large-N) kernels has run on this spec")
    ref, (R, N, T, KT) = last
    ws = ref()
    if ws is None:
        raise RuntimeError("mdgrad_amd: the trajectory's workspace has been released (ask before the backward pass ends)")
    out = torch.empty(R, T, dtype=torch.int32, device=ws.device)
    rc = _lib.load().mdg_traj_large_list_builds(ptr(ws), R, N, T, KT, ptr(out), stream_ptr(ws.device))
    if rc == 1:
        return None
    check(rc, "mdg_traj_large_list_builds")
    return out


class RdfFuse:
    """An `rdf` observable (observable.py) that a fused trajectory launch evaluates on the fly: centres, width and
    pair cutoff of the observable and the frames frame_start + k frame_stride it is called on.  Registered on the
    integrator by the observable itself the first time it sees (a time slice of) a fused trajectory; later launches
    deposit the histogram inside the trajectory kernels (mdg_traj_fwd_small_rdf) and take dL/d(raw) in the adjoint
    (mdg_traj_adj_small_rdf) -- see `fused_traj` and `rdf.forward`."""

    def __init__(self, obs, start, stride):
        import weakref
        self.obs = weakref.ref(obs)
        self.mu = obs.offsets.detach().to(torch.float32).contiguous()
        self.nbins, self.coeff, self.spacing = int(obs.nbins), float(obs.coeff), float(obs.spacing)
        self.mu0 = float(obs.r_axis[0])
        self.cutoff, self.n_atoms = float(obs.cutoff_boundary), int(obs.natoms)
        self.cell = tuple(float(x) for x in obs.cell.tolist())
        self.start, self.stride = int(start), int(stride)

    def struct(self):
        return _lib.MdgRdfFuse(self.mu.data_ptr(), self.nbins, self.coeff, self.mu0, self.spacing, self.cutoff, self.start,
                               self.stride)

    def matches(self, obs, start, stride):
        return self.obs() is obs and self.start == int(start) and self.stride == int(stride)

    def fits(self, spec, dev):
        cs = spec.cell_struct
        return (self.obs() is not None and self.n_atoms == spec.n_atoms and self.mu.device == dev
                and bool(cs.diag) and all(abs(cs.h[4 * c] - self.cell[c]) <= 1e-6 * abs(self.cell[c]) for c in range(3)))


def fused_traj(v0, q0, pv0, t, theta, spec, time_dim=None):
    """FusedTrajFn.apply plus the bookkeeping of the fused observable: returns (v_t, q_t[, pv_t]) with q_t tagged so
    that an `rdf` called on it (or on a slice of it along time) finds the histogram the launch already made, or
    registers itself for the next launch."""
    outs = FusedTrajFn.apply(v0, q0, pv0, t, theta, spec, True)   # (direct six-argument callers keep the plain output tuple)
    n = 3 if spec.ensemble == 0 else 2
    tag_trajectory(outs[1], spec, outs[n] if len(outs) > n else None,
                   (1 if v0.dim() == 3 else 0) if time_dim is None else time_dim)
    return tuple(outs[:n])


def tag_trajectory(q_t, spec, raw, time_dim):
    q_t._mdg_traj = (spec, time_dim, spec.rdf_hint if raw is not None else None, raw)


def _stale_launch(ctx, spec, R, T, dev, calls, launch):
    """One launch of the stale-list kernels (topology_update_freq > 1: lists rebuilt at the calls whose running count is a
    multiple of the frequency, md.py:200-204; on the large path the host loop of the library decides per call whether it
    rebuilds, round 6).  `launch(freq, count0, lists)` runs with the integrator's persistent lists and call counter, which
    then advances by the right-hand-side calls the reference makes: `calls` = 2 per interval in the forward pass, 3 in the
    adjoint (the dL/dt evaluation and two augmented ones, sovlers.py:258-266).  Returns the lists."""
    integ = spec._integrator
    if getattr(integ, "_stale_code", None) is None and ctx.stale_code is not None:
        # a generic force / odeint call on this integrator between the fused forward and this backward (logging,
        # an observable) dropped the fused lists (md.update_topology): the forward's own lists -- held on ctx --
        # are the ones its saved frames were integrated with; the call counter keeps what the calls in between
        # made of it, as the reference's would
        integ._stale_code = ctx.stale_code
    code = integ.stale_lists(R, spec.n_atoms, dev, large=ctx.large)
    launch(int(ctx.stale_freq), int(integ.update_count), ptr(code))
    integ.update_count += calls * (T - 1)
    integ._stale_fused_dirty = True        # (the generic path's own lists are older than these now: md.update_topology)
    return code


class FusedTrajFn(torch.autograd.Function):
    """odeint_adjoint(NoseHooverChain|NVE, (v0,q0[,pv0]), t) in two launches: the forward
    trajectory and, on backward, the reference's adjoint sweep (torchmd/sovlers.py:196-293).
    States may carry a leading replica dimension [R,N,3]."""

    @staticmethod
    def forward(ctx, v0, q0, pv0, t, theta, spec, fuse=False):
        lib = _lib.load()
        require_gpu(v0, "v0"), require_gpu(q0, "q0"), require_gpu(t, "t")
        # the gradient of an output the loss does not use arrives as None, not as a trajectory-sized block of zeros that
        # the adjoint launch would read frame by frame (its g_v / g_q / g_pv are nullable)
        ctx.set_materialize_grads(False)
        batched = v0.dim() == 3
        R = v0.shape[0] if batched else 1
        N, T = spec.n_atoms, t.shape[0]
        dev = v0.device
        nhc = spec.ensemble == 0
        Cn = len(spec.Q)
        v0c, q0c = v0.detach().contiguous(), q0.detach().contiguous()
        pv0c = pv0.detach().contiguous() if nhc else None
        tc = t.detach().to(torch.float32).contiguous()
        thc = theta.detach().contiguous() if theta is not None and theta.numel() else None
        v_t = torch.empty(R, T, N, 3, device=dev)
        q_t = torch.empty(R, T, N, 3, device=dev)
        pv_t = torch.empty(R, T, Cn, device=dev) if nhc else None
        prm = spec.params(R, T)
        # the route is decided here, once, and kept on ctx for backward: multi-launch (large) or one-workgroup / ring
        # kernels, stale lists or not, the RDF fused in or not (`fuse`: only fused_traj / odeint_adjoint ask), forces kept or not
        ctx.large, ctx.stale_freq, ctx.table = bool(spec.large), int(spec.stale_freq), bool(spec.table)
        ctx.ws, ctx.lists_ok, ctx.stale_code = None, False, None
        fuse = spec.rdf_hint if fuse else None
        if fuse is not None and (spec.large or spec.table or thc is None or not fuse.fits(spec, dev)
                                 or not lib.mdg_traj_rdf_supported(C.byref(prm), C.byref(spec.cell_struct),
                                                                   C.byref(spec.terms), C.byref(fuse.struct()))):
            fuse = None
        ctx.fuse = fuse
        raw = None
        # the wave-per-replica kernels keep the force of every saved frame for the adjoint's first evaluation of each
        # interval (mdg_traj_*_ft: 4 R T N 3 bytes, written once and read once; 1.06 GB at 16 384 x 50 x 108 atoms)
        f_t = None
        if not ctx.large and not ctx.stale_freq and lib.mdg_traj_ring_taken(
                C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)):
            f_t = torch.empty(R, T, N, 3, device=dev)
        ctx.f_t = f_t
        args = (C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms), ptr(thc), ptr(spec.mass), ptr(tc),
                ptr(v0c), ptr(q0c), ptr(pv0c), ptr(v_t), ptr(q_t), ptr(pv_t))

        def run(fn, *extras):                      # the forward launch: the common arguments, then the route's own
            check(fn(*args, *extras, stream_ptr(dev)), fn.__name__)

        if ctx.large:
            ws = torch.empty(int(lib.mdg_traj_large_workspace(R, N, T, spec.n_theta_total)), device=dev)
            flags = torch.zeros(8, dtype=torch.int32, device=dev)
            out = (ptr(ws), ptr(flags))
        else:
            bad = torch.zeros(R, dtype=torch.int32, device=dev)
            out = (ptr(bad),)
        if fuse is not None:
            # the observable rides along: raw soft histogram of the selected frames of all replicas
            raw = torch.empty(fuse.nbins, device=dev)
            run(lib.mdg_traj_fwd_small_rdf_ft, ptr(f_t), *out, C.byref(fuse.struct()), ptr(raw))
        elif ctx.stale_freq:
            fn = lib.mdg_traj_fwd_large_stale if ctx.large else lib.mdg_traj_fwd_small_stale
            # (the lists this pass ended with: what its backward continues from)
            ctx.stale_code = _stale_launch(ctx, spec, R, T, dev, 2, lambda *tail: run(fn, *out, *tail))
        elif ctx.large:
            run(lib.mdg_traj_fwd_large, *out)
        else:
            run(lib.mdg_traj_fwd_small_ft, ptr(f_t), *out)
        if ctx.large:
            fl = flags.tolist()                    # one sync per trajectory (neighbour buffer / table range check)
            if fl[0]:
                raise RuntimeError("mdgrad_amd: an atom has %d neighbours within the cutoff; the fused large-N "
                                   "kernel holds 256 per atom" % fl[0])
            if fl[3]:
                raise RuntimeError("mdgrad_amd: a pair came closer than the first node of the tabulated pair "
                                   "potential; lower `table_rmin` on the integrator or set `fused_table = False`")
            ctx.ws, bad = ws, flags[1:2]
            spec._last_large = (weakref.ref(ws), (R, N, T, spec.n_theta_total))    # (ops.large_list_builds)
            ctx.lists_ok = not fl[4]               # every frame's candidate list was stored: the adjoint re-tests them
            LARGE_STATS["lists_incomplete"] += int(bool(fl[4]))
        if ctx.table and not ctx.large:
            # tabulated user pair module: a live pair closer than the first table node has no valid entry
            # (one host sync per trajectory, table mode only)
            if bool((bad & 2).any()):
                raise RuntimeError(
                    "mdgrad_amd: a pair came closer than table_rmin * cutoff = %.4g, below the first node of the "
                    "tabulated pair potential; lower `table_rmin` on the integrator or set `fused_table = False` "
                    "to evaluate the module per pair" % math.sqrt(spec.u0))
        ctx.spec, ctx.batched, ctx.nhc = spec, batched, nhc
        ctx.nonfinite = bad
        saved = [tc, v_t, q_t] + ([pv_t] if nhc else []) + ([thc] if thc is not None else [])
        ctx.has_theta = thc is not None
        ctx.save_for_backward(*saved)
        outs = (v_t, q_t, pv_t) if nhc else (v_t, q_t)
        if not batched:
            outs = tuple(o[0] for o in outs)
        if raw is not None:
            outs = outs + (raw,)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        spec, nhc = ctx.spec, ctx.nhc
        saved = list(ctx.saved_tensors)
        tc, v_t, q_t = saved[0], saved[1], saved[2]
        pv_t = saved[3] if nhc else None
        thc = saved[-1] if ctx.has_theta else None
        R, T, N = v_t.shape[0], v_t.shape[1], spec.n_atoms
        dev = v_t.device
        if ctx.nonfinite is not None and bool((ctx.nonfinite & 1).any()):
            raise RuntimeError("mdgrad_amd: the forward trajectory reached a non-finite state (time step too large "
                               "or overlapping atoms); its adjoint is undefined")

        def prep(g, like):
            if g is None:
                return None
            g = g.detach()
            if not ctx.batched:
                g = g[None]
            return g.expand_as(like).contiguous()

        gv = prep(grads[0], v_t)
        gq = prep(grads[1], q_t)
        gp = prep(grads[2], pv_t) if nhc else None
        fuse = ctx.fuse
        g_raw = grads[3 if nhc else 2] if fuse is not None else None
        if g_raw is not None and ctx.needs_input_grad[3]:
            # gradients w.r.t. the time grid read the frame gradients: materialise the observable's share
            sel = q_t[:, fuse.start::fuse.stride].contiguous()
            gsel = torch.empty_like(sel)
            cs = spec.cell_struct
            check(lib.mdg_rdf_bwd_uniform(ptr(sel), sel.shape[0] * sel.shape[1], N, C.byref(cs), fuse.cutoff, None,
                                          ptr(fuse.mu), fuse.spacing, fuse.coeff, fuse.nbins,
                                          ptr(g_raw.detach().to(torch.float32).contiguous()), ptr(gsel), stream_ptr(dev)),
                  "mdg_rdf_bwd")
            gq = torch.zeros_like(q_t) if gq is None else gq.clone()
            gq[:, fuse.start::fuse.stride] += gsel
            g_raw = None
        # a fit of the potential's parameters never asks for the gradient of the initial state: the ring adjoint (the route
        # that kept the forces) then takes null outputs and skips the work only they need; the other routes always fill them
        want_state = any(ctx.needs_input_grad[0:3]) or ctx.f_t is None
        adj_v = torch.empty(R, N, 3, device=dev) if want_state else None
        adj_q = torch.empty(R, N, 3, device=dev) if want_state else None
        adj_p = torch.empty(R, len(spec.Q), device=dev) if nhc and want_state else None
        KT = spec.n_theta_total
        adj_th = torch.zeros(R, KT, device=dev) if KT else None
        prm = spec.params(R, T)
        table, ws, lists_ok = ctx.table, ctx.ws, ctx.lists_ok
        frames = (ptr(thc), ptr(spec.mass), ptr(tc), ptr(v_t), ptr(q_t), ptr(pv_t))
        grads_ = (ptr(gv), ptr(gq), ptr(gp), ptr(adj_v), ptr(adj_q), ptr(adj_p), ptr(adj_th))

        def run(fn, terms, *extras, prm=prm, f_t=()):
            # the adjoint launch: the common arguments (the _ft entry points take the forward's forces after the frames),
            # then the route's own
            check(fn(C.byref(prm), C.byref(spec.cell_struct), C.byref(terms), *frames, *f_t, *grads_, *extras,
                     stream_ptr(dev)), fn.__name__)

        def launch(terms, search=False):
            # the route the forward took (ctx); the fused RDF only while its gradient has not been folded into gq above
            if g_raw is not None:
                gr = g_raw.detach().to(torch.float32).contiguous()
                run(lib.mdg_traj_adj_small_rdf_ft, terms, C.byref(fuse.struct()), ptr(gr), f_t=(ptr(ctx.f_t),))
                return None
            if ctx.stale_freq:
                flags = torch.zeros(8, dtype=torch.int32, device=dev) if ctx.large else None
                fn = lib.mdg_traj_adj_large_stale if ctx.large else lib.mdg_traj_adj_small_stale
                out = (ptr(ws), ptr(flags)) if ctx.large else ()
                _stale_launch(ctx, spec, R, T, dev, 3, lambda *tail: run(fn, terms, *out, *tail))
                return flags
            if ctx.large:
                # the stored candidate lists of the forward pass serve the adjoint unless one overflowed there (or, flag
                # 5 below, a midpoint moved past their skin): block = -1 asks for fresh searches
                # (a loop, not a recursive call: a closure that names itself is a reference cycle, and this one would
                #  keep ctx -- with the trajectory's multi-GB workspace -- alive until the cyclic collector runs)
                pl = type(prm).from_buffer_copy(prm)
                for search in ((search,) if (search or not lists_ok or spec.block == -1) else (False, True)):
                    pl.block = -1 if (search or not lists_ok or spec.block == -1) else 0
                    flags = torch.zeros(8, dtype=torch.int32, device=dev)
                    run(lib.mdg_traj_adj_large, terms, ptr(ws), ptr(flags), prm=pl)
                    if pl.block == -1 or not int(flags[5]):
                        break
                    LARGE_STATS["adjoint_redone_with_searches"] += 1
                return flags
            run(lib.mdg_traj_adj_small_ft, terms, f_t=(ptr(ctx.f_t),))
            return None

        def check_large(flags):
            # the adjoint evaluates forces / Hessian-vector products at its own (midpoint) positions: a neighbour
            # buffer overflow or a blow-up there must not pass silently (one host sync, large path only)
            f = flags.tolist()
            if f[0]:
                raise RuntimeError("mdgrad_amd: an atom has %d neighbours within the cutoff in the adjoint sweep; "
                                   "the fused large-N kernel holds 256 per atom" % f[0])
            if f[1]:
                raise RuntimeError("mdgrad_amd: non-finite state in the fused large-N adjoint sweep")
            return f

        if table:
            # fixed-point scale of the in-kernel table-gradient scatter: the largest single contribution
            # 1/2 h (D . w_ij) is put near 2^30; the kernels accumulate int64 words and flag a single contribution at or
            # beyond 2^62 / (the contributions one word can receive) -- ~2^40 at 50 frames of 108 atoms --, so a sum cannot
            # leave the word unflagged however far the adjoint grows along the trajectory; one host sync
            lam = max([float(g.abs().max()) for g in (gv, gq) if g is not None] + [1e-30])
            h = float((tc[1:] - tc[:-1]).abs().max())
            est = max(0.5 * h * 2.0 * spec.terms.t[0].cutoff * lam / float(spec.mass.min()), 1e-30)
            S = max(-100, min(100, int(math.floor(30 - math.log2(est)))))
            for attempt in range(4):
                terms = type(spec.terms).from_buffer_copy(spec.terms)
                terms.t[0].c = 2.0 ** S
                flags = launch(terms)
                bad = bool(check_large(flags)[2]) if flags is not None else not bool(torch.isfinite(adj_th[:, 0]).all())
                if not bad:
                    break
                S -= 14                                    # adjoint grew past the range: coarser fixed point
            else:
                raise RuntimeError("mdgrad_amd: the table-gradient accumulation overflowed (adjoint magnitudes "
                                   "above ~2^%d of the incoming gradients)" % (40 - S))
        else:
            flags = launch(spec.terms)
            if flags is not None:
                check_large(flags)
        if not ctx.batched and want_state:
            adj_v, adj_q = adj_v[0], adj_q[0]
            adj_p = adj_p[0] if nhc else None
        gth = adj_th.sum(0) if adj_th is not None else None
        g_t = None
        if ctx.needs_input_grad[3]:
            g_t = _time_vjps(spec, tc, v_t, q_t, pv_t, gv, gq, gp)
        return adj_v, adj_q, adj_p, g_t, gth, None, None


def _time_vjps(spec, t, v_t, q_t, pv_t, gv, gq, gp):
    """dL/dt of the adjoint (`time_vjps`, torchmd/sovlers.py:258-266,289-293): dL/dt_k = f(y_k) . dL/dy_k for
    k >= 1 and dL/dt_0 = -(their sum); the right-hand side does not depend on t, so the adjoint of time is not
    changed by the augmented integration.  Nobody on the hot path consumes it (the reference's drivers do not
    either), so it is computed on request only -- one force evaluation per saved frame on the generic HIP ops."""
    integ = spec._integrator
    if integ is None:
        raise NotImplementedError("mdgrad_amd: dL/dt needs the integrator behind the fused spec")
    R, T = v_t.shape[0], v_t.shape[1]
    nhc = pv_t is not None
    stacked = spec.n_rep > 1
    zero = lambda like: torch.zeros_like(like)
    out = torch.zeros(T, device=v_t.device, dtype=t.dtype)
    with torch.no_grad():
        for k in range(1, T):
            frames = [None] if stacked else range(R)
            for r in frames:
                if stacked:                                     # System.replicate: the model takes the stacked state
                    v, q = v_t[:, k].reshape(-1, 3), q_t[:, k].reshape(-1, 3)
                    pv = pv_t[:, k] if nhc else None
                    g_v = gv[:, k].reshape(-1, 3) if gv is not None else zero(v)
                    g_q = gq[:, k].reshape(-1, 3) if gq is not None else zero(q)
                    g_p = (gp[:, k] if gp is not None else zero(pv)) if nhc else None
                else:
                    v, q = v_t[r, k], q_t[r, k]
                    pv = pv_t[r, k] if nhc else None
                    g_v = gv[r, k] if gv is not None else zero(v)
                    g_q = gq[r, k] if gq is not None else zero(q)
                    g_p = (gp[r, k] if gp is not None else zero(pv)) if nhc else None
                integ.model._reset_topology(q)
                F = integ.model.force(q)
                if nhc:
                    a, _, b = integ.rhs_from_force((v, q, pv), F)
                    out[k] += (a * g_v).sum() + (v * g_q).sum() + (b * g_p).sum()
                else:
                    out[k] += (F * g_v).sum() + (v * g_q).sum()              # NVE: dv/dt = F (md.py:145-148)
        out[0] = -out[1:].sum()
    return out


# ----------------------------------------------------------------------------- rdf
RDF_LIST_ATOMS = 2048        # from this size on the RDF runs over a cell-list neighbour list instead of all N^2 pairs


def _rdf_pair_table(g_raw, mu, coeff, cutoff, nodes=4096):
    """The RDF loss as a pair 'potential' phi(d) = sum_k g_k exp(coeff (d - mu_k)^2): its table for the
    MDG_PAIR_TABLE kind -- c1(u) = phi'(r)/r and du * dc1/du on a uniform grid in u = r^2 (csrc/common.hpp)."""
    lo = max(float(mu[0]) - 6.0 / math.sqrt(-2.0 * coeff), 0.05)
    u0, u1 = lo * lo, float(cutoff) ** 2
    du = (u1 - u0) / (nodes - 1)
    r = (u0 + du * torch.arange(nodes, device=mu.device, dtype=torch.float32)).sqrt()[:, None]
    x = r - mu[None, :]
    e = torch.exp(coeff * x * x) * g_raw[None, :]
    p1 = (2.0 * coeff * x * e).sum(1)                                    # phi'
    p2 = ((2.0 * coeff + (2.0 * coeff * x) ** 2) * e).sum(1)             # phi''
    r = r[:, 0]
    c1 = p1 / r
    dc1 = (p2 / r - p1 / (r * r)) / (2.0 * r)                            # d(phi'/r)/du
    return torch.stack((c1, du * dc1), 1).reshape(-1).contiguous(), u0, du


def _rdf_list_cutoff(cutoff, coeff, mu_last):
    """Cutoff of the pair search of the list-based RDF paths."""
    if mu_last is None or not coeff < 0:
        return float(cutoff)
    # The pair search is trimmed to the reach of the Gaussians, and the bound follows the user's `width`: the
    # fine grid of the list kernels ends 5.3 / s beyond the last centre (s = sqrt(-coeff log2 e)), where a pair's
    # term in the LAST bin is exp2(-5.3^2) = 2^-28.1 of a peak term -- small, not zero: with ~ as many pairs in
    # the dropped shell as around the last centre, the last bin loses < 2^-24 of its count (half an ulp of the
    # fp32 sum) and every other bin less.  Never beyond the reference's own cutoff_boundary = end + 0.5
    # (observable.py:52), which wide Gaussians reach first (tests: width x3, x8 at 2 744 atoms vs the oracle).
    return min(float(cutoff), float(mu_last) + 1.02 * 5.3 / math.sqrt(-coeff * 1.4426950408889634) + 1e-6)


RDF_FWD_VARIANTS = ("direct", "block8", "lane", "half", "fine")      # MDG_RDF_FWD_* of include/mdgrad_hip.h
RDF_BWD_VARIANTS = ("atom", "table", "frame")                        # MDG_RDF_BWD_*


def rdf_route(F, N, nbins, spacing, coeff, cutoff, cell_struct, mask):
    """Where RdfRawFn sends F frames of N atoms (no GPU needed): ("cell", None, None) -- the sweep over the cell bins
    (csrc/rdf_cell.hip) --, ("list", None, None) -- a cell-list neighbour list --, or ("frames", fwd, bwd) with the
    kernel variants of csrc/rdf.hip (RDF_FWD_VARIANTS / RDF_BWD_VARIANTS; None where the library refuses the shape).
    cutoff: that of the pair search (_rdf_list_cutoff)."""
    lib = _lib.load()
    if (N >= RDF_LIST_ATOMS and mask is None and spacing > 0 and cell_struct.diag
            and _use_cell_list(N, cell_struct, float(cutoff))
            and lib.mdg_rdf_ell_supported(float(spacing), float(coeff), nbins)):
        direct = RDF_CELL_DIRECT and lib.mdg_rdf_cell_supported(N, C.byref(cell_struct), float(cutoff))
        return ("cell" if direct else "list"), None, None
    shape = (F, N, nbins, float(spacing), float(coeff), int(cell_struct.diag), int(mask is not None), None)
    fwd, bwd = lib.mdg_rdf_fwd_variant(*shape), lib.mdg_rdf_bwd_variant(*shape)
    return "frames", (RDF_FWD_VARIANTS[fwd] if fwd >= 0 else None), (RDF_BWD_VARIANTS[bwd] if bwd >= 0 else None)


def rdf_plan(direction, F, N, nbins, spacing, coeff, cell_struct, mask):
    """The launch plan of csrc/rdf.hip for this shape (no GPU needed), direction "fwd" or "bwd": the MDG_RDF_PLAN_INFO words
    of mdg_rdf_fwd_variant / mdg_rdf_bwd_variant by name, and from mdg_rdf_fine_grid the forward's fine integer grid
    (fine_bins of width fine_h from mu[0] - fine_reach: also the one the cell sweep and the list route count on) and the
    backward table's nodes per centre spacing (table_sub)."""
    lib = _lib.load()
    info = (C.c_int32 * 6)()
    fn = getattr(lib, "mdg_rdf_%s_variant" % direction)
    v = fn(F, N, nbins, float(spacing), float(coeff), int(cell_struct.diag), int(mask is not None), info)
    if v < 0:
        return None
    out = dict(variant=(RDF_FWD_VARIANTS if direction == "fwd" else RDF_BWD_VARIANTS)[v], R=info[0], waves=info[1],
               workgroups=info[2], lds_bytes=info[3], stride=info[4])
    bins, sub, h, reach = C.c_int32(0), C.c_int32(0), C.c_float(0.0), C.c_float(0.0)
    lib.mdg_rdf_fine_grid(float(spacing), float(coeff), nbins, C.byref(bins), C.byref(h), C.byref(reach), C.byref(sub))
    if direction == "fwd":
        out.update(rows128=bool(info[5]), fine_bins=bins.value, fine_h=h.value, fine_reach=reach.value)
    else:
        out.update(cells=info[5], table_sub=sub.value)
    return out


class RdfRawFn(torch.autograd.Function):
    """raw[k] = sum over frames and i<j pairs (d < cutoff) of exp(coeff (d - mu_k)^2)
    (the GaussianSmearing(...).sum(0) of torchmd/observable.py:70)."""

    @staticmethod
    def forward(ctx, xyz, mu, coeff, cutoff, cell_struct, mask, spacing=0.0, mu_last=None):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x = xyz.detach().contiguous()
        x3 = x.reshape(-1, x.shape[-2], 3)
        F, N, B = x3.shape[0], x3.shape[1], mu.shape[0]
        dev = x.device
        raw = torch.empty(B, device=dev)
        muc = mu.detach().to(torch.float32).contiguous()
        list_cut = _rdf_list_cutoff(cutoff, coeff, mu_last)
        route = rdf_route(F, N, B, spacing, coeff, list_cut, cell_struct, mask)[0]
        ctx.ell = None
        if route == "frames":
            partial = torch.empty(int(lib.mdg_rdf_partial_size(F, N, B)), device=dev)
            check(lib.mdg_rdf_fwd_uniform(ptr(x3), F, N, C.byref(cell_struct), float(cutoff), ptr(mask), ptr(muc),
                                          float(spacing), float(coeff), B, ptr(raw), ptr(partial), stream_ptr(dev)),
                  "mdg_rdf_fwd")
        else:
            # large systems: pair search through the cell list (frames = groups of one list), every listed pair
            # counted on the fine integer grid; the gradient is a tabulated pair force over the same list
            x3 = x3.reshape(F * N, 3)
            cutoff = list_cut
            if route == "cell":
                # ... without materialising the list: search + count in one sweep over the cell bins (csrc/rdf_cell.hip);
                # the backward pass sweeps the same bins with the tabulated pair force
                ctx.ell = torch.empty(int(lib.mdg_rdf_cell_scratch(F, N, C.byref(cell_struct), float(cutoff))) + 4,
                                      dtype=torch.int32, device=dev)
                check(lib.mdg_rdf_fwd_cell(ptr(x3), F, N, C.byref(cell_struct), float(cutoff), ptr(muc), float(spacing),
                                           float(coeff), B, ptr(raw), ptr(ctx.ell), stream_ptr(dev)), "mdg_rdf_fwd_cell")
            else:
                ctx.ell = ell = build_ell(x3, cell_struct, cutoff, group=N)
                check(lib.mdg_rdf_fwd_ell(ptr(x3), F * N, C.byref(cell_struct), ptr(ell.col), ptr(ell.shift), ptr(ell.cnt),
                                          ell.max_nbr, ptr(muc), float(spacing), float(coeff), B, ptr(raw), stream_ptr(dev)),
                      "mdg_rdf_fwd_ell")
        ctx.args = (float(coeff), float(cutoff), cell_struct, mask, xyz.shape, float(spacing))
        ctx.save_for_backward(x3, muc)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        lib = _lib.load()
        x3, muc = ctx.saved_tensors
        coeff, cutoff, cell_struct, mask, shape, spacing = ctx.args
        if ctx.ell is not None:
            nodes = 4096
            table, u0, du = _rdf_pair_table(g_raw.detach().to(torch.float32), muc, coeff, cutoff, nodes)
            term = make_term(dict(kind=MDG_PAIR_TABLE, p=nodes, a=u0, phi=du, c=1.0), cutoff, 0, 2 * nodes, None)
            if torch.is_tensor(ctx.ell):                              # the forward call's cell bins (csrc/rdf_cell.hip)
                Nn = int(shape[-2])
                Fn = int(x3.shape[0]) // Nn                                # (saved positions are flat [F N, 3])
                gx = torch.empty_like(x3)
                check(lib.mdg_rdf_bwd_cell(Fn, Nn, C.byref(cell_struct), float(cutoff), C.byref(term), ptr(table),
                                           ptr(ctx.ell), ptr(gx), stream_ptr(x3.device)), "mdg_rdf_bwd_cell")
                return gx.reshape(shape), None, None, None, None, None, None, None
            o = pair_eval(ctx.ell, x3, term, table, energy=False, grad=True)
            return o["grad"].reshape(shape), None, None, None, None, None, None, None
        F, N, B = x3.shape[0], x3.shape[1], muc.shape[0]
        gx = torch.empty_like(x3)
        gr = g_raw.detach().to(torch.float32).contiguous()
        check(lib.mdg_rdf_bwd_uniform(ptr(x3), F, N, C.byref(cell_struct), cutoff, ptr(mask), ptr(muc), spacing,
                                      coeff, B, ptr(gr), ptr(gx), stream_ptr(x3.device)), "mdg_rdf_bwd")
        return gx.reshape(shape), None, None, None, None, None, None, None


# ----------------------------------------------------------------------------- angle distribution
ADF_CHUNK_BYTES = 1 << 30    # neighbour-list memory (col + shift + cnt) per chunk of frames in AdfRawFn
ADF_CHUNK_FRAMES = None      # when set: frames per chunk (tests force several chunks with it)


def _adf_chunk_frames(F, N, cell_struct, cutoff):
    if ADF_CHUNK_FRAMES is not None:
        return max(1, min(F, int(ADF_CHUNK_FRAMES)))
    per_frame = N * (8 * estimate_max_nbr(N, cell_struct, cutoff) + 4)
    return max(1, min(F, ADF_CHUNK_BYTES // per_frame, (2 ** 31 - 1) // N))


class AdfRawFn(torch.autograd.Function):
    """raw[b] = sum over frames and ordered triplets (i, j, k) of the neighbour list (j the centre, k != i) of
    exp(coeff (theta_ijk - mu_b)^2) -- the GaussianSmearing(angles).sum(0) of torchmd/observable.py:148 (csrc/adf.hip, K14).
    xyz: [F, N, 3] frames.  The lists are built in chunks of frames so that their memory stays near ADF_CHUNK_BYTES; the
    backward pass reuses the forward's list when there was one chunk and rebuilds the chunks one at a time otherwise, so one
    chunk's list is alive at any time."""

    @staticmethod
    def forward(ctx, xyz, mu, coeff, cutoff, cell_struct, mask, spacing):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N, B = x3.shape[0], x3.shape[1], mu.shape[0]
        dev = x3.device
        muc = mu.detach().to(device=dev, dtype=torch.float32).contiguous()
        fc = _adf_chunk_frames(F, N, cell_struct, cutoff)
        scratch = torch.empty(int(lib.mdg_adf_partial_size(fc, N, 1, B)), dtype=torch.int64, device=dev)
        raw, keep = None, None
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = build_ell(flat, cell_struct, cutoff, mask, group=N)
            part = torch.empty(B, device=dev)
            check(lib.mdg_adf_fwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), float(cutoff), ptr(ell.col), ptr(ell.cnt),
                                  ell.max_nbr, ptr(muc), float(spacing), float(coeff), B, ptr(part), ptr(scratch),
                                  stream_ptr(dev)), "mdg_adf_fwd")
            raw = part if raw is None else raw + part
            # only a single chunk's list is kept for the backward pass: with several chunks each list is released here
            # (stream order makes the caching allocator's reuse safe), so at most one chunk's list is alive at a time
            keep = ell if (f0 == 0 and f1 == F) else None
            del ell
        ctx.ell = keep
        ctx.args = (float(coeff), float(cutoff), cell_struct, mask, float(spacing), fc, xyz.shape)
        ctx.save_for_backward(x3, muc)
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        lib = _lib.load()
        x3, muc = ctx.saved_tensors
        coeff, cutoff, cell_struct, mask, spacing, fc, shape = ctx.args
        F, N, B = x3.shape[0], x3.shape[1], muc.shape[0]
        gr = g_raw.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x3)
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = ctx.ell if ctx.ell is not None else build_ell(flat, cell_struct, cutoff, mask, group=N)
            check(lib.mdg_adf_bwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), float(cutoff), ptr(ell.col), ptr(ell.cnt),
                                  ell.max_nbr, ptr(muc), float(spacing), float(coeff), B, ptr(gr), ptr(gx[f0:f1]),
                                  stream_ptr(x3.device)), "mdg_adf_bwd")
        return gx.reshape(shape), None, None, None, None, None, None


class AdfFramesFn(torch.autograd.Function):
    """raw[f, b] = the histogram of AdfRawFn for frame f alone (csrc/adf.hip, K35): the kernel side of
    observable.angle_distribution.per_frame; AdfRawFn's histogram is the sum of these rows.  xyz: [F, N, 3] frames.  The lists
    are built in the frame chunks of AdfRawFn (`_adf_chunk_frames`), kept for the backward pass when there was one chunk and
    rebuilt one at a time otherwise.  A frame's row depends on the frame and on the width of the list alone (the fixed-point
    scale is n_atoms max_nbr (max_nbr - 1) / 2 deep), and that width is `estimate_max_nbr`'s unless a row outgrows it, so a
    chunked run gives the bits of the single-chunk run.  Differentiable once with respect to the positions."""

    @staticmethod
    def forward(ctx, xyz, mu, coeff, cutoff, cell_struct, mask, spacing):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N, B = x3.shape[0], x3.shape[1], mu.shape[0]
        dev = x3.device
        muc = mu.detach().to(device=dev, dtype=torch.float32).contiguous()
        fc = _adf_chunk_frames(F, N, cell_struct, cutoff)
        raw, keep = torch.empty(F, B, device=dev), None
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = build_ell(flat, cell_struct, cutoff, mask, group=N)
            check(lib.mdg_adf_frames_fwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), float(cutoff), ptr(ell.col), ptr(ell.cnt),
                                         ell.max_nbr, ptr(muc), float(spacing), float(coeff), B, ptr(raw[f0:f1]),
                                         stream_ptr(dev)), "mdg_adf_frames_fwd")
            keep = ell if (f0 == 0 and f1 == F) else None
            del ell
        ctx.ell = keep
        ctx.args = (float(coeff), float(cutoff), cell_struct, mask, float(spacing), fc, xyz.shape)
        ctx.save_for_backward(x3, muc)
        return raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_raw):
        lib = _lib.load()
        x3, muc = ctx.saved_tensors
        coeff, cutoff, cell_struct, mask, spacing, fc, shape = ctx.args
        F, N, B = x3.shape[0], x3.shape[1], muc.shape[0]
        gr = g_raw.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x3)
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = ctx.ell if ctx.ell is not None else build_ell(flat, cell_struct, cutoff, mask, group=N)
            check(lib.mdg_adf_frames_bwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), float(cutoff), ptr(ell.col), ptr(ell.cnt),
                                         ell.max_nbr, ptr(muc), float(spacing), float(coeff), B, ptr(gr[f0:f1]), ptr(gx[f0:f1]),
                                         stream_ptr(x3.device)), "mdg_adf_frames_bwd")
        return gx.reshape(shape), None, None, None, None, None, None


# ----------------------------------------------------------------------------- bond-orientational order
BOND_ORDER_CHUNK_FRAMES = None      # when set: frames per chunk of BondOrderFn (tests force several chunks with it)


def _bond_order_chunk_frames(F, N, cell_struct, cutoff):
    if BOND_ORDER_CHUNK_FRAMES is not None:
        return max(1, min(F, int(BOND_ORDER_CHUNK_FRAMES)))
    return _adf_chunk_frames(F, N, cell_struct, cutoff)


class BondOrderFn(torch.autograd.Function):
    """(A [F, N, K], n [F, N]): the Steinhardt moments A_lm(i) = sum_j w(r_ij) Y_lm(s_ij) and n_i = sum_j w(r_ij) of every atom
    of xyz [F, N, 3] over its row of the neighbour list at `cutoff` (csrc/bond_order.hip, K29): the kernel side of
    observable.bond_order.  ls: 1..4 distinct l in 1..12, K = sum (2l+1).  The kernel writes A component-major; the returned A
    is the [F, N, K] view of that buffer.  The lists are built in chunks of frames like AdfRawFn's; the backward pass reuses
    the forward's list when there was one chunk and rebuilds the chunks one at a time otherwise.  The torch.ops layer serves
    the launches when it is loaded (_torch_ops.get()), the ctypes bindings otherwise: the same kernels either way.
    Differentiable once with respect to the positions."""

    @staticmethod
    def forward(ctx, xyz, ls, cutoff, r_in, cell_struct, mask):
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N = x3.shape[0], x3.shape[1]
        ls = tuple(int(l) for l in ls)
        K = sum(2 * l + 1 for l in ls)
        dev = x3.device
        tops = _torch_ops.get()
        lib = _lib.load()
        ls_c = (C.c_int32 * len(ls))(*ls)
        fc = _bond_order_chunk_frames(F, N, cell_struct, cutoff)
        A, n, keep = None, torch.empty(F, N, device=dev), None
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = build_ell(flat, cell_struct, cutoff, mask, group=N)
            if tops is not None:
                part, n_part = tops.bond_order_fwd(flat, f1 - f0, N, _torch_ops.cell_args(cell_struct), float(cutoff), float(r_in),
                                                   ell.col, ell.cnt, list(ls))
                n[f0:f1] = n_part.view(f1 - f0, N)
            else:
                part = torch.empty(K, (f1 - f0) * N, device=dev)
                check(lib.mdg_bond_order_fwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), float(cutoff), float(r_in), ptr(ell.col),
                                             ptr(ell.cnt), ell.max_nbr, ls_c, len(ls), ptr(part), ptr(n[f0:f1]), stream_ptr(dev)),
                      "mdg_bond_order_fwd")
            if f0 == 0 and f1 == F:
                A, keep = part.view(K, F, N), ell
            else:
                A = torch.empty(K, F, N, device=dev) if A is None else A
                A[:, f0:f1] = part.view(K, f1 - f0, N)
            del ell
        ctx.ell = keep
        ctx.args = (ls, float(cutoff), float(r_in), cell_struct, mask, fc, xyz.shape)
        ctx.save_for_backward(x3)
        return A.permute(1, 2, 0), n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gA, gn):
        (x3,) = ctx.saved_tensors
        ls, cutoff, r_in, cell_struct, mask, fc, shape = ctx.args
        F, N = x3.shape[0], x3.shape[1]
        tops = _torch_ops.get()
        lib = _lib.load()
        ls_c = (C.c_int32 * len(ls))(*ls)
        gA, gn = gA.detach().to(torch.float32), gn.detach().to(torch.float32)
        gx = torch.empty_like(x3)
        for f0 in range(0, F, fc):
            f1 = min(F, f0 + fc)
            flat = x3[f0:f1].reshape(-1, 3)
            ell = ctx.ell if ctx.ell is not None else build_ell(flat, cell_struct, cutoff, mask, group=N)
            ga, gw = gA[f0:f1].contiguous().view((f1 - f0) * N, -1), gn[f0:f1].contiguous().view(-1)        # gA row-major
            if tops is not None:
                gx[f0:f1] = tops.bond_order_bwd(flat, f1 - f0, N, _torch_ops.cell_args(cell_struct), cutoff, r_in, ell.col, ell.cnt,
                                                list(ls), ga, gw).view(f1 - f0, N, 3)
            else:
                check(lib.mdg_bond_order_bwd(ptr(flat), f1 - f0, N, C.byref(cell_struct), cutoff, r_in, ptr(ell.col), ptr(ell.cnt),
                                             ell.max_nbr, ls_c, len(ls), ptr(ga), ptr(gw), ptr(gx[f0:f1]), stream_ptr(x3.device)),
                      "mdg_bond_order_bwd")
        return gx.reshape(shape), None, None, None, None, None


# ----------------------------------------------------------------------------- pair virial (pressure)
class VirialFn(torch.autograd.Function):
    """W[f] = -sum_terms sum_pairs r phi'(r) of every frame of xyz [F, N, 3] (csrc/virial.hip, K15): the configurational part
    of thermo.Pressure.  theta = the terms' parameters packed in term order (torch.cat of the modules' parameters, so the
    gradient flows back into them like PairEnergyFn's); terms = MdgTerms of built-in forms whose theta_off follow that
    packing; masks keeps the terms' selection masks alive.  Differentiable once."""

    @staticmethod
    def forward(ctx, xyz, theta, cell_struct, terms, masks):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N = x3.shape[0], x3.shape[1]
        th = theta.detach().to(device=x3.device, dtype=torch.float32).contiguous()
        K = th.numel()
        ws = torch.empty(int(lib.mdg_virial_workspace(F, N, K)), device=x3.device)
        W = torch.empty(F, device=x3.device)
        check(lib.mdg_virial_fwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(terms), ptr(th) if K else None, ptr(W), ptr(ws),
                                 stream_ptr(x3.device)), "mdg_virial_fwd")
        ctx.args = (cell_struct, terms, masks, xyz.shape, theta.shape)
        ctx.save_for_backward(x3, th)
        return W

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gW):
        lib = _lib.load()
        x3, th = ctx.saved_tensors
        cell_struct, terms, masks, xshape, tshape = ctx.args
        F, N, K = x3.shape[0], x3.shape[1], th.numel()
        g = gW.detach().to(torch.float32).contiguous()
        ws = torch.empty(int(lib.mdg_virial_workspace(F, N, K)), device=x3.device)
        gx = torch.empty_like(x3)
        gth = torch.empty(K, device=x3.device) if K else None
        check(lib.mdg_virial_bwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(terms), ptr(th) if K else None, ptr(g), ptr(gx),
                                 ptr(gth), ptr(ws), stream_ptr(x3.device)), "mdg_virial_bwd")
        return gx.reshape(xshape), (gth.reshape(tshape) if K else None), None, None, None


# ----------------------------------------------------------------------------- pair energy of every frame (reweighting)
class EnergyFramesFn(torch.autograd.Function):
    """U[f] = sum_terms sum_pairs phi(r) of every frame of xyz [F, N, 3] (csrc/energy.hip, K31): the kernel side of
    thermo.PotentialEnergy.  theta, terms, masks: as VirialFn.  Differentiable once.  The backward pass runs the full-row
    sweep when the positions need a gradient and the once-per-pair parameters-only sweep otherwise (detached frames: the
    reweighting case); `EnergyFramesFn.last_route` names the one the last backward pass took ("full" | "theta")."""

    last_route = None

    @staticmethod
    def forward(ctx, xyz, theta, cell_struct, terms, masks):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N = x3.shape[0], x3.shape[1]
        th = theta.detach().to(device=x3.device, dtype=torch.float32).contiguous()
        K = th.numel()
        ws = torch.empty(int(lib.mdg_energy_frames_workspace(F, N, K)), device=x3.device)
        U = torch.empty(F, device=x3.device)
        check(lib.mdg_energy_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(terms), ptr(th) if K else None, ptr(U),
                                        ptr(ws), stream_ptr(x3.device)), "mdg_energy_frames_fwd")
        ctx.args = (cell_struct, terms, masks, xyz.shape, theta.shape)
        ctx.save_for_backward(x3, th)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        lib = _lib.load()
        x3, th = ctx.saved_tensors
        cell_struct, terms, masks, xshape, tshape = ctx.args
        F, N, K = x3.shape[0], x3.shape[1], th.numel()
        want_x, want_th = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and K > 0
        if not want_x and not want_th:
            return None, None, None, None, None
        g = gU.detach().to(torch.float32).contiguous()
        ws = torch.empty(int(lib.mdg_energy_frames_workspace(F, N, K)), device=x3.device)
        gx = torch.empty_like(x3) if want_x else None
        gth = torch.empty(K, device=x3.device) if want_th else None
        check(lib.mdg_energy_frames_bwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(terms), ptr(th) if K else None, ptr(g),
                                        ptr(gx), ptr(gth), ptr(ws), stream_ptr(x3.device)), "mdg_energy_frames_bwd")
        EnergyFramesFn.last_route = "full" if want_x else "theta"
        return (gx.reshape(xshape) if want_x else None), (gth.reshape(tshape) if want_th else None), None, None, None


# ----------------------------------------------------------------------------- tabulated pair energy of every frame
class EnergyTableFn(torch.autograd.Function):
    """U[f] = sum_pairs phi~(d^2) of every frame of xyz [F, N, 3] (csrc/energy_table.hip, K33): the kernel side of
    thermo.TabulatedEnergy.  table [2 p]: the nodes (phi_g, du dphi/du_g) on the grid u_g = u0 + g du in u = r^2 whose last node
    is cutoff^2 (p within EAM_TABLE_NODES); mask: [N, N] uint8 or None.  Differentiable once with respect to the positions and
    the nodes.  The backward pass runs the full-row sweep when the positions need a gradient and the once-per-pair nodes-only
    sweep otherwise (detached frames: the reweighting case); `EnergyTableFn.last_route` names the one the last backward pass
    took ("full" | "nodes").  `EnergyTableFn.last_below` is the device word (int32 [1]) of the last forward pass: the number of
    pairs below the first node, which take the constant first node value."""

    last_route = None
    last_below = None

    @staticmethod
    def forward(ctx, xyz, table, cell_struct, p, u0, du, cutoff, mask):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N = x3.shape[0], x3.shape[1]
        tb = table.detach().to(device=x3.device, dtype=torch.float32).contiguous()
        if tb.numel() != 2 * int(p):
            raise ValueError("EnergyTableFn: the table must hold 2 p = %d floats, got %d" % (2 * int(p), tb.numel()))
        ws = torch.empty(int(lib.mdg_energy_table_workspace(F, N, int(p))), device=x3.device)
        U = torch.empty(F, device=x3.device)
        below = torch.empty(1, dtype=torch.int32, device=x3.device)
        check(lib.mdg_energy_table_fwd(ptr(x3), F, N, C.byref(cell_struct), ptr(tb), int(p), float(u0), float(du), float(cutoff),
                                       ptr(mask), ptr(U), ptr(below), ptr(ws), stream_ptr(x3.device)), "mdg_energy_table_fwd")
        EnergyTableFn.last_below = below
        ctx.args = (cell_struct, int(p), float(u0), float(du), float(cutoff), mask, xyz.shape, table.shape)
        ctx.save_for_backward(x3, tb)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        lib = _lib.load()
        x3, tb = ctx.saved_tensors
        cell_struct, p, u0, du, cutoff, mask, xshape, tshape = ctx.args
        F, N = x3.shape[0], x3.shape[1]
        want_x, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not want_x and not want_t:
            return (None,) * 8
        g = gU.detach().to(torch.float32).contiguous()
        ws = torch.empty(int(lib.mdg_energy_table_workspace(F, N, p)), device=x3.device)
        gx = torch.empty_like(x3) if want_x else None
        gt = torch.empty(2 * p, device=x3.device) if want_t else None
        check(lib.mdg_energy_table_bwd(ptr(x3), F, N, C.byref(cell_struct), ptr(tb), p, u0, du, cutoff, ptr(mask), ptr(g),
                                       ptr(gx), ptr(gt), ptr(ws), stream_ptr(x3.device)), "mdg_energy_table_bwd")
        EnergyTableFn.last_route = "full" if want_x else "nodes"
        return ((gx.reshape(xshape) if want_x else None), (gt.reshape(tshape) if want_t else None)) + (None,) * 6


# ----------------------------------------------------------------------------- many-body energies of every frame: the scaffold
def _frames_begin(ctx, xyz):
    """The start of a frame energy's forward pass: (x3, U, side) = the detached contiguous frames [F, N, 3], the output [F]
    and side(cols) -> the [F, cols] buffer the launch fills for the backward pass (dU_dtheta, or rho) when one of the inputs
    1 .. 3 (the model's parameters) requires grad, else None."""
    require_gpu(xyz, "xyz")
    x3 = xyz.detach()
    x3 = x3 if x3.is_contiguous() else x3.contiguous()
    want = any(ctx.needs_input_grad[1:4])
    return x3, torch.empty(x3.shape[0], device=x3.device), lambda cols: x3.new_empty(x3.shape[0], cols) if want else None


def _frames_list_grad(x3, g, cell_struct, cutoff, evaluate):
    """gx[f] = g[f] * dU/dx of frame f through a term's list kernel: the frames stacked as groups of N behind a list searched
    at `cutoff`, in the frame chunks of AdfRawFn; evaluate(ell, flat, n_frames) -> the [n_frames N, 3] gradient."""
    F, N = x3.shape[0], x3.shape[1]
    gx = torch.empty_like(x3)
    fc = _adf_chunk_frames(F, N, cell_struct, cutoff)
    for f0 in range(0, F, fc):
        f1 = min(F, f0 + fc)
        flat = x3[f0:f1].reshape(-1, 3)
        ell = build_ell(flat, cell_struct, cutoff, None, group=N)
        torch.mul(evaluate(ell, flat, f1 - f0).view(f1 - f0, N, 3), g[f0:f1, None, None], out=gx[f0:f1])
        del ell
    return gx


def _frames_theta_bwd(ctx, g, dU, shapes):
    """The parameter part of a frame energy's backward pass: sum_f g[f] dU[f, :] (mdg_frames_theta_bwd), cut into the
    parameters of `shapes` (inputs 1, 2, ... of the autograd function) where they require grad."""
    lib = _lib.load()
    F, n = dU.shape
    out = torch.empty(n, device=dU.device)
    check(lib.mdg_frames_theta_bwd(ptr(g), ptr(dU), F, n, ptr(out), stream_ptr(dU.device)), "mdg_frames_theta_bwd")
    gth, pos = [], 0
    for k, shape in enumerate(shapes):
        m = int(np.prod(shape))
        gth.append(out[pos:pos + m].reshape(shape) if ctx.needs_input_grad[1 + k] else None)
        pos += m
    return gth


def _frames_backward(ctx, fn, gU, x3, xshape, cell_struct, side, params, cutoff, evaluate, routes):
    """The backward pass of a frame energy `fn`: (gx, gp) = the position gradient through the term's list kernel
    (_frames_list_grad at cutoff(), called on that route only) where xyz requires grad, and the three parameter gradients
    params(g) where the forward pass kept `side` (it is None when no parameter requires grad).  fn.last_route <- routes[0]
    (parameters alone), routes[1] (positions alone) or routes[2] (both)."""
    g = gU.detach().to(torch.float32).contiguous()
    gp = params(g) if side is not None else [None, None, None]
    gx = None
    if ctx.needs_input_grad[0]:
        gx = _frames_list_grad(x3, g, cell_struct, float(cutoff()), evaluate).reshape(xshape)
    fn.last_route = (routes[2] if side is not None else routes[1]) if gx is not None else routes[0]
    return gx, gp


# ----------------------------------------------------------------------------- Stillinger-Weber energy of every frame
SW_FRAMES_MAX_ATOMS = 1024


def sw_frames_row_cap():
    """Neighbours inside a sigma that csrc/sw_frames.hip keeps per atom; a frame with a longer row comes out NaN."""
    return int(_lib.load().mdg_sw_frames_row_cap())


class SWFramesFn(torch.autograd.Function):
    """U[f] = the Stillinger-Weber energy of every frame of xyz [F, N, 3] (csrc/sw_frames.hip, K34): the kernel side of
    thermo.StillingerWeberEnergy.  epsilon, sigma, lam: the module's parameters (or buffers), through which the gradient flows;
    theta: the device float [3] = (epsilon, sigma, lam) the kernel reads; consts: MdgSWConsts; list_scale: the position
    gradient's list is searched at list_scale a sigma.  Differentiable once.

    When a parameter requires grad the forward launch also emits dU_dtheta [F, 3], and the parameter part of the backward pass
    is the fixed-order sum_f gU[f] dU_dtheta[f] (mdg_frames_theta_bwd): no pair or triplet is visited again.  The position
    gradient, off the reweighting path, goes through the list kernel of K23 (mdg_sw_eval): the frames stacked as groups of N
    behind a list searched at list_scale a sigma (sigma of the forward call, read on the host there: one read per backward
    pass, none on the parameters-only route), in the frame chunks of AdfRawFn, every frame's rows scaled by gU[f].
    `SWFramesFn.last_route` names what the last backward pass ran: "theta" (the sum alone: detached frames, the reweighting
    case) or "full" (the list kernel as well)."""

    last_route = None

    @staticmethod
    def forward(ctx, xyz, epsilon, sigma, lam, theta, cell_struct, consts, list_scale):
        lib = _lib.load()
        x3, U, side = _frames_begin(ctx, xyz)
        _check_theta(theta)
        F, N, dU = x3.shape[0], x3.shape[1], side(3)
        check(lib.mdg_sw_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(consts), ptr(theta), ptr(U), ptr(dU),
                                    stream_ptr(x3.device)), "mdg_sw_frames_fwd")
        ctx.args = (cell_struct, consts, float(list_scale), xyz.shape, [p.shape for p in (epsilon, sigma, lam)])
        ctx.save_for_backward(x3, theta.detach() if ctx.needs_input_grad[0] else None, dU)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        x3, th, dU = ctx.saved_tensors
        cell_struct, consts, list_scale, xshape, pshapes = ctx.args

        def evaluate(ell, flat, nf):
            return sw_eval(ell, flat, consts, th, energy=False, grad=True)["grad"]
        gx, gth = _frames_backward(ctx, SWFramesFn, gU, x3, xshape, cell_struct, dU,
                                   lambda g: _frames_theta_bwd(ctx, g, dU, pshapes), lambda: list_scale * consts.a * float(th[1]), evaluate,
                                   ("theta", "full", "full"))
        return (gx,) + tuple(gth) + (None, None, None, None)


# ----------------------------------------------------------------------------- embedded-atom energy of every frame
EAM_FRAMES_MAX_ATOMS = 1024


def eam_table_frames_lds_floats():
    """The largest pair-and-density table set (in floats) that csrc/eam_frames.hip reads from a workgroup copy in LDS."""
    return int(_lib.load().mdg_eam_table_frames_lds_floats())


class EAMTableFramesFn(torch.autograd.Function):
    """U[f] = the tabulated embedded-atom energy of every frame of xyz [F, N, 3] (csrc/eam_frames.hip, K36): the kernel side of
    thermo.EAMEnergy for interface.EAM.  pair_nodes, density_nodes, embed_nodes: the module's node tensors, through which the
    gradient flows; tables: the flat float32 device image the kernel reads; types: device int32 [N], one frame's species;
    consts: MdgEAMTableConsts.  Differentiable once.

    When a node tensor requires grad the forward launch also keeps rho [F, N], and the node part of the backward pass is
    mdg_eam_table_frames_nodes_bwd: one more walk over the frames with a fixed-point scatter, no list and no host read.  The
    position gradient, off the reweighting path, goes through the list kernel of K27 (mdg_eam_table_eval) on the frames stacked
    as groups of N, every frame's rows scaled by gU[f]; with both wanted each takes its own route.
    `EAMTableFramesFn.last_route` names what the last backward pass ran: "nodes" (detached frames, the reweighting case),
    "positions" or "full" (both).  `table_mode` (class attribute): -1 = the entry point chooses where the r-tables are read from
    (a workgroup copy in LDS for small sets in the wave-per-frame shape, global memory otherwise), 0 = global memory, 1 = LDS."""

    last_route = None
    table_mode = -1

    @staticmethod
    def forward(ctx, xyz, pair_nodes, density_nodes, embed_nodes, tables, types, cell_struct, consts):
        lib = _lib.load()
        x3, U, side = _frames_begin(ctx, xyz)
        require_gpu(tables, "tables")
        require_gpu(types, "types", dtype=torch.int32)
        F, N = x3.shape[0], x3.shape[1]
        if tables.numel() != eam_table_size(consts) or types.numel() != N:
            raise ValueError("EAMTableFramesFn: tables must hold %d floats and types %d entries (got %d, %d)"
                             % (eam_table_size(consts), N, tables.numel(), types.numel()))
        rho = side(N)
        tb = tables.detach()
        if rho is not None or ctx.needs_input_grad[0]:
            tb = tb.clone()                                   # (the module's mirror is rewritten when the nodes are stepped)
        check(lib.mdg_eam_table_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), ptr(types), C.byref(consts), ptr(tb),
                                           int(EAMTableFramesFn.table_mode), ptr(U), ptr(rho), stream_ptr(x3.device)),
              "mdg_eam_table_frames_fwd")
        ctx.args = (cell_struct, consts, xyz.shape, [p.shape for p in (pair_nodes, density_nodes, embed_nodes)],
                    [p.dtype for p in (pair_nodes, density_nodes, embed_nodes)])
        ctx.save_for_backward(x3, tb, types, rho)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        lib = _lib.load()
        x3, tb, types, rho = ctx.saved_tensors
        cell_struct, consts, xshape, pshapes, pdtypes = ctx.args
        F, N = x3.shape[0], x3.shape[1]

        def nodes(g):
            out = torch.empty(eam_table_size(consts), device=x3.device)
            fx = torch.empty(eam_table_fx_size(consts), dtype=torch.int64, device=x3.device)
            check(lib.mdg_eam_table_frames_nodes_bwd(ptr(x3), F, N, C.byref(cell_struct), ptr(types), C.byref(consts), ptr(tb),
                                                     ptr(g), ptr(rho), ptr(out), ptr(fx), stream_ptr(x3.device)),
                  "mdg_eam_table_frames_nodes_bwd")
            gn, pos = [None, None, None], 0
            for k in range(3):
                n = int(np.prod(pshapes[k]))
                if ctx.needs_input_grad[1 + k]:
                    gn[k] = out[pos:pos + n].reshape(pshapes[k]).to(pdtypes[k])
                pos += n
            return gn

        def evaluate(ell, flat, nf):
            return eam_table_eval(ell, flat, types.repeat(nf), consts, tb, energy=False, grad=True)["grad"]
        gx, gn = _frames_backward(ctx, EAMTableFramesFn, gU, x3, xshape, cell_struct, rho, nodes, lambda: consts.rc, evaluate,
                                  ("nodes", "positions", "full"))
        return (gx,) + tuple(gn) + (None, None, None, None)


class EAMFramesFn(torch.autograd.Function):
    """U[f] = the Sutton-Chen energy of every frame of xyz [F, N, 3] (csrc/eam_frames.hip, K37): the kernel side of
    thermo.EAMEnergy for interface.SuttonChen.  epsilon, a, c: the module's parameters (or buffers), through which the gradient
    flows; theta: the device float [3] = (epsilon, a, c) the kernel reads; consts: MdgEAMConsts.  Differentiable once.

    When a parameter requires grad the forward launch also emits dU_dtheta [F, 3], and the parameter part of the backward pass
    is the fixed-order sum_f gU[f] dU_dtheta[f] (mdg_frames_theta_bwd): no pair is visited again.  The
    position gradient, off the reweighting path, goes through the list kernel of K24 (mdg_eam_eval) on the frames stacked as
    groups of N, every frame's rows scaled by gU[f].  `EAMFramesFn.last_route` names what the last backward pass ran: "theta"
    (the sum alone: detached frames, the reweighting case), "positions" or "full" (both)."""

    last_route = None

    @staticmethod
    def forward(ctx, xyz, epsilon, a, c, theta, cell_struct, consts):
        lib = _lib.load()
        x3, U, side = _frames_begin(ctx, xyz)
        _check_theta(theta)
        F, N, dU = x3.shape[0], x3.shape[1], side(3)
        check(lib.mdg_eam_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(consts), ptr(theta), ptr(U), ptr(dU),
                                     stream_ptr(x3.device)), "mdg_eam_frames_fwd")
        ctx.args = (cell_struct, consts, xyz.shape, [p.shape for p in (epsilon, a, c)])
        ctx.save_for_backward(x3, theta.detach() if ctx.needs_input_grad[0] else None, dU)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        x3, th, dU = ctx.saved_tensors
        cell_struct, consts, xshape, pshapes = ctx.args

        def evaluate(ell, flat, nf):
            return eam_eval(ell, flat, consts, th, energy=False, grad=True)["grad"]
        gx, gth = _frames_backward(ctx, EAMFramesFn, gU, x3, xshape, cell_struct, dU,
                                   lambda g: _frames_theta_bwd(ctx, g, dU, pshapes), lambda: consts.rc, evaluate,
                                   ("theta", "positions", "full"))
        return (gx,) + tuple(gth) + (None, None, None)


# ----------------------------------------------------------------------------- Tersoff energy of every frame
TERSOFF_FRAMES_MAX_ATOMS = 1024


def tersoff_frames_row_cap():
    """Neighbours inside R + D that csrc/tersoff_frames.hip keeps per atom; a frame with a longer row comes out NaN."""
    return int(_lib.load().mdg_tersoff_frames_row_cap())


class TersoffFramesFn(torch.autograd.Function):
    """U[f] = the Tersoff energy of every frame of xyz [F, N, 3] (csrc/tersoff_frames.hip, K38): the kernel side of
    thermo.TersoffEnergy for interface.Tersoff.  A, B, h: the module's parameters (or buffers), through which the gradient
    flows; theta: the device float [3] = (A, B, h) the kernel reads; consts: MdgTersoffConsts.  Differentiable once.

    When a parameter requires grad the forward launch also emits dU_dtheta [F, 3], and the parameter part of the backward pass
    is the fixed-order sum_f gU[f] dU_dtheta[f] (mdg_frames_theta_bwd): no bond is visited again.  The position gradient, off
    the reweighting path, goes through the list kernels of K25 (mdg_tersoff_eval) on the frames stacked as groups of N behind
    a list searched at R + D, bond_work sized per chunk, every frame's rows scaled by gU[f].  `TersoffFramesFn.last_route`
    names what the last backward pass ran: "theta" (the sum alone: detached frames, the reweighting case) or "full" (the list
    kernels as well)."""

    last_route = None

    @staticmethod
    def forward(ctx, xyz, A, B, h, theta, cell_struct, consts):
        lib = _lib.load()
        x3, U, side = _frames_begin(ctx, xyz)
        _check_theta(theta)
        F, N, dU = x3.shape[0], x3.shape[1], side(3)
        th = theta.detach()
        if ctx.needs_input_grad[0]:
            th = th.clone()                                   # (the module's mirror is rewritten when the parameters are stepped)
        check(lib.mdg_tersoff_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), C.byref(consts), ptr(th), ptr(U), ptr(dU),
                                         stream_ptr(x3.device)), "mdg_tersoff_frames_fwd")
        ctx.args = (cell_struct, consts, xyz.shape, [p.shape for p in (A, B, h)])
        ctx.save_for_backward(x3, th if ctx.needs_input_grad[0] else None, dU)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        x3, th, dU = ctx.saved_tensors
        cell_struct, consts, xshape, pshapes = ctx.args

        def evaluate(ell, flat, nf):
            return tersoff_eval(ell, flat, consts, th, energy=False, grad=True)["grad"]
        gx, gth = _frames_backward(ctx, TersoffFramesFn, gU, x3, xshape, cell_struct, dU,
                                   lambda g: _frames_theta_bwd(ctx, g, dU, pshapes), lambda: consts.R + consts.D, evaluate,
                                   ("theta", "full", "full"))
        return (gx,) + tuple(gth) + (None, None, None)


class TersoffMultiFramesFn(torch.autograd.Function):
    """U[f] = the multi-species Tersoff energy of every frame of xyz [F, N, 3] (csrc/tersoff_frames.hip, K38): the kernel side
    of thermo.TersoffEnergy for interface.TersoffMulti.  A [S, S], B [S, S], h [S]: the module's parameters (or buffers), through
    which the gradient flows; tables: the device table image the kernel reads (TersoffMulti._tables()); types: device int32
    [N], one frame's species; cutoff: max (R + D), where the position gradient's list is searched.  Differentiable once.

    The routes are TersoffFramesFn's: dU_dtheta [F, 2 S^2 + S] from the forward launch in the order (A.flat, B.flat, h), the
    parameter part of the backward pass by mdg_frames_theta_bwd, the position gradient through the list kernels of K26
    (mdg_tersoff_multi_eval) with `types` tiled per chunk.  `TersoffMultiFramesFn.last_route`: "theta" or "full"."""

    last_route = None

    @staticmethod
    def forward(ctx, xyz, A, B, h, tables, types, n_species, cell_struct, cutoff):
        lib = _lib.load()
        x3, U, side = _frames_begin(ctx, xyz)
        require_gpu(tables, "tables")
        require_gpu(types, "types", dtype=torch.int32)
        F, N, S = x3.shape[0], x3.shape[1], int(n_species)
        if not 1 <= S <= TERSOFF_MULTI_MAX_SPECIES:
            raise ValueError("mdgrad_amd: n_species must lie in [1, %d] (got %r)" % (TERSOFF_MULTI_MAX_SPECIES, n_species))
        if tables.numel() != 8 * S * (S + 1) or not tables.is_contiguous() or types.numel() != N or not types.is_contiguous():
            raise ValueError("TersoffMultiFramesFn: tables must hold %d floats and types %d entries (got %d, %d)"
                             % (8 * S * (S + 1), N, tables.numel(), types.numel()))
        dU = side(2 * S * S + S)
        tb = tables.detach()
        if ctx.needs_input_grad[0]:
            tb = tb.clone()                                   # (the module's mirror is rewritten when the parameters are stepped)
        check(lib.mdg_tersoff_multi_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), ptr(types), S, ptr(tb), ptr(U), ptr(dU),
                                               stream_ptr(x3.device)), "mdg_tersoff_multi_frames_fwd")
        ctx.args = (cell_struct, S, float(cutoff), xyz.shape, [p.shape for p in (A, B, h)])
        ctx.save_for_backward(x3, tb if ctx.needs_input_grad[0] else None, types if ctx.needs_input_grad[0] else None, dU)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gU):
        x3, tb, types, dU = ctx.saved_tensors
        cell_struct, S, cutoff, xshape, pshapes = ctx.args

        def evaluate(ell, flat, nf):
            return tersoff_multi_eval(ell, flat, types.repeat(nf), S, tb, energy=False, grad=True)["grad"]
        gx, gth = _frames_backward(ctx, TersoffMultiFramesFn, gU, x3, xshape, cell_struct, dU,
                                   lambda g: _frames_theta_bwd(ctx, g, dU, pshapes), lambda: cutoff, evaluate,
                                   ("theta", "full", "full"))
        return (gx,) + tuple(gth) + (None, None, None, None, None)


# ----------------------------------------------------------------------------- smeared pair count of every frame
RDF_FRAMES_MAX_ATOMS, RDF_FRAMES_MAX_BINS = 1024, 1024


def rdf_frames_reach(spacing, coeff):
    """R of csrc/rdf_frames.hip: a pair is summed over the 2R + 1 centres around its nearest one, R = ceil(5.3 / (s spacing)),
    s = sqrt(-coeff log2 e) -- the float32 arithmetic of the library."""
    f = np.float32
    s2 = f(-f(coeff) * f(1.4426950408889634))
    return int(np.ceil(f(5.3) / f(np.sqrt(s2) * f(spacing))))


class RdfFramesFn(torch.autograd.Function):
    """raw[f, k] = sum_{i<j, 0<d<cutoff} exp(coeff (d - mu_k)^2) of every frame of xyz [F, N, 3] (csrc/rdf_frames.hip, K32):
    the kernel side of observable.rdf.per_frame.  mu [nbins]: equally spaced centres on the device; mask: [N, N] uint8 or
    None.  Differentiable once with respect to the positions."""

    @staticmethod
    def forward(ctx, xyz, mu, spacing, coeff, cutoff, cell_struct, mask):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N, B = x3.shape[0], x3.shape[1], mu.numel()
        raw = torch.empty(F, B, device=x3.device)
        check(lib.mdg_rdf_frames_fwd(ptr(x3), F, N, C.byref(cell_struct), float(cutoff), ptr(mask), ptr(mu), float(spacing),
                                     float(coeff), B, ptr(raw), stream_ptr(x3.device)), "mdg_rdf_frames_fwd")
        ctx.args = (float(spacing), float(coeff), float(cutoff), cell_struct, mask, xyz.shape)
        ctx.save_for_backward(x3, mu)
        return raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_raw):
        lib = _lib.load()
        x3, mu = ctx.saved_tensors
        spacing, coeff, cutoff, cell_struct, mask, shape = ctx.args
        F, N, B = x3.shape[0], x3.shape[1], mu.numel()
        g = g_raw.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x3)
        check(lib.mdg_rdf_frames_bwd(ptr(x3), F, N, C.byref(cell_struct), cutoff, ptr(mask), ptr(mu), spacing, coeff, B, ptr(g),
                                     ptr(gx), stream_ptr(x3.device)), "mdg_rdf_frames_bwd")
        return gx.reshape(shape), None, None, None, None, None, None


# ----------------------------------------------------------------------------- static structure factor
class SkFn(torch.autograd.Function):
    """S[f, b] = mean over bin b of |sum_i w_i exp(i k.x_fi)|^2 / norm for every frame of xyz [F, N, 3] (csrc/sk.hip, K16):
    the kernel side of observable.structure_factor.  kvec int32 [M, 3] (integer wave vectors sorted by bin) and seg int32
    [B + 1] (the bins' segment offsets) live on the device; weights [N] or None, norm = sum of the squared weights.  The
    weights and wave vectors are constants; differentiable once with respect to the positions (rho is recomputed)."""

    @staticmethod
    def forward(ctx, xyz, cell_struct, weights, norm, kvec, seg):
        lib = _lib.load()
        require_gpu(xyz, "xyz")
        x3 = xyz.detach()
        x3 = x3 if x3.is_contiguous() else x3.contiguous()
        F, N, M, B = x3.shape[0], x3.shape[1], kvec.shape[0], seg.numel() - 1
        ws = torch.empty(int(lib.mdg_sk_workspace(F, N, M)), device=x3.device)
        S = torch.empty(F, B, device=x3.device)
        check(lib.mdg_sk_fwd(ptr(x3), F, N, C.byref(cell_struct), ptr(weights), float(norm), ptr(kvec), M, ptr(seg), B, ptr(S),
                             ptr(ws), stream_ptr(x3.device)), "mdg_sk_fwd")
        ctx.args = (cell_struct, weights, norm, kvec, seg, xyz.shape)
        ctx.save_for_backward(x3)
        return S

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gS):
        lib = _lib.load()
        (x3,) = ctx.saved_tensors
        cell_struct, weights, norm, kvec, seg, xshape = ctx.args
        F, N, M, B = x3.shape[0], x3.shape[1], kvec.shape[0], seg.numel() - 1
        g = gS.detach().to(torch.float32).contiguous()
        ws = torch.empty(int(lib.mdg_sk_workspace(F, N, M)), device=x3.device)
        gx = torch.empty_like(x3)
        check(lib.mdg_sk_bwd(ptr(x3), F, N, C.byref(cell_struct), ptr(weights), float(norm), ptr(kvec), M, ptr(seg), B, ptr(g),
                             ptr(gx), ptr(ws), stream_ptr(x3.device)), "mdg_sk_bwd")
        return gx.reshape(xshape), None, None, None, None, None


# ----------------------------------------------------------------------------- velocity observables
class VacfFn(torch.autograd.Function):
    """vacf[t] = mean(v[t:] * v[:-t]) for t = 0 .. n_lags-1 (torchmd/observable.py:153-163) as one fused pass."""

    @staticmethod
    def forward(ctx, vel, n_lags):
        lib = _lib.load()
        require_gpu(vel, "vel")
        v = vel.detach().contiguous()
        T, M = v.shape[0], v[0].numel()
        out = torch.empty(n_lags, device=v.device)
        ws = torch.empty(int(lib.mdg_vacf_workspace(n_lags)), device=v.device)
        check(lib.mdg_vacf_fwd(ptr(v), T, M, n_lags, ptr(out), ptr(ws), stream_ptr(v.device)), "mdg_vacf_fwd")
        ctx.save_for_backward(v)
        ctx.n_lags = n_lags
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (v,) = ctx.saved_tensors
        gv = torch.empty_like(v)
        gc = g.detach().to(torch.float32).contiguous()
        check(lib.mdg_vacf_bwd(ptr(v), ptr(gc), v.shape[0], v[0].numel(), ctx.n_lags, ptr(gv), stream_ptr(v.device)),
              "mdg_vacf_bwd")
        return gv, None


class MsdFn(torch.autograd.Function):
    """M_2[row, tau] (and M_4 with fourth=True) of x [n_batch, T, n_cols, 3] over the lags tau = 0 .. n_lags-1 (csrc/msd.hip,
    K17): the kernel side of observable.msd.  The n_cols columns are n_cols / group replicas of `group` atoms; row =
    batch * (n_cols / group) + replica.  weights [group] on the device or None; a constant.  Returns (M_2, M_4 or None), each
    [rows, n_lags].  Differentiable once with respect to the positions.  The torch.ops layer serves it when it is loaded
    (_torch_ops.get()), the ctypes bindings otherwise: the same kernels either way."""

    @staticmethod
    def forward(ctx, x, group, weights, n_lags, origin_stride, fourth):
        require_gpu(x, "x")
        x4 = x.detach()
        x4 = x4 if x4.is_contiguous() else x4.contiguous()
        nb, T, nc = x4.shape[0], x4.shape[1], x4.shape[2]
        tops = _torch_ops.get()
        if tops is not None:
            m2, m4 = tops.msd_fwd(x4, int(group), weights, int(n_lags), int(origin_stride), bool(fourth))
            m4 = m4 if fourth else None                     # (the op returns an empty tensor there)
        else:
            lib = _lib.load()
            rows = nb * (nc // group if group > 0 and nc % group == 0 else 0)
            m2 = torch.empty(rows, n_lags, device=x4.device)
            m4 = torch.empty(rows, n_lags, device=x4.device) if fourth else None
            ws = torch.empty(max(int(lib.mdg_msd_workspace(nb, nc, group, n_lags, int(fourth))), 2), device=x4.device)
            check(lib.mdg_msd_fwd(ptr(x4), nb, T, nc, group, ptr(weights), n_lags, origin_stride, ptr(m2), ptr(m4), ptr(ws),
                                  stream_ptr(x4.device)), "mdg_msd_fwd")
        ctx.args = (group, weights, n_lags, origin_stride, fourth, x.shape)
        ctx.save_for_backward(x4)
        return m2, m4

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g2, g4):
        (x4,) = ctx.saved_tensors
        group, weights, n_lags, origin_stride, fourth, xshape = ctx.args
        nb, T, nc = x4.shape[0], x4.shape[1], x4.shape[2]
        rows = nb * (nc // group)
        g2 = (torch.zeros(rows, n_lags, device=x4.device) if g2 is None else g2.detach().to(torch.float32).contiguous())
        g4 = None if (not fourth or g4 is None) else g4.detach().to(torch.float32).contiguous()
        tops = _torch_ops.get()
        if tops is not None:
            gx = tops.msd_bwd(x4, int(group), weights, int(n_lags), int(origin_stride), g2, g4)
        else:
            lib = _lib.load()
            gx = torch.empty_like(x4)
            ws = torch.empty(max(int(lib.mdg_msd_workspace(nb, nc, group, n_lags, int(fourth))), 2), device=x4.device)
            check(lib.mdg_msd_bwd(ptr(x4), nb, T, nc, group, ptr(weights), n_lags, origin_stride, ptr(g2), ptr(g4), ptr(gx),
                                  ptr(ws), stream_ptr(x4.device)), "mdg_msd_bwd")
        return gx.reshape(xshape), None, None, None, None, None


ISF_WS_BYTES = 1 << 30          # IsfFn: rows per launch are chosen so that one call's workspace stays below this


class IsfFn(torch.autograd.Function):
    """F[row, b, tau] of x [n_batch, T, n_cols, 3] over the lags tau = 0 .. n_lags-1 (csrc/isf.hip, K18): the kernel side of
    observable.intermediate_scattering.  kind 0: coherent, 1: self.  The n_cols columns are n_cols / group replicas of `group`
    atoms; row = batch * (n_cols / group) + replica.  kvec int32 [M, 3], seg int32 [B + 1] on the device and seg_host (its
    host copy) as for SkFn; weights [group] on the device or None, norm = sum of the squared weights; all constants.  Returns
    [rows, B, n_lags].  The rows go through the kernels in chunks (whole batch entries, or runs of replicas of one batch entry)
    whose workspace stays below ISF_WS_BYTES; a row's result does not depend on the chunking.  Differentiable once with respect
    to the positions.  The torch.ops layer serves it when it is loaded (_torch_ops.get()), the ctypes bindings otherwise."""

    @staticmethod
    def _chunks(kind, nb, reps, T, group, M, n_lags):
        """[(b0, b1, r0, r1)]: batch entries b0:b1 with replicas r0:r1 per call."""
        per_row = 4 * max(int(_lib.load().mdg_isf_workspace(kind, 1, T, group, M, n_lags)), 1)
        n = max(1, ISF_WS_BYTES // per_row)
        if n >= reps:
            step = min(nb, n // reps)
            return [(b0, min(nb, b0 + step), 0, reps) for b0 in range(0, nb, step)]
        return [(b, b + 1, r0, min(reps, r0 + n)) for b in range(nb) for r0 in range(0, reps, n)]

    @staticmethod
    def forward(ctx, x, kind, group, cell_struct, weights, norm, kvec, seg, seg_host, n_lags, origin_stride):
        require_gpu(x, "x")
        x4 = x.detach()
        x4 = x4 if x4.is_contiguous() else x4.contiguous()
        nb, T, nc = x4.shape[0], x4.shape[1], x4.shape[2]
        if group < 1 or nc % group:
            raise ValueError("IsfFn: the columns (%d) must be a multiple of the group (%d)" % (nc, group))
        reps, M, B = nc // group, kvec.shape[0], seg.numel() - 1
        kind, group, n_lags, origin_stride = int(kind), int(group), int(n_lags), int(origin_stride)
        tops = _torch_ops.get()
        lib = _lib.load()
        cell = _torch_ops.cell_args(cell_struct) if tops is not None else None
        chunks = IsfFn._chunks(kind, nb, reps, T, group, M, n_lags)
        F = None if len(chunks) == 1 else torch.empty(nb, reps, B, n_lags, device=x4.device)
        for b0, b1, r0, r1 in chunks:
            xs = x4[b0:b1]
            if tops is not None:
                out = tops.isf_fwd(xs, kind, group, r0, r1 - r0, cell, weights, float(norm), kvec, seg, seg_host, n_lags,
                                   origin_stride)
            else:
                rows = (b1 - b0) * (r1 - r0)
                out = torch.empty(rows, B, n_lags, device=x4.device)
                ws = torch.empty(max(int(lib.mdg_isf_workspace(kind, rows, T, group, M, n_lags)), 1), device=x4.device)
                check(lib.mdg_isf_fwd(kind, ptr(xs), b1 - b0, T, nc, group, r0, r1 - r0, C.byref(cell_struct), ptr(weights),
                                      float(norm), ptr(kvec), M, ptr(seg), B, n_lags, origin_stride, ptr(out), ptr(ws),
                                      stream_ptr(x4.device)), "mdg_isf_fwd")
            if F is None:
                F = out
            else:
                F[b0:b1, r0:r1] = out.reshape(b1 - b0, r1 - r0, B, n_lags)
        ctx.args = (kind, group, cell_struct, weights, norm, kvec, seg, seg_host, n_lags, origin_stride, x.shape)
        ctx.save_for_backward(x4)
        return F.reshape(nb * reps, B, n_lags)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF):
        (x4,) = ctx.saved_tensors
        kind, group, cell_struct, weights, norm, kvec, seg, seg_host, n_lags, origin_stride, xshape = ctx.args
        nb, T, nc = x4.shape[0], x4.shape[1], x4.shape[2]
        reps, M, B = nc // group, kvec.shape[0], seg.numel() - 1
        g = gF.detach().to(torch.float32).reshape(nb, reps, B, n_lags)
        tops = _torch_ops.get()
        lib = _lib.load()
        cell = _torch_ops.cell_args(cell_struct) if tops is not None else None
        gx = torch.empty_like(x4)                       # every element is written by exactly one call below
        for b0, b1, r0, r1 in IsfFn._chunks(kind, nb, reps, T, group, M, n_lags):
            xs, gs, gxs = x4[b0:b1], g[b0:b1, r0:r1], gx[b0:b1]
            gs = gs if gs.is_contiguous() else gs.contiguous()
            if tops is not None:
                tops.isf_bwd(xs, kind, group, r0, r1 - r0, cell, weights, float(norm), kvec, seg, seg_host, n_lags,
                             origin_stride, gs, gxs)
            else:
                rows = (b1 - b0) * (r1 - r0)
                ws = torch.empty(max(int(lib.mdg_isf_workspace(kind, rows, T, group, M, n_lags)), 1), device=x4.device)
                check(lib.mdg_isf_bwd(kind, ptr(xs), b1 - b0, T, nc, group, r0, r1 - r0, C.byref(cell_struct), ptr(weights),
                                      float(norm), ptr(kvec), M, ptr(seg), B, n_lags, origin_stride, ptr(gs), ptr(gxs), ptr(ws),
                                      stream_ptr(x4.device)), "mdg_isf_bwd")
        return (gx.reshape(xshape),) + (None,) * 10


class TemperatureFn(torch.autograd.Function):
    """Kinetic temperature sum_n m_n |v_n|^2 / n_dof of every frame of v [F, N, 3] in one launch."""

    @staticmethod
    def forward(ctx, vel, mass, n_dof):
        lib = _lib.load()
        require_gpu(vel, "vel")
        v = vel.detach().contiguous()
        F, N = v.shape[0], v.shape[1]
        out = torch.empty(F, device=v.device)
        check(lib.mdg_temperature(ptr(v), ptr(mass), F, N, float(n_dof), ptr(out), stream_ptr(v.device)), "mdg_temperature")
        ctx.save_for_backward(v, mass)
        ctx.n_dof = float(n_dof)
        return out

    @staticmethod
    def backward(ctx, g):
        v, mass = ctx.saved_tensors
        return (2.0 / ctx.n_dof) * g[:, None, None] * mass[None, :, None] * v, None, None


# ----------------------------------------------------------------------------- thermostat algebra
def nhc_rhs(v, f, pv, mass, Q, T, n_dof, n_rep, n_group):
    """(a, dpv) of NoseHooverChain.forward given the force (torchmd/md.py:221-240), one launch.
    T: device tensor [1] (read by the kernel, so that a captured graph follows update_T)."""
    lib = _lib.load()
    for t_, nm in ((v, "v"), (f, "f"), (pv, "p_v")):
        require_gpu(t_, nm)
    v, f, pv = v.contiguous(), f.contiguous(), pv.contiguous()
    a, dpv = torch.empty_like(v), torch.empty_like(pv)
    check(lib.mdg_nhc_rhs(ptr(v), ptr(f), ptr(pv), ptr(mass), ptr(Q), ptr(T), float(n_dof), int(n_rep),
                          int(n_group), int(pv.shape[-1]), ptr(a), ptr(dpv), stream_ptr(v.device)), "mdg_nhc_rhs")
    return a, dpv


def nhc_vjp(v, pv, lv, lq, lp, mass, Q, n_rep, n_group):
    """(Gv, Gp): thermostat part of the vjp of the NHC right-hand side, one launch."""
    lib = _lib.load()
    for t_, nm in ((v, "v"), (lv, "lv"), (lq, "lq")):
        require_gpu(t_, nm)
    v, pv, lv, lq, lp = v.contiguous(), pv.contiguous(), lv.contiguous(), lq.contiguous(), lp.contiguous()
    Gv, Gp = torch.empty_like(v), torch.empty_like(pv)
    check(lib.mdg_nhc_vjp(ptr(v), ptr(pv), ptr(lv), ptr(lq), ptr(lp), ptr(mass), ptr(Q), int(n_rep), int(n_group),
                          int(pv.shape[-1]), ptr(Gv), ptr(Gp), stream_ptr(v.device)), "mdg_nhc_vjp")
    return Gv, Gp


def _touched(*tensors):
    """Tensors a kernel wrote through raw pointers: bump their version counters (md._EOM.update_topology skips a
    rebuild for the same tensor object at the same version)."""
    for x in tensors:
        torch.autograd.graph.increment_version(x)


class NhvWork:
    """Buffers of the fused NH-Verlet half-step kernels (csrc/nhc.hip: mdg_nhv_*) for one integrator: the
    intermediate states of a forward step / an adjoint interval, allocated once (a captured HIP graph needs fixed
    addresses anyway)."""

    def __init__(self, integ, like_v, like_pv):
        z = lambda x: torch.empty_like(x)
        self.mass, self.Q, self.n_dof = integ.mass, integ.Q, float(integ.N_dof)
        self.R, self.n, self.C = int(integ.n_rep), int(integ.n_group), int(like_pv.shape[-1])
        self.dv_h, self.qn, self.dp_h = z(like_v), z(like_v), z(like_pv)
        self.v, self.q, self.pv, self.w = z(like_v), z(like_v), z(like_pv), z(like_v)
        self.vh, self.qm, self.pm = z(like_v), z(like_v), z(like_pv)
        self.lvh, self.lqh, self.lph, self.wh = z(like_v), z(like_v), z(like_pv), z(like_v)
        self._T = integ._T_device
        # cross-workgroup partial sums + tickets of the multi-workgroup launches (zeroed once; the kernels hand the
        # tickets back at zero)
        self.scratch = torch.zeros(int(_lib.load().mdg_nhv_scratch_floats(self.R, self.n)), device=like_v.device)

    def _a(self):
        return ptr(self.mass), ptr(self.Q), ptr(self._T()), self.n_dof

    def kick(self, v, q, pv, f, t, k):
        lib = _lib.load()
        m, Q, T, nd = self._a()
        check(lib.mdg_nhv_kick(ptr(v), ptr(q), ptr(pv), ptr(f), m, Q, T, nd, ptr(t), ptr(k), self.R, self.n, self.C,
                               ptr(self.dv_h), ptr(self.dp_h), ptr(self.qn), ptr(self.scratch), stream_ptr(v.device)),
              "mdg_nhv_kick")
        _touched(self.qn)
        return self.qn

    def finish(self, v, q, pv, f, fn, t, k, out, advance=False):
        """advance: the launch also sets k <- k + 1 (no separate increment)."""
        lib = _lib.load()
        m, Q, T, nd = self._a()
        check(lib.mdg_nhv_finish(ptr(v), ptr(q), ptr(pv), ptr(f), ptr(self.dv_h), ptr(self.dp_h), ptr(self.qn),
                                 ptr(fn.contiguous()), m, Q, T, nd, ptr(t), ptr(k), int(bool(advance)), self.R, self.n, self.C, ptr(out[0]),
                                 ptr(out[1]), ptr(out[2]), ptr(self.scratch), stream_ptr(v.device)), "mdg_nhv_finish")
        _touched(v, q, pv, f, *out)
        if advance:
            _touched(k)

    def adj_pre(self, ans, lv, i):
        lib = _lib.load()
        check(lib.mdg_nhv_adj_pre(ptr(ans[0]), ptr(ans[1]), ptr(ans[2]), ptr(lv), ptr(self.mass), ptr(i), self.R, self.n,
                                  self.C, ptr(self.v), ptr(self.q), ptr(self.pv), ptr(self.w), stream_ptr(lv.device)),
              "mdg_nhv_adj_pre")
        _touched(self.q, self.w)
        return self.q, self.w

    def adj_mid(self, lam, f, dwf, t, i):
        lib = _lib.load()
        m, Q, T, nd = self._a()
        check(lib.mdg_nhv_adj_mid(ptr(self.v), ptr(self.q), ptr(self.pv), ptr(lam[0]), ptr(lam[1]), ptr(lam[2]),
                                  ptr(f.contiguous()), ptr(dwf.contiguous()), m, Q, T, nd, ptr(t), ptr(i), self.R, self.n,
                                  self.C, ptr(self.vh), ptr(self.qm), ptr(self.pm), ptr(self.lvh), ptr(self.lqh),
                                  ptr(self.lph), ptr(self.wh), ptr(self.scratch), stream_ptr(f.device)), "mdg_nhv_adj_mid")
        _touched(self.qm, self.wh)
        return self.qm, self.wh

    def adj_end(self, lam, dwf, t, i, gout, advance=False):
        """advance: the launch also sets i <- i - 1."""
        lib = _lib.load()
        check(lib.mdg_nhv_adj_end(ptr(self.vh), ptr(self.pm), ptr(self.lvh), ptr(self.lqh), ptr(self.lph),
                                  ptr(dwf.contiguous()), ptr(self.mass), ptr(self.Q), ptr(t), ptr(i), int(bool(advance)), ptr(gout[0]),
                                  ptr(gout[1]), ptr(gout[2]), self.R, self.n, self.C, ptr(lam[0]), ptr(lam[1]), ptr(lam[2]),
                                  ptr(self.scratch), stream_ptr(dwf.device)), "mdg_nhv_adj_end")
        _touched(*lam)
        if advance:
            _touched(i)


# ----------------------------------------------------------------------------- Langevin (BAOAB) algebra
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def _mulhilo32(m, x):
    """(high, low) 32-bit words of m * x for a constant m < 2^32 and an int64 tensor x of values < 2^32, without leaving
    the positive range of int64: x is split into 16-bit halves."""
    xl, xh = x & 0xFFFF, x >> 16
    pl, ph = m * xl, m * xh                                   # < 2^48
    return (ph + (pl >> 16)) >> 16, (pl + ((ph & 0xFFFF) << 16)) & _U32


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123) with integer tensor ops: `counter` four and `key` two int64 tensors (or ints) holding
    32-bit words; returns the four output words as int64 tensors.  The integers are the device's (csrc/langevin.hip)."""
    c = [torch.as_tensor(x, dtype=torch.int64) for x in counter]
    dev = next((x.device for x in c if x.dim()), c[0].device)
    c = [x.to(dev) for x in c]
    k0, k1 = (torch.as_tensor(x, dtype=torch.int64).to(dev) for x in key)
    c0, c1, c2, c3 = torch.broadcast_tensors(*c)
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return c0, c1, c2, c3


def lgv_noise_torch(seed, step, n, dtype=torch.float64, device="cpu"):
    """xi [n, 3] of (seed, step) in torch ops: the integers of mdg_lgv_noise, the normals in `dtype`."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    a = torch.arange(n, dtype=torch.int64, device=device)
    x = philox4x32_10((a, step & _U32, step >> 32, 0), (seed & _U32, seed >> 32))
    u = [((w >> 9).to(dtype) + 0.5) * 2.0 ** -23 for w in x]
    r0, r1 = torch.sqrt(-2.0 * torch.log(u[0])), torch.sqrt(-2.0 * torch.log(u[2]))
    two_pi = 2.0 * math.pi
    return torch.stack((r0 * torch.cos(two_pi * u[1]), r0 * torch.sin(two_pi * u[1]), r1 * torch.cos(two_pi * u[3])), 1)


def _rng_words(seed, step0, device):
    """(seed, step0) as the device int64[2] the mdg_lgv_* kernels read (two's complement of the unsigned 64-bit values)."""
    s64 = lambda x: ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)
    return torch.tensor([s64(seed), s64(step0)], dtype=torch.int64).to(device)


def lgv_noise(seed, step, n, device):
    """xi [n, 3] (float32) of (seed, step) from mdg_lgv_noise: the stream of the Langevin kernels, for tests."""
    lib = _lib.load()
    rng = _rng_words(seed, step, device)
    require_gpu(rng, "rng", dtype=torch.int64)
    xi = torch.empty(int(n), 3, device=rng.device)
    check(lib.mdg_lgv_noise(ptr(rng), 0, int(n), ptr(xi), stream_ptr(rng.device)), "mdg_lgv_noise")
    return xi


class LgvWork:
    """Buffers of the Langevin half-step kernels (csrc/langevin.hip: mdg_lgv_*) for one integrator, allocated once (a
    captured HIP graph needs fixed addresses): the intermediate state of a forward step / an adjoint interval, the
    device words (seed, step0) of the noise stream, the per-workgroup partial sums of the friction gradient."""

    def __init__(self, integ, like_v):
        z = lambda: torch.empty_like(like_v)
        dev = like_v.device
        self.mass, self.n = integ.mass, int(like_v.shape[0])
        self.v2, self.qn, self.q, self.w = z(), z(), z(), z()
        self._T, self._gamma = integ._T_device, integ._gamma_device
        self.rng = torch.zeros(2, dtype=torch.int64, device=dev)
        self._rng_val = (0, 0)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.gpart = torch.zeros(int(_lib.load().mdg_lgv_blocks(self.n)), device=dev)
        self.gbar = torch.zeros(1, device=dev)

    def set_rng(self, seed, step0):
        """The noise stream of the next launches (a copy into the device words: captured graphs follow)."""
        if self._rng_val != (int(seed), int(step0)):
            self._rng_val = (int(seed), int(step0))
            self.rng.copy_(_rng_words(seed, step0, "cpu"))

    def kick(self, v, q, f, t, k):
        check(_lib.load().mdg_lgv_kick(ptr(v), ptr(q), ptr(f), ptr(self.mass), ptr(self._gamma()), ptr(self._T()), ptr(t), ptr(k),
                                       ptr(self.rng), self.n, ptr(self.v2), ptr(self.qn), stream_ptr(v.device)), "mdg_lgv_kick")
        _touched(self.qn)
        return self.qn

    def finish(self, v, q, f, fn, t, k, out, advance=False):
        """advance: the launch also sets k <- k + 1."""
        check(_lib.load().mdg_lgv_finish(ptr(v), ptr(q), ptr(f), ptr(self.v2), ptr(self.qn), ptr(fn.contiguous()), ptr(self.mass),
                                         ptr(t), ptr(k), int(bool(advance)), self.n, ptr(out[0]), ptr(out[1]), ptr(self.ticket),
                                         stream_ptr(v.device)), "mdg_lgv_finish")
        _touched(v, q, f, *out)
        if advance:
            _touched(k)

    def adj_pre(self, ans, lv, t, i):
        check(_lib.load().mdg_lgv_adj_pre(ptr(ans[1]), ptr(lv), ptr(self.mass), ptr(t), ptr(i), self.n, ptr(self.q), ptr(self.w),
                                          stream_ptr(lv.device)), "mdg_lgv_adj_pre")
        _touched(self.q, self.w)
        return self.q, self.w

    def adj_step(self, ans, lam, f, dwf, t, i, gout, want_gamma=False, advance=False):
        """advance: the launch also sets i <- i - 1.  Returns (q_{i-1}, the merged w of the next force-vjp)."""
        check(_lib.load().mdg_lgv_adj_step(ptr(ans[0]), ptr(ans[1]), ptr(f.contiguous()), ptr(dwf.contiguous()), ptr(self.mass),
                                           ptr(self._gamma()), ptr(self._T()), ptr(t), ptr(i), int(bool(advance)), ptr(self.rng),
                                           ptr(gout[0]), ptr(gout[1]), int(bool(want_gamma)), self.n, ptr(lam[0]), ptr(lam[1]),
                                           ptr(self.q), ptr(self.w), ptr(self.gpart), ptr(self.ticket), stream_ptr(f.device)),
              "mdg_lgv_adj_step")
        _touched(lam[0], lam[1], self.q, self.w)
        if advance:
            _touched(i)
        return self.q, self.w

    def gamma_bar(self):
        """The friction gradient of the sweep since the last `gpart.zero_()`: the slots added in slot order."""
        check(_lib.load().mdg_lgv_gamma_sum(ptr(self.gpart), self.n, ptr(self.gbar), stream_ptr(self.gbar.device)),
              "mdg_lgv_gamma_sum")
        return self.gbar.clone()


# ----------------------------------------------------------------------------- graph ops (SchNet)
class GraphTopo:
    """Edge topology for the message-passing kernels: ELL list + undirected edge ids + the
    reference-format half list (nbr int64 [E,2], raw image flags [E,3])."""

    def __init__(self, ell):
        self.ell = ell
        self.nbr, self.offsets, self.eid = ell.half_list(with_edge_id=True)
        self.n_atoms, self.n_edges = ell.n_atoms, int(self.nbr.shape[0])
        self._bucketed = None

    def bucketed(self, bucket):
        """The same topology with the edge arrays padded (inert rows, see StaticTopo) to a multiple of
        `bucket`: the edge-wise GEMM shapes then repeat from one neighbour rebuild to the next, which is
        what lets the hipBLASLt kernels (2x faster than rocBLAS on [E,128] operands) be used without
        paying its per-shape heuristic search at every call."""
        if self._bucketed is None or self._bucketed.n_edges % bucket:
            cap = (self.n_edges + bucket - 1) // bucket * bucket
            t = object.__new__(GraphTopo)
            t.ell, t.eid, t.n_atoms, t.n_edges, t._bucketed = self.ell, self.eid, self.n_atoms, cap, None
            t.nbr = torch.full((cap, 2), -1, dtype=torch.int64, device=self.nbr.device)
            t.nbr[:self.n_edges] = self.nbr
            t.offsets = torch.zeros(cap, 3, device=self.nbr.device)
            t.offsets[:self.n_edges] = self.offsets
            t.offsets[self.n_edges:, 0] = StaticTopo.PAD_OFFSET
            t.padded = True
            self._bucketed = t
        return self._bucketed


class StaticTopo:
    """GraphTopo with a fixed edge capacity (see EllList.half_list_padded): every edge-wise tensor has
    `capacity` rows whatever the current pair count, so the whole evaluation can be captured into a
    HIP graph and replayed after each neighbour rebuild."""

    PAD_OFFSET = 1.0e4            # raw image flag of a padding row: |delta| = 1e4, every Gaussian is exactly 0

    padded = True

    def __init__(self, ell, capacity, need):
        self.ell = ell
        self.nbr, self.offsets, self.eid, self.n_valid = ell.half_list_padded(capacity, self.PAD_OFFSET, need)
        self.n_atoms, self.n_edges = ell.n_atoms, int(capacity)


class VerletList:
    """Persistent fixed-capacity neighbour list with Verlet reuse (mdg_nbr_verlet_rebuild, csrc/nbr.hip): searched with
    cutoff + skin, kept while every atom stays within skin / 2 of where it was built (decided on the device, no host
    sync), consumed through the exact per-pair cutoff test (`edge_geom` masks, `pair_eval` re-checks) -- so every
    evaluation sees the pair set a fresh search at the cutoff would find.  All buffers live as long as the object: a
    captured HIP graph replays the same addresses."""

    def __init__(self, n_atoms, group, cell_struct, cutoff, skin, mask, max_nbr, capacity, device):
        lib = _lib.load()
        self.n_atoms, self.group, self.cell_struct = int(n_atoms), int(group), cell_struct
        self.cutoff, self.skin, self.mask = float(cutoff), float(skin), mask
        self.list_cutoff = self.cutoff + self.skin
        self.max_nbr, self.capacity = int(max_nbr), int(capacity)
        self.sig = (self.max_nbr, self.capacity)
        i32 = dict(dtype=torch.int32, device=device)
        self.col, self.shift = torch.zeros(n_atoms, max_nbr, **i32), torch.zeros(n_atoms, max_nbr, **i32)
        self.cnt = torch.zeros(n_atoms, **i32)
        self.nbr = torch.full((capacity, 2), -1, dtype=torch.int64, device=device)
        self.offsets = torch.zeros(capacity, 3, device=device)
        self.offsets[:, 0] = StaticTopo.PAD_OFFSET
        self.eid = torch.zeros(n_atoms, max_nbr, **i32)
        self.n_valid = torch.zeros(1, **i32)
        self.row_base = torch.zeros(n_atoms + 1, **i32)
        self.pos_build = torch.full((n_atoms, 3), float("nan"), device=device)
        self.state = torch.zeros(4, **i32)
        self.use_cell = bool(_use_cell_list(group, cell_struct, self.list_cutoff) and max_nbr <= 512)
        ns = int(lib.mdg_nbr_cell_scratch_groups(n_atoms, group, C.byref(cell_struct), self.list_cutoff)) if self.use_cell else 1
        self.scratch = torch.zeros(max(1, ns), **i32)
        self.ell = EllList(n_atoms, max_nbr, self.col, self.shift, self.cnt, cell_struct, self.cutoff, mask)
        self.ell.verlet = True
        self.topo = _VerletTopo(self)

    def rebuild(self, xyz, need):
        """Decide on the device whether the stored list still serves `xyz`; search again if not."""
        lib = _lib.load()
        x = xyz.detach().contiguous()
        check(lib.mdg_nbr_verlet_rebuild(ptr(x), self.n_atoms, self.group, C.byref(self.cell_struct), self.list_cutoff,
                                         0.5 * self.skin, ptr(self.mask), int(self.use_cell), ptr(self.col), ptr(self.shift),
                                         ptr(self.cnt), self.max_nbr, self.capacity, float(StaticTopo.PAD_OFFSET), ptr(self.nbr),
                                         ptr(self.offsets), ptr(self.eid), ptr(self.n_valid), ptr(need), ptr(self.pos_build),
                                         ptr(self.state), ptr(self.row_base), ptr(self.scratch), stream_ptr(x.device)),
              "mdg_nbr_verlet_rebuild")

    def builds(self):
        """Searches so far (one host sync; diagnostics and tests)."""
        return int(self.state[3].item())


class _VerletTopo:
    """The StaticTopo view of a VerletList (same attributes; `verlet` tells the geometry kernel to mask)."""

    padded = True

    def __init__(self, vl):
        self.ell, self.nbr, self.offsets, self.eid, self.n_valid = vl.ell, vl.nbr, vl.offsets, vl.eid, vl.n_valid
        self.n_atoms, self.n_edges = vl.n_atoms, vl.capacity
        self.verlet = (vl.cell_struct, vl.cutoff)


def _edge_diff(x, topo):
    lib = _lib.load()
    require_gpu(x, "x")
    x = x.contiguous()
    out = torch.empty(topo.n_edges, x.shape[1], device=x.device)
    check(lib.mdg_edge_diff(ptr(x), ptr(topo.nbr), topo.n_edges, x.shape[1], ptr(out), stream_ptr(x.device)),
          "mdg_edge_diff")
    return out


def _edge_scatter(g, topo):
    lib = _lib.load()
    require_gpu(g, "g")
    g = g.contiguous()
    e = topo.ell
    out = torch.empty(topo.n_atoms, g.shape[1], device=g.device)
    check(lib.mdg_edge_scatter(ptr(g), ptr(e.col), ptr(topo.eid), ptr(e.cnt), topo.n_atoms, e.max_nbr, g.shape[1],
                               ptr(out), stream_ptr(g.device)), "mdg_edge_scatter")
    return out


def _cfconv_agg(h, W, topo):
    lib = _lib.load()
    require_gpu(h, "h"), require_gpu(W, "W")
    h, W = h.contiguous(), W.contiguous()
    e = topo.ell
    out = torch.empty(topo.n_atoms, h.shape[1], device=h.device)
    check(lib.mdg_cfconv_agg(ptr(h), ptr(W), ptr(e.col), ptr(topo.eid), ptr(e.cnt), topo.n_atoms, e.max_nbr,
                             h.shape[1], ptr(out), stream_ptr(h.device)), "mdg_cfconv_agg")
    return out


def _edge_prod(a, b, topo):
    lib = _lib.load()
    require_gpu(a, "a"), require_gpu(b, "b")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(topo.n_edges, a.shape[1], device=a.device)
    check(lib.mdg_edge_prod(ptr(a), ptr(b), ptr(topo.nbr), topo.n_edges, a.shape[1], ptr(out),
                            stream_ptr(a.device)), "mdg_edge_prod")
    return out


class EdgeDiffFn(torch.autograd.Function):
    """out[e] = x[i_e] - x[j_e]  (linear; transpose = EdgeScatterFn)."""

    @staticmethod
    def forward(ctx, x, topo):
        ctx.topo = topo
        return _edge_diff(x.detach(), topo)

    @staticmethod
    def backward(ctx, g):
        return EdgeScatterFn.apply(g, ctx.topo), None


class EdgeScatterFn(torch.autograd.Function):
    """out[n] = sum_{e: i_e = n} g[e] - sum_{e: j_e = n} g[e]  (transpose of EdgeDiffFn)."""

    @staticmethod
    def forward(ctx, g, topo):
        ctx.topo = topo
        return _edge_scatter(g.detach(), topo)

    @staticmethod
    def backward(ctx, gn):
        return EdgeDiffFn.apply(gn, ctx.topo), None


class CfconvAggFn(torch.autograd.Function):
    """m[n] = sum over neighbours j of n of h[j] * W[edge(n,j)]: the cfconv message plus both
    scatter_adds of nff/nn/graphconv.py:43-53 in one gather (bilinear, closed under d/d.)."""

    @staticmethod
    def forward(ctx, h, W, topo):
        ctx.topo = topo
        ctx.save_for_backward(h, W)
        return _cfconv_agg(h.detach(), W.detach(), topo)

    @staticmethod
    def backward(ctx, gm):
        h, W = ctx.saved_tensors
        gh = CfconvAggFn.apply(gm, W, ctx.topo) if ctx.needs_input_grad[0] else None
        gW = EdgeProdFn.apply(h, gm, ctx.topo) if ctx.needs_input_grad[1] else None
        return gh, gW, None


class EdgeProdFn(torch.autograd.Function):
    """out[e] = a[i_e] b[j_e] + a[j_e] b[i_e]."""

    @staticmethod
    def forward(ctx, a, b, topo):
        ctx.topo = topo
        ctx.save_for_backward(a, b)
        return _edge_prod(a.detach(), b.detach(), topo)

    @staticmethod
    def backward(ctx, gE):
        a, b = ctx.saved_tensors
        ga = CfconvAggFn.apply(b, gE, ctx.topo) if ctx.needs_input_grad[0] else None
        gb = CfconvAggFn.apply(a, gE, ctx.topo) if ctx.needs_input_grad[1] else None
        return ga, gb, None


# ----------------------------------------------------------------------------- dense algebra closure
def _atb(A, B):
    lib = _lib.load()
    require_gpu(A, "A"), require_gpu(B, "B")
    A, B = A.contiguous(), B.contiguous()
    tops = _torch_ops.get()
    if tops is not None:
        return tops.atb(A, B)
    E, M, N = A.shape[0], A.shape[1], B.shape[1]
    out = torch.empty(M, N, device=A.device)
    ws = torch.empty(max(1, int(lib.mdg_atb_workspace(E, M, N))), device=A.device)
    check(lib.mdg_atb(ptr(A), ptr(B), E, M, N, ptr(out), ptr(ws), stream_ptr(A.device)), "mdg_atb")
    return out


def _atb2(A, B, A2, B2):
    """A^T B + A2^T B2 (same shapes) in one split-K launch pair (csrc/atb.hip mdg_atb2)."""
    lib = _lib.load()
    for x, nm in ((A, "A"), (B, "B"), (A2, "A2"), (B2, "B2")):
        require_gpu(x, nm)
    A, B, A2, B2 = A.contiguous(), B.contiguous(), A2.contiguous(), B2.contiguous()
    E, M, N = A.shape[0], A.shape[1], B.shape[1]
    assert A2.shape == A.shape and B2.shape == B.shape, "atb2: the two pairs must have the same shapes"
    out = torch.empty(M, N, device=A.device)
    ws = torch.empty(max(1, int(lib.mdg_atb_workspace(E, M, N))), device=A.device)
    check(lib.mdg_atb2(ptr(A), ptr(B), ptr(A2), ptr(B2), E, M, N, ptr(out), ptr(ws), stream_ptr(A.device)), "mdg_atb2")
    return out


def _mm(A, W):
    """A[E,K] @ W[K,N] on the hand-written MFMA node kernel (mdg_dense, csrc/dense.hip) -- round 6: no library GEMM behind
    `Dense` on the autograd path either (nff/nn/layers.py:86-134) -- for 2-D f32 HIP operands with K a multiple of 4; W may be
    the transposed view of a Linear weight (read in place, Linear layout) or a contiguous [K,N] matrix.  Anything else: matmul."""
    if (A.is_cuda and A.dim() == 2 and W.dim() == 2 and A.dtype == torch.float32 and W.dtype == torch.float32
            and A.shape[0] > 0 and A.shape[1] % 4 == 0 and A.shape[1] <= DENSE_MAX_K and A.is_contiguous()):
        if W.t().is_contiguous():
            return dense(W.t(), A)[0]
        return dense(W.contiguous(), A, trans=True)[0]
    return A.matmul(W)


class MMFn(torch.autograd.Function):
    """A[E,K] @ W[K,N] on the MFMA node kernel (`_mm`); its weight gradient is the tall-skinny
    A^T g, which goes to AtBFn.  {MMFn, AtBFn} is closed under differentiation."""

    @staticmethod
    def forward(ctx, A, W):
        ctx.save_for_backward(A, W)
        return _mm(A.detach(), W.detach())

    @staticmethod
    def backward(ctx, g):
        A, W = ctx.saved_tensors
        gA = MMFn.apply(g, W.t()) if ctx.needs_input_grad[0] else None
        gW = AtBFn.apply(A, g) if ctx.needs_input_grad[1] else None
        return gA, gW


class AtBFn(torch.autograd.Function):
    """A[E,M]^T @ B[E,N] with split-K over the edges on the f32 MFMA (csrc/atb.hip)."""

    @staticmethod
    def forward(ctx, A, B):
        ctx.save_for_backward(A, B)
        if A.is_cuda and A.dtype == torch.float32:
            return _atb(A.detach(), B.detach())
        return A.detach().t().matmul(B.detach())

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        gA = MMFn.apply(B, g.t()) if ctx.needs_input_grad[0] else None
        gB = MMFn.apply(A, g) if ctx.needs_input_grad[1] else None
        return gA, gB


TALL_ROWS = 8192      # (analytic.py: from here on a^T b goes to the split-K kernel)


def linear(x, weight, bias=None):
    """F.linear for 2-D f32 HIP x on the hand-written kernels: the product on the MFMA node kernel (`_mm`), the weight
    gradient x^T g on the split-K kernel (AtBFn); other inputs (CPU, other dtypes, widths that are no multiple of 4) take
    torch's own."""
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.shape[1] % 4 == 0
            and x.shape[0] > 0):
        return torch.nn.functional.linear(x, weight, bias)
    y = MMFn.apply(x, weight.t())
    return y if bias is None else y + bias


def mm(a, w):
    return MMFn.apply(a, w) if a.shape[0] >= TALL_ROWS else a.matmul(w)


def atb(a, b):
    return AtBFn.apply(a, b) if a.shape[0] >= TALL_ROWS else a.t().matmul(b)


# ----------------------------------------------------------------------------- cfconv filter (MFMA)
def filter_reference(d, mu, width, W1, b1, W2, b2):
    """The filter network in plain torch ops (nff/nn/modules.py:531-541): used for the
    derivative formulas' cross-check in tests and for inputs the fused kernel does not take."""
    g = torch.exp(-0.5 / width.pow(2) * (d[:, None] - mu).pow(2))
    h1 = torch.nn.functional.softplus(torch.nn.functional.linear(g, W1, b1)) - math.log(2.0)
    return torch.nn.functional.linear(h1, W2, b2)


class CfconvFilterFn(torch.autograd.Function):
    """W[E,F] = Dense2(ssp(Dense1(smear(d)))) in one MFMA kernel (csrc/cfconv_filter.hip).
    backward is written out with torch ops (GEMMs on rocBLAS), so it is differentiable again:
    the adjoint's second-order pass goes through it without a hand-derived third kernel."""

    @staticmethod
    def forward(ctx, d, mu, width, W1, b1, W2, b2, bf16=False):
        lib = _lib.load()
        require_gpu(d, "d")
        args = [x.detach().contiguous() for x in (d, mu, width, W1, b1, W2, b2)]
        E, G, F = args[0].shape[0], args[1].shape[0], args[5].shape[0]
        out = torch.empty(E, F, device=d.device)
        fn = lib.mdg_cfconv_filter_bf16 if bf16 else lib.mdg_cfconv_filter
        check(fn(ptr(args[0]), E, ptr(args[1]), ptr(args[2]), G, ptr(args[3]), ptr(args[4]),
                 ptr(args[5]), ptr(args[6]), F, ptr(out), stream_ptr(d.device)), "mdg_cfconv_filter")
        ctx.save_for_backward(d, mu, width, W1, b1, W2, b2)
        return out

    @staticmethod
    def backward(ctx, gW):
        d, mu, width, W1, b1, W2, b2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        c = -0.5 / width.pow(2)
        x = d[:, None] - mu
        g = torch.exp(c * x.pow(2))
        a1 = linear(g, W1, b1)
        gh1 = mm(gW, W2)
        ga1 = gh1 * torch.sigmoid(a1)
        gd = gmu = gwidth = gW1 = gb1 = gW2 = gb2 = None
        if need[0] or need[1] or need[2]:
            gg = mm(ga1, W1) * g
            if need[0] or need[1]:
                t = gg * (2 * c * x)
                gd = t.sum(1) if need[0] else None
                gmu = -t.sum(0) if need[1] else None
            if need[2]:
                gwidth = (gg * x.pow(2)).sum(0) / width.pow(3)
        if need[3]:
            gW1 = atb(ga1, g)
        if need[4]:
            gb1 = ga1.sum(0)
        if need[5]:
            h1 = torch.nn.functional.softplus(a1) - math.log(2.0)
            gW2 = atb(gW, h1)
        if need[6]:
            gb2 = gW.sum(0)
        return gd, gmu, gwidth, gW1, gb1, gW2, gb2, None


# ----------------------------------------------------------------------------- fused interaction block
class FilterNet:
    """Device-side description of one SchNetConv filter network for the fused kernels (csrc/cfconv_fused.hip):
    Gaussian centres / coefficients and the two Dense layers, as contiguous fp32 tensors kept alive here."""

    bf16_reverse = True                          # ... and in the reverse sweep of the filter network (mdg_cfconv_bwd_bf16)

    def __init__(self, mu, coef, W1, b1, W2, b2, bf16=False, rows16=False):
        self.bf16 = bool(bf16)                   # bf16 MFMA operands in the forward / tangent / aggregation sweeps
        # ... and bf16 MIRRORS of the gathered node matrices (mdg_cfconv_*_rows16: a precision option of its own, see
        # include/mdgrad_hip.h); the callers hand cfconv_fwd / cfconv_bwd torch.bfloat16 matrices then
        self.rows16 = bool(rows16 and bf16 and self.bf16_reverse and
                           _lib.load().mdg_cfconv_rows16_supported(int(mu.shape[0]), int(W2.shape[0])))
        # the reverse sweep with parameter gradients can hand out d/d b2 as well (a spare padded column, mdg_cfconv_bwd_theta)
        self.b2col = bool(_lib.load().mdg_cfconv_bias_column(int(mu.shape[0])))
        self.t = [x.detach().to(torch.float32).contiguous() for x in (mu, coef, W1, b1, W2, b2)]
        self.G, self.F = int(self.t[0].shape[0]), int(self.t[4].shape[0])
        self.mu, self.coef, self.W1, self.b1, self.W2, self.b2 = self.t
        s = _lib.MdgFilterNet()
        s.mu, s.coef, s.W1, s.b1, s.W2, s.b2 = (x.data_ptr() for x in self.t)
        s.n_gauss, s.n_filters = self.G, self.F
        self.struct = s

    @staticmethod
    def supported(n_gauss, n_filters):
        return bool(_lib.load().mdg_cfconv_supported(int(n_gauss), int(n_filters)))


def edge_geom(x, topo, w=None):
    """(d, uhat[, dd, ddel]) per edge of the half list: nff/nn/models/schnet.py:142 and its tangent along w."""
    lib = _lib.load()
    require_gpu(x, "x")
    x = x.contiguous()
    verlet = getattr(topo, "verlet", None)       # a list searched with a skin: pairs beyond the cutoff get d = -1
    tops = _torch_ops.get()
    if tops is not None and verlet is None:
        d, uhat, dd, ddel = tops.edge_geom(x, w.contiguous() if w is not None else None, topo.nbr, topo.offsets)
        return (d, uhat, dd, ddel) if w is not None else (d, uhat, None, None)
    E, dev = topo.n_edges, x.device
    d, uhat = torch.empty(E, device=dev), torch.empty(E, 3, device=dev)
    dd = ddel = None
    if w is not None:
        w = w.contiguous()
        dd, ddel = torch.empty(E, device=dev), torch.empty(E, 3, device=dev)
    if verlet is not None:
        check(lib.mdg_edge_geom_masked(ptr(x), ptr(w), ptr(topo.nbr), ptr(topo.offsets), E, C.byref(verlet[0]), float(verlet[1]),
                                       ptr(d), ptr(uhat), ptr(dd), ptr(ddel), stream_ptr(dev)), "mdg_edge_geom_masked")
        return d, uhat, dd, ddel
    check(lib.mdg_edge_geom(ptr(x), ptr(w), ptr(topo.nbr), ptr(topo.offsets), E, ptr(d), ptr(uhat), ptr(dd), ptr(ddel),
                            stream_ptr(dev)), "mdg_edge_geom")
    return d, uhat, dd, ddel


def edge_geom_bwd(d_b, dd_b, d, dd, uhat, ddel, topo):
    """(F, d(w.F)/dx) per atom from the per-edge adjoints (d_b None: force only)."""
    lib = _lib.load()
    e = topo.ell
    dev = dd_b.device
    tops = _torch_ops.get()
    if tops is not None:
        force, dwf = tops.edge_geom_bwd(d_b, dd_b, d, dd, uhat, ddel, e.col, topo.eid, e.cnt)
        return force, (dwf if d_b is not None else None)
    force = torch.empty(topo.n_atoms, 3, device=dev)
    dwf = torch.empty(topo.n_atoms, 3, device=dev) if d_b is not None else None
    check(lib.mdg_edge_geom_bwd(ptr(d_b), ptr(dd_b), ptr(d), ptr(dd), ptr(uhat), ptr(ddel), ptr(e.col), ptr(topo.eid),
                                ptr(e.cnt), topo.n_atoms, e.max_nbr, ptr(force), ptr(dwf), stream_ptr(dev)),
          "mdg_edge_geom_bwd")
    return force, dwf


def cfconv_fwd(fnet, d, dd, h, hd, topo, want_sums=False):
    """(m, md, hsum, hdsum): filter generation + gather-multiply + per-atom sum in one kernel; with dd the
    forward-mode tangent rides along (hd may be None: no node tangent yet)."""
    lib = _lib.load()
    require_gpu(h, "h", dtype=None)
    if h.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("mdgrad_amd: h must be float32 (or a bfloat16 mirror for the rows16 kernels), got %s" % h.dtype)
    h = h.contiguous()
    hd = hd.contiguous() if hd is not None else None
    e = topo.ell
    N, dev = topo.n_atoms, h.device
    r16 = h.dtype == torch.bfloat16               # bf16 mirrors of the node rows: the rows16 kernels
    if r16:
        assert fnet.bf16 and (hd is None or hd.dtype == torch.bfloat16), "cfconv_fwd: bf16 node rows go with the bf16 filter kernels"
    tops = _torch_ops.get()
    if tops is not None:
        m, md, hsum, hdsum = tops.cfconv_fwd(fnet.mu, fnet.coef, fnet.W1, fnet.b1, fnet.W2, fnet.b2, bool(fnet.bf16), d, dd,
                                             h, hd, e.col, topo.eid, e.cnt, bool(want_sums))
        return (m, md if dd is not None else None, hsum if want_sums else None,
                hdsum if (want_sums and hd is not None) else None)
    m = torch.empty(N, fnet.F, device=dev)
    md = torch.empty(N, fnet.F, device=dev) if dd is not None else None
    hsum = torch.empty(N, fnet.F, device=dev) if want_sums else None
    hdsum = torch.empty(N, fnet.F, device=dev) if (want_sums and hd is not None) else None
    fn = lib.mdg_cfconv_fwd_rows16 if r16 else (lib.mdg_cfconv_fwd_bf16 if fnet.bf16 else lib.mdg_cfconv_fwd)
    check(fn(C.byref(fnet.struct), ptr(d), ptr(dd), ptr(h), ptr(hd), ptr(e.col), ptr(topo.eid), ptr(e.cnt),
             N, e.max_nbr, ptr(m), ptr(md), ptr(hsum), ptr(hdsum), stream_ptr(dev)), "mdg_cfconv_fwd")
    return m, md, hsum, hdsum


def cfconv_filter_stash(fnet, d, dd, topo):
    """(st_s, st_sd): the first Dense layer of the filter network once per undirected edge (mdg_cfconv_filter_stash) --
    [E, W] bf16 rows of s = ssp(a) and, with dd, of the tangent sd = sigmoid(a) a_dot; st_sd is None without dd."""
    lib = _lib.load()
    assert fnet.bf16, "the stash holds the bf16 operands of the bf16 kernels"
    E, dev = topo.n_edges, d.device
    W = int(lib.mdg_cfconv_stash_width(fnet.G))
    st_s = torch.empty(E, W, device=dev, dtype=torch.bfloat16)
    st_sd = torch.empty(E, W, device=dev, dtype=torch.bfloat16) if dd is not None else None
    check(lib.mdg_cfconv_filter_stash(C.byref(fnet.struct), ptr(d), ptr(dd), E, ptr(getattr(topo, "n_valid", None)), ptr(st_s),
                                      ptr(st_sd), stream_ptr(dev)), "mdg_cfconv_filter_stash")
    return st_s, st_sd


def cfconv_fwd_stashed(fnet, st_s, st_sd, d, h, hd, topo):
    """(m, md) of cfconv_fwd with the second filter layer's operands read from the stash (bitwise the same outputs); the
    tangent sweep iff st_sd is given."""
    lib = _lib.load()
    e = topo.ell
    N, dev = topo.n_atoms, h.device
    r16 = h.dtype == torch.bfloat16
    m = torch.empty(N, fnet.F, device=dev)
    md = torch.empty(N, fnet.F, device=dev) if st_sd is not None else None
    check(lib.mdg_cfconv_fwd_stashed(C.byref(fnet.struct), ptr(st_s), ptr(st_sd), ptr(d), ptr(h.contiguous()),
                                     ptr(hd.contiguous()) if hd is not None else None, ptr(e.col), ptr(topo.eid), ptr(e.cnt), N,
                                     e.max_nbr, ptr(m), ptr(md), int(r16), stream_ptr(dev)), "mdg_cfconv_fwd_stashed")
    return m, md


def cfconv_bwd(fnet, d, dd, topo, h, hd, mb, mdb, d_b, dd_b, want_theta=False, want_smear=False, want_b2=False):
    """Adjoint of the filter network (see include/mdgrad_hip.h): accumulates into d_b / dd_b in place and returns
    (gW1, gb1, gW2) when want_theta -- plus (gmu, gcoef), the gradients of the Gaussian centres and coefficients, when
    want_smear (trainable radial basis) -- plus gb2, the gradient of the second layer's bias, LAST when want_b2
    (`fnet.b2col`: mdg_cfconv_bwd_theta)."""
    lib = _lib.load()
    dev = h.device
    h, mdb = h.contiguous(), mdb.contiguous()
    hd = hd.contiguous() if hd is not None else None
    mb = mb.contiguous() if mb is not None else None
    bf16 = bool(fnet.bf16 and fnet.bf16_reverse)
    r16 = h.dtype == torch.bfloat16               # bf16 mirrors of the four gathered matrices: mdg_cfconv_bwd_rows16
    if r16:
        assert bf16 and all(t is None or t.dtype == torch.bfloat16 for t in (hd, mb, mdb)), \
            "cfconv_bwd: bf16 node rows come for all gathered matrices, with the bf16 filter kernels"
    if want_b2:
        assert want_theta and fnet.b2col, "cfconv_bwd: the bias gradient comes with the parameter gradients (FilterNet.b2col)"
        gW1, gb1 = torch.empty(fnet.G, fnet.G, device=dev), torch.empty(fnet.G, device=dev)
        gW2, gb2 = torch.empty(fnet.F, fnet.G, device=dev), torch.empty(fnet.F, device=dev)
        gmu = gcf = None
        if want_smear:
            gmu, gcf = torch.empty(fnet.G, device=dev), torch.empty(fnet.G, device=dev)
        ws = torch.empty(max(1, int(lib.mdg_cfconv_bwd_workspace(fnet.G, fnet.F, topo.n_edges))), device=dev)
        flags = (_lib.CFCONV_BF16 if bf16 else 0) | (_lib.CFCONV_ROWS16 if r16 else 0)
        check(lib.mdg_cfconv_bwd_theta(C.byref(fnet.struct), ptr(d), ptr(dd), ptr(topo.nbr), topo.n_edges, int(h.shape[0]), ptr(h),
                                       ptr(hd), ptr(mb), ptr(mdb), ptr(d_b), ptr(dd_b), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2),
                                       ptr(gmu), ptr(gcf), ptr(ws), ptr(getattr(topo, "n_valid", None)), flags, stream_ptr(dev)),
              "mdg_cfconv_bwd_theta")
        return (gW1, gb1, gW2, gmu, gcf, gb2) if want_smear else (gW1, gb1, gW2, gb2)
    tops = _torch_ops.get()
    if tops is not None and not want_smear:
        out = tops.cfconv_bwd(fnet.mu, fnet.coef, fnet.W1, fnet.b1, fnet.W2, fnet.b2, d, dd, topo.nbr, int(topo.n_edges), h, hd,
                              mb, mdb, d_b, dd_b, getattr(topo, "n_valid", None), bool(want_theta), bf16)
        return tuple(out) if want_theta else None
    gW1 = gb1 = gW2 = gmu = gcf = ws = None
    if want_theta:
        gW1, gb1 = torch.empty(fnet.G, fnet.G, device=dev), torch.empty(fnet.G, device=dev)
        gW2 = torch.empty(fnet.F, fnet.G, device=dev)
        ws = torch.empty(max(1, int(lib.mdg_cfconv_bwd_workspace(fnet.G, fnet.F, topo.n_edges))), device=dev)
    nv = ptr(getattr(topo, "n_valid", None))
    if want_smear:
        assert want_theta, "the basis gradients come with the parameter gradients"
        gmu, gcf = torch.empty(fnet.G, device=dev), torch.empty(fnet.G, device=dev)
    if r16:
        check(lib.mdg_cfconv_bwd_rows16(C.byref(fnet.struct), ptr(d), ptr(dd), ptr(topo.nbr), topo.n_edges, int(h.shape[0]), ptr(h),
                                        ptr(hd), ptr(mb), ptr(mdb), ptr(d_b), ptr(dd_b), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gmu),
                                        ptr(gcf), ptr(ws), nv, stream_ptr(dev)), "mdg_cfconv_bwd_rows16")
        return ((gW1, gb1, gW2, gmu, gcf) if want_smear else (gW1, gb1, gW2)) if want_theta else None
    if want_smear:
        check(lib.mdg_cfconv_bwd_smear(C.byref(fnet.struct), ptr(d), ptr(dd), ptr(topo.nbr), topo.n_edges, ptr(h), ptr(hd), ptr(mb),
                                       ptr(mdb), ptr(d_b), ptr(dd_b), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gmu), ptr(gcf), ptr(ws), nv,
                                       int(bf16), stream_ptr(dev)), "mdg_cfconv_bwd_smear")
        return gW1, gb1, gW2, gmu, gcf
    fn = lib.mdg_cfconv_bwd_bf16 if bf16 else lib.mdg_cfconv_bwd
    check(fn(C.byref(fnet.struct), ptr(d), ptr(dd), ptr(topo.nbr), topo.n_edges, ptr(h), ptr(hd), ptr(mb),
             ptr(mdb), ptr(d_b), ptr(dd_b), ptr(gW1), ptr(gb1), ptr(gW2), ptr(ws), nv, stream_ptr(dev)), "mdg_cfconv_bwd")
    return (gW1, gb1, gW2) if want_theta else None


DENSE_MAX_K = 4096       # (k > 256 runs as k-slabs of 256 inside mdg_dense)


def dense(W, x0, trans=False, bias=None, act=False, mul=None, res=None, x1=None, res1=None, want_sig=False):
    """Node-level Dense with fused epilogue on the f32 MFMA (csrc/dense.hip):
    out0 = act(x0 B + bias) * mul + res ; out1 = act'(.) (x1 B) + res1 with B = W^T (trans False) or W (True).
    Returns (out0, sig0, out1)."""
    lib = _lib.load()
    require_gpu(x0, "x0")
    x0 = x0.contiguous()
    W = W.detach().contiguous()
    N, K = x0.shape
    M = W.shape[1] if trans else W.shape[0]
    assert (W.shape[0] if trans else W.shape[1]) == K, "dense: shape mismatch"
    dev = x0.device
    cont = lambda t: t.contiguous() if t is not None else None
    tops = _torch_ops.get()
    if tops is not None:
        out0, sig, out1 = tops.dense_ssp(W, bool(trans), bool(act), x0, cont(bias), cont(mul), cont(res), cont(x1), cont(res1),
                                         bool(want_sig))
        return out0, (sig if (act and want_sig) else None), (out1 if x1 is not None else None)
    out0 = torch.empty(N, M, device=dev)
    sig = torch.empty(N, M, device=dev) if (act and want_sig) else None
    out1 = None
    if x1 is not None:
        x1 = x1.contiguous()
        out1 = torch.empty(N, M, device=dev)
    cont = lambda t: t.contiguous() if t is not None else None
    check(lib.mdg_dense(ptr(W), int(bool(trans)), int(bool(act)), N, K, M, ptr(x0), ptr(cont(bias)), ptr(cont(mul)),
                        ptr(cont(res)), ptr(out0), ptr(sig), ptr(x1), ptr(cont(res1)), ptr(out1), stream_ptr(dev)),
          "mdg_dense")
    return out0, sig, out1


# ----------------------------------------------------------------------------- fused elementwise pieces
def smear(d, mu, c):
    lib = _lib.load()
    E, G = d.shape[0], mu.shape[0]
    g, phi = torch.empty(E, G, device=d.device), torch.empty(E, G, device=d.device)
    check(lib.mdg_smear(ptr(d.contiguous()), ptr(mu.contiguous()), ptr(c.contiguous()), E, G, ptr(g), ptr(phi),
                        stream_ptr(d.device)), "mdg_smear")
    return g, phi


def ssp(a, with_sigmoid=False):
    lib = _lib.load()
    a = a.contiguous()
    s = torch.empty_like(a)
    sa = torch.empty_like(a) if with_sigmoid else None
    check(lib.mdg_ssp(ptr(a), a.numel(), ptr(s), ptr(sa), stream_ptr(a.device)), "mdg_ssp")
    return (s, sa) if with_sigmoid else s


def mul_row(x, y, r=None):
    lib = _lib.load()
    x, y = x.contiguous(), y.contiguous()
    o = torch.empty_like(x)
    check(lib.mdg_mul_row(ptr(x), ptr(y), ptr(r.contiguous()) if r is not None else None, x.shape[0], x.shape[1],
                          ptr(o), stream_ptr(x.device)), "mdg_mul_row")
    return o


def ssp_dual_bwd(sa, xd, sdb, sb):
    lib = _lib.load()
    sa, xd, sdb, sb = sa.contiguous(), xd.contiguous(), sdb.contiguous(), sb.contiguous()
    xdb, xb = torch.empty_like(sa), torch.empty_like(sa)
    check(lib.mdg_ssp_dual_bwd(ptr(sa), ptr(xd), ptr(sdb), ptr(sb), sa.numel(), ptr(xdb), ptr(xb),
                               stream_ptr(sa.device)), "mdg_ssp_dual_bwd")
    return xdb, xb


def ssp_dual_bwd_t(sa, td, sdb, sb):
    """ssp_dual_bwd with the tangent stored as t_dot = sa * x_dot."""
    lib = _lib.load()
    sa, td, sdb, sb = sa.contiguous(), td.contiguous(), sdb.contiguous(), sb.contiguous()
    tops = _torch_ops.get()
    if tops is not None:
        return tuple(tops.ssp_dual_bwd_t(sa, td, sdb, sb))
    xdb, xb = torch.empty_like(sa), torch.empty_like(sa)
    check(lib.mdg_ssp_dual_bwd_t(ptr(sa), ptr(td), ptr(sdb), ptr(sb), sa.numel(), ptr(xdb), ptr(xb),
                                 stream_ptr(sa.device)), "mdg_ssp_dual_bwd_t")
    return xdb, xb


def readout_head(sy, syd, L2):
    """(ydb, yb) = (sy * L2, (1 - sy) * syd * L2): the seeds of the reverse sweep through the readout, one launch
    (csrc/elem.hip); syd None: first-order pass, yb None."""
    lib = _lib.load()
    require_gpu(sy, "sy")
    sy = sy.contiguous()
    syd = syd.contiguous() if syd is not None else None
    l2 = L2.detach().reshape(-1).contiguous()
    ydb = torch.empty_like(sy)
    yb = torch.empty_like(sy) if syd is not None else None
    check(lib.mdg_readout_head(ptr(sy), ptr(syd), ptr(l2), sy.shape[0], sy.shape[1], ptr(ydb), ptr(yb),
                               stream_ptr(sy.device)), "mdg_readout_head")
    return ydb, yb


class ThetaAccum:
    """A flat parameter-gradient buffer in `params` order (tinydiffeq.py:106-108) that kernels accumulate into directly:
    `flat[offset(p) ...] += alpha * (t[idx] - t[idx - 1]) * value` with the time grid and the frame index on the device
    (sovlers.py:160; t = idx = None: plain alpha)."""

    def __init__(self, params, flat=None, t=None, idx=None):
        self.params = list(params)
        self.off, n = {}, 0
        for p in self.params:
            self.off[id(p)] = n
            n += p.numel()
        self.n = n
        self.flat = flat if flat is not None else torch.zeros(n, device=self.params[0].device, dtype=torch.float32)
        assert self.flat.numel() == n and self.flat.is_contiguous()
        self.t, self.idx = t, idx

    def views(self):
        return [self.flat[self.off[id(p)]:self.off[id(p)] + p.numel()].view(p.shape) for p in self.params]


class GradJobs:
    """Collects the reductions of one adjoint evaluation and issues them as two launches per <= 32 jobs
    (mdg_grad_jobs, csrc/gradjobs.hip)."""

    def __init__(self):
        self.jobs, self.keep = [], []

    def _add(self, kind, off, rows, m, n, A, B=None, A2=None, B2=None, row_map=None):
        ts = [x.contiguous() if x is not None else None for x in (A, B, A2, B2)]
        self.keep.extend(ts)
        if row_map is not None:
            self.keep.append(row_map)
        self.jobs.append((kind, int(off), int(rows), int(m), int(n), ts, row_map))

    def atb(self, off, A, B, A2=None, B2=None, row_map=None):
        """flat[off ...] <- A^T B (+ A2^T B2), [m, n] row-major (rows re-mapped through row_map)."""
        self._add(_lib.GRAD_ATB, off, A.shape[0], A.shape[1], B.shape[1], A, B, A2, B2, row_map)

    def colsum(self, off, A, B=None, A2=None, B2=None):
        """flat[off ...] <- sum over rows of A (.* B) (+ A2 (.* B2))."""
        self._add(_lib.GRAD_COLSUM, off, A.shape[0], A.shape[1], 0, A, B, A2, B2)

    def axpy(self, off, A):
        """flat[off ...] <- A (already reduced)."""
        self._add(_lib.GRAD_AXPY, off, 1, A.numel(), 0, A.reshape(-1))

    def run(self, acc, alpha=1.0, accumulate=True):
        lib = _lib.load()
        dev = acc.flat.device
        for c0 in range(0, len(self.jobs), _lib.GRAD_JOBS_MAX):
            chunk = self.jobs[c0:c0 + _lib.GRAD_JOBS_MAX]
            arr = (_lib.MdgGradJob * len(chunk))()
            for j, (kind, off, rows, m, n, ts, row_map) in zip(arr, chunk):
                j.A, j.B, j.A2, j.B2 = (x.data_ptr() if x is not None else None for x in ts)
                j.row_map = row_map.data_ptr() if row_map is not None else None
                j.rows, j.m, j.n, j.kind, j.out_off = rows, m, n, kind, off
            need = int(lib.mdg_grad_jobs_workspace(arr, len(chunk)))
            if need < 0:
                check(1, "mdg_grad_jobs_workspace")
            ws = torch.empty(max(1, need), device=dev, dtype=torch.float32)
            self.keep.append(ws)
            check(lib.mdg_grad_jobs(arr, len(chunk), ptr(acc.flat), float(alpha), ptr(acc.t), ptr(acc.idx), int(bool(accumulate)),
                                    ptr(ws), stream_ptr(dev)), "mdg_grad_jobs")


class _ChainOut:
    __slots__ = ("out0", "out1", "sig", "pre0", "pre1", "out0_h", "out1_h")


class RowChain:
    """A chain of node-level Dense layers as ONE launch (mdg_row_chain, csrc/rowchain.hip): every stage reads the
    previous stage's outputs from on-chip memory (or `in0` / `in1`) and leaves global copies of its outputs in fresh
    [n_rows, M] tensors.  `dual`: primal + tangent rows (or the two adjoints) share the weights.  `x3`: MDG_CHAIN_X3, the
    products as three bf16 MFMAs on split operands (the rows16 precision option's companion, `chain_x3`)."""

    def __init__(self, n_rows, dual, device, x3=0):
        # x3: 0, or the flag MDG_CHAIN_X3 (2) / MDG_CHAIN_X6 (4) (True: X3)
        self.N, self.dual, self.dev, self.x3 = int(n_rows), bool(dual), device, (2 if x3 is True else int(x3))
        self.stages, self.keep, self.words = [], [], []

    @staticmethod
    def supported(*widths):
        return all(1 <= int(w) <= _lib.CHAIN_MAX_WIDTH for w in widths)

    def stage(self, W, trans=False, bias=None, act=False, mode=0, in0=None, in1=None, res0=None, res1=None, aux0=None,
              aux1=None, want_sig=False, want_pre=(False, False), store=True, mirror=False):
        """-> the stage's output tensors (out0, out1, sig, pre0, pre1; None where not produced).  mirror: bf16 copies
        out0_h / out1_h of the outputs as well (what the rows16 cfconv kernels gather); with store=False only they are
        written."""
        # (host cost matters: a stacked SchNet pass builds ~70 chains, and below ~1 ms of GPU work per MD step the launch
        #  thread is what the GPU waits for -- the descriptors are packed as plain integers, MdgChainStage's layout)
        assert len(self.stages) < _lib.CHAIN_MAX_STAGES, "row chain: too many stages"
        if not W.is_contiguous():
            W = W.contiguous()
        K, M = (W.shape[0], W.shape[1]) if trans else (W.shape[1], W.shape[0])
        N, dev, dual = self.N, self.dev, self.dual
        o = _ChainOut()
        f32, head = torch.float32, mode == _lib.CHAIN_HEAD
        o.out0 = torch.empty(N, M, device=dev, dtype=f32) if store else None
        o.out1 = torch.empty(N, M, device=dev, dtype=f32) if (store and dual) else None
        o.sig = torch.empty(N, M, device=dev, dtype=f32) if (act and want_sig) else None
        o.pre0 = torch.empty(N, M, device=dev, dtype=f32) if (head and want_pre[0]) else None
        o.pre1 = torch.empty(N, M, device=dev, dtype=f32) if (head and want_pre[1] and dual) else None
        o.out0_h = torch.empty(N, M, device=dev, dtype=torch.bfloat16) if mirror else None
        o.out1_h = torch.empty(N, M, device=dev, dtype=torch.bfloat16) if (mirror and dual) else None
        words, keep = self.words, self.keep
        words.append(W.data_ptr())
        keep.append(W)
        for t in (bias, in0, in1, res0, res1, aux0, aux1):
            if t is None:
                words.append(0)
            else:
                if not t.is_contiguous():
                    t = t.contiguous()
                keep.append(t)
                words.append(t.data_ptr())
        for t in (o.out0, o.out1, o.sig, o.pre0, o.pre1, o.out0_h, o.out1_h):
            words.append(0 if t is None else t.data_ptr())
        words.append(int(K) | (int(M) << 32))                       # int32 K, M
        words.append((1 if trans else 0) | ((1 if act else 0) << 32))   # int32 trans, act
        words.append(int(mode))                                     # int32 mode, pad_
        self.stages.append(o)
        return o

    def run(self):
        lib = _lib.load()
        buf = _array("Q", self.words)                               # [n_stages] MdgChainStage, 18 x 8 bytes each
        assert len(self.words) == 18 * len(self.stages) and C.sizeof(_lib.MdgChainStage) == 144
        check(lib.mdg_row_chain(buf.buffer_info()[0], len(self.stages), self.N, int(self.dual) | self.x3, stream_ptr(self.dev)),
              "mdg_row_chain")


def rows_to_bf16(x):
    """Round-to-nearest-even bf16 copy of an f32 node matrix [N, M] (M a multiple of 4): mdg_rows_to_bf16."""
    lib = _lib.load()
    require_gpu(x, "x")
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(lib.mdg_rows_to_bf16(ptr(x), x.shape[0], x.shape[1], x.shape[1], ptr(out), stream_ptr(x.device)), "mdg_rows_to_bf16")
    return out


def smear_bwd(gdb, gb, g, phi, dd, c, d_b, dd_b):
    """Accumulates into d_b (and dd_b when gdb is given) in place."""
    lib = _lib.load()
    gb = gb.contiguous()
    gdb = gdb.contiguous() if gdb is not None else None
    check(lib.mdg_smear_bwd(ptr(gdb), ptr(gb), ptr(g), ptr(phi), ptr(dd), ptr(c.contiguous()), g.shape[0], g.shape[1],
                            ptr(d_b), ptr(dd_b), stream_ptr(g.device)), "mdg_smear_bwd")
