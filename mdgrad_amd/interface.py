"""Energy calculators with the reference's interface (torchmd/interface.py):
GeneralInteraction :33-57, PairPotentials :217-300, Electrostatics :303-361 (as CoulombPotentials), Stack :364-403;
StillingerWeber (three-body), StillingerWeberMulti (the same for several species), SuttonChen (embedded-atom), EAM (tabulated embedded-atom, alloys), Tersoff (bond-order) and TersoffMulti (the same for several species) -- none of them has a counterpart in the reference
(GNNPotentials lives in mdgrad_amd.nn).  forward(xyz) -> energy; _reset_topology(xyz) rebuilds the neighbour list.
"""
import inspect
import math
import os

import numpy as np
import torch
from torch.nn import ModuleDict

from . import _lib, ops, units
from .potentials import is_builtin_form
from .topology import compute_dis, get_offsets


def _accumulate_list(accum, params, grads):
    """flat[offset(p)] += weight * g for a member that returned its parameter gradients as a list."""
    jobs = ops.GradJobs()
    for p, g in zip(params, grads):
        if g is not None:
            jobs.axpy(accum.off[id(p)], g.detach().to(torch.float32))
    jobs.run(accum, alpha=1.0, accumulate=True)


class GeneralInteraction(torch.nn.Module):
    def __init__(self, system):
        super().__init__()
        self.system = system
        self.device = system.device
        self.cell = torch.Tensor(system.get_cell()).to(system.device)     # interface.py:55-56
        self.cell.requires_grad = True
        self._cell_struct = _lib.make_cell(system.get_cell())
        self._group = getattr(system, "group_size", system.get_number_of_atoms())
        self._static = None          # fixed-capacity configuration (persistent once created)
        self._static_on = False      # ... and whether _reset_topology uses it

    def _shared_ell(self, xyz, cache):
        """Exact-size ELL list at xyz; members of one Stack with the same cutoff / selection / grouping share
        it within a rebuild (`cache` is the Stack's per-call dict)."""
        key = (float(self.cutoff), None if self._mask is None else self._mask.data_ptr(), self._group)
        if cache is not None and key in cache:
            return cache[key]
        ell = ops.build_ell(xyz.detach(), self._cell_struct, self.cutoff, self._mask, group=self._group)
        if cache is not None:
            cache[key] = ell
        return ell

    def _shared_static_ell(self, xyz, cache, st):
        """Fixed-capacity ELL list (no host sync); members of one Stack with the same cutoff / selection / grouping
        and row capacity share one search per rebuild, like _shared_ell (the first member's `need` buffer carries
        the overflow report for all of them)."""
        key = ("static", float(self.cutoff), None if self._mask is None else self._mask.data_ptr(), self._group,
               int(st["max_nbr"]))
        if cache is not None and key in cache:
            return cache[key]
        ell = ops.build_ell(xyz.detach(), self._cell_struct, self.cutoff, self._mask, max_nbr=st["max_nbr"],
                            group=self._group, need=st["need"])
        if cache is not None:
            cache[key] = ell
        return ell

    # Verlet reuse of the fixed-capacity lists (graph replay / sync-free eager passes only): the list is searched with
    # cutoff * (1 + verlet_skin) and kept while no atom has moved more than half the skin; consumers re-apply the exact
    # cutoff, so every evaluation sees the pair set of a fresh search (ops.VerletList).  0 switches it off.
    verlet_skin = float(os.environ.get("MDG_VERLET_SKIN", "0.02"))

    def _verlet_list(self, xyz, cache, st):
        key = ("verlet", float(self.cutoff), None if self._mask is None else self._mask.data_ptr(), self._group)
        if cache is not None and key in cache:
            return cache[key]
        vl = st.get("verlet")
        skin = self.verlet_skin * float(self.cutoff)
        # everything the stored list was searched with: a changed cutoff / skin / selection / cell / grouping rebuilds it
        sig = (int(st["max_nbr"]), int(st["capacity"]), float(self.cutoff), float(skin),
               None if self._mask is None else self._mask.data_ptr(), bytes(self._cell_struct), int(self._group))
        if vl is None or vl.sig != sig or vl.n_atoms != xyz.shape[0]:
            vl = st["verlet"] = ops.VerletList(xyz.shape[0], self._group, self._cell_struct, self.cutoff,
                                               skin, self._mask, sig[0], sig[1], xyz.device)
            vl.sig = sig
        vl.rebuild(xyz, st["need"])
        if cache is not None:
            cache[key] = vl
        return vl

    # -- fixed-capacity neighbour lists (HIP-graph capture of the integrator steps, mdgrad_amd/graphs.py) --
    def supports_static_topology(self):
        return False

    def static_overflow(self):
        """True when a fixed-capacity rebuild since the last check did not fit (one host sync); the
        capacities are enlarged so that the caller can redo the pass."""
        st = self._static
        if st is None:
            return False
        need = st["need"].tolist()
        if need[0] <= st["max_nbr"] and need[1] <= st.get("capacity", 1 << 62):
            return False
        if need[0] > st["max_nbr"]:
            st["max_nbr"] = min(self._group - 1, (int(need[0] * 1.25) + 15) // 8 * 8)
        if need[1] > st.get("capacity", 1 << 62):
            st["capacity"] = (int(need[1] * 1.25) + 1023) // 1024 * 1024
        st["need"].zero_()
        st["version"] += 1
        return True

    def static_version(self):
        return -1 if self._static is None else self._static["version"]


def _cat_f32(ps, out=None):
    """The tensors of `ps`, flattened and concatenated as float32 (into `out` when given)."""
    return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps], out=out)


class _DeviceMirror:
    """Host-visible parameters mirrored into a persistent flat float32 device buffer that the kernels read.  `sources()`
    returns the tensors, `pack(tensors, out=None)` writes their flat float32 image into `out` (or returns a fresh one);
    `numel`: the size of that image when it is not the summed size of the sources.  get() refreshes the buffer when a source
    changed (address or version counter); inside a HIP-graph capture it returns the buffer as it is -- the replaying pass
    refreshes it once before its first replay (`prepare_pass`), so the captured steps carry no torch op for it -- or, when
    there is no buffer yet, a freshly packed tensor.  get(fresh=True) rewrites the buffer whatever the version counters say
    (an edit through `p.data` moves none)."""

    def __init__(self, sources, pack=_cat_f32, numel=None):
        self.sources, self.pack, self.numel = sources, pack, numel
        self.buf, self.key = None, None

    def get(self, fresh=False):
        ps = self.sources()
        n = sum(p.numel() for p in ps) if self.numel is None else self.numel
        capturing = ps[0].is_cuda and torch.cuda.is_current_stream_capturing()
        buf = self.buf
        if buf is None or buf.numel() != n or buf.device != ps[0].device:
            if capturing:
                return self.pack(ps)
            buf = self.buf = torch.empty(n, device=ps[0].device, dtype=torch.float32)
            self.key = None
        if capturing:
            return buf
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if fresh or self.key != key:
            self.pack(ps, out=buf)
            self.key = key
        return buf


class _ListTerm(GeneralInteraction):
    """A term evaluated on the ELL neighbour list of its cutoff and selection (`self._ell`): the choice of the list at a
    rebuild, the fixed-capacity configuration, and the all-pairs search of the torch restatements."""

    _ell = None

    def _hip_ok(self, xyz=None):
        if xyz is not None and (not xyz.is_cuda or xyz.dtype != torch.float32):
            return False
        return self.analytic and self._ell is not None

    def _takes_verlet_list(self):
        """Whether every evaluation on `_ell` re-applies the exact cutoff per pair, so that a list searched with a skin serves."""
        return True

    def _reset_topology(self, xyz, _cache=None):
        self._topo_stamp = object()
        st = self._static if self._static_on else None
        vkey = ("verlet", float(self.cutoff), None if self._mask is None else self._mask.data_ptr(), self._group)
        if st is not None and _cache is not None and vkey in _cache and self._takes_verlet_list():
            self._ell = _cache[vkey].ell             # a Stack member's Verlet list (exact cutoff re-applied per pair)
        elif st is not None:
            self._ell = self._shared_static_ell(xyz, _cache, st)
        else:
            self._ell = self._shared_ell(xyz, _cache)

    def supports_static_topology(self):
        return self._hip_ok()

    def set_static_topology(self, on=True):
        self._static_on = bool(on)
        if on and self._static is None:
            longest = int(self._ell.cnt.max().item())
            self._static = dict(max_nbr=min(self._group - 1, (int(longest * 1.25) + 15) // 8 * 8),
                                need=torch.zeros(2, dtype=torch.int32, device=self.device), version=0)

    def _all_pairs(self, xyz, rc, mask=None):
        """Half list (i, j, image offsets) at xyz of every pair of a replica closer than rc (and selected by `mask`), by
        torch ops with the reference's minimum image and selection (torchmd/topology.py:30-73)."""
        n, R = self._group, self._n_rep
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        iu = torch.triu_indices(n, n, offset=1, device=xyz.device)
        x = xyz.detach().reshape(R, n, 3)
        D = x[:, iu[1]] - x[:, iu[0]]
        s = D.matmul(cell.inverse())
        o = -(s > 0.5).to(xyz) + (s < -0.5).to(xyz)
        d2 = (D + o.matmul(cell)).pow(2).sum(-1)
        keep = (d2 < rc ** 2) & (d2 != 0)
        if mask is not None:
            keep &= mask.to(xyz.device).bool()[iu[0], iu[1]][None, :]
        rep, idx = torch.nonzero(keep, as_tuple=True)
        return iu[0][idx] + rep * n, iu[1][idx] + rep * n, o[rep, idx]


class _StaticTerm:
    """Mixin of a term on a static table: nothing to search at a rebuild, and under fixed capacities (HIP-graph capture)
    nothing can overflow."""

    def _hip_ok(self, xyz=None):
        if xyz is not None and (not xyz.is_cuda or xyz.dtype != torch.float32):
            return False
        return self.analytic

    def _reset_topology(self, xyz):
        pass

    def supports_static_topology(self):
        return self._hip_ok()

    def set_static_topology(self, on=True):
        pass

    def static_overflow(self):
        return False

    def static_version(self):
        return 0


def _param_tail(gw, param, alpha, want_theta, accum):
    """The parameter part of force_vjp (the third element of its tuple) for a term with one parameter tensor: `gw` =
    d(w.dU/dx)/dparam up to the factor `alpha` (-1 or -conversion), None when the parameter is not trainable.  With
    `accum` (ops.ThetaAccum) alpha * gw is added into its flat buffer and None returned."""
    if not want_theta:
        return None
    if gw is None:
        return [] if accum is None else None
    if accum is not None:
        jobs = ops.GradJobs()
        jobs.axpy(accum.off[id(param)], gw)
        jobs.run(accum, alpha=alpha, accumulate=True)
        return None
    gw = gw.reshape(param.shape)
    return [-gw if alpha == -1.0 else alpha * gw]


def _theta_flat_tail(pthw, thetas, want_theta, accum):
    """The parameter part of force_vjp for a term whose per-atom table `pthw` [N, P] holds, column block by column block, the
    terms of d(w.dU/dx)/dthetas flattened in the order of `thetas` (None when none of them is trainable); the result is minus
    its column sums, in the fixed order of mdg_grad_jobs, shaped like the parameters.  With `accum` (ops.ThetaAccum) they are
    added into its flat buffer and None returned."""
    if not want_theta:
        return None
    if pthw is None:
        return [] if accum is None else None
    trainable = [isinstance(p, torch.nn.Parameter) for p in thetas]
    starts = np.cumsum([0] + [p.numel() for p in thetas]).tolist()
    if accum is not None:
        jobs = ops.GradJobs()
        offs = [accum.off.get(id(p)) for p, t in zip(thetas, trainable) if t]
        if len(offs) == len(thetas) and None not in offs and all(o == offs[0] + s for o, s in zip(offs, starts)):
            jobs.colsum(offs[0], pthw)                           # the parameters are adjacent in the flat buffer, in this order
        else:
            for k, (p, t) in enumerate(zip(thetas, trainable)):
                if t and accum.off.get(id(p)) is not None:
                    jobs.colsum(accum.off[id(p)], pthw[:, starts[k]:starts[k + 1]])
        jobs.run(accum, alpha=-1.0, accumulate=True)
        return None
    gw = ops.theta_sum(pthw, alpha=-1.0)
    return [gw[starts[k]:starts[k + 1]].reshape(p.shape) for k, (p, t) in enumerate(zip(thetas, trainable)) if t]


class _KernelTerm:
    """Mixin of a term whose kernels sit behind an ops.*Term with an `_eval` (ops.SWTerm and its kin, ops._ChargeTerm):
    the energy through ops.TermEnergyFn and the force of the analytic-adjoint protocol (md._EOM.rhs_vjp, Stack.force /
    force_vjp), expressed through `_term(xyz)`, the ops.*Term on the current list or table and parameters, and `_thetas()`,
    the parameters.  force_vjp differs in its parameter part and is written by the two families below."""

    accepts_into = True
    accepts_accum = True
    analytic = True

    def _term(self, xyz):
        raise NotImplementedError

    def forward(self, xyz):
        if self._hip_ok(xyz):
            return ops.TermEnergyFn.apply(xyz.contiguous(), self._term(xyz), *self._thetas())
        return self._torch_energy(xyz)

    def supports_force_vjp(self):
        return self._hip_ok()

    def force(self, xyz, into=None):
        """F = -dU/dx in one call of the term's kernels; `into` (a force buffer of another Stack member): added onto it in
        the same call and returned."""
        o = self._term(xyz)._eval(xyz.detach(), energy=False, grad=True, into=None if into is None else (into, None), scale=-1.0)
        return o["grad"]


class _ManyBodyTerm(_KernelTerm, _ListTerm):
    """A many-body term on the ELL list whose kernels return per-atom parameter terms (ops.SWTerm and its kin): _KernelTerm
    with the parameter part of force_vjp and the persistent scratch of a two-pass kernel.  A module adds its parameters
    (`_thetas`), their device mirror, `_torch_energy` and its presets."""

    _work = None
    _work_size = None            # ops.*_work_size of a kernel pair with a per-slot scratch

    def _scratch(self):
        """The scratch of the bond pass, four floats per slot of the current list: persistent, so that a captured graph
        sees a fixed address (under static topology max_nbr is fixed); re-allocated when a rebuild made the list wider."""
        need = self._work_size(self._ell)
        if self._work is None or self._work.device != self._ell.col.device or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=self._ell.col.device)
        return self._work

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, [d(w.F)/dtheta for every trainable parameter of `_thetas`, shaped like it]) in one call plus the
        fixed-order reduction of the parameter part; `accum` (ops.ThetaAccum): that part is added into its flat buffer
        instead (None returned).  `into` = (F, dq) buffers of another Stack member: this term's force and d(w.F)/dx are
        added onto them in the same call."""
        need = bool(want_theta) and any(isinstance(p, torch.nn.Parameter) for p in self._thetas())
        o = self._term(xyz)._eval(xyz.detach(), w=w.detach(), energy=False, grad=True, into=into, scale=-1.0, want_theta=need)
        return o["grad"], o["hw"], _theta_flat_tail(o["pthw"], self._thetas(), want_theta, accum)


class _ChargeTerm(_KernelTerm):
    """Mixin of a point-charge term (ops._ChargeTerm): _KernelTerm with the charges as the one parameter, their per-atom
    device buffer `_q_atom()` and the charge part of force_vjp, scaled by what the term's kernel leaves out
    (ops._ChargeTerm.pot_scale)."""

    def _thetas(self):
        return (self.charges,)

    def prepare_pass(self):
        if self._hip_ok():
            self._q_atom()

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, [d(w.F)/dcharges]) in one evaluation plus the fixed-order reduction of the charge part; `accum`
        (ops.ThetaAccum): that part is added into its flat buffer instead (None returned).  `into` = (F, dq) buffers of
        another Stack member: this term's force and d(w.F)/dx are added onto them in the same launch."""
        need = bool(want_theta) and isinstance(self.charges, torch.nn.Parameter)
        term = self._term(xyz)
        o = term._eval(xyz.detach(), w=w.detach(), energy=False, grad=True, into=into, scale=-1.0, want_pot=need)
        gw = term.charge_grad(o["potw"]) if need else None
        return o["grad"], o["hw"], _param_tail(gw, self.charges, -term.pot_scale, want_theta, accum)


class _LazyTopology:
    """(nbr_list, pair_dis, offsets) of PairPotentials._reset_topology, materialised on demand
    (the integrators ignore the return value; materialising costs a host sync)."""

    def __init__(self, owner, xyz):
        self._owner, self._xyz, self._val = owner, xyz, None

    def _get(self):
        if self._val is None:
            nbr, off = self._owner._ell.half_list()
            dis = compute_dis(self._xyz, nbr, off, self._owner.cell.detach()).reshape(-1)
            self._val = (nbr, dis, off)
        return self._val

    def __iter__(self):
        return iter(self._get())

    def __getitem__(self, k):
        return self._get()[k]

    def __len__(self):
        return 3


def batch_to(batch, device):
    """nff/utils/cuda.py:6-10."""
    return {k: (v.to(device) if hasattr(v, 'to') else v) for k, v in batch.items()}


class GNNPotentials(GeneralInteraction):
    """torchmd/interface.py:86-136.  `inputs` is the batch dict the SchNet consumes
    ('nxyz', 'num_atoms', 'energy', 'nbr_list', 'offsets'); `_reset_topology` rebuilds the list
    with the HIP builder and also stores the per-atom topology the cfconv kernels use."""

    def __init__(self, system, gnn, cutoff, ex_pairs=None):
        super().__init__(system)
        self.gnn = gnn
        self.cutoff = cutoff
        self.inputs = batch_to(self.system.get_batch(), self.device)
        self.inputs['cell'] = self.cell.detach()
        self.ex_pairs = ex_pairs
        self._mask = ops.build_mask(self._group, None, ex_pairs, system.device)
        self.to(self.device)
        self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))

    def _reset_topology(self, xyz, _cache=None):
        self._topo_stamp = object()                  # identity of this rebuild (see md._EOM.update_topology)
        st = self._static if self._static_on else None
        if st is not None and self.verlet_skin > 0 and self._verlet_consumers_ok():
            topo = self._verlet_list(xyz, _cache, st).topo               # (rebuilt only when an atom left its half-skin ball)
        elif st is not None:
            topo = ops.StaticTopo(self._shared_static_ell(xyz, _cache, st), st["capacity"], st["need"])
        else:
            topo = ops.GraphTopo(self._shared_ell(xyz, _cache))
        self.inputs['nbr_list'], self.inputs['offsets'] = topo.nbr, topo.offsets
        self.inputs['_topo'] = topo

    def supports_static_topology(self):
        return self.supports_force_vjp()

    def _verlet_consumers_ok(self):
        """A list searched with a skin is only handed to consumers that re-apply the exact cutoff per pair: the fused
        interaction-block kernels (`ops.edge_geom` -> mdg_edge_geom_masked marks pairs beyond the cutoff, the cfconv
        kernels skip them).  The unfused chain (`analytic._primal`: n_gaussians > 64, `fused_block = False`, filter
        counts the fused kernels do not take) reads every listed pair at full weight -- the filter has no cutoff
        envelope -- so it gets the exact fixed-capacity list."""
        from .nn import analytic
        return self.supports_force_vjp() and analytic.fused_ok(self.gnn)

    def set_static_topology(self, on=True):
        """Fixed capacities (neighbours per atom, edges) sized from the current list with ~25 % head room."""
        self._static_on = bool(on)
        if on and self._static is None:
            topo = self.inputs['_topo']
            longest = int(topo.ell.cnt.max().item())
            grow = 1.25 * (1.0 + self.verlet_skin) ** 3              # head room, and the skin's extra candidates
            self._static = dict(max_nbr=min(self._group - 1, (int(longest * grow) + 15) // 8 * 8),
                                capacity=(int(topo.n_edges * grow) + 1023) // 1024 * 1024,
                                need=torch.zeros(2, dtype=torch.int32, device=self.device), version=0)

    def forward(self, xyz):
        results = self.gnn(self.inputs, xyz)
        return results['energy']

    # -- analytic-adjoint protocol: hand-derived SchNet passes (mdgrad_amd/nn/analytic.py) ---------
    analytic = True

    def supports_force_vjp(self):
        from .nn import analytic
        return self.analytic and analytic.supported(self.gnn) and not getattr(self.gnn, "cartesian_offsets", False)

    def _z(self):
        z = getattr(self, "_z_cache", None)
        if z is None or z.shape[0] != self.inputs['nxyz'].shape[0]:
            z = self._z_cache = self.inputs['nxyz'][:, 0].long()
        return z

    def force(self, xyz):
        from .nn import analytic
        return analytic.force(self.gnn, self._z(), xyz, self.inputs['_topo'], self.inputs['offsets'], want_energy=False)[1]

    accepts_accum = True

    def prepare_pass(self):
        """Once per trajectory pass, before HIP-graph replays: state the captured steps read but do not recompute (the
        embedding rows of the atoms, which change with every optimizer step)."""
        from .nn import analytic
        if self.supports_force_vjp():
            analytic.refresh_embedding(self.gnn, self._z())

    def force_vjp(self, xyz, w, want_theta=True, accum=None):
        """`accum` (ops.ThetaAccum): the parameter gradients are added into its flat buffer (weighted on the device) and
        None is returned in their place."""
        from .nn import analytic
        _, F, dq, gth = analytic.force_vjp(self.gnn, self._z(), xyz, w, self.inputs['_topo'], self.inputs['offsets'],
                                           want_theta=want_theta, want_energy=False, accum=accum)
        return F, dq, gth


class PairPotentials(_ListTerm):
    """torchmd/interface.py:217-300.  `pair_model` is a module instance (the code's signature)
    or, as in the README snippet, a class plus its keyword arguments."""

    def __init__(self, system, pair_model, cutoff=2.5, index_tuple=None, ex_pairs=None,
                 nbr_list_device=None, **model_kwargs):
        super().__init__(system)
        if inspect.isclass(pair_model):
            pair_model = pair_model(**model_kwargs)
        elif model_kwargs:
            raise TypeError("unexpected keyword arguments %s" % list(model_kwargs))
        self.nbr_list_device = system.device if nbr_list_device is None else nbr_list_device
        self.model = pair_model.to(system.device)
        self.cutoff = cutoff
        self.index_tuple = index_tuple
        self.ex_pairs = ex_pairs
        self._mask = ops.build_mask(self._group, index_tuple, ex_pairs, system.device)
        self._nbr_override = None
        self._theta_mirror = _DeviceMirror(self._mdg_params)
        self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))

    # -- kernel-facing description ------------------------------------------------------
    def builtin(self):
        return is_builtin_form(self.model)

    def _mdg_params(self):
        return self.model.mdg_params()

    def mdg_term(self, theta_off=0):
        params = self.model.mdg_params()
        return ops.make_term(self.model.mdg_term(), self.cutoff, theta_off,
                             sum(p.numel() for p in params), self._mask)

    # -- reference attributes -----------------------------------------------------------
    @property
    def nbr_list(self):
        """[P,2] int64 half list.  (The reference parks it on the CPU, interface.py:259; it
        stays on the device here.)"""
        return self._ell.half_list()[0]

    @property
    def offsets(self):
        return self._ell.half_list()[1]

    def _takes_verlet_list(self):
        return self.builtin()                        # (the module path reads every listed pair)

    def _reset_topology(self, xyz, _cache=None):
        super()._reset_topology(xyz, _cache)
        return _LazyTopology(self, xyz.detach())

    def supports_static_topology(self):
        # module pair models differentiate phi(r) with the autograd engine, whose worker thread cannot
        # take part in a stream capture here (segfault at capture end on ROCm 7): eager launches for them
        return self.builtin()

    def set_static_topology(self, on=True):
        fresh = on and self._static is None
        super().set_static_topology(on)
        if fresh and not self.builtin():              # module path works on the half list: edge capacity too
            pairs = int(self._ell.half_list()[0].shape[0])
            self._static["capacity"] = (int(pairs * 1.25) + 1023) // 1024 * 1024

    # -- analytic-adjoint protocol: used by the integrators' rhs_vjp --------------------------------
    analytic = True            # False: user-defined pair modules go through the autograd double-backward path

    def supports_force_vjp(self):
        return self.builtin() or self.analytic

    # user-defined pair module phi(r) (pairMLP ...): phi', phi'' and the parameter vjp by autograd over the
    # [P] pair distances only; geometry and the per-atom sums on the HIP list (no float atomics)
    def _phi(self, r):
        return self.model(r)

    def _module_pairs(self, xyz):
        st = self._static if self._static_on else None
        topo = ops.GraphTopo(self._ell) if st is None else ops.StaticTopo(self._ell, st["capacity"], st["need"])
        cellm = self.cell.detach()
        cellm = torch.diag(cellm) if cellm.dim() == 1 else cellm
        delta = ops._edge_diff(xyz, topo) - topo.offsets.matmul(cellm)        # compute_dis, topology.py:9-10
        d = delta.pow(2).sum(1).sqrt()
        return topo, delta / d[:, None], d

    def _module_force(self, xyz):
        topo, uhat, d = self._module_pairs(xyz)
        with torch.enable_grad():
            r = d.detach().requires_grad_(True)
            (g1,) = torch.autograd.grad(self._phi(r[:, None]).sum(), r)
        return -ops._edge_scatter(g1[:, None] * uhat, topo)

    def _module_force_vjp(self, xyz, w, want_theta):
        topo, uhat, d = self._module_pairs(xyz)
        ddel = ops._edge_diff(w, topo)
        a = (uhat * ddel).sum(1)                                             # rhat . (w_i - w_j)
        params = [p for p in self.model.parameters() if p.requires_grad] if want_theta else []
        with torch.enable_grad():
            r = d.detach().requires_grad_(True)
            (g1,) = torch.autograd.grad(self._phi(r[:, None]).sum(), r, create_graph=True)
            # S = w . grad U = sum_p phi'(r_p) a_p :  dS/dr_p = phi''(r_p) a_p ,  dS/dtheta = d(w . grad U)/dtheta
            grads = torch.autograd.grad((g1 * a).sum(), [r] + params, allow_unused=True)
        g1 = g1.detach()
        g2a = grads[0]
        hv = g2a[:, None] * uhat + (g1 / d)[:, None] * (ddel - a[:, None] * uhat)
        F = -ops._edge_scatter(g1[:, None] * uhat, topo)
        by_id = {id(p): g_ for p, g_ in zip(params, grads[1:])}
        gth = [(-by_id[id(p)] if by_id.get(id(p)) is not None else torch.zeros_like(p))
               for p in self.model.parameters()] if want_theta else None
        return F, -ops._edge_scatter(hv, topo), gth

    def _theta(self, like):
        """(flat parameter vector of the pair form, its parameters): the vector is the device mirror of the parameters
        (_DeviceMirror; re-allocated when their total size changes)."""
        params = self.model.mdg_params()
        if not params:
            return like.new_zeros(0), params
        return self._theta_mirror.get(), params

    def prepare_pass(self):
        if self.builtin():
            self._theta(self.cell)

    accepts_into = True

    def force(self, xyz, into=None):
        """F = -dU/dx in one kernel launch; `into` (a force buffer of another Stack member): added onto it in the same
        launch and returned."""
        if not self.builtin():
            f = self._module_force(xyz.detach().contiguous())
            return f if into is None else into.add_(f)
        theta, _ = self._theta(xyz)
        o = ops.pair_eval(self._ell, xyz.detach().contiguous(), self.mdg_term(0), theta, energy=False, grad=True,
                          into=None if into is None else (into, None), scale=-1.0, theta_grads=False)
        return o["grad"]

    accepts_accum = True

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, [d(w.F)/dtheta_p for p in parameters()]) -- what double autograd yields at
        torchmd/sovlers.py:229-233 -- in one kernel launch (force + Hessian-vector product + mixed term).  `accum`
        (ops.ThetaAccum): the parameter part is added into its flat buffer instead (None returned).  `into` = (F, dq)
        buffers of another Stack member: this term's force and d(w.F)/dx are added onto them in the same launch."""
        if not self.builtin():
            out = self._module_force_vjp(xyz.detach().contiguous(), w.detach().contiguous(), want_theta)
            if into is not None:
                out = (into[0].add_(out[0]), into[1].add_(out[1]), out[2])
            if accum is None or out[2] is None:
                return out
            _accumulate_list(accum, self.parameters(), out[2])
            return out[0], out[1], None
        theta, params = self._theta(xyz)
        o = ops.pair_eval(self._ell, xyz.detach().contiguous(), self.mdg_term(0), theta, w=w.detach().contiguous(),
                          energy=False, grad=True, into=into, scale=-1.0, theta_grads=bool(want_theta))
        if accum is not None and want_theta:
            if params:
                jobs, pos = ops.GradJobs(), 0
                offs = [accum.off[id(p)] for p in params]
                if all(offs[k + 1] == offs[k] + params[k].numel() for k in range(len(params) - 1)):
                    jobs.axpy(offs[0], o["gtheta_w"])               # the term's parameters are adjacent in the flat buffer
                else:
                    for p, o_ in zip(params, offs):
                        jobs.axpy(o_, o["gtheta_w"][pos:pos + p.numel()])
                        pos += p.numel()
                jobs.run(accum, alpha=-1.0, accumulate=True)
            return o["grad"], o["hw"], None
        if not want_theta:
            return o["grad"], o["hw"], None
        gth, pos = [], 0
        for p in params:
            n = p.numel()
            gth.append(-o["gtheta_w"][pos:pos + n].reshape(p.shape))
            pos += n
        return o["grad"], o["hw"], gth

    def forward(self, xyz):
        if self.builtin():
            params = self.model.mdg_params()
            theta = (torch.cat([p.reshape(-1) for p in params]) if params
                     else xyz.new_zeros(0))
            return ops.PairEnergyFn.apply(xyz.contiguous(), theta, self._ell, self.mdg_term(0))
        # user-defined pair module (e.g. an MLP): distances with torch ops on the device
        nbr, off = self._ell.half_list()
        pair_dis = compute_dis(xyz, nbr, off, self.cell)
        return self.model(pair_dis).sum()


class TPairPotentials(PairPotentials):
    """Temperature-dependent pair model u(r, kB T) (torchmd/interface.py:139-215; e.g. potentials.TpairMLP)."""

    def __init__(self, system, pair_model, T, cutoff=2.5, index_tuple=None, ex_pairs=None, nbr_list_device=None):
        super().__init__(system, pair_model, cutoff=cutoff, index_tuple=index_tuple, ex_pairs=ex_pairs,
                         nbr_list_device=nbr_list_device)
        self.T = T

    def builtin(self):
        return False

    def _phi(self, r):
        from . import units
        return self.model(r, units.kB * self.T)

    def forward(self, xyz):
        nbr, off = self._ell.half_list()
        return self._phi(compute_dis(xyz, nbr, off, self.cell)).sum()            # interface.py:207-215


class _BondedTerm(_StaticTerm, torch.nn.Module):
    """Common part of BondPotentials / AnglePotentials: the static topology table on the device and the analytic-adjoint
    protocol (force / force_vjp) on mdg_bonded_eval (csrc/bonded.hip) -- one launch for energy, force and the
    Hessian-vector product, so a polymer Stack(pair + bond [+ angle] [+ GNN]) (demo/fold.py:131-161) keeps the analytic
    adjoint and HIP-graph replay instead of the reference's double backward.  No trainable parameters (k, ro / thetao are
    plain numbers in the reference); given as tensors that require grad they switch the term to the reference's torch
    ops so that autograd reaches them.  (`_reset_topology` is _StaticTerm's no-op; AnglePotentials has none in the reference
    and therefore cannot be a member of a Stack there.)"""

    _kind = None
    accepts_into = True
    accepts_accum = True
    analytic = True

    def __init__(self, system, top):
        super().__init__()
        self.system = system
        self.device = system.device
        self.cell = torch.Tensor(system.get_cell()).diag().to(self.device)      # interface.py:429-431
        self.top = top.to(self.device)
        self._n_atoms = system.get_number_of_atoms()
        self._table = None

    def _consts(self):
        raise NotImplementedError

    def _hip_ok(self, xyz=None):
        """The HIP kernel serves float32 device positions with plain-number constants.  Constants that require grad, and
        float64 device positions, take the reference's torch ops on the device instead; host tensors are refused
        by the kernel entry as everywhere (no CPU path)."""
        if xyz is not None and xyz.is_cuda and xyz.dtype != torch.float32:
            return False
        return self.analytic and not any(torch.is_tensor(c) and c.requires_grad for c in self._consts())

    def table(self):
        k, x0 = [float(c) for c in self._consts()]
        t = self._table
        if t is None or t.k != k or t.x0 != x0:
            t = self._table = ops.BondedTable(self._kind, self.top, self._n_atoms, self.cell.detach().cpu().tolist(), k, x0,
                                              self.device)
        return t

    def _torch_energy(self, xyz):
        raise NotImplementedError

    def forward(self, xyz):
        if self._hip_ok(xyz):
            return ops.BondedEnergyFn.apply(xyz.contiguous(), self.table())
        return self._torch_energy(xyz)

    # -- analytic-adjoint protocol (md._EOM.rhs_vjp, Stack.force / force_vjp) -------------------------------------
    def supports_force_vjp(self):
        return self._hip_ok()

    def force(self, xyz, into=None):
        o = ops.bonded_eval(self.table(), xyz.detach(), into=None if into is None else (into, None), scale=-1.0)
        return o["grad"]

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, []) -- the term has no parameters."""
        o = ops.bonded_eval(self.table(), xyz.detach(), w=w.detach(), into=into, scale=-1.0)
        return o["grad"], o["hw"], ([] if (want_theta and accum is None) else None)

    def set_static_topology(self, on=True):          # (the rest of the protocol: _StaticTerm)
        self.table()


class BondPotentials(_BondedTerm):
    """Harmonic term in the SQUARED bond length, 1/2 k (|b|^2 - ro)^2 (torchmd/interface.py:406-456; the polymer demo's
    bonded term, demo/fold.py:131).  `top` = [n_bonds, 2] atom indices; orthorhombic minimum image with the non-strict
    test of topology.get_offsets (topology.py:75-80)."""

    _kind = _lib.BONDED_BOND

    def __init__(self, system, top, k, ro):
        super().__init__(system, top)
        self.k, self.ro = k, ro

    def _consts(self):
        return self.k, self.ro

    def _torch_energy(self, xyz):
        b = xyz[self.top[:, 0]] - xyz[self.top[:, 1]]
        b = b + get_offsets(b, self.cell, self.device) * self.cell
        return 0.5 * self.k * (b.pow(2).sum(-1) - self.ro).pow(2).sum(-1)


class AnglePotentials(_BondedTerm):
    """Harmonic angle term 1/2 k (theta - theta0)^2 over triples (i, j, k) centred on j
    (torchmd/interface.py:457-510).

    With b1 = x_i - x_j and b2 = x_k - x_j (each re-imaged with topology.get_offsets on cell.diag()) the angle is
    theta = atan2(|b1 x b2|, b1.b2) and d theta/db comes from the cross product: the reference's acos(b1.b2 / sqrt(|b1|^2 |b2|^2))
    loses ~2.5e-7 / sin^2 theta of the force in float32 and divides by zero at collinearity; this form stays accurate for a
    stiff chain (theta0 = pi) down to sin theta ~ 1e-5.  A term with |b1 x b2|^2 <= eps^2 |b1|^2 |b2|^2, eps = 2^-20 (three
    collinear atoms -- a rod built along an axis --, or a bond vector of length zero), keeps its energy (theta = 0 or pi) and
    contributes zero force and zero H.w: theta has a kink there, zero is its symmetric subgradient (the convention of
    csrc/adf.hip and DihedralPotentials).  The HIP kernel and `_torch_energy` are the same function."""

    _kind = _lib.BONDED_ANGLE
    _eps = 2.0 ** -20

    def __init__(self, system, top, k, thetao):
        super().__init__(system, top)
        self.k, self.thetao = k, thetao

    def _consts(self):
        return self.k, self.thetao

    def _torch_energy(self, xyz):
        b1 = xyz[self.top[:, 0]] - xyz[self.top[:, 1]]
        b2 = xyz[self.top[:, 2]] - xyz[self.top[:, 1]]
        b1 = b1 + get_offsets(b1, self.cell, self.device) * self.cell
        b2 = b2 + get_offsets(b2, self.cell, self.device) * self.cell
        C, dot = torch.cross(b1, b2, dim=-1).pow(2).sum(-1), (b1 * b2).sum(-1)
        regular = C > self._eps ** 2 * b1.pow(2).sum(-1) * b2.pow(2).sum(-1)
        one = torch.ones_like(C)
        theta = torch.where(regular, torch.atan2(torch.where(regular, C, one).sqrt(), torch.where(regular, dot, one)),
                            torch.atan2(C.detach().sqrt(), dot.detach()))            # collinear: 0 or pi, no gradient
        return 0.5 * self.k * (theta - self.thetao).pow(2).sum(-1)


class DihedralPotentials(_StaticTerm, torch.nn.Module):
    """Torsion term over quadruples (i, j, k, l): U = sum_terms sum_{m = 0..4} coeffs[type, m] cos^m phi, the reference's
    "multiharmonic" dihedral form (nff/nn/modules.py:253-257); no counterpart in torchmd/interface.py.

    With b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k (each re-imaged with topology.get_offsets on cell.diag(), like
    BondPotentials / AnglePotentials), n1 = b1 x b2 and n2 = b2 x b3:  cos phi = n1.n2 / sqrt(|n1|^2 |n2|^2), which is
    compute_dihe (torchmd/observable.py:181-197) of the row.  The energy is a polynomial in cos phi: no acos, no singularity at
    phi = 0 or pi (the reference's acos(cos / 1.000001) fudge is not reproduced).  A term with three collinear atoms,
    |n1|^2 <= eps^2 |b1|^2 |b2|^2 or |n2|^2 <= eps^2 |b2|^2 |b3|^2 with eps = 2^-20, is skipped: no energy, force or gradient.

    `top` [n_terms, 4]; `coeffs` [5] or [n_types, 5], held as the parameter `coeffs` (trainable=False: a buffer); `types`
    [n_terms] in [0, n_types) picks the row of every term (default: row 0).  from_opls builds it from OPLS constants.

    A Stack member like BondPotentials: forward(xyz) is differentiable twice in xyz and once in coeffs on the HIP kernels
    (ops.DihedralTerm, csrc/dihedral.hip), and force / force_vjp serve the analytic adjoint and HIP-graph replay -- also
    while coeffs requires grad: d(w.F)/dcoeffs comes out of the same launch.  float64 or host positions take the torch
    restatement `_torch_energy`."""

    accepts_into = True
    accepts_accum = True
    analytic = True

    def __init__(self, system, top, coeffs, types=None, trainable=True):
        super().__init__()
        self.system = system
        self.device = system.device
        self.cell = torch.Tensor(system.get_cell()).diag().to(self.device)
        self._n_atoms = system.get_number_of_atoms()
        c = torch.as_tensor(coeffs, dtype=torch.float32).detach().clone()
        if c.dim() not in (1, 2) or c.shape[-1] != 5:
            raise ValueError("DihedralPotentials: coeffs must be [5] or [n_types, 5], got %s" % (tuple(c.shape),))
        c = c.to(self.device)
        if trainable:
            self.coeffs = torch.nn.Parameter(c)
        else:
            self.register_buffer("coeffs", c)
        self.n_types = 1 if c.dim() == 1 else int(c.shape[0])
        self.top = torch.as_tensor(top).to(torch.long).reshape(-1, 4).to(self.device)
        self.types = None if types is None else torch.as_tensor(types).to(torch.long).reshape(-1).to(self.device)
        self._table = ops.DihedralTable(self.top, self._n_atoms, self.cell.detach().cpu().tolist(), self.device, types=self.types,
                                        n_types=self.n_types)

    @staticmethod
    def opls_to_multiharmonic(V):
        """OPLS constants V1..V4 [..., 4] of sum_m V_m / 2 (1 + (-1)^(m+1) cos(m phi)) (nff/nn/modules.py:259-264) -> the
        coefficients [..., 5] of the same energy as a polynomial in cos phi:
        [V1/2 + V2 + V3/2, V1/2 - 3 V3/2, -V2 + 4 V4, 2 V3, -4 V4]."""
        V = torch.as_tensor(V)
        V = V if V.is_floating_point() else V.to(torch.get_default_dtype())
        v1, v2, v3, v4 = V.unbind(-1)
        return torch.stack([v1 / 2 + v2 + v3 / 2, v1 / 2 - 3 * v3 / 2, -v2 + 4 * v4, 2 * v3, -4 * v4], -1)

    @classmethod
    def from_opls(cls, system, top, V, types=None, trainable=True):
        return cls(system, top, cls.opls_to_multiharmonic(V), types=types, trainable=trainable)

    def table(self):
        return self._table

    def _torch_energy(self, xyz):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and coeffs)."""
        top = self.top.to(xyz.device)
        cell = self.cell.to(xyz)
        i, j, k, l = top.unbind(1)
        b1, b2, b3 = xyz[j] - xyz[i], xyz[k] - xyz[j], xyz[l] - xyz[k]
        b1, b2, b3 = (b + get_offsets(b, cell, xyz.device).to(xyz) * cell for b in (b1, b2, b3))
        n1, n2 = torch.cross(b1, b2, dim=-1), torch.cross(b2, b3, dim=-1)
        N1, N2 = n1.pow(2).sum(-1), n2.pow(2).sum(-1)
        eps2 = 2.0 ** -40
        ok = (N1 > eps2 * b1.pow(2).sum(-1) * b2.pow(2).sum(-1)) & (N2 > eps2 * b2.pow(2).sum(-1) * b3.pow(2).sum(-1))
        one = torch.ones_like(N1)
        c = (n1 * n2).sum(-1) / torch.where(ok, N1 * N2, one).sqrt()
        a = self.coeffs.to(xyz).reshape(-1, 5)
        a = a[self.types.to(xyz.device)] if self.types is not None else a[:1].expand(c.shape[0], 5)
        u = a[:, 0] + c * (a[:, 1] + c * (a[:, 2] + c * (a[:, 3] + c * a[:, 4])))
        return torch.where(ok, u, torch.zeros_like(u)).sum(-1)

    def forward(self, xyz):
        if self._hip_ok(xyz):
            return ops.TermEnergyFn.apply(xyz.contiguous(), ops.DihedralTerm(self._table, self.coeffs), self.coeffs)
        return self._torch_energy(xyz)

    # -- analytic-adjoint protocol (md._EOM.rhs_vjp, Stack.force / force_vjp) -------------------------------------
    def supports_force_vjp(self):
        return self._hip_ok()

    def force(self, xyz, into=None):
        o = ops.dihedral_eval(self._table, xyz.detach(), self.coeffs, into=None if into is None else (into, None), scale=-1.0)
        return o["grad"]

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, [d(w.F)/dcoeffs]) in one launch plus the fixed-order reduction of the parameter part; `accum`
        (ops.ThetaAccum): that part is added into its flat buffer instead (None returned)."""
        need = bool(want_theta) and isinstance(self.coeffs, torch.nn.Parameter)
        o = ops.dihedral_eval(self._table, xyz.detach(), self.coeffs, w=w.detach(), into=into, scale=-1.0, terms=need)
        gw = ops.dihedral_coeff_grad(self._table, o["c_term"], o["cd_term"], want_u=False)[1] if need else None
        return o["grad"], o["hw"], _param_tail(gw, self.coeffs, -1.0, want_theta, accum)


class CoulombPotentials(_ChargeTerm, _ListTerm):
    """Point-charge electrostatics as a damped shifted-force real-space sum (Wolf et al. 1999; Fennell and Gezelter 2006):
    pairwise, O(N), no reciprocal part, energy and force continuous at the cutoff.  The working counterpart of the
    reference's Electrostatics (torchmd/interface.py:303-361), which overwrites q1 (so it multiplies q_j * q_j) and carries a
    minus sign that makes like charges attract; with alpha = 0 and shift = "none" this class is the bare truncated Coulomb
    sum that class meant to write.

    With charges q_i, cutoff rc, damping alpha >= 0, E(r) = erfc(alpha r) and G(r) = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2):

        psi(r)   = E(r)/r - c0 + c1 (r - rc)
        psi'(r)  = -E/r^2 - G/r + c1
        psi''(r) = 2E/r^3 + 2G/r^2 + 2 alpha^2 G

        shift = "none":       c0 = 0,         c1 = 0
        shift = "potential":  c0 = E(rc)/rc,  c1 = 0
        shift = "force":      c0 = E(rc)/rc,  c1 = E(rc)/rc^2 + G(rc)/rc     (default)

        U = conversion * [ 1/2 sum_i sum_{j in row(i)} q_i q_j psi(r_ij)  -  s sum_i q_i^2 ]
        s = c0/2 + alpha/sqrt(pi)                                            (s = 0 with self_energy=False)

    row(i) is the neighbour row of the ELL list exactly as PairPotentials uses it: the same minimum image, the same
    (d2 < rc^2) & (d2 != 0) test and the same index_tuple / ex_pairs mask (ops.build_mask); pairs stay inside their replica.
    Excluded pairs simply do not interact (within an Ewald sum, EwaldExclusions adds their erf correction).  `conversion`
    defaults to units.ke (eV Angstrom / e^2); reduced-unit users pass 1.0.

    `charges`: [n] with n = system.group_size (one replica's atoms, tiled over the replicas of System.replicate(R)), or
    [n_types] together with `types` [n]; the parameter `charges` when trainable, otherwise a buffer.  The charges are not
    constrained: neutrality is the user's business, and a cell that is not neutral has no Ewald limit -- the sum then
    depends on the cutoff and alpha.  (The reciprocal part is a term of its own: with shift="none", EwaldReciprocal on top
    of this class completes the Ewald sum -- see `ewald`.)

    forward(xyz) is differentiable twice in xyz and once in charges on the HIP kernel (ops.CoulombTerm,
    csrc/coulomb.hip); force / force_vjp serve the analytic adjoint and HIP-graph replay, also while charges requires grad:
    d(w.F)/dcharges comes from the same launch plus a fixed-order reduction.  float64 or host positions take the torch
    restatement `_torch_energy`."""

    def __init__(self, system, charges, cutoff, alpha=0.0, shift="force", types=None, index_tuple=None, ex_pairs=None,
                 conversion=units.ke, self_energy=True, trainable=False):
        super().__init__(system)
        self.cutoff = float(cutoff)
        self.alpha, self.shift, self.self_energy = float(alpha), shift, bool(self_energy)
        self.conversion = float(conversion)
        self._consts = ops.coulomb_consts(self.cutoff, self.alpha, shift, self.conversion, self.self_energy)
        n = self._group
        q = torch.as_tensor(charges, dtype=torch.float32).detach().clone().reshape(-1)
        if types is None:
            if q.numel() != n:
                raise ValueError("CoulombPotentials: charges must hold one entry per atom of a replica (%d), got %d; pass "
                                 "`types` with per-type charges" % (n, q.numel()))
            self.types = None
        else:
            ty = torch.as_tensor(types).detach().to(torch.long).reshape(-1).cpu()
            if ty.numel() != n:
                raise ValueError("CoulombPotentials: types must hold one entry per atom of a replica (%d), got %d" % (n, ty.numel()))
            if ty.numel() and (int(ty.min()) < 0 or int(ty.max()) >= q.numel()):
                raise ValueError("CoulombPotentials: types must lie in [0, %d)" % q.numel())
            self.types = ty.to(self.device)
        self._slot = None if self.types is None else self.types.to(torch.int32).contiguous()
        self.n_slots = int(q.numel())
        q = q.to(self.device)
        if trainable:
            self.charges = torch.nn.Parameter(q)
        else:
            self.register_buffer("charges", q)
        self.index_tuple, self.ex_pairs = index_tuple, ex_pairs
        self._mask = ops.build_mask(n, index_tuple, ex_pairs, system.device)
        self._n_rep = system.get_number_of_atoms() // n
        self._ell = None
        self._q_mirror = _DeviceMirror(self._thetas, self._pack_charges, numel=self._n_rep * n)
        if torch.device(self.device).type == "cuda":
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))

    # -- the per-atom charge buffer the kernel reads (the lists are _ListTerm's, those of PairPotentials) ----------
    def _expand(self, charges):
        """charges [n] or [n_types] -> one charge per atom of the (replica-stacked) system."""
        q = charges if self.types is None else charges[self.types.to(charges.device)]
        return q.repeat(self._n_rep) if self._n_rep > 1 else q

    def _pack_charges(self, ps, out=None):
        q = self._expand(ps[0].detach())
        return q.contiguous() if out is None else out.copy_(q)

    def _q_atom(self):
        """charges[types] tiled over the replicas: the device mirror of the charges (_DeviceMirror)."""
        return self._q_mirror.get()

    def _term(self, xyz=None):
        return ops.CoulombTerm(self._ell, self._consts, self._q_atom(), self._slot, self.n_slots)

    # -- energy ----------------------------------------------------------------------------------------------------
    def _pairs(self, xyz):
        """Half list (i, j, image offsets) at xyz: the device list of the last rebuild when there is one (a list searched
        with a skin is cut to the exact cutoff in _torch_energy), else every pair of a replica by torch ops with the
        reference's minimum image and selection (torchmd/topology.py:30-73)."""
        if self._ell is not None and xyz.is_cuda:
            nbr, off = self._ell.half_list()
            return nbr[:, 0], nbr[:, 1], off.to(xyz)
        return self._all_pairs(xyz, self.cutoff, self._mask)

    def _torch_energy(self, xyz):
        """The same energy in torch ops on the half list, in the dtype and on the device of xyz (differentiable by autograd in
        xyz and charges)."""
        k = self._consts
        i, j, off = self._pairs(xyz)
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        d = xyz[i] - xyz[j] - off.matmul(cell)
        d2 = d.pow(2).sum(-1)
        inside = (d2 < k.rc * k.rc) & (d2 != 0)
        r = torch.where(inside, d2, torch.ones_like(d2)).sqrt()
        E = torch.erfc(k.alpha * r) if k.alpha != 0.0 else torch.ones_like(r)
        psi = E / r - k.c0 + k.c1 * (r - k.rc)
        q = self._expand(self.charges.to(xyz))
        pair = torch.where(inside, q[i] * q[j] * psi, torch.zeros_like(psi)).sum()
        return k.conversion * (pair - k.self_s * q.pow(2).sum())


class _MovingCutoff:
    """Mixin of a list term whose support radius moves with a trainable `sigma` (StillingerWeber, StillingerWeberMulti).  The
    kernel applies every entry's own support test with the live sigma, so any list searched with a radius at or above the
    support radius is exact; the module only keeps its list sufficient: it is searched with `self.cutoff`, which is kept while
    rc <= cutoff <= `cutoff_keep` rc and otherwise reset to `cutoff_reset` rc, and `static_version()` changes with it, so
    captured graphs are rebuilt.  A class supplies `_support_radius()`: rc of the current sigma by ONE host read, raising the
    class's errors; it is called only outside a HIP-graph capture and only when sigma's version counter moved."""

    cutoff_reset = 1.02          # a reset list is searched with this multiple of the support radius ...
    cutoff_keep = 1.05           # ... and kept while radius <= cutoff <= this multiple of the radius (design constants)

    def _init_cutoff(self, system):
        """The state of the protocol, and half the shortest height of the cell, which no support radius may exceed."""
        h = np.asarray(system.get_cell(), dtype=np.float64)
        h = np.diag(h) if h.ndim == 1 else h
        vol = abs(float(np.linalg.det(h)))
        self._half_height = 0.5 * min(vol / float(np.linalg.norm(np.cross(h[(d + 1) % 3], h[(d + 2) % 3]))) for d in range(3))
        self.cutoff, self._cut_ver, self._list_ver, self._sig_key = None, 0, -1, None

    def _support_radius(self):
        raise NotImplementedError

    def _sync_cutoff(self):
        """Apply the cutoff rule to the current sigma; True when the cutoff was reset.  Inside a capture, or while sigma's
        version counter has not moved, nothing is read."""
        s = self.sigma
        if s.is_cuda and torch.cuda.is_current_stream_capturing():
            return False
        key = (s.data_ptr(), s._version)
        if key == self._sig_key:
            return False
        self._sig_key = key
        rc = self._support_radius()
        if self.cutoff is not None and rc <= self.cutoff <= self.cutoff_keep * rc:
            return False
        self.cutoff = self.cutoff_reset * rc
        self._cut_ver += 1
        return True

    def static_version(self):
        return (super().static_version(), self._cut_ver)

    def _reset_topology(self, xyz, _cache=None):
        self._sync_cutoff()
        super()._reset_topology(xyz, _cache)         # (a Stack member's Verlet list serves: the support test is per entry)
        self._list_ver = self._cut_ver

    def set_static_topology(self, on=True):
        self._sync_cutoff()
        super().set_static_topology(on)

    def _current_list(self, xyz):
        """The list to evaluate on: rebuilt here when sigma has moved the cutoff since the last search (never inside a
        capture, where sigma is not read)."""
        self._sync_cutoff()
        if self._list_ver != self._cut_ver:
            self._reset_topology(xyz.detach())
        return self._ell


class StillingerWeber(_MovingCutoff, _ManyBodyTerm):
    """Stillinger-Weber potential for one species (Stillinger and Weber 1985): a short-ranged pair term plus a three-body
    term that prefers the angle cos0 between the bonds of every atom to its near neighbours -- tetrahedral silicon
    (`silicon`) and monatomic coarse-grained water (`mW`, Molinero and Moore 2009).  With rc = a sigma:

        U    = sum_{i<j} phi2(r_ij) + sum_i sum_{j<k in row(i)} phi3(r_ij, r_ik, cos theta_jik)
        phi2 = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - a sigma))                    r < a sigma, else 0
        phi3 = lam eps (cos theta - cos0)^2 exp(gamma sigma/(r_ij - a sigma)) exp(gamma sigma/(r_ik - a sigma))

    row(i) is the neighbour row of the ELL list that PairPotentials would use at the cutoff a sigma: the same minimum image
    and the same (d2 < rc^2) & (d2 != 0) test; triplets stay inside their replica (System.replicate).  There is no fixed
    topology: the triplets are those of the current list.

    `epsilon`, `sigma` and `lam` are the parameters when trainable, otherwise buffers; a, gamma, cos0, A, B and the integer
    exponents 0 <= q < p <= 12 are constants.  Not covered: `index_tuple`, `ex_pairs` (both rejected) and per-type or
    multi-species parameters (one (epsilon, sigma, lam) for all atoms): those are StillingerWeberMulti's.

    A trainable sigma moves the cutoff a sigma.  The kernel always applies r < a sigma with the live sigma, so a list
    searched with a larger radius is exact; the list is searched with `self.cutoff`, which is kept while
    a sigma <= cutoff <= `cutoff_keep` a sigma and otherwise reset to `cutoff_reset` a sigma (sigma is read on the host
    then, outside a HIP-graph capture only and only when its version counter moved; `static_version()` changes with the
    cutoff, so captured graphs are rebuilt).

    forward(xyz) is differentiable twice in xyz and once in (epsilon, sigma, lam) on the HIP kernel (ops.SWTerm,
    csrc/sw.hip); force / force_vjp serve the analytic adjoint and HIP-graph replay, also while the parameters require grad:
    d(w.F)/d(epsilon, sigma, lam) comes from the same launch plus a fixed-order reduction.  float64 or host positions take
    the torch restatement `_torch_energy`."""

    # 1 kcal/mol in eV: 4184 J/mol over (1.602176634e-19 J/eV * 6.02214076e23 /mol), the exact SI values of 2019
    KCAL_PER_MOL = 4184.0 / (1.602176634e-19 * 6.02214076e23)

    def __init__(self, system, epsilon, sigma, lam=21.0, a=1.80, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584,
                 p=4, q=0, trainable=True, index_tuple=None, ex_pairs=None):
        super().__init__(system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("StillingerWeber: index_tuple and ex_pairs are not supported (one species, every pair)")
        self._consts = ops.sw_consts(epsilon, sigma, lam, a, gamma, cos0, A, B, p, q)
        k = self._consts
        self.a, self.gamma, self.cos0, self.A, self.B, self.p, self.q = k.a, k.gamma, k.cos0, k.A, k.B, int(k.p), int(k.q)
        self._init_cutoff(system)
        if k.a * k.sigma > self._half_height:
            raise ValueError("StillingerWeber: a * sigma = %g exceeds half the shortest cell height (%g)"
                             % (k.a * k.sigma, self._half_height))
        for name, v in (("epsilon", k.epsilon), ("sigma", k.sigma), ("lam", k.lam)):
            t = torch.tensor([v], dtype=torch.float32, device=self.device)
            if trainable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self._ell = None
        self._theta_mirror = _DeviceMirror(self._thetas)
        self._sync_cutoff()
        if torch.device(self.device).type == "cuda":
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._theta()

    @classmethod
    def silicon(cls, system, **kw):
        """Stillinger and Weber's silicon: epsilon = 2.1683 eV, sigma = 2.0951 Angstrom, lam = 21."""
        kw.setdefault("lam", 21.0)
        return cls(system, 2.1683, 2.0951, **kw)

    @classmethod
    def mW(cls, system, **kw):
        """Molinero and Moore's monatomic water: epsilon = 6.189 kcal/mol (in eV), sigma = 2.3925 Angstrom, lam = 23.15."""
        kw.setdefault("lam", 23.15)
        return cls(system, 6.189 * cls.KCAL_PER_MOL, 2.3925, **kw)

    # -- the cutoff the list is searched with: _MovingCutoff on a sigma -----------------------------------------------
    def _support_radius(self):
        rc = self.a * float(self.sigma.detach())              # (one host read per change of sigma)
        if not rc > 0.0:
            raise ValueError("StillingerWeber: sigma must stay positive (got %g)" % (rc / self.a))
        return rc

    # -- the device copy of (epsilon, sigma, lam) the kernel reads -------------------------------------------------
    def _thetas(self):
        return self.epsilon, self.sigma, self.lam

    def _theta(self):
        """(epsilon, sigma, lam) as the kernel reads them: their device mirror (_DeviceMirror)."""
        return self._theta_mirror.get()

    def prepare_pass(self):
        self._sync_cutoff()
        if self._hip_ok():
            self._theta()

    # -- energy ----------------------------------------------------------------------------------------------------
    def _torch_energy(self, xyz):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in
        epsilon, sigma, lam): the pairs inside a sigma, then every triplet as two entries of one atom's row."""
        eps, sig, lam = (p.to(xyz).reshape(()) for p in (self.epsilon, self.sigma, self.lam))
        rc = self.a * sig
        i, j, off = self._all_pairs(xyz, float(rc.detach()))
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        d = xyz[i] - xyz[j] - off.matmul(cell)
        r = d.pow(2).sum(-1).sqrt()
        sr = sig / r
        phi2 = self.A * eps * (self.B * sr ** self.p - sr ** self.q) * torch.exp(sig / (r - rc))
        # rows: every pair as (centre, unit vector centre -> end, g), grouped by centre into a padded [N, K] table
        N = xyz.shape[0]
        centre = torch.cat([i, j])
        u = torch.cat([-d, d]) / torch.cat([r, r])[:, None]
        g = torch.exp(self.gamma * sig / (torch.cat([r, r]) - rc))
        order = torch.argsort(centre, stable=True)
        centre, u, g = centre[order], u[order], g[order]
        cnt = torch.bincount(centre, minlength=N)
        K = int(cnt.max()) if centre.numel() else 0
        if K < 2:
            return phi2.sum()
        start = torch.cumsum(cnt, 0) - cnt
        slot = torch.arange(centre.numel(), device=xyz.device) - start[centre]
        U = xyz.new_zeros(N, K, 3).index_put((centre, slot), u)
        G = xyz.new_zeros(N, K).index_put((centre, slot), g)             # (padding: g = 0, no contribution)
        t = torch.triu_indices(K, K, offset=1, device=xyz.device)
        c = (U[:, t[0]] * U[:, t[1]]).sum(-1)
        phi3 = lam * eps * (c - self.cos0) ** 2 * G[:, t[0]] * G[:, t[1]]
        return phi2.sum() + phi3.sum()

    def _term(self, xyz):
        return ops.SWTerm(self._current_list(xyz), self._consts, self._theta())


class StillingerWeberMulti(_MovingCutoff, _ManyBodyTerm):
    """Stillinger-Weber potential for 1 <= S <= 4 species in the convention of LAMMPS `pair_style sw`: compounds and mixtures
    (CdTe, GaN, SiGe, mW water with a solute) from tables per ordered pair and per triplet of species.  Atom i has the species
    t_i = `types`[i]; with a = t_i (the centre), b = t_j, c = t_k

        U      = 1/2 sum_i sum_{j != i} phi2_ab(r_ij) + sum_i sum_{j<k in row(i)} phi3_abc(r_ij, r_ik, cos theta_jik)
        phi2_ab  = A_ab eps_ab [B_ab (sigma_ab/r)^p_ab - (sigma_ab/r)^q_ab] exp(sigma_ab / (r - a_ab sigma_ab))   r < a_ab sigma_ab, else 0
        g_ab     = exp(gamma_ab sigma_ab / (r - a_ab sigma_ab))                                                   r < a_ab sigma_ab, else 0
        phi3_abc = K_a{bc} (cos theta - cos0_abc)^2 g_ab(r_ij) g_ac(r_ik),    K_a{bc} = (lam_abc eps3_abc + lam_acb eps3_acb) / 2

    The pair constants (epsilon, sigma, a, gamma, A, B, p, q) are [S, S] tables, row = the species of the centre, column =
    the species of the end (the convention of TersoffMulti); a LAMMPS file supplies them from its (a, b, b) lines.  (lam,
    epsilon3, cos0) are [S, S, S] tables (centre, end, end) from the (a, b, c) lines.  The two ends of a triplet are unordered:
    cos0 must be symmetric in them (anything else is rejected) and the strength enters through the symmetrised K, so the
    energy is a function of every table entry; dU/dlam[a, b, c] and dU/dlam[a, c, b] each receive half of their class's
    derivative, times their own epsilon3.  The pair tables need not be symmetric: U2 = 1/2 sum_i sum_j phi2_{t_i t_j}, so the
    force of a pair is the derivative of (phi2_ab + phi2_ba) / 2.  [a, b] and [b, a] are separate entries that the
    constructors fill equally: a fit that wants them tied ties their gradients (sums the two and writes the sum to both).

    StillingerWeberMulti(system, types, species) takes S one-species sets (dicts with epsilon, sigma, lam and optionally a,
    gamma, cos0, A, B, p, q; PUBLISHED holds silicon and mW) and mixes them (`mix`) by this rule, which is a definition of
    this class and not a claim about any published compound set: sigma_ab, a_ab, gamma_ab are arithmetic means, epsilon_ab
    = sqrt(epsilon_a epsilon_b); A, B, p, q, cos0 are those of the centre; with lam_ab = sqrt(lam_a lam_b),
    lam_abc = sqrt(lam_ab lam_ac) and epsilon3_abc = sqrt(epsilon_ab epsilon_ac), so that lam_abc epsilon3_abc =
    sqrt(lam_ab epsilon_ab lam_ac epsilon_ac).  `from_tables` takes the tables themselves and `from_sw_file` reads a LAMMPS
    `.sw` file, which is how published compound sets reach the class.  S = 1 with epsilon3 = epsilon is StillingerWeber.
    `types` holds one entry per atom of a replica, in [0, S); every replica of System.replicate has the same species.

    `epsilon` [S, S], `sigma` [S, S] and `lam` [S, S, S] are float32 parameters when trainable, otherwise buffers; everything
    else is constant.  The cutoff is max_ab a_ab sigma_ab; a trainable sigma moves it, by the rule and the design constants of
    StillingerWeber: the list is searched with `cutoff_reset` times it and kept while it stays within `cutoff_keep` (one host
    read per change of sigma, never inside a HIP-graph capture; `static_version()` changes with the cutoff).  The kernel
    applies each entry's own support r < a_ab sigma_ab with the live sigma, so a list searched with a larger radius or a skin
    is exact.  Not covered (ValueError where it can be asked for): `index_tuple`, `ex_pairs`, S > 4, non-integer exponents,
    the pressure of the term, the fused trajectory kernels (a Stack holding the term stays on force / force_vjp).

    forward(xyz) is differentiable twice in xyz and once in (epsilon, sigma, lam) on the HIP kernel (ops.SWMultiTerm,
    csrc/sw_multi.hip: the kernel of csrc/sw_core.hpp with every constant looked up by species in a device table); force / force_vjp serve the
    analytic adjoint and HIP-graph replay, also while the parameters require grad.  float64 or host positions take the torch
    restatement `_torch_energy`."""

    MAX_SPECIES = ops.SW_MULTI_MAX_SPECIES
    DEFAULTS = dict(a=1.80, gamma=1.20, cos0=-1.0 / 3.0, A=7.049556277, B=0.6022245584, p=4, q=0)   # StillingerWeber's
    PUBLISHED = dict(silicon=dict(epsilon=2.1683, sigma=2.0951, lam=21.0),
                     mW=dict(epsilon=6.189 * StillingerWeber.KCAL_PER_MOL, sigma=2.3925, lam=23.15))

    def __init__(self, system, types, species, trainable=True, index_tuple=None, ex_pairs=None):
        pair, triplet = self.mix(species)
        self._setup(system, types, pair, triplet, trainable, index_tuple, ex_pairs)

    @classmethod
    def from_tables(cls, system, types, pair, triplet, trainable=True, index_tuple=None, ex_pairs=None):
        """The term from its tables: pair = dict of [S, S] arrays epsilon, sigma, a, gamma, A, B, p, q (row = centre species,
        column = end species), triplet = dict of [S, S, S] arrays lam, epsilon3, cos0 (centre, end, end)."""
        self = cls.__new__(cls)
        self._setup(system, types, pair, triplet, trainable, index_tuple, ex_pairs)
        return self

    @classmethod
    def mix(cls, species):
        """(pair, triplet) tables of S one-species sets under the mixing rule of the class docstring, in float64."""
        species = list(species)
        S = len(species)
        if not 1 <= S <= cls.MAX_SPECIES:
            raise ValueError("StillingerWeberMulti: species must hold 1 to %d parameter sets (got %d)" % (cls.MAX_SPECIES, S))
        for a, p in enumerate(species):
            missing = [k for k in ("epsilon", "sigma", "lam") if k not in p]
            if missing:
                raise ValueError("StillingerWeberMulti: species[%d] lacks %s" % (a, ", ".join(missing)))
            unknown = [k for k in p if k not in ("epsilon", "sigma", "lam") and k not in cls.DEFAULTS]
            if unknown:
                raise ValueError("StillingerWeberMulti: species[%d] has unknown keys %s" % (a, ", ".join(unknown)))
        col = lambda k: np.array([float(p.get(k, cls.DEFAULTS.get(k))) for p in species], dtype=np.float64)
        if not ((col("epsilon") > 0.0) & (col("lam") >= 0.0)).all():
            raise ValueError("StillingerWeberMulti: every species needs epsilon > 0 and lam >= 0")
        geo = lambda v: np.sqrt(np.outer(v, v))
        mean = lambda v: 0.5 * (v[:, None] + v[None, :])
        row = lambda v: np.repeat(v[:, None], S, axis=1)                      # the centre's value
        pair = dict(epsilon=geo(col("epsilon")), sigma=mean(col("sigma")), a=mean(col("a")), gamma=mean(col("gamma")),
                    A=row(col("A")), B=row(col("B")), p=row(col("p")), q=row(col("q")))
        lam2 = geo(col("lam"))
        triplet = dict(lam=np.sqrt(lam2[:, :, None] * lam2[:, None, :]),
                       epsilon3=np.sqrt(pair["epsilon"][:, :, None] * pair["epsilon"][:, None, :]),
                       cos0=np.repeat(np.repeat(col("cos0")[:, None, None], S, axis=1), S, axis=2))
        return pair, triplet

    @staticmethod
    def read_sw_file(path, elements):
        """(pair, triplet) tables of a LAMMPS `.sw` file for the species `elements` (the element name of each species index).
        `#` starts a comment; an entry is 14 whitespace-separated tokens `e1 e2 e3 epsilon sigma a lambda gamma costheta0 A B
        p q tol` (e1 = the centre) and may continue over several lines.  Entries that name an element not in `elements` are
        skipped.  The pair tables come from the (a, b, b) entries, lam, epsilon3 (the entry's epsilon) and cos0 from the
        (a, b, c) entries; `tol` is ignored (this class has no tolerance cutoff for the exponential).  ValueError: a missing
        or repeated entry (naming the triplet), a non-integer exponent, tokens that do not form whole entries."""
        elements = [str(e) for e in elements]
        S = len(elements)
        if not 1 <= S <= StillingerWeberMulti.MAX_SPECIES or len(set(elements)) != S:
            raise ValueError("StillingerWeberMulti: elements must hold 1 to %d distinct names (got %r)"
                             % (StillingerWeberMulti.MAX_SPECIES, elements))
        with open(path) as f:
            tokens = [t for line in f for t in line.split("#", 1)[0].split()]
        if len(tokens) % 14:
            raise ValueError("StillingerWeberMulti: %s holds %d tokens, not a whole number of 14-token entries" % (path, len(tokens)))
        index = {e: k for k, e in enumerate(elements)}
        seen = {}
        for n in range(0, len(tokens), 14):
            names, rest = tokens[n:n + 3], tokens[n + 3:n + 14]
            try:
                vals = [float(v) for v in rest]
            except ValueError:
                raise ValueError("StillingerWeberMulti: %s: entry %s has a non-numeric field (%r)" % (path, " ".join(names), rest))
            if any(e not in index for e in names):
                continue
            key = tuple(index[e] for e in names)
            if key in seen:
                raise ValueError("StillingerWeberMulti: %s: the triplet %s appears twice" % (path, " ".join(names)))
            if vals[8] != int(vals[8]) or vals[9] != int(vals[9]):
                raise ValueError("StillingerWeberMulti: %s: the triplet %s has non-integer exponents p = %r, q = %r (not covered)"
                                 % (path, " ".join(names), vals[8], vals[9]))
            seen[key] = vals
        pair = {k: np.zeros((S, S)) for k in ops.SW_MULTI_PAIR}
        triplet = {k: np.zeros((S, S, S)) for k in ops.SW_MULTI_TRIPLET}
        for a in range(S):
            for b in range(S):
                for c in range(S):
                    if (a, b, c) not in seen:
                        raise ValueError("StillingerWeberMulti: %s has no entry for the triplet %s %s %s"
                                         % (path, elements[a], elements[b], elements[c]))
                    eps, sig, aa, lam, gam, cos0, A, B, p, q, _tol = seen[(a, b, c)]
                    triplet["lam"][a, b, c], triplet["epsilon3"][a, b, c], triplet["cos0"][a, b, c] = lam, eps, cos0
                    if b == c:
                        for k, v in zip(ops.SW_MULTI_PAIR, (eps, sig, aa, gam, A, B, p, q)):
                            pair[k][a, b] = v
        return pair, triplet

    @classmethod
    def from_sw_file(cls, system, types, path, elements, trainable=True, index_tuple=None, ex_pairs=None):
        """The term from a LAMMPS `.sw` file (`read_sw_file`): `elements` lists the element name of each species index."""
        pair, triplet = cls.read_sw_file(path, elements)
        return cls.from_tables(system, types, pair, triplet, trainable=trainable, index_tuple=index_tuple, ex_pairs=ex_pairs)

    def _setup(self, system, types, pair, triplet, trainable, index_tuple, ex_pairs):
        _ListTerm.__init__(self, system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("StillingerWeberMulti: index_tuple and ex_pairs are not supported (every pair interacts)")
        for name, keys, given in (("pair", ops.SW_MULTI_PAIR, pair), ("triplet", ops.SW_MULTI_TRIPLET, triplet)):
            missing = [k for k in keys if k not in given]
            if missing:
                raise ValueError("StillingerWeberMulti: %s lacks %s" % (name, ", ".join(missing)))
        S = int(np.asarray(pair["epsilon"]).shape[0]) if np.asarray(pair["epsilon"]).ndim == 2 else -1
        if S > self.MAX_SPECIES:
            raise ValueError("StillingerWeberMulti: S = %d species; at most %d are supported" % (S, self.MAX_SPECIES))
        try:
            self._image = ops.sw_multi_tables(pair, triplet)                   # (validates every entry)
        except ValueError as e:
            raise ValueError(str(e).replace("mdgrad_amd:", "StillingerWeberMulti:")) from None
        self.n_species = S
        self._pair = {k: np.asarray(pair[k], dtype=np.float64).reshape(S, S) for k in ops.SW_MULTI_PAIR}
        self._triplet = {k: np.asarray(triplet[k], dtype=np.float64).reshape(S, S, S) for k in ops.SW_MULTI_TRIPLET}
        ty = np.asarray(torch.as_tensor(types).detach().cpu().numpy()).reshape(-1)
        if ty.shape[0] != self._group:
            raise ValueError("StillingerWeberMulti: types must hold one entry per atom of a replica (%d), got %d"
                             % (self._group, ty.shape[0]))
        if not np.issubdtype(ty.dtype, np.integer) or ty.min() < 0 or ty.max() >= S:
            raise ValueError("StillingerWeberMulti: types must be integers in [0, %d)" % S)
        self._init_cutoff(system)
        rc = float((self._pair["a"] * self._pair["sigma"]).max())
        if rc > self._half_height:
            raise ValueError("StillingerWeberMulti: max a * sigma = %g exceeds half the shortest cell height (%g)"
                             % (rc, self._half_height))
        for name in ("epsilon", "sigma", "lam"):
            t = torch.tensor((self._triplet if name == "lam" else self._pair)[name], dtype=torch.float32, device=self.device)
            if trainable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self.types = torch.as_tensor(np.tile(ty.astype(np.int32), self._n_rep), device=self.device)   # one entry per atom
        self._ell = None
        self._template = torch.as_tensor(self._image, device=self.device)
        self._a32 = torch.tensor(self._pair["a"], dtype=torch.float32, device=self.device)
        self._e3 = torch.tensor(self._triplet["epsilon3"], dtype=torch.float32, device=self.device)
        self._table_mirror = _DeviceMirror(self._thetas, pack=self._pack_tables, numel=int(self._image.shape[0]))
        self._sync_cutoff()
        if torch.device(self.device).type == "cuda":
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._tables()

    # -- the cutoff the list is searched with: _MovingCutoff on max_ab a_ab sigma_ab -----------------------------------
    def _support_radius(self):
        sd = self.sigma.detach()
        rc, smin = torch.stack([(self._a32.to(sd.device) * sd).max(), sd.min()]).tolist()   # (one host read per change of sigma)
        if not smin > 0.0:
            raise ValueError("StillingerWeberMulti: every sigma must stay positive (got %g)" % smin)
        if rc > self._half_height:
            raise ValueError("StillingerWeberMulti: max a * sigma = %g exceeds half the shortest cell height (%g)"
                             % (rc, self._half_height))
        return rc

    # -- the device table the kernel reads: the constants plus what follows from the current (epsilon, sigma, lam) -----
    def _thetas(self):
        return self.epsilon, self.sigma, self.lam

    def _pack_tables(self, ps, out=None):
        """The table image (ops.sw_multi_tables) with the current epsilon, sigma, lam and the entries derived from them
        (a sigma, gamma sigma, A epsilon, the symmetrised K), by device ops only."""
        S = self.n_species
        eps, sig, lam = (p.detach().to(torch.float32) for p in ps)
        tmpl = self._template.to(eps.device)
        out = tmpl.clone() if out is None else out.copy_(tmpl)
        n2 = ops.SW_MULTI_PAIR_FLOATS * S * S
        pair, cpair = out[:n2].view(S * S, ops.SW_MULTI_PAIR_FLOATS), tmpl[:n2].view(S * S, ops.SW_MULTI_PAIR_FLOATS)
        eps, sig = eps.reshape(-1), sig.reshape(-1)
        pair[:, 0].copy_(eps)
        pair[:, 1].copy_(sig)
        pair[:, 2].copy_(cpair[:, 9] * sig)
        pair[:, 3].copy_(cpair[:, 4] * sig)
        pair[:, 10].copy_(cpair[:, 5] * eps)
        le = lam * self._e3.to(eps.device)
        out[n2:].view(S, S, S, ops.SW_MULTI_TRIPLET_FLOATS)[..., 0].copy_(0.5 * (le + le.transpose(1, 2)))
        return out

    def _tables(self):
        """The derived constants as the kernel reads them: a device mirror (_DeviceMirror) rewritten when epsilon, sigma or
        lam changed, so that the captured steps carry no host value of a parameter."""
        return self._table_mirror.get()

    def prepare_pass(self):
        self._sync_cutoff()
        if self._hip_ok():
            self._tables()

    # -- energy ----------------------------------------------------------------------------------------------------
    def _torch_energy(self, xyz):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in
        epsilon, sigma, lam): every pair as two directed bonds with the constants of (centre species, end species), grouped
        by centre into a padded [N, K] table, then every triplet as two entries of one atom's row."""
        const = lambda v: torch.as_tensor(v, dtype=xyz.dtype, device=xyz.device)
        eps, sig, lam = (p.to(xyz) for p in (self.epsilon, self.sigma, self.lam))
        a_t = const(self._pair["a"])
        i, j, off = self._all_pairs(xyz, float((a_t * sig.detach()).max()))
        if i.numel() == 0:
            return xyz.sum() * 0.0
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        dv = xyz[i] - xyz[j] - off.matmul(cell)
        r = dv.pow(2).sum(-1).sqrt()
        ty = self.types.to(xyz.device).long()
        N = xyz.shape[0]
        centre, end = torch.cat([i, j]), torch.cat([j, i])
        u, r2 = torch.cat([-dv, dv]) / torch.cat([r, r])[:, None], torch.cat([r, r])
        ta, tb = ty[centre], ty[end]
        sg = sig[ta, tb]
        rc = a_t[ta, tb] * sg
        inside = r2 < rc
        rs = torch.where(inside, r2, 0.5 * rc.detach())                  # (a harmless r outside the support: no 1/0, no nan)
        per = lambda name: const(self._pair[name])[ta, tb]
        sr = sg / rs
        phi2 = per("A") * eps[ta, tb] * (per("B") * sr ** per("p") - sr ** per("q")) * torch.exp(sg / (rs - rc))
        U2 = 0.5 * torch.where(inside, phi2, torch.zeros_like(phi2)).sum()
        g = torch.where(inside, torch.exp(per("gamma") * sg / (rs - rc)), torch.zeros_like(rs))
        order = torch.argsort(centre, stable=True)
        centre, u, g, tb = centre[order], u[order], g[order], tb[order]
        cnt = torch.bincount(centre, minlength=N)
        K = int(cnt.max())
        if K < 2:
            return U2
        start = torch.cumsum(cnt, 0) - cnt
        slot = torch.arange(centre.numel(), device=xyz.device) - start[centre]
        Uv = xyz.new_zeros(N, K, 3).index_put((centre, slot), u)
        G = xyz.new_zeros(N, K).index_put((centre, slot), g)                # (padding: g = 0, no contribution)
        Tb = torch.zeros(N, K, dtype=torch.long, device=xyz.device).index_put((centre, slot), tb)
        t = torch.triu_indices(K, K, offset=1, device=xyz.device)
        cth = (Uv[:, t[0]] * Uv[:, t[1]]).sum(-1)
        ca, cb, cc = ty[:, None].expand(N, t.shape[1]), Tb[:, t[0]], Tb[:, t[1]]
        le = lam * const(self._triplet["epsilon3"])
        Kt = 0.5 * (le[ca, cb, cc] + le[ca, cc, cb])
        phi3 = Kt * (cth - const(self._triplet["cos0"])[ca, cb, cc]) ** 2 * G[:, t[0]] * G[:, t[1]]
        return U2 + phi3.sum()

    def _term(self, xyz):
        return ops.SWMultiTerm(self._current_list(xyz), self.types, self.n_species, self._tables())


class SuttonChen(_ManyBodyTerm):
    """Sutton-Chen embedded-atom potential for one species (Sutton and Chen 1990; the Finnis-Sinclair form of the
    embedded-atom method): the cohesion of an fcc metal as a function of the local density, not a sum over pairs.  With
    the parameters epsilon (energy), a (length), c (dimensionless) and the integer exponents n > m >= 1:

        U      = sum_i [ 1/2 sum_{j != i} phi(r_ij)  -  epsilon c sqrt(rho_i) ]
        rho_i  = sum_{j != i} f(r_ij)
        phi(r) = epsilon S_n(r),   f(r) = S_m(r)
        S_k(r) = (a/r)^k - (a/rc)^k + k (r - rc) (a/rc)^k / rc     for r < rc, else exactly 0     (shift="force")
        S_k(r) = (a/r)^k                                            for r < rc, else exactly 0     (shift="none")

    shift="force" (the default) makes S_k and S_k' vanish at rc = `cutoff`, the convention of CoulombPotentials; by convexity
    S_k >= 0, so rho_i >= 0.  shift="none" is the potential as published.  An atom with no neighbour inside rc has
    rho_i = 0; its embedding energy, F'(rho_i) and F''(rho_i) are defined as exactly 0 (F = -epsilon c sqrt(rho)).
    A property of the model, whatever the shift: with the square-root embedding F'(rho) diverges as rho -> 0, so the
    force between the two atoms of an isolated pair has a step at rc (2 F' f' tends to a constant there).  It is irrelevant
    in condensed phases, where every atom keeps neighbours well inside rc.

    The pair set, the minimum image and the (d2 < rc^2) & (d2 != 0) test are those of PairPotentials at the cutoff rc;
    the replicas of System.replicate never see each other.  `cutoff` is an absolute length and does not move with a.

    `epsilon`, `a` and `c` are one-element float32 parameters when trainable, otherwise buffers; n, m, cutoff and shift
    are constants.  Not covered: `index_tuple`, `ex_pairs` (both rejected), several species, tabulated embedding functions.
    `copper`, `nickel`, `silver` and `gold` carry the published constants (epsilon in eV, a in Angstrom), cutoff 2 a by default.

    forward(xyz) is differentiable twice in xyz and once in (epsilon, a, c) on the HIP kernels (ops.EAMTerm,
    csrc/eam.hip: a density pass, then a force pass that reads the neighbours' embedding derivatives); force / force_vjp
    serve the analytic adjoint and HIP-graph replay, also while the parameters require grad.  float64 or host positions take
    the torch restatement `_torch_energy`."""

    PUBLISHED = {"copper": (1.2382e-2, 3.61, 39.432, 9, 6), "nickel": (1.5707e-2, 3.52, 39.432, 9, 6),
                 "silver": (2.5415e-3, 4.09, 144.41, 12, 6), "gold": (1.2793e-2, 4.08, 34.408, 10, 8)}

    def __init__(self, system, epsilon, a, c, n, m, cutoff, shift="force", trainable=True, index_tuple=None, ex_pairs=None):
        super().__init__(system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("SuttonChen: index_tuple and ex_pairs are not supported (one species, every pair)")
        self._consts = ops.eam_consts(epsilon, a, c, n, m, cutoff, shift)
        k = self._consts
        self.n, self.m, self.cutoff, self.shift = int(k.n), int(k.m), float(k.rc), shift
        h = np.asarray(system.get_cell(), dtype=np.float64)
        h = np.diag(h) if h.ndim == 1 else h
        vol = abs(float(np.linalg.det(h)))
        self._half_height = 0.5 * min(vol / float(np.linalg.norm(np.cross(h[(d + 1) % 3], h[(d + 2) % 3]))) for d in range(3))
        if self.cutoff > self._half_height:
            raise ValueError("SuttonChen: cutoff = %g exceeds half the shortest cell height (%g)"
                             % (self.cutoff, self._half_height))
        for name, v in (("epsilon", k.epsilon), ("a", k.a), ("c", k.c)):
            t = torch.tensor([v], dtype=torch.float32, device=self.device)
            if trainable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self._ell = None
        self._theta_mirror = _DeviceMirror(self._thetas)
        self._work = None
        if torch.device(self.device).type == "cuda":
            # the scratch of the density pass: persistent, so that a captured graph sees a fixed address
            self._work = torch.empty(system.get_number_of_atoms(), 4, dtype=torch.float32, device=self.device)
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._theta()

    @classmethod
    def _published(cls, name, system, cutoff, kw):
        eps, a, c, n, m = cls.PUBLISHED[name]
        return cls(system, eps, a, c, n, m, 2.0 * a if cutoff is None else cutoff, **kw)

    @classmethod
    def copper(cls, system, cutoff=None, **kw):
        """Sutton and Chen's copper: epsilon = 1.2382e-2 eV, a = 3.61 Angstrom, c = 39.432, n = 9, m = 6."""
        return cls._published("copper", system, cutoff, kw)

    @classmethod
    def nickel(cls, system, cutoff=None, **kw):
        """Sutton and Chen's nickel: epsilon = 1.5707e-2 eV, a = 3.52 Angstrom, c = 39.432, n = 9, m = 6."""
        return cls._published("nickel", system, cutoff, kw)

    @classmethod
    def silver(cls, system, cutoff=None, **kw):
        """Sutton and Chen's silver: epsilon = 2.5415e-3 eV, a = 4.09 Angstrom, c = 144.41, n = 12, m = 6."""
        return cls._published("silver", system, cutoff, kw)

    @classmethod
    def gold(cls, system, cutoff=None, **kw):
        """Sutton and Chen's gold: epsilon = 1.2793e-2 eV, a = 4.08 Angstrom, c = 34.408, n = 10, m = 8."""
        return cls._published("gold", system, cutoff, kw)

    # -- the device copy of (epsilon, a, c) the kernels read (the lists are _ListTerm's, those of PairPotentials) --
    def _thetas(self):
        return self.epsilon, self.a, self.c

    def _theta(self):
        """(epsilon, a, c) as the kernels read them: their device mirror (_DeviceMirror), so that the captured steps carry
        no host value of a parameter."""
        return self._theta_mirror.get()

    def prepare_pass(self):
        if self._hip_ok():
            self._theta()

    # (not the base's: the density pass keeps four floats per atom, sized by the positions, not per list slot)
    def _scratch(self, xyz):
        if self._work is None or self._work.device != xyz.device or self._work.shape[0] != xyz.shape[0]:
            self._work = torch.empty(xyz.shape[0], 4, dtype=torch.float32, device=xyz.device)
        return self._work

    # -- energy ----------------------------------------------------------------------------------------------------
    def _shape(self, r, a, k):
        s = (a / r) ** k
        if self.shift == "none":
            return s
        q = (a / self.cutoff) ** k
        return s - q + k * (r - self.cutoff) * q / self.cutoff

    def _torch_energy(self, xyz, thetas=None):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in
        epsilon, a, c).  `thetas`: (epsilon, a, c) as the caller holds them (thermo.EAMEnergy casts them once for all its
        frames, so that their gradient is summed over the frames in the dtype of xyz)."""
        eps, a, c = (p.to(xyz).reshape(()) for p in (thetas or (self.epsilon, self.a, self.c)))
        i, j, off = self._all_pairs(xyz, self.cutoff)
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        d = xyz[i] - xyz[j] - off.matmul(cell)
        r = d.pow(2).sum(-1).sqrt()
        f = self._shape(r, a, self.m)
        rho = xyz.new_zeros(xyz.shape[0]).index_add(0, torch.cat([i, j]), torch.cat([f, f]))
        dense = rho > 0                                      # rho = 0: no embedding energy, and no 0/0 in its derivatives
        root = torch.where(dense, rho, torch.ones_like(rho)).sqrt() * dense.to(xyz)
        return eps * (self._shape(r, a, self.n).sum() - c * root.sum())

    def _term(self, xyz):
        return ops.EAMTerm(self._ell, self._consts, self._theta(), self._scratch(xyz))


def _hermite(nodes, which, x, x0, h):
    """Table `which[m]` of `nodes` [K, n, 2] at x[m]: the cubic-Hermite interpolant of the node entries (value, h * derivative)
    on the grid x0 + g h, continued linearly below the first and above the last node (differentiable in x and in nodes)."""
    n = nodes.shape[1]
    u = (x - x0) / h
    g = u.detach().floor().clamp(0, n - 2).long()
    t = u - g.to(u)
    lo, hi = nodes[which, g], nodes[which, g + 1]
    c = t.clamp(0.0, 1.0)
    s = 1.0 - c
    inside = (1.0 + 2.0 * c) * s * s * lo[:, 0] + c * s * s * lo[:, 1] + c * c * (3.0 - 2.0 * c) * hi[:, 0] - c * c * s * hi[:, 1]
    below, above = lo[:, 0] + t * lo[:, 1], hi[:, 0] + (t - 1.0) * hi[:, 1]
    return torch.where(t < 0, below, torch.where(t > 1, above, inside))


def _five_point(y):
    """h * dy/dx at every point of the uniform samples y [..., n] by the formula LAMMPS builds its setfl splines from:
    (y[m-2] - y[m+2] + 8 (y[m+1] - y[m-1])) / 12 inside, central differences next to the ends, one-sided at the ends."""
    y = np.asarray(y, dtype=np.float64)
    d = np.empty_like(y)
    d[..., 0], d[..., -1] = y[..., 1] - y[..., 0], y[..., -1] - y[..., -2]
    d[..., 1], d[..., -2] = 0.5 * (y[..., 2] - y[..., 0]), 0.5 * (y[..., -1] - y[..., -3])
    d[..., 2:-2] = (y[..., :-4] - y[..., 4:] + 8.0 * (y[..., 3:-1] - y[..., 1:-3])) / 12.0
    return d


class EAM(_ManyBodyTerm):
    """Tabulated embedded-atom potential for 1 <= S <= 4 species (Daw and Baskes 1984; the "eam/alloy" form in which the
    potentials of Mishin, Zhou, Mendelev are distributed as setfl files).  Atom i has the species t_i = `types`[i]; with
    a = t_i, b = t_j:

        U     = sum_i [ 1/2 sum_{j != i} phi_ab(r_ij) + F_a(rho_i) ]
        rho_i = sum_{j != i} f_b(r_ij)

    The density an atom contributes depends on its own species only, and phi_ab = phi_ba is stored once per unordered pair:
    S (S + 1) / 2 pair tables, pair (a, b) at index hi (hi + 1) / 2 + lo (the lower triangle: 00, 10, 11, 20, ...).  The pair
    set, the minimum image and the 0 < r < rc test are those of SuttonChen at rc = `cutoff`; the replicas of System.replicate
    never see each other; a list searched with a skin is exact.

    Every function is a cubic-Hermite interpolant on a uniform grid; a node entry is (value, h * derivative), the convention
    of the tabulated pair model.  phi and f are tabulated in r on r_g = r_min + g h_r, g = 0 .. n_r - 1, with r_{n_r - 1} =
    cutoff; F in rho on rho_g = rho_min + g h_rho over `rho_range` = (rho_min, rho_max).  4 <= n_r, n_rho <= 4096.  Outside
    its grid (r < r_min; rho < rho_min or rho > rho_max) a function continues linearly with the end node's value and slope:
    every argument has a finite, C1 value.  An atom without a neighbour inside the cutoff has rho = 0 and gets F_a(0) from
    the table -- unlike SuttonChen, where its embedding energy is exactly 0.

    The nodes are the parameters: `pair_nodes` [S (S + 1) / 2, n_r, 2], `density_nodes` [S, n_r, 2], `embed_nodes`
    [S, n_rho, 2].  `trainable` names those that are nn.Parameters ("pair", "density", "embed"; True = all, False = none),
    the rest are buffers; `dtype` is their storage type (the kernels read a float32 mirror).  With pin_cutoff=True (the
    default) the last node of every phi and f table is held at (0, 0), so that energy and force are continuous at the
    cutoff: the constructor sets those entries to zero and their gradient entries come back as exact zeros.

    `from_functions` tabulates Python callables, `from_sutton_chen` is the tabulated twin of SuttonChen, `from_setfl` /
    `write_setfl` read and write the setfl text format.  Not covered: functions given as nn.Modules and re-tabulated per
    pass, the Finnis-Sinclair form with a density function per pair (f_ab) and funcfl files, `index_tuple` and `ex_pairs`
    (both rejected), the pressure of the term, the fused trajectory kernels (a Stack holding the term stays off them).

    forward(xyz) is differentiable twice in xyz and once in the nodes on the HIP kernels (ops.EAMTableTerm,
    csrc/eam_table.hip: the two passes of csrc/eam.hip with every function looked up by species in a device table, and an
    order-independent fixed-point scatter for the node gradients); force / force_vjp serve the analytic adjoint and
    HIP-graph replay, also while the nodes require grad.  float64 or host positions take the torch restatement
    `_torch_energy`."""

    MAX_SPECIES = ops.EAM_TABLE_MAX_SPECIES
    TABLES = ("pair", "density", "embed")

    def __init__(self, system, types, pair_nodes, density_nodes, embed_nodes, cutoff, r_min, rho_range,
                 trainable=("pair", "density", "embed"), pin_cutoff=True, dtype=torch.float32, index_tuple=None, ex_pairs=None):
        super().__init__(system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("EAM: index_tuple and ex_pairs are not supported (every pair interacts)")
        if trainable is True or trainable is False:
            trainable = self.TABLES if trainable else ()
        trainable = tuple(trainable)
        if any(name not in self.TABLES for name in trainable):
            raise ValueError("EAM: trainable names tables among %r (got %r)" % (self.TABLES, trainable))
        nodes = [torch.as_tensor(v).detach().to("cpu", torch.float64).clone() for v in (pair_nodes, density_nodes, embed_nodes)]
        if any(v.dim() != 3 or v.shape[2] != 2 for v in nodes):
            raise ValueError("EAM: every node tensor is [tables, nodes, 2] (got %s)" % ([tuple(v.shape) for v in nodes],))
        S, n_r, n_rho = int(nodes[1].shape[0]), int(nodes[1].shape[1]), int(nodes[2].shape[1])
        if not 1 <= S <= self.MAX_SPECIES:
            raise ValueError("EAM: S = %d species; 1 to %d are supported" % (S, self.MAX_SPECIES))
        if tuple(nodes[0].shape) != (S * (S + 1) // 2, n_r, 2) or int(nodes[2].shape[0]) != S:
            raise ValueError("EAM: for S = %d species on n_r = %d nodes pair_nodes is [%d, %d, 2] and embed_nodes [%d, n_rho, 2] "
                             "(got %s, %s)" % (S, n_r, S * (S + 1) // 2, n_r, S, tuple(nodes[0].shape), tuple(nodes[2].shape)))
        if not all(bool(torch.isfinite(v).all()) for v in nodes):
            raise ValueError("EAM: the node entries must be finite")
        rho_range = tuple(float(v) for v in rho_range)
        if len(rho_range) != 2:
            raise ValueError("EAM: rho_range = (rho_min, rho_max) (got %r)" % (rho_range,))
        self._consts = ops.eam_table_consts(S, n_r, n_rho, r_min, cutoff, rho_range[0], rho_range[1], pin_cutoff)
        k = self._consts
        self.n_species, self.n_r, self.n_rho, self.pin_cutoff = S, n_r, n_rho, bool(pin_cutoff)
        self.cutoff, self.r_min, self.rho_range = float(k.rc), float(k.r_min), rho_range
        self.h_r, self.h_rho = float(k.h_r), float(k.h_rho)
        ty = np.asarray(torch.as_tensor(types).detach().cpu().numpy()).reshape(-1)
        if ty.shape[0] != self._group:
            raise ValueError("EAM: types must hold one entry per atom of a replica (%d), got %d" % (self._group, ty.shape[0]))
        if not np.issubdtype(ty.dtype, np.integer) or ty.min() < 0 or ty.max() >= S:
            raise ValueError("EAM: types must be integers in [0, %d)" % S)
        h = np.asarray(system.get_cell(), dtype=np.float64)
        h = np.diag(h) if h.ndim == 1 else h
        vol = abs(float(np.linalg.det(h)))
        self._half_height = 0.5 * min(vol / float(np.linalg.norm(np.cross(h[(d + 1) % 3], h[(d + 2) % 3]))) for d in range(3))
        if self.cutoff > self._half_height:
            raise ValueError("EAM: cutoff = %g exceeds half the shortest cell height (%g)" % (self.cutoff, self._half_height))
        if self.pin_cutoff:
            nodes[0][:, -1, :] = 0.0
            nodes[1][:, -1, :] = 0.0
        self._select, pos = [], 0
        for name, v in zip(self.TABLES, nodes):
            t = v.to(self.device, dtype)
            if name in trainable:
                setattr(self, name + "_nodes", torch.nn.Parameter(t))
                self._select.append((pos, pos + t.numel()))
            else:
                self.register_buffer(name + "_nodes", t)
            pos += t.numel()
        self.trainable = tuple(name for name in self.TABLES if name in trainable)
        self.density_at_origin = None                                   # f_b(0) of a setfl file, kept for write_setfl
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self.types = torch.as_tensor(np.tile(ty.astype(np.int32), self._n_rep), device=self.device)   # one entry per atom
        self._ell = None
        self._table_mirror = _DeviceMirror(self._nodes)
        self._work, self._fx = None, None
        if torch.device(self.device).type == "cuda":
            # the scratch of the density pass and of the fixed-point scatter: persistent, so that a captured graph sees fixed addresses
            self._work = torch.empty(system.get_number_of_atoms(), 4, dtype=torch.float32, device=self.device)
            self._fx = torch.empty(ops.eam_table_fx_size(k), dtype=torch.int64, device=self.device)
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._tables()

    # -- constructors ----------------------------------------------------------------------------------------------
    @staticmethod
    def tabulate(fn, x0, x1, n):
        """[n, 2] float64 node entries (value, h * derivative) of `fn` on n points from x0 to x1.  `fn` maps a float64 tensor
        to a tensor of its shape and is differentiated by autograd, or is a pair (fn, dfn) with the derivative supplied."""
        x = torch.linspace(float(x0), float(x1), int(n), dtype=torch.float64)
        h = (float(x1) - float(x0)) / (int(n) - 1)
        if isinstance(fn, (tuple, list)):
            y, dy = fn[0](x), fn[1](x)
        else:
            with torch.enable_grad():
                xg = x.clone().requires_grad_(True)
                y = fn(xg)
                (dy,) = torch.autograd.grad(y.sum(), xg)
        return torch.stack([torch.as_tensor(y).detach().double(), h * torch.as_tensor(dy).detach().double()], -1)

    @classmethod
    def from_functions(cls, system, types, pair, density, embed, cutoff, r_min, rho_range, n_r=1024, n_rho=1024, **kw):
        """The term from Python callables, tabulated in float64 (`tabulate`): `density` and `embed` hold one function per
        species; `pair` one per unordered species pair, as a dict keyed (a, b) (either order) or a list in the order of the
        lower triangle (00, 10, 11, 20, ...)."""
        density, embed = list(density), list(embed)
        S = len(density)
        if len(embed) != S or not 1 <= S <= cls.MAX_SPECIES:
            raise ValueError("EAM: density and embed hold one function per species, 1 to %d of them (got %d, %d)"
                             % (cls.MAX_SPECIES, S, len(embed)))
        order = [(a, b) for a in range(S) for b in range(a + 1)]
        if isinstance(pair, dict):
            missing = [ab for ab in order if ab not in pair and ab[::-1] not in pair]
            if missing:
                raise ValueError("EAM: pair lacks a function for the species pairs %r" % (missing,))
            pair = [pair[ab] if ab in pair else pair[ab[::-1]] for ab in order]
        pair = list(pair)
        if len(pair) != len(order):
            raise ValueError("EAM: pair holds %d functions for %d species (got %d)" % (len(order), S, len(pair)))
        pn = torch.stack([cls.tabulate(f, r_min, cutoff, n_r) for f in pair])
        dn = torch.stack([cls.tabulate(f, r_min, cutoff, n_r) for f in density])
        en = torch.stack([cls.tabulate(f, rho_range[0], rho_range[1], n_rho) for f in embed])
        return cls(system, types, pn, dn, en, cutoff, r_min, rho_range, **kw)

    @classmethod
    def from_sutton_chen(cls, system, preset_or_constants, cutoff=None, shift="force", rho_range=None, r_min=None, n_r=1024,
                         n_rho=1024, **kw):
        """The tabulated twin of SuttonChen: phi = epsilon S_n, f = S_m, F = -epsilon c sqrt(rho) for a preset name of
        SuttonChen.PUBLISHED or the constants (epsilon, a, c, n, m); cutoff 2 a and r_min a / 2 by default.  rho_range defaults
        to (rho_lo / 2, 3 rho_hi / 2) of the densities at the system's positions; rho_min must be positive, because sqrt(rho)
        has no finite slope at 0."""
        eps, a, c, n, m = SuttonChen.PUBLISHED[preset_or_constants] if isinstance(preset_or_constants, str) else preset_or_constants
        eps, a, c, n, m = float(eps), float(a), float(c), int(n), int(m)
        cutoff = 2.0 * a if cutoff is None else float(cutoff)
        r_min = 0.5 * a if r_min is None else float(r_min)
        if shift not in ops.EAM_SHIFTS:
            raise ValueError("EAM: shift must be 'force' or 'none' (got %r)" % (shift,))

        def S(k):
            q = (a / cutoff) ** k if shift == "force" else 0.0
            return (lambda r: (a / r) ** k - q + k * (r - cutoff) * q / cutoff), (lambda r: -k * (a / r) ** k / r + k * q / cutoff)
        Sn, Sm = S(n), S(m)
        if rho_range is None:
            probe = cls.__new__(cls)
            GeneralInteraction.__init__(probe, system)
            probe._n_rep = system.get_number_of_atoms() // probe._group
            x = torch.as_tensor(np.asarray(system.get_positions()), dtype=torch.float64)
            i, j, off = probe._all_pairs(x, cutoff)
            cell = probe.cell.detach().to(x)
            cell = torch.diag(cell) if cell.dim() == 1 else cell
            r = (x[i] - x[j] - off.matmul(cell)).pow(2).sum(-1).sqrt()
            rho = x.new_zeros(x.shape[0]).index_add(0, torch.cat([i, j]), torch.cat([Sm[0](r)] * 2))
            rho_range = (0.5 * float(rho.min()), 1.5 * float(rho.max()))
        if not float(rho_range[0]) > 0.0:
            raise ValueError("EAM.from_sutton_chen: rho_min must be positive: sqrt(rho) has no finite slope at 0 (got %r)" % (rho_range[0],))
        pair = (lambda r: eps * Sn[0](r)), (lambda r: eps * Sn[1](r))
        embed = (lambda p: -eps * c * p.sqrt()), (lambda p: -0.5 * eps * c / p.sqrt())
        ty = np.zeros(getattr(system, "group_size", system.get_number_of_atoms()), dtype=np.int64)
        kw.setdefault("pin_cutoff", shift == "force")        # (as published the functions do not vanish at the cutoff)
        return cls.from_functions(system, ty, [pair], [Sm], [embed], cutoff, r_min, rho_range, n_r, n_rho, **kw)

    @staticmethod
    def read_setfl(path_or_file):
        """The content of a setfl ("eam/alloy") text file: dict(comments [3], elements [S], header [S] (atomic number, mass,
        lattice constant, lattice), n_rho, d_rho, n_r, d_r, cutoff, F [S, n_rho], f [S, n_r], z2r [S (S + 1) / 2, n_r] =
        r phi(r) in the order of the lower triangle), numbers in float64."""
        text = path_or_file.read() if hasattr(path_or_file, "read") else open(path_or_file).read()
        lines = text.splitlines()
        if len(lines) < 6:
            raise ValueError("EAM: not a setfl file (fewer than six lines)")
        head = lines[3].split()
        S = int(head[0])
        elements = head[1:1 + S]
        if len(elements) != S or S < 1:
            raise ValueError("EAM: line 4 of a setfl file is 'N element_1 ... element_N' (got %r)" % lines[3])
        g = lines[4].replace("D", "E").replace("d", "e").split()
        n_rho, d_rho, n_r, d_r, cutoff = int(g[0]), float(g[1]), int(g[2]), float(g[3]), float(g[4])
        tok = " ".join(lines[5:]).split()
        pos, header, F, f = 0, [], [], []
        num = lambda t: float(t.replace("D", "E").replace("d", "e"))
        need = S * (4 + n_rho + n_r) + S * (S + 1) // 2 * n_r
        if len(tok) < need:
            raise ValueError("EAM: the setfl file holds %d entries after line 5, %d are needed" % (len(tok), need))
        for _ in range(S):
            header.append((int(tok[pos]), num(tok[pos + 1]), num(tok[pos + 2]), tok[pos + 3]))
            pos += 4
            F.append([num(t) for t in tok[pos:pos + n_rho]])
            pos += n_rho
            f.append([num(t) for t in tok[pos:pos + n_r]])
            pos += n_r
        z = []
        for _ in range(S * (S + 1) // 2):
            z.append([num(t) for t in tok[pos:pos + n_r]])
            pos += n_r
        return dict(comments=lines[:3], elements=elements, header=header, n_rho=n_rho, d_rho=d_rho, n_r=n_r, d_r=d_r, cutoff=cutoff,
                    F=np.array(F, dtype=np.float64), f=np.array(f, dtype=np.float64), z2r=np.array(z, dtype=np.float64))

    @classmethod
    def from_setfl(cls, system, types, path_or_file, elements=None, **kw):
        """The term from a setfl ("eam/alloy") file.  `elements` selects and orders the file's elements as species 0, 1, ...
        (default: all, in file order).  The file tabulates F on rho = g d_rho and f, r phi on r = g d_r, g from 0: the grid
        point r = 0 is dropped (r_min = d_r, r phi divided by r on the rest), and rc is the largest grid point that does not
        exceed the file's cutoff, so n_r = floor(cutoff / d_r) nodes are kept.  Node slopes come from the five-point formula
        LAMMPS builds its splines from, applied on the file's full grid to F, f and r phi (phi' = (r phi)' / r - phi / r);
        the node values are the file's, so pin_cutoff defaults to False here.  f(0) is kept in `density_at_origin` for
        `write_setfl`."""
        d = cls.read_setfl(path_or_file)
        names = d["elements"]
        elements = list(names) if elements is None else list(elements)
        if any(e not in names for e in elements):
            raise ValueError("EAM: the setfl file holds %r, not %r" % (names, [e for e in elements if e not in names]))
        idx = [names.index(e) for e in elements]
        gc = min(int(math.floor(d["cutoff"] / d["d_r"] + 1e-9)), d["n_r"] - 1)
        if gc < 4 or d["n_rho"] < 4:
            raise ValueError("EAM: the setfl grids are too short (n_rho = %d, %d points of r inside the cutoff)" % (d["n_rho"], gc))
        r = d["d_r"] * np.arange(1, gc + 1)
        tri = lambda a, b: max(a, b) * (max(a, b) + 1) // 2 + min(a, b)
        z, dz = d["z2r"], _five_point(d["z2r"])
        pair = []
        for a in range(len(idx)):
            for b in range(a + 1):
                p = tri(idx[a], idx[b])
                phi = z[p, 1:gc + 1] / r
                pair.append(np.stack([phi, dz[p, 1:gc + 1] / r - d["d_r"] * phi / r], -1))
        dens = np.stack([d["f"][idx, 1:gc + 1], _five_point(d["f"])[idx, 1:gc + 1]], -1)
        emb = np.stack([d["F"][idx], _five_point(d["F"])[idx]], -1)
        kw.setdefault("pin_cutoff", False)
        self = cls(system, types, np.stack(pair), dens, emb, float(r[-1]), d["d_r"], (0.0, (d["n_rho"] - 1) * d["d_rho"]), **kw)
        self.density_at_origin = d["f"][idx, 0].copy()
        self.elements, self.setfl_header = elements, [d["header"][k] for k in idx]
        return self

    def write_setfl(self, path_or_file, elements=None, header=None, comments=None):
        """The node values as a setfl file (the inverse of `from_setfl` for them; the slopes are not part of the format).  The
        grids must be those of the format: rho_min = 0 and r_min = h_r.  f(0) is `density_at_origin` when the term was read
        from a file, otherwise the linear continuation; r phi at r = 0 is written as 0."""
        if abs(self.rho_range[0]) > 0.0 or abs(self.r_min - self.h_r) > 1e-9 * self.h_r:
            raise ValueError("EAM.write_setfl: a setfl grid starts at 0: rho_min = 0 and r_min = h_r are needed (got %r, %r, h_r = %r)"
                             % (self.rho_range[0], self.r_min, self.h_r))
        S = self.n_species
        elements = list(elements or getattr(self, "elements", None) or ["X%d" % a for a in range(S)])
        header = list(header or getattr(self, "setfl_header", None) or [(0, 1.0, 0.0, "fcc")] * S)
        comments = list(comments or ["tabulated embedded-atom potential", "written by mdgrad_amd.interface.EAM.write_setfl", ""])
        pn, dn, en = (v.detach().cpu().double().numpy() for v in self._nodes())
        r = self.r_min + self.h_r * np.arange(self.n_r)
        f0 = dn[:, 0, 0] - dn[:, 0, 1] if self.density_at_origin is None else np.asarray(self.density_at_origin)
        out = [str(c) for c in comments[:3]] + ["%d %s" % (S, " ".join(elements))]
        out.append("%d %.17g %d %.17g %.17g" % (self.n_rho, self.h_rho, self.n_r + 1, self.h_r, self.cutoff))
        rows = lambda v: [" ".join("%.17g" % x for x in v[k:k + 5]) for k in range(0, len(v), 5)]
        for a in range(S):
            out.append("%d %.17g %.17g %s" % tuple(header[a]))
            out += rows(en[a, :, 0]) + rows(np.concatenate([[f0[a]], dn[a, :, 0]]))
        for p in range(S * (S + 1) // 2):
            out += rows(np.concatenate([[0.0], r * pn[p, :, 0]]))
        text = "\n".join(out) + "\n"
        if hasattr(path_or_file, "write"):
            path_or_file.write(text)
        else:
            with open(path_or_file, "w") as fh:
                fh.write(text)

    # -- the device tables the kernels read: the flat float32 image (pair, density, embed) of the nodes ---------------
    def _nodes(self):
        return self.pair_nodes, self.density_nodes, self.embed_nodes

    def _thetas(self):
        """The trainable node tensors, in the order of parameters()."""
        return tuple(getattr(self, name + "_nodes") for name in self.trainable)

    def _tables(self):
        """The nodes as the kernels read them: a device mirror (_DeviceMirror) rewritten when a node tensor changed, so that
        the captured steps carry no host value of a parameter."""
        return self._table_mirror.get()

    def prepare_pass(self):
        if self._hip_ok():
            self._tables()

    # (not the base's: the density pass keeps four floats per atom, sized by the positions, not per list slot)
    def _scratch(self, xyz):
        if self._work is None or self._work.device != xyz.device or self._work.shape[0] != xyz.shape[0]:
            self._work = torch.empty(xyz.shape[0], 4, dtype=torch.float32, device=xyz.device)
        if self._fx is None or self._fx.device != xyz.device:
            self._fx = torch.empty(ops.eam_table_fx_size(self._consts), dtype=torch.int64, device=xyz.device)
        return self._work

    # -- energy ----------------------------------------------------------------------------------------------------
    def _torch_energy(self, xyz, nodes=None):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in the
        three node tensors).  `nodes`: the three node tensors as the caller holds them (thermo.EAMEnergy casts them once for
        all its frames, so that their gradient is summed over the frames in the dtype of xyz)."""
        pn, dn, en = (v.to(xyz) for v in (nodes or self._nodes()))
        if self.pin_cutoff:                                   # the last node of phi and f is held at (0, 0): no gradient reaches it
            keep = torch.ones(self.n_r, 1, dtype=xyz.dtype, device=xyz.device)
            keep[-1] = 0.0
            pn, dn = pn * keep, dn * keep
        i, j, off = self._all_pairs(xyz, self.cutoff)
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        r = (xyz[i] - xyz[j] - off.matmul(cell)).pow(2).sum(-1).sqrt()
        ty = self.types.to(xyz.device).long()
        a, b = ty[i], ty[j]
        hi, lo = torch.maximum(a, b), torch.minimum(a, b)
        phi = _hermite(pn, hi * (hi + 1) // 2 + lo, r, self.r_min, self.h_r)
        to_i, to_j = _hermite(dn, b, r, self.r_min, self.h_r), _hermite(dn, a, r, self.r_min, self.h_r)
        rho = xyz.new_zeros(xyz.shape[0]).index_add(0, torch.cat([i, j]), torch.cat([to_i, to_j]))
        return phi.sum() + _hermite(en, ty, rho, self.rho_range[0], self.h_rho).sum()

    def _term(self, xyz):
        work = self._scratch(xyz)
        return ops.EAMTableTerm(self._ell, self.types, self._consts, self._tables(), work, self._fx, self._select)

    def force_vjp(self, xyz, w, want_theta=True, accum=None, into=None):
        """(F, d(w.F)/dx, [d(w.F)/dnodes for every trainable node tensor, shaped like it]) in one call of the term's kernels;
        `accum` (ops.ThetaAccum): the node part is added into its flat buffer at the parameters' offsets instead (None
        returned).  `into` = (F, dq) buffers of another Stack member: this term's force and d(w.F)/dx are added onto them."""
        ps = self._thetas()
        need = bool(want_theta) and len(ps) > 0
        o = self._term(xyz)._eval(xyz.detach(), w=w.detach(), energy=False, grad=True, into=into, scale=-1.0, want_theta=need)
        if not want_theta:
            return o["grad"], o["hw"], None
        if not ps:
            return o["grad"], o["hw"], ([] if accum is None else None)
        g = o["gtabw"]
        if accum is None:
            return o["grad"], o["hw"], [-g[a:b].reshape(p.shape) for p, (a, b) in zip(ps, self._select)]
        jobs = ops.GradJobs()
        for p, (a, b) in zip(ps, self._select):
            if accum.off.get(id(p)) is not None:
                jobs.axpy(accum.off[id(p)], g[a:b])
        jobs.run(accum, alpha=-1.0, accumulate=True)
        return o["grad"], o["hw"], None


class Tersoff(_ManyBodyTerm):
    """Tersoff bond-order potential for one species (Tersoff 1988 for silicon, 1989 for carbon; the LAMMPS convention): the
    strength of a bond depends on the bond's environment, so silicon, carbon, germanium and their amorphous or defective
    networks are described without a hard-wired tetrahedral angle.

        U       = 1/2 sum_i sum_{j != i} fc(r_ij) [ A exp(-lam1 r_ij) - b_ij B exp(-lam2 r_ij) ]
        b_ij    = (1 + (beta zeta_ij)^n)^(-1/(2n))
        zeta_ij = sum_{k != i, j} fc(r_ik) g(cos theta_jik) exp[ (lam3 (r_ij - r_ik))^m ]                 m = 1 or 3
        g(x)    = gamma (1 + c^2/d^2 - c^2/(d^2 + (h - x)^2))
        fc(r)   = 1 for r <= R - D;  1/2 - 1/2 sin(pi (r - R) / (2 D)) for R - D < r < R + D;  exactly 0 for r >= R + D

    A bond with zeta_ij = 0 (no third atom inside the cutoff) has b_ij = 1, and every derivative of b_ij there is defined
    as exactly 0.  A property of the model, whatever the implementation: for n < 1 (both published sets) db/dzeta diverges
    as zeta -> 0, so the second derivative of U diverges as a third atom crosses R + D next to a bond that had none; in
    condensed phases every bond keeps third atoms well inside the cutoff.

    The cutoff is R + D, an absolute length that no parameter moves.  The pair set, the minimum image and the
    (d2 < rc^2) & (d2 != 0) test are those of PairPotentials at that cutoff; the replicas of System.replicate never see
    each other.  The kernels apply the support of fc per pair, so a list searched with a skin is exact.

    `A`, `B` and `h` are one-element float32 parameters when trainable, otherwise buffers; everything else is a constant.
    Not covered: `index_tuple`, `ex_pairs` (both rejected), several species (one parameter set for all atoms, no mixing
    rules).  `silicon` and `carbon` carry the published constants (energies in eV, lengths in Angstrom).

    forward(xyz) is differentiable twice in xyz and once in (A, B, h) on the HIP kernels (ops.TersoffTerm,
    csrc/tersoff.hip: a bond pass that stores dU/dzeta per list slot, then a force pass that reads the neighbours' slots);
    force / force_vjp serve the analytic adjoint and HIP-graph replay, also while the parameters require grad.  float64 or
    host positions take the torch restatement `_torch_energy`, which keeps the published form of g."""

    _work_size = staticmethod(ops.tersoff_work_size)
    PUBLISHED = {"silicon": dict(A=1830.8, B=471.18, lam1=2.4799, lam2=1.7322, beta=1.1e-6, n=0.78734, c=1.0039e5, d=16.217,
                                 h=-0.59825, R=2.85, D=0.15),
                 "carbon": dict(A=1393.6, B=346.74, lam1=3.4879, lam2=2.2119, beta=1.5724e-7, n=0.72751, c=38049.0, d=4.3484,
                                h=-0.57058, R=1.95, D=0.15)}

    def __init__(self, system, A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3=0.0, m=3, gamma=1.0, trainable=True,
                 index_tuple=None, ex_pairs=None):
        super().__init__(system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("Tersoff: index_tuple and ex_pairs are not supported (one species, every pair)")
        self._consts = ops.tersoff_consts(A, B, lam1, lam2, beta, n, c, d, h, R, D, lam3, m, gamma)
        k = self._consts
        self.cutoff = float(k.R + k.D)
        cell = np.asarray(system.get_cell(), dtype=np.float64)
        cell = np.diag(cell) if cell.ndim == 1 else cell
        vol = abs(float(np.linalg.det(cell)))
        self._half_height = 0.5 * min(vol / float(np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3]))) for a in range(3))
        if self.cutoff > self._half_height:
            raise ValueError("Tersoff: R + D = %g exceeds half the shortest cell height (%g)" % (self.cutoff, self._half_height))
        for name, v in (("A", k.A), ("B", k.B), ("h", k.h)):
            t = torch.tensor([v], dtype=torch.float32, device=self.device)
            if trainable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self._ell = None
        self._theta_mirror = _DeviceMirror(self._thetas)
        self._work = None
        if torch.device(self.device).type == "cuda":
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._scratch()
            self._theta()

    @classmethod
    def silicon(cls, system, **kw):
        """Tersoff's silicon (1988, Si(C)): A = 1830.8 eV, B = 471.18 eV, lam1 = 2.4799, lam2 = 1.7322 / Angstrom,
        beta = 1.1e-6, n = 0.78734, c = 1.0039e5, d = 16.217, h = -0.59825, R = 2.85, D = 0.15 Angstrom."""
        return cls(system, **dict(cls.PUBLISHED["silicon"], **kw))

    @classmethod
    def carbon(cls, system, **kw):
        """Tersoff's carbon (1989): A = 1393.6 eV, B = 346.74 eV, lam1 = 3.4879, lam2 = 2.2119 / Angstrom, beta = 1.5724e-7,
        n = 0.72751, c = 38049, d = 4.3484, h = -0.57058, R = 1.95, D = 0.15 Angstrom."""
        return cls(system, **dict(cls.PUBLISHED["carbon"], **kw))

    # -- the device copy of (A, B, h) the kernels read (the lists are _ListTerm's, those of PairPotentials) --------
    def _thetas(self):
        return self.A, self.B, self.h

    def _theta(self):
        """(A, B, h) as the kernels read them: their device mirror (_DeviceMirror), so that the captured steps carry no
        host value of a parameter."""
        return self._theta_mirror.get()

    def prepare_pass(self):
        if self._hip_ok():
            self._theta()
            self._scratch()

    # -- energy ----------------------------------------------------------------------------------------------------
    def _torch_energy(self, xyz, params=None):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in
        A, B, h), with g in its published form: every pair as two directed bonds, grouped by centre into a padded [N, K]
        table, zeta as a sum over the [N, K, K] pairs of entries of one row.  params: (A, B, h) to take instead of the
        module's (a caller that evaluates many frames casts them once)."""
        k = self._consts
        A, B, h = (p.to(xyz).reshape(()) for p in (params if params is not None else (self.A, self.B, self.h)))
        i, j, off = self._all_pairs(xyz, self.cutoff)
        if i.numel() == 0:
            return xyz.sum() * 0.0
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        dv = xyz[i] - xyz[j] - off.matmul(cell)
        r = dv.pow(2).sum(-1).sqrt()
        taper = 0.5 - 0.5 * torch.sin((0.5 * math.pi / k.D) * (r - k.R))
        fc = torch.where(r <= k.R - k.D, torch.ones_like(r), torch.where(r < k.R + k.D, taper, torch.zeros_like(r)))
        N = xyz.shape[0]
        centre = torch.cat([i, j])
        u, r2, fc2 = torch.cat([-dv, dv]) / torch.cat([r, r])[:, None], torch.cat([r, r]), torch.cat([fc, fc])
        order = torch.argsort(centre, stable=True)
        centre, u, r2, fc2 = centre[order], u[order], r2[order], fc2[order]
        cnt = torch.bincount(centre, minlength=N)
        K = int(cnt.max())
        start = torch.cumsum(cnt, 0) - cnt
        slot = torch.arange(centre.numel(), device=xyz.device) - start[centre]
        U = xyz.new_zeros(N, K, 3).index_put((centre, slot), u)
        Rr = xyz.new_ones(N, K).index_put((centre, slot), r2)
        F = xyz.new_zeros(N, K).index_put((centre, slot), fc2)              # (padding: fc = 0, no bond and no third atom)
        cos = (U[:, :, None, :] * U[:, None, :, :]).sum(-1)                  # [N, j, k]
        g = k.gamma * (1.0 + k.c ** 2 / k.d ** 2 - k.c ** 2 / (k.d ** 2 + (h - cos) ** 2))
        E = torch.exp((k.lam3 * (Rr[:, :, None] - Rr[:, None, :])) ** int(k.m)) if k.lam3 != 0.0 else torch.ones_like(cos)
        other = 1.0 - torch.eye(K, dtype=xyz.dtype, device=xyz.device)
        zeta = (F[:, None, :] * g * E * other).sum(-1)
        bonded = zeta > 0                                     # zeta = 0: b = 1, and no 0 * inf in its derivatives
        z = torch.where(bonded, zeta, torch.ones_like(zeta))
        b = torch.where(bonded, (1.0 + (k.beta * z) ** k.n) ** (-0.5 / k.n), torch.ones_like(zeta))
        return 0.5 * (F * (A * torch.exp(-k.lam1 * Rr) - b * B * torch.exp(-k.lam2 * Rr))).sum()

    def _term(self, xyz):
        return ops.TersoffTerm(self._ell, self._consts, self._theta(), self._scratch())


class TersoffMulti(_ManyBodyTerm):
    """Tersoff bond-order potential for 1 <= S <= 4 species (Tersoff 1989, "Modeling solid-state chemistry: interatomic
    potentials for multicomponent systems"; the LAMMPS convention with lam3 = 0): SiC, SiGe and their alloys from the
    one-species sets and the paper's mixing rules.  Atom i has the species t_i = `types`[i]; with a = t_i, b = t_j, c = t_k

        U       = 1/2 sum_i sum_{j != i} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]
        b_ij    = (1 + (beta_a zeta_ij)^n_a)^(-1/(2 n_a)),        zeta_ij = 0: b_ij = 1 with every derivative 0 (as in Tersoff)
        zeta_ij = sum_{k != i, j} fc_ac(r_ik) g_a(cos theta_jik)
        g_a(x)  = gamma_a (1 + c_a^2/d_a^2 - c_a^2/(d_a^2 + (h_a - x)^2))
        fc_ab   = 1 for r <= R_ab - D_ab;  1/2 - 1/2 sin(pi (r - R_ab) / (2 D_ab)) inside;  exactly 0 for r >= R_ab + D_ab

    The pair constants (A, B, lam1, lam2, R, D) are [S, S] tables, row = the species of the centre of the directed bond,
    column = the species of its end; (beta, n, c, d, h, gamma) belong to the centre's species.  chi is folded into B_ab
    (B[a, b], a != b, is where chi lives), omega = 1.

    TersoffMulti(system, types, species, chi) takes S one-species sets (dicts with the keys of Tersoff.PUBLISHED and an
    optional gamma) and mixes them (`mix`): A_ab = sqrt(A_a A_b), B_ab = chi_ab sqrt(B_a B_b), lam_ab = (lam_a + lam_b) / 2
    for both exponents, and, with the paper's inner and outer radii R - D and R + D, the geometric means of each, from which
    R_ab and D_ab follow.  chi is [S, S], symmetric with unit diagonal (default: ones).  `from_tables` takes the tables
    themselves, for sets that do not follow the mixing rules.  `silicon_carbide` (types: 0 = Si, 1 = C; chi = 0.9776) and
    `silicon_germanium` (0 = Si, 1 = Ge; chi = 1.00061) carry the published constants; PUBLISHED adds germanium to Tersoff's.
    `types` holds one entry per atom of a replica, in [0, S); every replica of System.replicate has the same species.

    `A` [S, S], `B` [S, S] and `h` [S] are float32 parameters when trainable, otherwise buffers; everything else is constant.
    A[a, b] and A[b, a] (likewise B) are separate entries that the constructors fill equally: a fit that wants them tied
    ties their gradients (sums the two and writes the sum to both).

    The cutoff is max_ab (R_ab + D_ab), an absolute length that no parameter moves; the pair set, the minimum image and the
    test (d2 < rc^2) & (d2 != 0) are those of PairPotentials at that cutoff, and the kernels apply the support of fc_ab per
    list entry with the entry's own R_ab + D_ab, so a list searched with a skin is exact.  Not covered (ValueError where it
    can be asked for): lam3 != 0 (or m != 3 in a species set), angular constants that depend on the whole triplet,
    `index_tuple`, `ex_pairs`, S > 4, the pressure of the term.

    forward(xyz) is differentiable twice in xyz and once in (A, B, h) on the HIP kernels (ops.TersoffMultiTerm,
    csrc/tersoff_multi.hip: the two passes of csrc/tersoff.hip with every constant looked up by species in a device table);
    force / force_vjp serve the analytic adjoint and HIP-graph replay, also while the parameters require grad.  float64 or
    host positions take the torch restatement `_torch_energy`, which keeps the published form of g.  A Stack holding the
    term stays off the fused trajectory kernels."""

    _work_size = staticmethod(ops.tersoff_multi_work_size)
    MAX_SPECIES = ops.TERSOFF_MULTI_MAX_SPECIES
    PUBLISHED = dict(Tersoff.PUBLISHED,
                     germanium=dict(A=1769.0, B=419.23, lam1=2.4451, lam2=1.7047, beta=9.0166e-7, n=0.75627, c=1.0643e5,
                                    d=15.652, h=-0.43884, R=2.95, D=0.15))
    CHI = {"SiC": 0.9776, "SiGe": 1.00061}

    def __init__(self, system, types, species, chi=None, trainable=True, index_tuple=None, ex_pairs=None):
        pair, centre = self.mix(species, chi)
        self._setup(system, types, pair, centre, trainable, index_tuple, ex_pairs)

    @classmethod
    def from_tables(cls, system, types, pair, centre, trainable=True, index_tuple=None, ex_pairs=None):
        """The term from its tables: pair = dict of [S, S] arrays A, B, lam1, lam2, R, D (row = centre species, column = end
        species), centre = dict of [S] arrays beta, n, c, d, h, gamma."""
        self = cls.__new__(cls)
        self._setup(system, types, pair, centre, trainable, index_tuple, ex_pairs)
        return self

    @classmethod
    def silicon_carbide(cls, system, types, **kw):
        """Tersoff's SiC (1989): the silicon and carbon sets, chi_SiC = 0.9776.  types: 0 = Si, 1 = C."""
        chi = [[1.0, cls.CHI["SiC"]], [cls.CHI["SiC"], 1.0]]
        return cls(system, types, [cls.PUBLISHED["silicon"], cls.PUBLISHED["carbon"]], chi=chi, **kw)

    @classmethod
    def silicon_germanium(cls, system, types, **kw):
        """Tersoff's SiGe (1989): the silicon and germanium sets, chi_SiGe = 1.00061.  types: 0 = Si, 1 = Ge."""
        chi = [[1.0, cls.CHI["SiGe"]], [cls.CHI["SiGe"], 1.0]]
        return cls(system, types, [cls.PUBLISHED["silicon"], cls.PUBLISHED["germanium"]], chi=chi, **kw)

    @classmethod
    def mix(cls, species, chi=None):
        """(pair, centre) tables of S one-species sets under Tersoff's mixing rules (class docstring), in float64."""
        species = list(species)
        S = len(species)
        if not 1 <= S <= cls.MAX_SPECIES:
            raise ValueError("TersoffMulti: species must hold 1 to %d parameter sets (got %d)" % (cls.MAX_SPECIES, S))
        for a, p in enumerate(species):
            if float(p.get("lam3", 0.0)) != 0.0 or int(p.get("m", 3)) != 3:
                raise ValueError("TersoffMulti: species[%d] has lam3 = %r, m = %r; only lam3 = 0 (m = 3) is covered"
                                 % (a, p.get("lam3", 0.0), p.get("m", 3)))
            missing = [k for k in ("A", "B", "lam1", "lam2", "beta", "n", "c", "d", "h", "R", "D") if k not in p]
            if missing:
                raise ValueError("TersoffMulti: species[%d] lacks %s" % (a, ", ".join(missing)))
        X = np.ones((S, S)) if chi is None else np.asarray(chi, dtype=np.float64)
        if X.shape != (S, S) or not np.array_equal(X, X.T) or not (np.diag(X) == 1.0).all():
            raise ValueError("TersoffMulti: chi must be a symmetric [%d, %d] matrix with unit diagonal (got %r)"
                             % (S, S, X.tolist()))
        col = lambda k: np.array([float(p[k]) for p in species], dtype=np.float64)
        geo = lambda v: np.sqrt(np.outer(v, v))
        mean = lambda v: 0.5 * (v[:, None] + v[None, :])
        rin, rout = geo(col("R") - col("D")), geo(col("R") + col("D"))
        pair = dict(A=geo(col("A")), B=X * geo(col("B")), lam1=mean(col("lam1")), lam2=mean(col("lam2")),
                    R=0.5 * (rin + rout), D=0.5 * (rout - rin))
        centre = {k: col(k) for k in ("beta", "n", "c", "d", "h")}
        centre["gamma"] = np.array([float(p.get("gamma", 1.0)) for p in species], dtype=np.float64)
        return pair, centre

    def _setup(self, system, types, pair, centre, trainable, index_tuple, ex_pairs):
        _ListTerm.__init__(self, system)
        if index_tuple is not None or ex_pairs is not None:
            raise ValueError("TersoffMulti: index_tuple and ex_pairs are not supported (every pair interacts)")
        centre = dict(centre)
        S = int(np.asarray(centre["h"]).reshape(-1).shape[0])
        centre.setdefault("gamma", np.ones(S))
        if S > self.MAX_SPECIES:
            raise ValueError("TersoffMulti: S = %d species; at most %d are supported" % (S, self.MAX_SPECIES))
        self._image = ops.tersoff_multi_tables(pair, centre)                # (validates every entry)
        self.n_species = S
        self._pair = {k: np.asarray(pair[k], dtype=np.float64).reshape(S, S) for k in ops.TERSOFF_MULTI_PAIR}
        self._centre = {k: np.asarray(centre[k], dtype=np.float64).reshape(S) for k in ops.TERSOFF_MULTI_CENTRE}
        ty = np.asarray(torch.as_tensor(types).detach().cpu().numpy()).reshape(-1)
        if ty.shape[0] != self._group:
            raise ValueError("TersoffMulti: types must hold one entry per atom of a replica (%d), got %d" % (self._group, ty.shape[0]))
        if not np.issubdtype(ty.dtype, np.integer) or ty.min() < 0 or ty.max() >= S:
            raise ValueError("TersoffMulti: types must be integers in [0, %d)" % S)
        self.cutoff = float((self._pair["R"] + self._pair["D"]).max())
        cell = np.asarray(system.get_cell(), dtype=np.float64)
        cell = np.diag(cell) if cell.ndim == 1 else cell
        vol = abs(float(np.linalg.det(cell)))
        self._half_height = 0.5 * min(vol / float(np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3]))) for a in range(3))
        if self.cutoff > self._half_height:
            raise ValueError("TersoffMulti: max (R + D) = %g exceeds half the shortest cell height (%g)"
                             % (self.cutoff, self._half_height))
        for name in ("A", "B", "h"):
            t = torch.tensor((self._pair if name != "h" else self._centre)[name], dtype=torch.float32, device=self.device)
            if trainable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)
        self.index_tuple, self.ex_pairs, self._mask = None, None, None
        self._n_rep = system.get_number_of_atoms() // self._group
        self.types = torch.as_tensor(np.tile(ty.astype(np.int32), self._n_rep), device=self.device)   # one entry per atom
        self._ell = None
        self._template = torch.as_tensor(self._image, device=self.device)
        self._table_mirror = _DeviceMirror(self._thetas, pack=self._pack_tables, numel=int(self._image.shape[0]))
        self._work = None
        if torch.device(self.device).type == "cuda":
            self._reset_topology(torch.Tensor(system.get_positions()).to(system.device))
            self._scratch()
            self._tables()

    # -- the device table the kernels read: the constants plus the current (A, B, h) ------------------------------
    def _thetas(self):
        return self.A, self.B, self.h

    def _pack_tables(self, ps, out=None):
        """The table image (ops.tersoff_multi_tables) with the current A, B, h in their columns, by device ops only."""
        S = self.n_species
        A, B, h = (p.detach().to(torch.float32) for p in ps)
        out = self._template.to(A.device).clone() if out is None else out.copy_(self._template)
        pair, centre = out[:8 * S * S].view(S * S, 8), out[8 * S * S:].view(S, 8)
        pair[:, 0].copy_(A.reshape(-1))
        pair[:, 1].copy_(B.reshape(-1))
        centre[:, 0].copy_(h.reshape(-1))
        return out

    def _tables(self):
        """The derived constants as the kernels read them: a device mirror (_DeviceMirror) rewritten when A, B or h changed,
        so that the captured steps carry no host value of a parameter."""
        return self._table_mirror.get()

    def prepare_pass(self):
        if self._hip_ok():
            self._tables()
            self._scratch()

    # -- energy ----------------------------------------------------------------------------------------------------
    def _torch_energy(self, xyz, params=None):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and in
        A, B, h), with g in its published form: every pair as two directed bonds with the constants of (centre species, end
        species), grouped by centre into a padded [N, K] table, zeta as a sum over the [N, K, K] pairs of entries of a row.
        params: (A, B, h) to take instead of the module's (a caller that evaluates many frames casts them once)."""
        const = lambda v: torch.as_tensor(v, dtype=xyz.dtype, device=xyz.device)
        A, B, h = (p.to(xyz) for p in (params if params is not None else (self.A, self.B, self.h)))
        i, j, off = self._all_pairs(xyz, self.cutoff)
        if i.numel() == 0:
            return xyz.sum() * 0.0
        cell = self.cell.detach().to(xyz)
        cell = torch.diag(cell) if cell.dim() == 1 else cell
        dv = xyz[i] - xyz[j] - off.matmul(cell)
        r = dv.pow(2).sum(-1).sqrt()
        ty = self.types.to(xyz.device).long()
        N = xyz.shape[0]
        centre, end = torch.cat([i, j]), torch.cat([j, i])
        u, r2 = torch.cat([-dv, dv]) / torch.cat([r, r])[:, None], torch.cat([r, r])
        ta, tb = ty[centre], ty[end]
        Rab, Dab = const(self._pair["R"])[ta, tb], const(self._pair["D"])[ta, tb]
        taper = 0.5 - 0.5 * torch.sin((0.5 * math.pi / Dab) * (r2 - Rab))
        fc2 = torch.where(r2 <= Rab - Dab, torch.ones_like(r2), torch.where(r2 < Rab + Dab, taper, torch.zeros_like(r2)))
        vR = A[ta, tb] * torch.exp(-const(self._pair["lam1"])[ta, tb] * r2)
        vA = B[ta, tb] * torch.exp(-const(self._pair["lam2"])[ta, tb] * r2)
        order = torch.argsort(centre, stable=True)
        centre, u, fc2, vR, vA = centre[order], u[order], fc2[order], vR[order], vA[order]
        cnt = torch.bincount(centre, minlength=N)
        K = int(cnt.max())
        start = torch.cumsum(cnt, 0) - cnt
        slot = torch.arange(centre.numel(), device=xyz.device) - start[centre]
        U = xyz.new_zeros(N, K, 3).index_put((centre, slot), u)
        F = xyz.new_zeros(N, K).index_put((centre, slot), fc2)              # (padding: fc = 0, no bond and no third atom)
        VR = xyz.new_zeros(N, K).index_put((centre, slot), vR)
        VA = xyz.new_zeros(N, K).index_put((centre, slot), vA)
        cos = (U[:, :, None, :] * U[:, None, :, :]).sum(-1)                  # [N, j, k]
        per = lambda name: const(self._centre[name])[ty][:, None, None]      # the centre's constants
        c2, d2 = per("c") ** 2, per("d") ** 2
        g = per("gamma") * (1.0 + c2 / d2 - c2 / (d2 + (h[ty][:, None, None] - cos) ** 2))
        other = 1.0 - torch.eye(K, dtype=xyz.dtype, device=xyz.device)
        zeta = (F[:, None, :] * g * other).sum(-1)
        bonded = zeta > 0                                     # zeta = 0: b = 1, and no 0 * inf in its derivatives
        z = torch.where(bonded, zeta, torch.ones_like(zeta))
        beta, n = per("beta")[:, :, 0], per("n")[:, :, 0]
        b = torch.where(bonded, (1.0 + (beta * z) ** n) ** (-0.5 / n), torch.ones_like(zeta))
        return 0.5 * (F * (VR - b * VA)).sum()

    def _term(self, xyz):
        return ops.TersoffMultiTerm(self._ell, self.types, self.n_species, self._tables(), self._scratch())


class _EwaldMember(_ChargeTerm, _StaticTerm, torch.nn.Module):
    """Common part of EwaldReciprocal / EwaldExclusions, the members of an Ewald sum built on its real-space term `real`:
    what they refuse of it, the fields they adopt from it -- alpha, conversion, types, the charge slots, the replica layout
    and the `charges` tensor itself (the same Parameter object when trainable) --, the lengths of the diagonal cell, and the
    static table their kernels read.  `name` is the class name the messages carry; `why` = what a shifted, an undamped and
    a self-energy-free `real` would do to this member."""

    def __init__(self, system, real, name, why):
        super().__init__()
        if not isinstance(real, CoulombPotentials):
            raise ValueError("%s: `real` must be the CoulombPotentials carrying the real-space sum, got %s"
                             % (name, type(real).__name__))
        if real.shift != "none":
            raise ValueError("%s: the real-space term has shift=%r; the Ewald real-space sum is the plain "
                             "erfc(alpha r) / r (shift=\"none\")%s" % (name, real.shift, why[0]))
        if real.alpha == 0.0:
            raise ValueError("%s: the real-space term has alpha = 0 (the bare Coulomb sum): there is no splitting "
                             "and %s" % (name, why[1]))
        if not real.self_energy:
            raise ValueError("%s: the real-space term has self_energy=False; %s" % (name, why[2]))
        if getattr(system, "dim", 3) != 3:
            raise ValueError("%s: system.dim = %r; the sum is over a three-dimensional lattice" % (name, system.dim))
        full = torch.Tensor(system.get_cell())
        if full.dim() == 2 and bool((full - torch.diag(torch.diag(full)) != 0).any()):
            raise ValueError("%s: the cell must be diagonal (triclinic cells are not supported)" % name)
        self.system = system
        self.device = system.device
        self.cell = (full.diag() if full.dim() == 2 else full).to(self.device)
        self._real = (real,)                                     # (a tuple: not registered as a sub-module a second time)
        self.alpha, self.conversion, self.types = real.alpha, real.conversion, real.types
        if isinstance(real.charges, torch.nn.Parameter):
            self.charges = real.charges
        else:
            self.register_buffer("charges", real.charges)
        self._slot, self.n_slots = real._slot, real.n_slots
        self._group, self._n_rep = real._group, real._n_rep
        self._lengths = self.cell.detach().cpu().to(torch.float64).numpy()    # the float32 lengths the kernels see

    def table(self):
        return self._table

    def _hip_ok(self, xyz=None):
        return super()._hip_ok(xyz) and torch.device(self.device).type == "cuda"

    def _q_atom(self):
        return self._real[0]._q_atom()

    def _term(self, xyz=None):
        return self._ops_term(self._table, self._q_atom(), self._slot, self.n_slots)


class EwaldReciprocal(_EwaldMember):
    """The reciprocal-space part of the Ewald sum for the point charges of a CoulombPotentials (no counterpart in the
    reference).  With `real` = CoulombPotentials(system, charges, cutoff, alpha, shift="none", self_energy=True) the two
    terms together are the energy of the periodic system, independent of alpha up to the truncation of both sums:

        k(n)   = 2 pi (nx / Lx, ny / Ly, nz / Lz),  integer n != 0,  |k| <= k_cutoff
        rho(k) = sum_j q_j exp(i k.x_j)
        c(k)   = (4 pi / V) exp(-k^2 / (4 alpha^2)) / k^2                                  (host, float64 -> float32 table)
        U_rec  = conversion * [ sum_{k in half space} c(k) |rho(k)|^2  -  pi (sum_j q_j)^2 / (2 V alpha^2) ]

    on a diagonal cell of lengths L, V = Lx Ly Lz.  k and -k contribute equally, so only the half space of
    observable.sk_vectors is summed (nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and nz > 0); the second term is the
    neutralising background, zero for a neutral cell.  The self term -alpha / sqrt(pi) sum q_i^2 is carried by `real`
    (its self_s).  Every replica of System.replicate(R) has its own modes.

    alpha, conversion, types and the `charges` tensor itself are taken from `real`: the same Parameter object when
    trainable, so a Stack de-duplicates it and both terms add into the same gradient slot.  k_cutoff=None takes
    2 alpha sqrt(-ln accuracy); `ewald` chooses alpha from the real-space cutoff the same way.  Not supported (ValueError):
    a shifted or undamped `real`, one without self energy, index_tuple on `real`, triclinic cells, 2-D systems.  ex_pairs on
    `real` need the third member of the sum: excluded pairs keep their reciprocal interaction erf(alpha r) / r, which
    EwaldExclusions(system, real) removes -- pass it as `exclusions=` (or build all three with ewald(..., ex_pairs=));
    without it such a `real` is refused.

    forward(xyz) is differentiable twice in xyz and once in charges on the HIP kernels (ops.EwaldTerm, csrc/ewald.hip);
    force / force_vjp serve the analytic adjoint and HIP-graph replay like CoulombPotentials'.  float64 or host positions
    take the torch restatement `_torch_energy`.  A Stack holding the term stays off the fused trajectory kernels."""

    _ops_term = ops.EwaldTerm

    def __init__(self, system, real, k_cutoff=None, accuracy=1e-5, exclusions=None):
        super().__init__(system, real, "EwaldReciprocal",
                         (", a shifted one would be counted wrongly", "c(k) is undefined",
                          "the self term -alpha/sqrt(pi) sum q_i^2 of the Ewald sum would be missing"))
        if exclusions is not None and (not isinstance(exclusions, EwaldExclusions) or exclusions._real[0] is not real):
            raise ValueError("EwaldReciprocal: `exclusions` must be the EwaldExclusions built on the same real-space term")
        if real.index_tuple is not None or (real.ex_pairs is not None and exclusions is None):
            raise ValueError("EwaldReciprocal: the real-space term has index_tuple / ex_pairs; the erf correction that removes "
                             "excluded pairs from the reciprocal sum is not implemented for index_tuple, and for ex_pairs it is "
                             "a term of its own: pass exclusions=EwaldExclusions(system, real), or build the three members "
                             "with ewald(..., ex_pairs=)")
        if not 0.0 < float(accuracy) < 1.0:
            raise ValueError("EwaldReciprocal: accuracy must lie in (0, 1), got %r" % (accuracy,))
        self.accuracy = float(accuracy)
        self.k_cutoff = float(k_cutoff) if k_cutoff is not None else 2.0 * self.alpha * math.sqrt(-math.log(self.accuracy))
        self._table = ops.EwaldTable(_lib.make_cell(system.get_cell()), self._lengths, self.alpha, self.k_cutoff,
                                     self.conversion, self._n_rep, self._group, self.device)
        self.n_vectors = self._table.n_vecs

    def _torch_energy(self, xyz):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and
        charges)."""
        t = self._table
        k = (2.0 * math.pi * t.n_host.to(torch.float64) / torch.as_tensor(t.lengths)).to(xyz)          # [M, 3]
        cf = t.coef_host.to(xyz)
        q = self._real[0]._expand(self.charges.to(xyz))
        ph = xyz.matmul(k.t())
        A = (q[:, None] * torch.cos(ph)).reshape(t.n_rep, t.n_atoms, -1).sum(1)
        B = (q[:, None] * torch.sin(ph)).reshape(t.n_rep, t.n_atoms, -1).sum(1)
        Q = q.reshape(t.n_rep, t.n_atoms).sum(1)
        return self.conversion * ((cf * (A * A + B * B)).sum() - math.pi * Q.pow(2).sum() / (2.0 * t.volume * t.alpha ** 2))


class EwaldExclusions(_EwaldMember):
    """The third member of the Ewald sum for molecules: the erf correction for the excluded and scaled pairs of a
    CoulombPotentials (no counterpart in the reference).  The real-space term honours `ex_pairs` through its mask; the
    reciprocal sum runs over all charges and cannot leave a pair out.  With `real` = CoulombPotentials(system, charges, cutoff,
    alpha > 0, shift="none", self_energy=True, ex_pairs=P), E1(r) = erf(alpha r), G(r) = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2)
    and a scale s_p per pair p = (i, j) of P:

        chi(r)   = (s - E1) / r
        chi'(r)  = -(s - E1) / r^2 - G / r
        chi''(r) = 2 (s - E1) / r^3 + 2 G / r^2 + 2 alpha^2 G
        U_excl   = conversion * sum_{p in P, every replica} q_i q_j chi_{s_p}(r_ij)

    r_ij is the length of x_i - x_j re-imaged on the diagonal cell the way BondPotentials / DihedralPotentials re-image a
    bond vector (topology.get_offsets: non-strict >= on the +L/2 side, piecewise constant, no derivative), so wrapped and
    unwrapped frames give the same value.  s = 0 (the default): the pair is fully excluded -- the mask removes erfc/r, this
    term the erf/r of the reciprocal sum, together 1/r is gone; s = 0.5: the OPLS / AMBER 1-4 scaling; s = 1: chi equals the
    real-space psi of shift="none", the pair is back to its full interaction.  `scale`: None, one float, or one float per row
    of real.ex_pairs, each in [0, 1].  No self term and no background term here: both stay where they are.

    A coincident pair (r == 0: Drude particles, virtual sites) contributes the limits of the erf part -- energy
    -q_i q_j 2 alpha / sqrt(pi), zero gradient, (H w)_i = q_i q_j (4 alpha^3 / (3 sqrt(pi))) (w_i - w_j) -- and its s / r
    part is dropped, like the pair kernels' d2 != 0 test.

    The pairs, alpha, conversion, types and the `charges` tensor itself are taken from `real`: the same Parameter object
    when trainable, so a Stack de-duplicates it and all three terms add into one gradient slot.  ValueError: `real` without
    ex_pairs, shifted, undamped, without self energy or with index_tuple; a pair with i == j, an index outside the replica,
    a pair listed twice in either orientation (the mask is idempotent, this sum would subtract such a pair twice); a
    triclinic cell, system.dim != 3, a scale outside [0, 1].

    forward(xyz) is differentiable twice in xyz and once in charges on the HIP kernel (ops.EwaldExclTerm,
    csrc/ewald_excl.hip: below alpha r = 1 the erf part comes from the power series of erf(x)/x, whose closed form cancels
    in float32); force / force_vjp serve the analytic adjoint and HIP-graph replay like CoulombPotentials'.  float64 or host
    positions take the torch restatement `_torch_energy`.  A Stack holding the term stays off the fused trajectory
    kernels."""

    _ops_term = ops.EwaldExclTerm

    def __init__(self, system, real, scale=None):
        super().__init__(system, real, "EwaldExclusions",
                         ("", "nothing to correct", "it is not the real-space member of an Ewald sum"))
        if real.ex_pairs is None:
            raise ValueError("EwaldExclusions: the real-space term has no ex_pairs: there is nothing to correct")
        if real.index_tuple is not None:
            raise ValueError("EwaldExclusions: the real-space term has index_tuple; the Ewald sum runs over all charges")
        try:
            self._table = ops.EwaldExclTable(real.ex_pairs, scale, self._group, self._n_rep, self._lengths, self.alpha,
                                             self.conversion, self.device)
        except ValueError as e:
            raise ValueError("EwaldExclusions: " + str(e).replace("mdgrad_amd: ", "")) from None
        self.pairs, self.scale = self._table.pairs, self._table.scale

    def _torch_energy(self, xyz):
        """The same energy in torch ops, in the dtype and on the device of xyz (differentiable by autograd in xyz and
        charges)."""
        t = self._table
        rep = (torch.arange(t.n_rep) * t.n_atoms)[:, None]
        i = (t.pairs[:, 0][None, :] + rep).reshape(-1).to(xyz.device)
        j = (t.pairs[:, 1][None, :] + rep).reshape(-1).to(xyz.device)
        s = t.scale.repeat(t.n_rep).to(xyz)
        cell = self.cell.detach().to(xyz)
        d = xyz[i] - xyz[j]
        d = d + get_offsets(d.detach(), cell, xyz.device).to(xyz) * cell
        d2 = d.pow(2).sum(-1)
        apart = d2 != 0
        r = torch.where(apart, d2, torch.ones_like(d2)).sqrt()
        g0 = 2.0 * t.alpha / math.sqrt(math.pi)
        chi = torch.where(apart, (s - torch.erf(t.alpha * r)) / r, torch.full_like(r, -g0))
        q = self._real[0]._expand(self.charges.to(xyz))
        return self.conversion * (q[i] * q[j] * chi).sum()


def ewald(system, charges, cutoff, accuracy=1e-5, k_cutoff=None, ex_pairs=None, scale=None, **kw):
    """The members of an Ewald sum with both truncation errors near `accuracy` (relative): alpha = sqrt(-ln accuracy) /
    cutoff, so that erfc(alpha cutoff) ~ accuracy, and k_cutoff = 2 alpha sqrt(-ln accuracy).  Returns
    {"coulomb_real": CoulombPotentials(system, charges, cutoff, alpha=alpha, shift="none", **kw),
     "coulomb_recip": EwaldReciprocal(system, real, k_cutoff, accuracy)}, ready for Stack({..., **ewald(...)}); **kw: types,
    conversion, trainable of CoulombPotentials.  With `ex_pairs` ([P, 2] pairs of one replica whose charges do not interact,
    or interact scaled by `scale`: None, one float or one per pair) the real-space term masks them and a third member
    "coulomb_excl": EwaldExclusions(system, real, scale) removes them from the reciprocal sum."""
    if not 0.0 < float(accuracy) < 1.0:
        raise ValueError("ewald: accuracy must lie in (0, 1), got %r" % (accuracy,))
    alpha = math.sqrt(-math.log(float(accuracy))) / float(cutoff)
    if ex_pairs is None:
        if scale is not None:
            raise ValueError("ewald: scale given without ex_pairs")
        real = CoulombPotentials(system, charges, cutoff, alpha=alpha, shift="none", self_energy=True, **kw)
        return {"coulomb_real": real, "coulomb_recip": EwaldReciprocal(system, real, k_cutoff=k_cutoff, accuracy=accuracy)}
    real = CoulombPotentials(system, charges, cutoff, alpha=alpha, shift="none", self_energy=True, ex_pairs=ex_pairs, **kw)
    excl = EwaldExclusions(system, real, scale=scale)
    return {"coulomb_real": real,
            "coulomb_recip": EwaldReciprocal(system, real, k_cutoff=k_cutoff, accuracy=accuracy, exclusions=excl),
            "coulomb_excl": excl}


class Stack(torch.nn.Module):
    """torchmd/interface.py:364-403."""

    def __init__(self, model_dict, mode='sum'):
        super().__init__()
        self.models = ModuleDict(model_dict)

    # analytic-adjoint protocol: available when every member provides it
    def supports_force_vjp(self):
        return all(getattr(m, "supports_force_vjp", lambda: False)() for m in self.models.values())

    def prepare_pass(self):
        for m in self.models.values():
            getattr(m, "prepare_pass", lambda: None)()

    def _ordered(self):
        """Members that can add their result onto an existing buffer inside their own launch (pair terms) go last."""
        ms = list(self.models.values())
        return [m for m in ms if not getattr(m, "accepts_into", False)] + [m for m in ms if getattr(m, "accepts_into", False)]

    def force(self, x):
        out = None
        for m in self._ordered():
            if out is not None and getattr(m, "accepts_into", False):
                out = m.force(x, into=out)
                continue
            f = m.force(x)
            out = f if out is None else out + f
        return out

    accepts_accum = True

    def force_vjp(self, x, w, want_theta=True, accum=None):
        """Sum over members; the parameter gradients come back as a list aligned with self.parameters()
        (None when want_theta is False: the first augmented evaluation of an adjoint interval discards
        them, sovlers.py:141-143) -- or are added into `accum` (ops.ThetaAccum) by the members themselves."""
        F = dq = None
        by_id = {}
        for m in self._ordered():
            kw = {}
            if F is not None and getattr(m, "accepts_into", False):
                kw["into"] = (F, dq)                                   # this member's launch adds onto the running sums
            if accum is not None and want_theta:
                if getattr(m, "accepts_accum", False):
                    f, g, gth = m.force_vjp(x, w, want_theta=True, accum=accum, **kw)
                else:
                    f, g, gth = m.force_vjp(x, w, want_theta=True, **kw)
                if gth is not None:
                    _accumulate_list(accum, m.parameters(), gth)
            else:
                f, g, gth = m.force_vjp(x, w, want_theta=want_theta, **kw)
            if "into" in kw:
                F, dq = f, g
            else:
                F = f if F is None else F + f
                dq = g if dq is None else dq + g
            if want_theta and accum is None:
                for p, gp in zip(m.parameters(), gth):
                    by_id[id(p)] = gp if id(p) not in by_id else by_id[id(p)] + gp
        if not want_theta or accum is not None:
            return F, dq, None
        return F, dq, [by_id[id(p)] if id(p) in by_id else torch.zeros_like(p) for p in self.parameters()]

    def _reset_topology(self, x):
        self._topo_stamp = object()
        shared = {}                          # one neighbour search per distinct (cutoff, selection, grouping)
        # (members that own a stored Verlet list go first, so that pair terms with the same cutoff can use it)
        keys = sorted(self.models.keys(), key=lambda k: 0 if isinstance(self.models[k], GNNPotentials) else 1)
        for key in keys:
            m = self.models[key]
            if isinstance(m, GeneralInteraction):
                m._reset_topology(x, _cache=shared)
            else:
                m._reset_topology(x)

    def supports_static_topology(self):
        return all(getattr(m, "supports_static_topology", lambda: False)() for m in self.models.values())

    def set_static_topology(self, on=True):
        for m in self.models.values():
            m.set_static_topology(on)

    def static_overflow(self):
        return any([m.static_overflow() for m in self.models.values()])     # (no short-circuit: all get enlarged)

    def static_version(self):
        return tuple(m.static_version() for m in self.models.values())

    def forward(self, x):
        result = None
        for key in self.models.keys():
            new_result = self.models[key](x).sum().reshape(-1)
            result = new_result if result is None else result + new_result
        return result
