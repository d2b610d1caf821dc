"""torchmd/thermo.py:57-66 (`Temperature`) and `Pressure`: the reference's sketch (torchmd/thermo.py:17-54) uses undefined
names and does not run, so the definition is this module's -- kinetic part plus pair virial over (d V), see `Pressure`.
`PotentialEnergy`, the pair energy of every frame of a trajectory in one call, has no counterpart in the reference: the
per-frame thermodynamic observable and the energy side of trajectory reweighting (mdgrad_amd/reweight.py); `TabulatedEnergy`
is the same for learned pair modules (pairMLP ...), whose energy it tabulates, `StillingerWeberEnergy` for the one-species
three-body model (silicon, mW water), `EAMEnergy` for the embedded-atom models of the metals (Sutton-Chen and tabulated) and
`TersoffEnergy` for the bond-order models (Tersoff, TersoffMulti)."""
import torch

from . import ops
from .observable import Observable

_FORMS = "LJFamily / LennardJones / LennardJones69, ExcludedVolume, ModifiedMorse, Buck, Yukawa"


def _frames(self, x, name):
    """x [..., k N, 3] as frames [F, N, 3] and the shape of the per-frame result (the method `_frames` of the per-frame
    observables below)."""
    n = x.shape[-2] if x.dim() >= 2 else 0
    if n == 0 or x.shape[-1] != 3 or n % self.natoms:
        raise ValueError("%s: %s must be [..., k * %d, 3], got %s" % (type(self).__name__, name, self.natoms, tuple(x.shape)))
    k = n // self.natoms                             # replica-stacked state [..., k N, 3]: one value per replica
    lead = tuple(x.shape[:-2]) + ((k,) if k > 1 else ())
    return x.reshape(-1, self.natoms, 3), lead


class Temperature(Observable):
    def __init__(self, system):
        super().__init__(system)
        self.dof = getattr(system, "dim", 3) * self.natoms              # N_dof = N * dim (thermo.py:63)
        self.mass = torch.Tensor(system.get_masses()).to(self.device)[:self.natoms].contiguous()

    def forward(self, velocities):
        """Instantaneous kinetic temperature (energy units), sum(m v^2) / N_dof: a scalar for one frame [N, 3] like
        the reference, one value per frame for a trajectory [T, N, 3] or a batched one [R, T, N, 3] (one fused launch,
        csrc/observe.hip)."""
        lead = velocities.shape[:-2]                      # any leading shape: [], [T], [R, T] (batched fused trajectories)
        n = velocities.shape[-2]
        if n % self.natoms:
            raise ValueError("Temperature: %d atoms per frame is not a multiple of the system's %d" % (n, self.natoms))
        k = n // self.natoms                              # replica-stacked state [..., R N, 3]: one value per replica
        v = velocities.reshape(-1, self.natoms, 3)
        out = ops.TemperatureFn.apply(v, self.mass, self.dof)
        return out.reshape(*lead, k) if k > 1 else out.reshape(lead)


class Pressure(Observable):
    """Instantaneous pressure of pair-potential models, per frame:

        K = sum_i m_i |v_i|^2        W = -sum_terms sum_pairs r phi'(r)        P = (K + W) / (d V)

    with d = system.dim and V the volume of one replica's (diagonal) cell; equivalently N T_kin / V + W / (d V) with T_kin what
    `Temperature` returns.  The pair set of a term is the one PairPotentials sums the energy over (i < j, strict minimum
    image, 0 < d^2 < cutoff^2, the term's index_tuple / ex_pairs selection, its own cutoff), and W = -dU/ds at s = 1 for the
    uniform scaling q -> s q, L -> s L with that set held fixed.  `model` is a PairPotentials of a built-in form or a Stack of
    one to four of them; W and its gradient are HIP kernels (ops.VirialFn, csrc/virial.hip).  Differentiable once with
    respect to q, v and the terms' parameters."""

    def __init__(self, system, model):
        super().__init__(system)
        from .md import _pair_terms_of
        mods = _pair_terms_of(model)
        if mods is None:
            raise NotImplementedError("Pressure: the model must be a PairPotentials of a built-in form (%s) or a Stack of one "
                                      "to four of them; GNN, bonded and user-module (pairMLP ...) terms have no virial kernel"
                                      % _FORMS)
        cs = mods[0]._cell_struct
        if not cs.diag:
            raise ValueError("Pressure: the cell must be diagonal (triclinic cells are not supported)")
        self.dim = getattr(system, "dim", 3)
        self.mass = torch.Tensor(system.get_masses()).to(self.device)[:self.natoms].contiguous()
        self._cell_struct, self._mods = cs, mods
        terms, off = [], 0
        for m in mods:
            n = sum(p.numel() for p in m.model.mdg_params())
            terms.append(m.mdg_term(off))
            off += n
        self._terms = ops.make_terms(terms, off)
        self._masks = [m._mask for m in mods]

    _frames = _frames

    def virial(self, q):
        """W of every frame of q ([N, 3], [T, N, 3], [R, T, N, 3] or replica-stacked [..., k N, 3])."""
        x, lead = self._frames(q, "q")
        params = [p for m in self._mods for p in m.model.mdg_params()]
        theta = torch.cat([p.reshape(-1) for p in params]) if params else x.new_zeros(0)
        return ops.VirialFn.apply(x, theta, self._cell_struct, self._terms, self._masks).reshape(lead)

    def kinetic(self, v):
        """K = sum_i m_i |v_i|^2 of every frame of v (shapes as for `virial`)."""
        x, lead = self._frames(v, "v")
        return (self.mass[None, :, None] * x * x).sum((1, 2)).reshape(lead)

    def forward(self, q, v):
        if q.shape != v.shape:
            raise ValueError("Pressure: q %s and v %s must agree in shape" % (tuple(q.shape), tuple(v.shape)))
        return (self.kinetic(v) + self.virial(q)) / (self.dim * self.volume)


class PotentialEnergy(Observable):
    """Pair potential energy of every frame of a trajectory in one call:

        U[f] = sum_terms sum_{i<j} phi(r_ij)

    over the pair set PairPotentials sums the energy over (i < j, strict minimum image on the diagonal cell, 0 < d^2 <
    cutoff^2, the term's index_tuple / ex_pairs selection, its own cutoff) with the plain truncated phi (no shift): U[f] is the
    value `model(q[f])` gives.  `model` is a PairPotentials of a built-in form or a Stack of one to four of them, as for
    `Pressure`; `PotentialEnergy.from_terms` takes the pair modules themselves.  q: [N, 3], [T, N, 3], [R, T, N, 3] or
    replica-stacked [..., k N, 3] (a trailing k).  float32 device positions run the list-free HIP kernels (ops.EnergyFramesFn,
    csrc/energy.hip); host or float64 positions take the torch restatement `_torch_energy` (all pairs, chunked over frames,
    the same pair set).  Differentiable once with respect to q and the terms' parameters; when only the parameters need a
    gradient (detached frames: `reweight.Reweighting`) the backward pass is one once-per-pair launch.

    Not covered: tabulated or learned pair modules (pairMLP ...: the kernels tabulate their force, not their energy),
    many-body, bonded, charge and GNN terms, triclinic cells, more than 32 768 atoms.  `reweight.Reweighting` accepts any
    callable q -> U, so such a model can be reweighted with a function of the user's own; for learned PAIR modules that
    callable exists: `TabulatedEnergy`."""

    MAX_ATOMS = 32768

    def __init__(self, system, model):
        from .md import _pair_terms_of
        mods = _pair_terms_of(model)
        if mods is None:
            raise NotImplementedError(self._refusal())
        self._setup(system, [(m.model, float(m.cutoff), m._mask) for m in mods])

    @classmethod
    def from_terms(cls, system, terms):
        """From the pair modules themselves: terms = [(module, cutoff, index_tuple, ex_pairs), ...] (the selections may be
        None), one to four built-in forms.  Needs no neighbour list, so it also serves a system on the host."""
        self = cls.__new__(cls)
        terms = [tuple(t) + (None,) * (4 - len(t)) for t in terms]
        from .potentials import is_builtin_form
        if not 1 <= len(terms) <= 4 or not all(is_builtin_form(t[0]) for t in terms):
            raise NotImplementedError(cls._refusal())
        n = getattr(system, "group_size", system.get_number_of_atoms())
        self._setup(system, [(m.to(system.device), float(rc), ops.build_mask(n, it, ex, system.device)) for m, rc, it, ex in terms])
        return self

    @staticmethod
    def _refusal():
        return ("PotentialEnergy: the model must be a PairPotentials of a built-in form (%s) or a Stack of one to four of them; "
                "GNN, bonded, many-body and tabulated user-module (pairMLP ...) terms have no batched energy kernel (the "
                "tabulated kernels hold the force, not the energy).  reweight.Reweighting accepts any callable q -> U per "
                "frame: pass a function of your own for such a model" % _FORMS)

    def _setup(self, system, terms):
        Observable.__init__(self, system)
        from . import _lib
        cs = _lib.make_cell(system.get_cell())
        if not cs.diag:
            raise ValueError("PotentialEnergy: the cell must be diagonal (triclinic cells are not supported)")
        if self.natoms > self.MAX_ATOMS:
            raise ValueError("PotentialEnergy: at most %d atoms per frame, got %d" % (self.MAX_ATOMS, self.natoms))
        self._cell_struct = cs
        self._models = torch.nn.ModuleList([m for m, _, _ in terms])
        self._cutoffs = [rc for _, rc, _ in terms]
        self._masks = [mk for _, _, mk in terms]
        descr, off = [], 0
        for m, rc, mk in terms:
            n = sum(p.numel() for p in m.mdg_params())
            descr.append(ops.make_term(m.mdg_term(), rc, off, n, mk))
            off += n
        self._terms = ops.make_terms(descr, off)

    _frames = _frames

    def _torch_energy(self, x, budget=1 << 22):
        """The same sum by torch ops in x's dtype on x's device: all pairs of every frame, chunked over the frames."""
        F, N = x.shape[0], x.shape[1]
        iu = torch.triu_indices(N, N, offset=1, device=x.device)
        L = self.cell.detach().to(x)
        out = []
        step = max(1, budget // max(1, iu.shape[1]))
        for a in range(0, F, step):
            xa = x[a:a + step]
            D = xa[:, iu[1]] - xa[:, iu[0]]
            s = D.detach() * (1.0 / L)
            D = D + (-(s > 0.5).to(x) + (s < -0.5).to(x)) * L
            d2 = D.pow(2).sum(-1)
            U = x.new_zeros(xa.shape[0])
            for m, rc, mk in zip(self._models, self._cutoffs, self._masks):
                keep = (d2.detach() < rc ** 2) & (d2.detach() != 0)
                if mk is not None:
                    keep = keep & mk.to(x.device).bool()[iu[0], iu[1]][None, :]
                fi, pi = torch.nonzero(keep, as_tuple=True)
                U = U.index_add(0, fi, m(d2[fi, pi].sqrt()).to(x.dtype))
            out.append(U)
        return torch.cat(out)

    def forward(self, q):
        """U of every frame of q."""
        x, lead = self._frames(q, "q")
        if not (x.is_cuda and x.dtype == torch.float32):
            return self._torch_energy(x).reshape(lead)
        params = [p for m in self._models for p in m.mdg_params()]
        theta = torch.cat([p.reshape(-1) for p in params]) if params else x.new_zeros(0)
        return ops.EnergyFramesFn.apply(x, theta, self._cell_struct, self._terms, self._masks).reshape(lead)


class TabulatedEnergy(Observable):
    """Pair potential energy of every frame of a trajectory for LEARNED pair potentials (pairMLP or any nn.Module phi(r)), which
    `PotentialEnergy` refuses: the energy side of trajectory reweighting (`reweight.Reweighting`) for the models it was written
    for.

        U[f] = sum_{built-in members} sum_{i<j} phi(r_ij)  +  sum_{groups} sum_{i<j} phi~_group(r_ij^2)

    `model` is a PairPotentials or a Stack whose members are all PairPotentials, at least one of them a user module;
    `TabulatedEnergy.from_terms` takes the pair modules themselves.  Built-in members (the steep prior: LJFamily,
    ExcludedVolume ...) stay exact: they go through `PotentialEnergy`'s kernels (ops.EnergyFramesFn).  The user modules are
    grouped by (cutoff, selection mask); every forward call tabulates each group's sum of phi on the uniform grid in u = r^2 from
    (r_min cutoff)^2 to cutoff^2 -- `nodes` nodes (value, du dphi/du), the slopes by autograd with create_graph=True, as the
    integrators tabulate the force for the fused kernels; `nodes` and `r_min` default to their `table_nodes` and `table_rmin` --
    and one launch per group (ops.EnergyTableFn, csrc/energy_table.hip) sums the cubic-Hermite interpolant phi~ over the pair
    set of `PotentialEnergy` (i < j, strict minimum image on the diagonal cell, 0 < d^2 < cutoff^2, the selection, the plain
    truncated phi).  The node gradient the kernel returns flows through the tabulation into the module parameters; with
    detached frames (reweighting) the backward pass is one once-per-pair launch per group.  q: [N, 3], [T, N, 3], [R, T, N, 3] or
    replica-stacked [..., k N, 3].  float32 device positions run the kernels; host or float64 positions take the torch
    restatement `_torch_table_energy` (the same table, pair set and below-range rule).  Differentiable once.

    Range: a pair closer than r_min cutoff lies below the first node and takes the constant first node value (no force).  With
    `check_range=True` such a pair raises a RuntimeError (one host read per call, the rule of the fused tabulated path); with
    `check_range=False` nothing is read and the count of the last call stays available as `last_below`.

    The dynamics interpolate a table of phi'/r, this class a table of phi: the two differ by interpolation error.  That does not
    bias the reweighting estimator, whose weights use only energy differences between theta and theta_ref on the SAME table.

    Not covered: the virial of tabulated modules, temperature-dependent modules (TPairPotentials / TpairMLP), many-body, bonded,
    charge and GNN members, triclinic cells, more than 32 768 atoms."""

    MAX_ATOMS = 32768

    def __init__(self, system, model, nodes=None, r_min=None, check_range=True):
        from .interface import PairPotentials, Stack, TPairPotentials
        mods = [model] if isinstance(model, PairPotentials) else (list(model.models.values()) if isinstance(model, Stack) else None)
        if not mods or not all(isinstance(m, PairPotentials) for m in mods):
            raise NotImplementedError("TabulatedEnergy: the model must be a PairPotentials or a Stack whose members are all "
                                      "PairPotentials, at least one of them a user module phi(r) (pairMLP ...); GNN, bonded, "
                                      "many-body and charge members have no tabulated pair energy")
        if any(isinstance(m, TPairPotentials) for m in mods):
            raise NotImplementedError("TabulatedEnergy: temperature-dependent pair modules (TPairPotentials / TpairMLP) are not "
                                      "covered")
        self._setup(system, [(m.model, float(m.cutoff), m._mask) for m in mods], nodes, r_min, check_range)

    @classmethod
    def from_terms(cls, system, terms, nodes=None, r_min=None, check_range=True):
        """From the pair modules themselves: terms = [(module, cutoff, index_tuple, ex_pairs), ...] (the selections may be
        None).  Needs no neighbour list, so it also serves a system on the host."""
        self = cls.__new__(cls)
        terms = [tuple(t) + (None,) * (4 - len(t)) for t in terms]
        n = getattr(system, "group_size", system.get_number_of_atoms())
        self._setup(system, [(m.to(system.device), float(rc), ops.build_mask(n, it, ex, system.device)) for m, rc, it, ex in terms],
                    nodes, r_min, check_range)
        return self

    def _setup(self, system, terms, nodes, r_min, check_range):
        import numpy as np
        from . import _lib
        from .md import _EOM
        from .potentials import is_builtin_form
        Observable.__init__(self, system)
        if not all(isinstance(m, torch.nn.Module) for m, _, _ in terms):
            raise NotImplementedError("TabulatedEnergy: every term must be a pair module phi(r)")
        user = [t for t in terms if not is_builtin_form(t[0])]
        exact = [t for t in terms if is_builtin_form(t[0])]
        if not user:
            raise NotImplementedError("TabulatedEnergy: the model holds no user module (pairMLP ...); thermo.PotentialEnergy "
                                      "evaluates built-in pair forms exactly")
        cs = _lib.make_cell(system.get_cell())
        if not cs.diag:
            raise ValueError("TabulatedEnergy: the cell must be diagonal (triclinic cells are not supported)")
        if self.natoms > self.MAX_ATOMS:
            raise ValueError("TabulatedEnergy: at most %d atoms per frame, got %d" % (self.MAX_ATOMS, self.natoms))
        self.nodes = int(_EOM.table_nodes if nodes is None else nodes)
        self.r_min = float(_EOM.table_rmin if r_min is None else r_min)
        lo, hi = ops.EAM_TABLE_NODES
        if not lo <= self.nodes <= hi:
            raise ValueError("TabulatedEnergy: nodes must lie in [%d, %d], got %d" % (lo, hi, self.nodes))
        if not 0.0 <= self.r_min < 1.0:
            raise ValueError("TabulatedEnergy: r_min is a fraction of the cutoff in [0, 1), got %r" % (r_min,))
        self.check_range = bool(check_range)
        self.last_below = None
        self._cell_struct = cs
        self._exact = None
        if exact:
            self._exact = PotentialEnergy.__new__(PotentialEnergy)
            if len(exact) > 4:
                raise NotImplementedError("TabulatedEnergy: at most four built-in members beside the user modules")
            self._exact._setup(system, exact)
        self._groups = []
        for m, rc, mk in user:
            for g in self._groups:
                if g["cutoff"] == rc and ((mk is None and g["mask"] is None) or
                                          (mk is not None and g["mask"] is not None and torch.equal(mk, g["mask"]))):
                    g["mods"].append(m)
                    break
            else:
                # the float32 grid the kernel receives: u_g = u0 + g du, the last node at cutoff^2
                u0 = np.float32((self.r_min * rc) ** 2)
                du = np.float32((rc * rc - float(u0)) / (self.nodes - 1))
                self._groups.append(dict(mods=torch.nn.ModuleList([m]), cutoff=rc, mask=mk, u0=float(u0), du=float(du),
                                         inv_du=float(np.float32(1.0) / du)))
        self._user = torch.nn.ModuleList([g["mods"] for g in self._groups])

    _frames = _frames

    def grid(self, group=0):
        """(u0, du, nodes) of a group's table: float32 values, u_g = u0 + g du"""
        g = self._groups[group]
        return g["u0"], g["du"], self.nodes

    def tabulate(self, group=0, device=None):
        """The [2 nodes] table of a group, (phi_g, du dphi/du_g) on its grid, in the modules' dtype and differentiable with
        respect to their parameters."""
        g = self._groups[group]
        ps = list(g["mods"].parameters())
        dtype = ps[0].dtype if ps else torch.float32
        device = (ps[0].device if ps else self.device) if device is None else device
        with torch.enable_grad():
            u32 = g["u0"] + g["du"] * torch.arange(self.nodes, device=device, dtype=torch.float32)
            u = u32.to(dtype).requires_grad_(True)
            r = u.sqrt()[:, None]
            phi = sum(m(r).reshape(-1) for m in g["mods"])
            (dphi,) = torch.autograd.grad(phi.sum(), u, create_graph=True)
            return torch.stack((phi, g["du"] * dphi), 1).reshape(-1)

    def _torch_table_energy(self, x, table, g, budget=1 << 22):
        """(U [F], pairs below the first node) of one group by torch ops in x's dtype: all pairs of every frame, chunked over
        the frames; the kernel's grid arithmetic, pair set and below-range rule."""
        F, N, p = x.shape[0], x.shape[1], self.nodes
        iu = torch.triu_indices(N, N, offset=1, device=x.device)
        L = self.cell.detach().to(x)
        nd = table.to(x).reshape(p, 2)
        rc2, u0, inv_du = g["cutoff"] ** 2, g["u0"], g["inv_du"]
        sel = None if g["mask"] is None else g["mask"].to(x.device).bool()[iu[0], iu[1]][None, :]
        out, below = [], torch.zeros((), dtype=torch.int64, device=x.device)
        step = max(1, budget // max(1, iu.shape[1]))
        for a in range(0, F, step):
            xa = x[a:a + step]
            D = xa[:, iu[1]] - xa[:, iu[0]]
            s = D.detach() * (1.0 / L)
            D = D + (-(s > 0.5).to(x) + (s < -0.5).to(x)) * L
            d2 = D.pow(2).sum(-1)
            keep = (d2.detach() < rc2) & (d2.detach() != 0)
            if sel is not None:
                keep = keep & sel
            fi, pi = torch.nonzero(keep, as_tuple=True)
            d2 = d2[fi, pi]
            below = below + (d2.detach() < u0).sum()
            t = ((d2 - u0) * inv_du).clamp(0.0, float(p - 1))               # (no gradient below the first node)
            c = t.detach().floor().long().clamp(max=p - 2)
            fr = t - c.to(x)
            om = 1.0 - fr
            b0, b1, b2, b3 = (1.0 + 2.0 * fr) * om * om, fr * om * om, fr * fr * (3.0 - 2.0 * fr), fr * fr * (fr - 1.0)
            phi = b0 * nd[c, 0] + b1 * nd[c, 1] + b2 * nd[c + 1, 0] + b3 * nd[c + 1, 1]
            out.append(x.new_zeros(xa.shape[0]).index_add(0, fi, phi))
        return torch.cat(out), below

    def forward(self, q):
        """U of every frame of q."""
        x, lead = self._frames(q, "q")
        kernels = x.is_cuda and x.dtype == torch.float32
        U = None if self._exact is None else self._exact(x)
        below = []
        for k, g in enumerate(self._groups):
            table = self.tabulate(k, x.device)
            if kernels:
                Ug = ops.EnergyTableFn.apply(x, table, self._cell_struct, self.nodes, g["u0"], g["du"], g["cutoff"], g["mask"])
                below.append(ops.EnergyTableFn.last_below.to(torch.int64).reshape(()))
            else:
                Ug, nb = self._torch_table_energy(x, table, g)
                below.append(nb)
            U = Ug if U is None else U + Ug
        self.last_below = below[0] if len(below) == 1 else torch.stack(below).sum()
        if self.check_range:
            n = int(self.last_below)
            if n:
                raise RuntimeError("TabulatedEnergy: %d pair(s) came closer than r_min * cutoff = %.4g, below the first node of "
                                   "the tabulated pair energy; lower `r_min` (now %g) or pass check_range=False to let them "
                                   "take the first node's value" % (n, self.r_min * min(g["cutoff"] for g in self._groups),
                                                                    self.r_min))
        return U.reshape(lead)


class _ManyBodyEnergy(Observable):
    """What StillingerWeberEnergy, EAMEnergy and TersoffEnergy share: the checks of the constructor, the frame-by-frame torch
    restatement and the device copy of one replica's species.  A subclass names its models (`_model_types`), its refusal
    (`_REFUSAL`, with one %s for the model's class) and the arguments of its model's `_torch_energy` (`_torch_args`);
    `_typed` says whether the model carries per-atom `types`."""

    MAX_ATOMS = 1024
    _REFUSAL = None
    _typed = False
    _frames = _frames

    def __init__(self, system, model):
        from . import _lib
        name = type(self).__name__
        if not isinstance(model, self._model_types()):
            raise NotImplementedError(self._REFUSAL % type(model).__name__)
        super().__init__(system)
        cs = _lib.make_cell(system.get_cell())
        if not cs.diag:
            raise ValueError("%s: the cell must be diagonal (triclinic cells are not supported)" % name)
        if self.natoms > self.MAX_ATOMS:
            raise ValueError("%s: at most %d atoms per frame, got %d" % (name, self.MAX_ATOMS, self.natoms))
        if self.natoms != model._group:
            raise ValueError("%s: the model was built for %d atoms per replica, the system holds %d"
                             % (name, model._group, self.natoms))
        self.model = model
        self._cell_struct = cs
        self._half_cell = 0.5 * min(cs.h[0], cs.h[4], cs.h[8])
        self._types = None
        self._check_cutoff()

    def _check_cutoff(self):
        """The half-cell check on the model's fixed cutoff."""
        if self.model.cutoff > self._half_cell:
            raise ValueError("%s: cutoff = %g exceeds half the shortest cell length (%g): the minimum image no longer "
                             "holds every neighbour" % (type(self).__name__, self.model.cutoff, self._half_cell))

    def _torch_args(self, x):
        """What the model's `_torch_energy` takes after the frame."""
        return ()

    def _torch_energy(self, x):
        """The model's torch restatement, one frame at a time (each frame is one replica to it)."""
        m = self.model
        n_rep, m._n_rep = m._n_rep, 1
        types = m.types if self._typed else None
        if self._typed:
            m.types = types[:self.natoms]                 # (one entry per atom of the stacked system: one replica's)
        args = self._torch_args(x)
        try:
            return torch.stack([m._torch_energy(xf, *args).reshape(()) for xf in x])
        finally:
            m._n_rep = n_rep
            if self._typed:
                m.types = types

    def _device_types(self, device):
        """One replica's species as device int32 [N], copied once per device."""
        if self._types is None or self._types.device != device:
            self._types = self.model.types[:self.natoms].to(device=device, dtype=torch.int32).contiguous()
        return self._types


class StillingerWeberEnergy(_ManyBodyEnergy):
    """Stillinger-Weber energy of every frame of a trajectory in one call, which `PotentialEnergy` refuses: the energy side of
    trajectory reweighting (`reweight.Reweighting`) for the three-body models fitted to structure that a pair term cannot express
    (silicon, mW water).

        U[f] = sum_{i<j} phi2(r_ij) + sum_i sum_{j<k in row(i)} phi3(r_ij, r_ik, cos theta_jik)

    with the definition, pair set (strict minimum image on the diagonal cell, 0 < r < a sigma) and formulas of
    `interface.StillingerWeber`: U[f] is the value `model(q[f])` gives.  `model` is a StillingerWeber (one species); its
    parameters are read where they are, so the optimiser that steps them steps this energy.  q: [N, 3], [T, N, 3],
    [R, T, N, 3] or replica-stacked [..., k N, 3] (a trailing k).

    float32 device positions run ONE list-free launch (ops.SWFramesFn, csrc/sw_frames.hip): every atom finds its neighbours in
    its frame with the live device sigma, so a step of the trainable sigma costs nothing -- no neighbour list is searched and
    nothing is read on the host (sigma is read once per change of its version counter for the half-cell check below, never
    inside a HIP-graph capture).  The kernel reads (epsilon, sigma, lam) packed on the device at every call, so it follows the
    parameters however they were stepped.  When epsilon, sigma or lam requires grad the same launch emits dU[f]/d(epsilon, sigma, lam), and the parameter
    part of the backward pass is their fixed-order weighted sum: with detached frames (reweighting) the backward pass visits no
    pair or triplet at all.  A position gradient, off that path, goes through the model's list kernel (mdg_sw_eval) on the
    frames stacked behind a list searched at 1.02 a sigma (one host read of sigma per such backward pass).  Host or float64 positions take the model's torch restatement
    `_torch_energy`, frame by frame.  Differentiable once.

    An atom may hold at most `ops.sw_frames_row_cap()` = 64 neighbours inside a sigma (silicon and mW water hold 4 - 30); a
    frame with a longer row comes out NaN rather than truncated.  a sigma may not exceed half the shortest cell length
    (ValueError).

    Not covered: StillingerWeberMulti frame energies (embedded-atom models: `EAMEnergy`; Tersoff and TersoffMulti:
    `TersoffEnergy`), a StillingerWeber stacked with pair terms (add a `PotentialEnergy` of the pair terms: Reweighting takes
    any callable), the virial, more than 1024 atoms per frame, triclinic cells."""

    MAX_ATOMS = ops.SW_FRAMES_MAX_ATOMS
    _REFUSAL = ("StillingerWeberEnergy: the model must be an interface.StillingerWeber (one species); got "
                "%s.  StillingerWeberMulti, Tersoff, EAM, pair terms and Stacks have no batched "
                "Stillinger-Weber frame energy (built-in pair forms: thermo.PotentialEnergy; learned pair "
                "modules: thermo.TabulatedEnergy; SuttonChen and EAM: thermo.EAMEnergy; Tersoff and "
                "TersoffMulti: thermo.TersoffEnergy)")

    @staticmethod
    def _model_types():
        from .interface import StillingerWeber
        return StillingerWeber

    def _check_cutoff(self):
        """a sigma moves with the trainable sigma: the check is `_sync_cutoff`, repeated at every call."""
        self._sig_key = None
        self._sync_cutoff()

    def _sync_cutoff(self):
        """The half-cell check on a sigma; sigma is read on the host only when its version counter moved, and never inside a
        HIP-graph capture (StillingerWeber._sync_cutoff)."""
        s = self.model.sigma
        if s.is_cuda and torch.cuda.is_current_stream_capturing():
            return
        key = (s.data_ptr(), s._version)
        if key == self._sig_key:
            return
        rc = self.model.a * float(s.detach())                  # (one host read per change of sigma)
        if not rc > 0.0:
            raise ValueError("StillingerWeberEnergy: sigma must stay positive (got %g)" % (rc / self.model.a))
        if rc > self._half_cell:
            raise ValueError("StillingerWeberEnergy: a * sigma = %g exceeds half the shortest cell length (%g): the minimum "
                             "image no longer holds every neighbour" % (rc, self._half_cell))
        self._sig_key = key

    def forward(self, q):
        """U of every frame of q."""
        x, lead = self._frames(q, "q")
        self._sync_cutoff()
        if not (x.is_cuda and x.dtype == torch.float32):
            return self._torch_energy(x).reshape(lead)
        m = self.model
        theta = torch.cat([p.detach().reshape(-1) for p in (m.epsilon, m.sigma, m.lam)]).to(device=x.device, dtype=torch.float32)
        return ops.SWFramesFn.apply(x, m.epsilon, m.sigma, m.lam, theta, self._cell_struct, m._consts,
                                    m.cutoff_reset).reshape(lead)


class EAMEnergy(_ManyBodyEnergy):
    """Embedded-atom energy of every frame of a trajectory in one call: the energy side of trajectory reweighting
    (`reweight.Reweighting`) for the metals, whose trainable object is often the shape of tabulated functions -- thousands of
    node entries, all of whose gradients one weighted scatter gives at once.

        U[f] = sum_i [ 1/2 sum_{j != i} phi_ab(r_ij) + F_a(rho_i) ],   rho_i = sum_{j != i} f_b(r_ij)

    `model` is an `interface.EAM` (tabulated, 1 - 4 species) or an `interface.SuttonChen`; U[f] is the value `model(q[f])`
    gives, with the model's own conventions: its pair set (strict minimum image on the diagonal cell, 0 < r < cutoff with
    r = sqrtf(d2)), for EAM the linear continuation outside the grids and F_a(0) for an atom without a neighbour, for SuttonChen
    an embedding energy of exactly 0 for such an atom and both shifts; per-atom `types` of one replica (one replica is one
    frame).  q: [N, 3], [T, N, 3], [R, T, N, 3] or replica-stacked [..., k N, 3] (a trailing k).

    float32 device positions run ONE list-free launch (ops.EAMTableFramesFn / ops.EAMFramesFn, csrc/eam_frames.hip): every
    atom walks its frame once and has 1/2 sum phi and rho_i when the walk ends.  The parameters are read where they live, so the
    optimiser that steps them steps this energy: SuttonChen's (epsilon, a, c) are packed on the device at every call, EAM's
    nodes come from the model's float32 device mirror, refreshed as `EAM._tables()` refreshes it.  With detached frames
    (reweighting) the backward pass of SuttonChen visits no pair (the same launch emitted dU[f]/d(epsilon, a, c); their
    fixed-order weighted sum remains), and that of EAM is one more walk with an order-independent fixed-point scatter into the
    nodes.  A position gradient, off that path, goes through the model's list kernel on the stacked frames.  Host or float64
    positions take the model's torch restatement `_torch_energy`, frame by frame.  Differentiable once.

    The cutoff may not exceed half the shortest cell length (ValueError: the strict minimum image would miss neighbours).

    Not covered: StillingerWeberMulti frame energies (Tersoff and TersoffMulti: `TersoffEnergy`), an embedded-atom term
    stacked with pair terms (add a `PotentialEnergy` of the pair terms: Reweighting takes any callable), the virial, more than
    1024 atoms per frame, triclinic cells."""

    MAX_ATOMS = ops.EAM_FRAMES_MAX_ATOMS
    _REFUSAL = ("EAMEnergy: the model must be an interface.EAM or an interface.SuttonChen; got %s.  Stacks, "
                "Tersoff and Stillinger-Weber terms have no batched embedded-atom frame energy (one-species "
                "Stillinger-Weber: thermo.StillingerWeberEnergy; Tersoff and TersoffMulti: "
                "thermo.TersoffEnergy; built-in pair forms: thermo.PotentialEnergy; learned pair modules: "
                "thermo.TabulatedEnergy)")

    @staticmethod
    def _model_types():
        from .interface import EAM, SuttonChen
        return EAM, SuttonChen

    def __init__(self, system, model):
        super().__init__(system, model)
        self.tabulated = self._typed = isinstance(model, self._model_types()[0])

    def _torch_args(self, x):
        # (cast once: the parameter gradient is summed over the frames in the dtype of x and rounded to the parameters' once)
        m = self.model
        return (tuple(p.to(x) for p in (m._nodes() if self.tabulated else (m.epsilon, m.a, m.c))),)

    def forward(self, q):
        """U of every frame of q."""
        x, lead = self._frames(q, "q")
        if not (x.is_cuda and x.dtype == torch.float32):
            return self._torch_energy(x).reshape(lead)
        m = self.model
        if self.tabulated:
            tables = m._tables()
            if tables.device != x.device:
                tables = tables.to(x.device)
            return ops.EAMTableFramesFn.apply(x, m.pair_nodes, m.density_nodes, m.embed_nodes, tables,
                                              self._device_types(x.device), self._cell_struct, m._consts).reshape(lead)
        theta = torch.cat([p.detach().reshape(-1) for p in (m.epsilon, m.a, m.c)]).to(device=x.device, dtype=torch.float32)
        return ops.EAMFramesFn.apply(x, m.epsilon, m.a, m.c, theta, self._cell_struct, m._consts).reshape(lead)


class TersoffEnergy(_ManyBodyEnergy):
    """Tersoff bond-order energy of every frame of a trajectory in one call: the energy side of trajectory reweighting
    (`reweight.Reweighting`) for silicon, carbon, germanium and their alloys, whose trainable A, B and h are what a fit to an
    angle distribution or an RDF carries.

        U[f] = 1/2 sum_i sum_{j != i} fc_ab(r_ij) [ A_ab exp(-lam1_ab r_ij) - b_ij B_ab exp(-lam2_ab r_ij) ]

    `model` is an `interface.Tersoff` (one species) or an `interface.TersoffMulti` (1 - 4 species); U[f] is the value
    `model(q[f])` gives, with the model's own conventions: the strict minimum image on the diagonal cell, the support
    0 < r < R_ab + D_ab of the directed pair (centre species, end species) on r = sqrtf(d2), b = 1 with zero derivatives where
    zeta = 0, per-atom `types` of one replica (one replica is one frame).  q: [N, 3], [T, N, 3], [R, T, N, 3] or
    replica-stacked [..., k N, 3] (a trailing k).

    float32 device positions run ONE list-free launch (ops.TersoffFramesFn / ops.TersoffMultiFramesFn,
    csrc/tersoff_frames.hip): every atom finds its neighbours in its frame and runs the bond pass over them; no list is
    searched and nothing is read on the host.  The kernel reads (A, B, h) from the model's device mirror (`Tersoff._theta()`,
    `TersoffMulti._tables()`), rewritten here at every call, so it follows the parameters however they were stepped.  When A,
    B or h requires grad the same launch emits dU[f]/d(A, B, h), and the parameter part of the backward pass is their
    fixed-order weighted sum: with detached frames (reweighting) the backward pass visits no bond at all.  A position
    gradient, off that path, goes through the model's list kernels on the stacked frames behind a list searched at the
    model's cutoff.  Host or float64 positions take the model's torch restatement `_torch_energy`, frame by frame.
    Differentiable once.

    An atom may hold at most `ops.tersoff_frames_row_cap()` = 32 neighbours inside R + D (the covalent networks hold 3 - 10);
    a frame with a longer row comes out NaN rather than truncated.  The cutoff max (R + D) is absolute and may not exceed half
    the shortest cell length (ValueError at construction).

    Not covered: StillingerWeberMulti frame energies, the virial of the term, a Tersoff term stacked with pair terms in one
    launch (add a `PotentialEnergy` of the pair terms: Reweighting takes any callable), triclinic cells, more than 1024 atoms
    per frame, evaluation inside the fused trajectory launches."""

    MAX_ATOMS = ops.TERSOFF_FRAMES_MAX_ATOMS
    _REFUSAL = ("TersoffEnergy: the model must be an interface.Tersoff or an interface.TersoffMulti; got "
                "%s.  Stacks, Stillinger-Weber and embedded-atom terms have no batched Tersoff frame "
                "energy (one-species Stillinger-Weber: thermo.StillingerWeberEnergy; SuttonChen and EAM: "
                "thermo.EAMEnergy; built-in pair forms: thermo.PotentialEnergy; learned pair modules: "
                "thermo.TabulatedEnergy)")

    @staticmethod
    def _model_types():
        from .interface import Tersoff, TersoffMulti
        return Tersoff, TersoffMulti

    def __init__(self, system, model):
        super().__init__(system, model)
        self.multi = self._typed = isinstance(model, self._model_types()[1])

    def _torch_args(self, x):
        # (cast once: the parameter gradient is summed over the frames in the dtype of x and rounded to the parameters' once)
        m = self.model
        return (tuple(p.to(x) for p in (m.A, m.B, m.h)),)

    def _mirror(self, mirror, device):
        """The model's device image of (A, B, h), rewritten now (an edit through `.data` moves no version counter, so the
        mirror's own test would miss it); inside a HIP-graph capture it comes as it is."""
        buf = mirror.get(fresh=True)
        return buf if buf.device == device else buf.to(device)

    def forward(self, q):
        """U of every frame of q."""
        x, lead = self._frames(q, "q")
        if not (x.is_cuda and x.dtype == torch.float32):
            return self._torch_energy(x).reshape(lead)
        m = self.model
        if self.multi:
            tables = self._mirror(m._table_mirror, x.device)
            return ops.TersoffMultiFramesFn.apply(x, m.A, m.B, m.h, tables, self._device_types(x.device), m.n_species,
                                                  self._cell_struct, m.cutoff).reshape(lead)
        theta = self._mirror(m._theta_mirror, x.device)
        return ops.TersoffFramesFn.apply(x, m.A, m.B, m.h, theta, self._cell_struct, m._consts).reshape(lead)
