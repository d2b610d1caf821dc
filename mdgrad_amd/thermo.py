"""torchmd/thermo.py:57-66 (`Temperature`) and `Pressure`: the reference's sketch (torchmd/thermo.py:17-54) uses undefined
names and does not run, so the definition is this module's -- kinetic part plus pair virial over (d V), see `Pressure`."""
import torch

from . import ops
from .observable import Observable

_FORMS = "LJFamily / LennardJones / LennardJones69, ExcludedVolume, ModifiedMorse, Buck, Yukawa"


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

    def _frames(self, x, name):
        n = x.shape[-2] if x.dim() >= 2 else 0
        if n == 0 or x.shape[-1] != 3 or n % self.natoms:
            raise ValueError("Pressure: %s must be [..., k * %d, 3], got %s" % (name, self.natoms, tuple(x.shape)))
        k = n // self.natoms                             # replica-stacked state [..., k N, 3]: one value per replica
        lead = tuple(x.shape[:-2]) + ((k,) if k > 1 else ())
        return x.reshape(-1, self.natoms, 3), lead

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
