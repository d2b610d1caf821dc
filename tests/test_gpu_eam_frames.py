"""K36 / K37: the embedded-atom energy of every frame (thermo.EAMEnergy, ops.EAMTableFramesFn / ops.EAMFramesFn,
mdg_eam_table_frames_fwd, mdg_eam_table_frames_nodes_bwd, mdg_eam_frames_fwd, csrc/eam_frames.hip) against the float64
definitions of tests/eam_table_ref.py and tests/eam_ref.py, frame by frame, and against the list kernels K27 and K24.

Tolerance: the project's, K * 2^-24 * A per component with K = 64 (KTOL and `within` of tests/test_gpu_eam.py) and A = the float64
sum of the absolute contributions to that component of that frame that the references return (eam_table_ref.evaluate: A_U,
A_gtab, A_grad; eam_ref.evaluate: A_U, A_dth, A_grad); for L = sum_f g_f U_f the scale is sum_f |g_f| A_f.  U[f] against the list
kernel's model(q[f]): 2 K (two float32 kernels).  `within` prints the largest observed err / (2^-24 A) of every comparison.  No
case is left out of any comparison: with pin_cutoff and with shift="force" the functions vanish C1 at the cutoff, and every frame
seed used here keeps coulomb_ref.half_list's margin above MARGIN = 1e-5 (asserted for every frame of every case), so that
shift="none" selects the pairs of the float64 list.

Largest observed err / (2^-24 A) on an MI355X.  Tabulated (K36): U[f] 0.21 (two species, 4096 nodes; Cu-108 0.13, Cu-256 0.05,
gas 0.07), d(sum g U)/dnodes 2.37 (two species, 4096 nodes: global atomics; Cu-108 1.42, Cu-256 1.59, 48 nodes 0.88, gas 0.78),
U[f] against K27 0.14 of the doubled scale, d(sum g U)/dx through K27 below 0.005.  Sutton-Chen (K37): U[f] 0.85 (gas,
shift="none"; Cu-108 0.81, Cu-256 0.42), dU[f]/dtheta 0.69, d(sum g U)/dtheta 0.82 (after a *= 1.01; 0.71 on the gas), U[f] against
K24 0.73 of the doubled scale, d(sum g U)/dx through K24 5.53.  The position derivatives of the tables sit far below 1 for the
reason tests/test_gpu_eam_table.py gives (A counts both node values of a difference over h); K stays 64.

The float64 references of all frames are computed once per module and shared."""
import ctypes

import numpy as np
import pytest
import torch

import eam_ref as SC
import eam_table_ref as R
from test_gpu_eam import MARGIN, within, _gas37
from test_gpu_eam_table import _functions
from test_gpu_parity import DEV, mk_system

pytestmark = pytest.mark.gpu
F32 = np.float32
CU = SC.PUBLISHED["copper"]
RC, RMIN = 5.2, 1.8
BAD = {158, 161, 173, 197, 202, 211, 226}          # seeds whose frame holds a pair within 2e-5 of the cutoff (found on the CPU)
SEEDS = [s for s in range(108, 250) if s not in BAD][:130]


def _wrapped(names):
    """context: counts the calls of the list kernels ops.<name>"""
    from mdgrad_amd import ops

    class Ctx:
        def __enter__(self):
            self.calls, self.real = [], {n: getattr(ops, n) for n in names}
            for n in names:
                setattr(ops, n, (lambda real: lambda *a, **k: self.calls.append(1) or real(*a, **k))(self.real[n]))
            return self

        def __exit__(self, *exc):
            for n, f in self.real.items():
                setattr(ops, n, f)
    return Ctx()


class Case:
    """frames [F, N, 3] of one box and a model builder; the float64 references per frame, computed once and kept"""

    def __init__(self, frames, cell, build, tabulated):
        self.frames, self.cell = np.ascontiguousarray(frames, dtype=F32), np.asarray(cell, dtype=F32)
        self.F, self.N, self.build, self.tabulated = self.frames.shape[0], self.frames.shape[1], build, tabulated
        self._ref = {}

    def modules(self, system=None):
        from mdgrad_amd.thermo import EAMEnergy
        system = mk_system(self.frames[0], self.cell) if system is None else system
        model = self.build(system)
        assert model.cutoff <= 0.5 * float(self.cell.min())
        return model, EAMEnergy(system, model)

    def params(self, model):
        return (model.pair_nodes, model.density_nodes, model.embed_nodes) if self.tabulated else (model.epsilon, model.a, model.c)

    def _one(self, model, f):
        x = self.frames[f]
        if self.tabulated:
            lst = R.pairs(x, self.cell, model.cutoff)
            ref = R.evaluate(x, R.tables_of(model), lst, self.cell, model.types.cpu().long()[:self.N], R.grid_of(model),
                             pin=model.pin_cutoff)
            ref["dth"], ref["A_dth"] = ref["gtab"], ref["A_gtab"]
        else:
            lst = SC.pairs(x, self.cell, model.cutoff)
            ref = SC.evaluate(x, [float(p.detach()) for p in self.params(model)], lst, self.cell,
                              SC.consts(model.n, model.m, model.cutoff, model.shift))
        assert lst["margin"] >= MARGIN, "frame %d holds a pair on the cutoff: choose another seed" % f
        ref["rows"] = lst["rows"]
        return ref

    def reference(self, model, n=None):
        """dict of stacked float64 arrays for the first n frames at the module's float32 parameters"""
        key = tuple(float(p.detach().double().sum()) for p in self.params(model))
        n = self.F if n is None else n
        for f in range(n):
            if (key, f) not in self._ref:
                self._ref[(key, f)] = self._one(model, f)
        refs = [self._ref[(key, f)] for f in range(n)]
        out = {k: torch.stack([r[k] for r in refs]) for k in ("U", "A_U", "dth", "A_dth", "grad", "A_grad", "rho")}
        out["rows"] = [r["rows"] for r in refs]
        return out

    def q(self, n=None, requires_grad=False):
        return torch.tensor(self.frames[:n], device=DEV).requires_grad_(requires_grad)


def _fn(case):
    from mdgrad_amd import ops
    return ops.EAMTableFramesFn if case.tabulated else ops.EAMFramesFn


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def check_values(case, n=None, tag="", first=3):
    """U of one launch and the parameter gradient of L = sum_f g_f U_f against float64, the pinned entries, the first frames
    against the list kernel; asserts the reweighting route.  Returns (model, energy, reference, U, g)."""
    model, energy = case.modules()
    ref = case.reference(model, n)
    q = case.q(n)
    ps = case.params(model)
    _fn(case).last_route = None
    with _wrapped(["eam_table_eval", "eam_eval"]) as w:
        U = energy(q)
        assert U.shape == (q.shape[0],) and U.dtype == torch.float32
        within(U, ref["U"], ref["A_U"], tag + " U[f]")
        g = torch.tensor(np.random.default_rng(5).normal(0, 1, q.shape[0]), dtype=torch.float32, device=DEV)
        gth = _flat(torch.autograd.grad((U * g).sum(), ps, retain_graph=True))
        g64 = g.double().cpu()
        within(gth, (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0),
               tag + (" d(sum g U)/dnodes" if case.tabulated else " d(sum g U)/dtheta"))
        assert _fn(case).last_route == ("nodes" if case.tabulated else "theta") and not w.calls, "the list kernel was not called"
        if not case.tabulated:                       # the rows the launch emits = the gradient of each U[f] on its own
            eye = torch.eye(q.shape[0], device=DEV)
            k = min(q.shape[0], first)
            dU = torch.stack([_flat(torch.autograd.grad(U, ps, eye[f], retain_graph=True)) for f in range(k)])
            within(dU, ref["dth"][:k], ref["A_dth"][:k], tag + " dU[f]/dtheta (first frames)")
    if case.tabulated and model.pin_cutoff:
        m = R.pinned_mask(R.grid_of(model)).to(DEV)
        assert int(m.sum()) > 0 and float(gth[m].abs().max()) == 0.0, "pinned entries are exact zeros"
    k = min(q.shape[0], first)
    with torch.no_grad():
        Um = []
        for f in range(k):
            model._reset_topology(q[f])                      # (the list of K27 / K24 follows the positions only when asked to)
            Um.append(model(q[f]).reshape(()))
    within(U[:k], torch.stack(Um).double().cpu(), 2 * ref["A_U"][:k], tag + " U[f] against model(q[f]) (the list kernel)")
    return model, energy, ref, U, g


def _copper_table(n=1024, **kw):
    from mdgrad_amd.interface import EAM
    return lambda system: EAM.from_sutton_chen(system, "copper", cutoff=RC, r_min=RMIN, n_r=n, n_rho=n, **kw)


def _copper_sc(shift="force"):
    from mdgrad_amd.interface import SuttonChen
    eps, a, c, n, m = CU
    return lambda system: SuttonChen(system, eps, a, c, n, m, RC, shift=shift)


def _cu108_frames():
    xs = [SC.jittered_fcc(3, 3.61, 0.15, s) for s in SEEDS]
    return np.stack([x for x, _ in xs]), xs[0][1]


@pytest.fixture(scope="module")
def cu108():
    frames, cell = _cu108_frames()
    return dict(table=Case(frames, cell, _copper_table(), True), force=Case(frames, cell, _copper_sc("force"), False),
                none=Case(frames, cell, _copper_sc("none"), False))


# ------------------------------------------------------------------------------------------------ tabulated, Cu-108
@pytest.mark.parametrize("n", [1, 3, 130])
def test_cu108_table_values_and_node_gradients(cu108, n):
    """108 atoms: a wave per frame, four frames per workgroup; 130 frames end in a workgroup that is half empty.  1024-node
    tables: the r-tables are read from LDS and the node gradient is summed per workgroup in LDS (6144 words, the largest)."""
    from mdgrad_amd import ops
    case = cu108["table"]
    model, energy, ref, U, g = check_values(case, n, "cu108 table F=%d" % n)
    assert 2 * 2 * 1024 <= ops.eam_table_frames_lds_floats() and ops.eam_table_size(model._consts) == 6144
    rows = torch.cat(ref["rows"])
    assert int(rows.min()) >= 40 and int(rows.max()) >= 54
    # the bits of U do not depend on where the r-tables are read from (by size: the LDS copy here)
    try:
        ops.EAMTableFramesFn.table_mode = 0
        with torch.no_grad():
            U0 = energy(case.q(n))
    finally:
        ops.EAMTableFramesFn.table_mode = -1
    assert torch.equal(U0, U.detach())


# ------------------------------------------------------------------------------------------------ Cu-256: a workgroup per frame
@pytest.mark.parametrize("kind", ["table", "force"])
def test_cu256_a_workgroup_per_frame(kind):
    xs = [SC.jittered_fcc(4, 3.61, 0.15, s) for s in (257, 258)]
    case = Case(np.stack([x for x, _ in xs]), xs[0][1], _copper_table() if kind == "table" else _copper_sc(), kind == "table")
    assert case.N == 256
    model, energy, ref, U, g = check_values(case, None, "cu256 " + kind, first=1)
    if kind == "table":                      # by size this shape reads global memory; the LDS copy gives the same bits
        from mdgrad_amd import ops
        try:
            ops.EAMTableFramesFn.table_mode = 1
            with torch.no_grad():
                U1 = energy(case.q())
        finally:
            ops.EAMTableFramesFn.table_mode = -1
        assert torch.equal(U1, U.detach())


# ------------------------------------------------------------------------------------------------ two species
@pytest.mark.parametrize("n", [48, 4096])
def test_two_species_with_both_continuations(n):
    """The 108-atom box with alternating species; r_min above the closest pair and rho_max below the largest density, so both
    linear continuations are taken.  n = 4096 is the largest table set: r-tables from global memory, global atomics only."""
    from mdgrad_amd import ops
    from mdgrad_amd.interface import EAM
    frames, cell = _cu108_frames()
    types = np.arange(108) % 2
    build = lambda system: EAM.from_functions(system, types, *_functions(2.55), RC, 2.3, (40.0, 60.0), n, n)
    case = Case(frames[:3], cell, build, True)
    model, energy, ref, U, g = check_values(case, None, "two species n=%d" % n)
    lst = R.pairs(case.frames[0], cell, RC)
    m = R.node_margin(case.frames[0], R.tables_of(model), lst, cell, model.types.cpu().long(), R.grid_of(model))
    assert m["below"] > 0 and m["above"] > 0, m
    lds = 2 * (3 + 2) * n <= ops.eam_table_frames_lds_floats() and case.N <= 128
    assert lds == (n == 48) and (ops.eam_table_size(model._consts) <= 6144) == (n == 48), "both sides of both thresholds"
    # swapped species are far outside the tolerance
    tabs = R.tables_of(model)
    wrong = R.evaluate(case.frames[0], (tabs[0], tabs[1].flip(0), tabs[2]), lst, cell, model.types.cpu().long(), R.grid_of(model))
    assert abs(float(wrong["U"] - ref["U"][0])) > 100 * 64 * 2.0 ** -24 * float(ref["A_U"][0])


# ------------------------------------------------------------------------------------------------ gas: empty row, dimer, r = 0
def _gas_frames():
    x, box = _gas37()
    f1 = x.copy()
    f1[1] = f1[0]                                            # a coincident pair: r = 0, skipped
    return np.stack([x, f1]), box


@pytest.mark.parametrize("kind", ["table", "force", "none"])
def test_gas37_empty_row_dimer_and_coincident_atoms(kind):
    frames, box = _gas_frames()
    if kind == "table":
        lst0 = R.pairs(frames[0], box, RC)
        _, rho = SC.density(torch.tensor(frames[0]).double(), CU[1], lst0, box, SC.consts(9, 6, RC, "force"))
        low = float(rho[rho > 0].min())
        case = Case(frames, box, _copper_table(64, rho_range=(0.25 * low, 1.5 * float(rho.max()))), True)
    else:
        case = Case(frames, box, _copper_sc(kind), False)
    assert case.N == 37 and 37 % 64 != 0
    model, energy, ref, U, g = check_values(case, None, "gas37 " + kind, first=2)
    rows = ref["rows"][0].tolist()
    assert rows[33] == 0 and rows[34] == rows[35] == 1 and max(rows) >= 8
    assert bool((torch.tensor(frames[1][0]) == torch.tensor(frames[1][1])).all())
    assert bool(torch.isfinite(U).all()) and float(U[0].detach()) != float(U[1].detach())
    # the atom without a neighbour: F_a(0) from the table's continuation for EAM (a hundred times the tolerance of U: leaving
    # it out, or giving SuttonChen's atom anything but exactly 0, fails the comparison of U above)
    if kind == "table":
        en = model.embed_nodes.detach().cpu().double()[0, 0]
        f0 = float(en[0] + (0.0 - model.rho_range[0]) / model.h_rho * en[1])
        assert float(ref["rho"][0][33]) == 0.0 and abs(f0) > 100 * 64 * 2.0 ** -24 * float(ref["A_U"][0])
    else:
        assert float(ref["rho"][0][33]) == 0.0


# ------------------------------------------------------------------------------------------------ Sutton-Chen, Cu-108
@pytest.mark.parametrize("shift", ["force", "none"])
@pytest.mark.parametrize("n", [1, 130])
def test_cu108_sutton_chen_values_and_parameter_gradients(cu108, shift, n):
    check_values(cu108[shift], n, "cu108 SC %s F=%d" % (shift, n))


def test_a_step_of_a_is_followed(cu108):
    case = cu108["force"]
    n = 3
    model, energy = case.modules()
    q = case.q(n)
    with torch.no_grad():
        U0 = energy(q)
    model.a.data.mul_(1.01)
    ref = case.reference(model, n)                            # (keyed by the parameters: float64 at the new a)
    U = energy(q)
    within(U, ref["U"], ref["A_U"], "cu108 SC U[f] after a *= 1.01")
    dth = _flat(torch.autograd.grad(U.sum(), case.params(model)))
    within(dth, ref["dth"].sum(0), ref["A_dth"].sum(0), "cu108 SC d(sum U)/dtheta after a *= 1.01")
    assert not torch.equal(U.detach(), U0)


def test_stepped_nodes_are_followed(cu108):
    """The optimiser's in-place step of a node tensor reaches the kernel through the model's device mirror."""
    case = cu108["table"]
    model, energy = case.modules()
    q = case.q(2)
    with torch.no_grad():
        U0 = energy(q)
        model.embed_nodes.mul_(1.01)
        U1 = energy(q)
    ref = case.reference(model, 2)
    within(U1, ref["U"], ref["A_U"], "cu108 table U[f] after embed_nodes *= 1.01")
    assert not torch.equal(U0, U1)


# ------------------------------------------------------------------------------------------------ position route
@pytest.mark.parametrize("kind", ["table", "force"])
def test_position_gradient_against_float64(cu108, kind):
    case = cu108[kind]
    n = 3
    model, energy = case.modules()
    ref = case.reference(model, n)
    q = case.q(n, requires_grad=True)
    g = torch.tensor([1.0, -0.5, 2.0], device=DEV)
    U = energy(q)
    out = torch.autograd.grad((U * g).sum(), (q,) + tuple(case.params(model)))
    assert _fn(case).last_route == "full"
    g64 = g.double().cpu()
    within(out[0], g64[:, None, None] * ref["grad"], g64.abs()[:, None, None] * ref["A_grad"], "cu108 %s d(sum g U)/dx" % kind)
    within(_flat(out[1:]), (g64[:, None] * ref["dth"]).sum(0), (g64.abs()[:, None] * ref["A_dth"]).sum(0),
           "cu108 %s parameter gradient of the same backward pass" % kind)
    # positions alone
    for p in case.params(model):
        p.requires_grad_(False)
    U2 = energy(q)
    (gq,) = torch.autograd.grad((U2 * g).sum(), q)
    assert _fn(case).last_route == "positions" and torch.equal(gq, out[0]) and torch.equal(U2.detach(), U.detach())
    # shapes: a single frame, [R, T, N, 3], replica-stacked
    qd = case.q(4)
    with torch.no_grad():
        U4 = energy(qd)
        assert energy(qd[1]).shape == () and float(energy(qd[1])) == float(U4[1])
        assert torch.equal(energy(qd.reshape(2, 2, 108, 3)).reshape(4), U4)
        st = energy(torch.cat([qd[:2], qd[2:4]], dim=1))
    assert st.shape == (2, 2) and torch.equal(st[:, 0], U4[:2]) and torch.equal(st[:, 1], U4[2:4])


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("kind", ["table", "force"])
def test_bitwise_reproducible_and_frame_order(cu108, kind):
    case = cu108[kind]
    model, energy = case.modules()
    ps = case.params(model)
    q = case.q(130)
    g = torch.tensor(np.random.default_rng(11).normal(0, 1, 130), dtype=torch.float32, device=DEV)

    def run(x, gx):
        U = energy(x)
        return U.detach(), _flat(torch.autograd.grad((U * gx).sum(), ps))

    U1, t1 = run(q, g)
    U2, t2 = run(q, g)
    assert torch.equal(U1, U2) and torch.equal(t1, t2), "two launches give the same bits"
    perm = torch.tensor(np.random.default_rng(12).permutation(130), device=DEV)
    Up, tp = run(q[perm].contiguous(), g[perm].contiguous())
    assert torch.equal(Up, U1[perm]), "permuting the frames permutes U bit for bit"
    assert torch.equal(tp, t1), "... and leaves the parameter gradient unchanged bit for bit"
    # the value part does not depend on whether rho / dU_dtheta is kept
    with torch.no_grad():
        U0 = energy(q)
    for p in ps:
        p.requires_grad_(False)
    U3 = energy(q)
    assert not U3.requires_grad and torch.equal(U0, U1) and torch.equal(U3, U1)


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections(cu108):
    from mdgrad_amd.interface import PairPotentials, Stack, StillingerWeber, SuttonChen, Tersoff
    from mdgrad_amd.thermo import EAMEnergy
    case = cu108["force"]
    frames, cell = case.frames, case.cell
    system = mk_system(frames[0], cell)
    eps, a, c, n, m = CU
    for cls in (Stack, StillingerWeber, Tersoff, PairPotentials):
        with pytest.raises(NotImplementedError, match="got %s" % cls.__name__):
            EAMEnergy(system, cls.__new__(cls))
    tric = mk_system(frames[0], np.array([[10.83, 0, 0], [0.5, 10.83, 0], [0, 0, 10.83]]))
    with pytest.raises(ValueError, match="diagonal"):
        EAMEnergy(tric, SuttonChen(tric, eps, a, c, n, m, RC))
    big = mk_system(np.random.default_rng(0).uniform(0, 30.0, (1025, 3)), np.full(3, 30.0))
    with pytest.raises(ValueError, match="1024 atoms"):
        EAMEnergy(big, SuttonChen(big, eps, a, c, n, m, RC))
    for build in (_copper_sc(), _copper_table(64)):
        model = build(system)
        with pytest.raises(ValueError, match="built for 108 atoms per replica, the system holds 107"):
            EAMEnergy(mk_system(frames[0][:107], cell), model)
        with pytest.raises(ValueError, match="half the shortest cell length"):
            EAMEnergy(mk_system(np.mod(frames[0], 10.0), np.full(3, 10.0)), model)
        with pytest.raises(ValueError, match="k \\* 108"):
            EAMEnergy(system, model)(torch.zeros(3, 50, 3, device=DEV))


def test_c_entry_points_validate_their_arguments():
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its checks first
    cell, tric = _lib.make_cell([11.0, 11.0, 11.0]), _lib.make_cell([[11.0, 0, 0], [1.0, 11.0, 0], [0, 0, 11.0]])
    C = ctypes.byref(cell)

    def fails(rc, word):
        msg = lib.mdg_last_error()
        assert rc == -1 and word.encode() in msg, (rc, word, msg)

    # ---- K36
    def grids(**kw):
        b = ops.eam_table_consts(2, 64, 64, 1.8, 5.2, 1.0, 30.0)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    fw = lib.mdg_eam_table_frames_fwd
    fails(fw(None, 2, 8, C, p, grids(), p, -1, p, None, None), "null argument")
    fails(fw(p, 2, 8, None, p, grids(), p, -1, p, None, None), "null argument")
    fails(fw(p, 2, 8, C, p, None, p, -1, p, None, None), "null argument")
    fails(fw(p, 2, 8, C, None, grids(), p, -1, p, None, None), "types or tables")
    fails(fw(p, 2, 8, C, p, grids(), None, -1, p, None, None), "types or tables")
    fails(fw(p, 2, 8, C, p, grids(), p, -1, None, None, None), "null output U")
    fails(fw(p, 0, 8, C, p, grids(), p, -1, p, None, None), "empty")
    fails(fw(p, 2, 0, C, p, grids(), p, -1, p, None, None), "empty")
    fails(fw(p, 2, 1025, C, p, grids(), p, -1, p, None, None), "at most 1024 atoms")
    fails(fw(p, 1 << 24, 8, C, p, grids(), p, -1, p, None, None), "2^24 frames")
    fails(fw(p, 2, 8, ctypes.byref(tric), p, grids(), p, -1, p, None, None), "diagonal")
    fails(fw(p, 2, 8, C, p, grids(n_species=5), p, -1, p, None, None), "n_species")
    fails(fw(p, 2, 8, C, p, grids(n_species=0), p, -1, p, None, None), "n_species")
    fails(fw(p, 2, 8, C, p, grids(n_r=3), p, -1, p, None, None), "node counts")
    fails(fw(p, 2, 8, C, p, grids(n_rho=4097), p, -1, p, None, None), "node counts")
    fails(fw(p, 2, 8, C, p, grids(h_r=0.0), p, -1, p, None, None), "spacings")
    fails(fw(p, 2, 8, C, p, grids(h_rho=-1.0), p, -1, p, None, None), "spacings")
    fails(fw(p, 2, 8, C, p, grids(r_min=-0.1), p, -1, p, None, None), "r_min < rc")
    fails(fw(p, 2, 8, C, p, grids(rc=1.0), p, -1, p, None, None), "r_min < rc")
    fails(fw(p, 2, 8, C, p, grids(pin_cutoff=2), p, -1, p, None, None), "pin_cutoff")
    fails(fw(p, 2, 8, C, p, grids(), p, 2, p, None, None), "table_mode")
    fails(fw(p, 2, 8, C, p, grids(n_r=4096), p, 1, p, None, None), "table_mode 1 needs")
    bw = lib.mdg_eam_table_frames_nodes_bwd
    fails(bw(None, 2, 8, C, p, grids(), p, p, p, p, p, None), "null argument")
    fails(bw(p, 2, 8, C, p, grids(), p, None, p, p, p, None), "null input")
    fails(bw(p, 2, 8, C, p, grids(), p, p, None, p, p, None), "null input")
    fails(bw(p, 2, 8, C, p, grids(), p, p, p, None, p, None), "null output")
    fails(bw(p, 2, 8, C, p, grids(), p, p, p, p, None, None), "null output")
    fails(bw(p, 2, 1025, C, p, grids(), p, p, p, p, p, None), "at most 1024 atoms")
    fails(bw(p, 2, 8, ctypes.byref(tric), p, grids(), p, p, p, p, p, None), "diagonal")
    fails(bw(p, 2, 8, C, p, grids(n_rho=2), p, p, p, p, p, None), "node counts")

    # ---- K37
    def consts(**kw):
        b = ops.eam_consts(*CU, RC)
        for name, v in kw.items():
            setattr(b, name, v)
        return ctypes.byref(b)

    sc = lib.mdg_eam_frames_fwd
    fails(sc(None, 2, 8, C, consts(), p, p, None, None), "null argument")
    fails(sc(p, 2, 8, None, consts(), p, p, None, None), "null argument")
    fails(sc(p, 2, 8, C, None, p, p, None, None), "null argument")
    fails(sc(p, 2, 8, C, consts(), None, p, None, None), "theta is null")
    fails(sc(p, 2, 8, C, consts(), p, None, None, None), "null output")
    fails(sc(p, 0, 8, C, consts(), p, p, None, None), "empty")
    fails(sc(p, 2, 1025, C, consts(), p, p, None, None), "at most 1024 atoms")
    fails(sc(p, 2, 8, ctypes.byref(tric), consts(), p, p, None, None), "diagonal")
    fails(sc(p, 2, 8, C, consts(rc=0.0), p, p, None, None), "rc > 0")
    fails(sc(p, 2, 8, C, consts(n=17), p, p, None, None), "exponents")
    fails(sc(p, 2, 8, C, consts(m=9), p, p, None, None), "exponents")
    fails(sc(p, 2, 8, C, consts(m=0), p, p, None, None), "exponents")
    fails(sc(p, 2, 8, C, consts(shift=2), p, p, None, None), "shift")
    assert ops.EAM_FRAMES_MAX_ATOMS == 1024 and ops.eam_table_frames_lds_floats() == 8192
