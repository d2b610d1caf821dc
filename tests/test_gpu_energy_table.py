"""thermo.TabulatedEnergy on the GPU (csrc/energy_table.hip, ops.EnergyTableFn) against the float64 reference of
tests/energy_table_ref.py.

Error measure and rule of tests/test_gpu_energy_frames.py: |kernel - ref64| over the reference's scale (U: the sum over the
pairs of |phi~|; dU/dq: per atom and component the sum over the atom's pairs; dU/dnodes: per entry the sum of |basis|), the
largest over atoms / entries.  Allowed: MARGIN x floor, MARGIN = 10, floor = the float32 restatement of the formulas on the CPU
against float64, at least 2^-24 -- nothing comes from the kernel.  With an upstream gU per frame dL/dq[f] is compared with
gU_f dU_f/dq over |gU_f| x scale, and dL/dnodes with sum_f gU_f dU_f/dnodes over sum_f |gU_f| scale_f, the frames' floors weighted
the same way.

Tables carry independent noise on every node and slope (energy_table_ref.lj_energy_table): a wrong cell, swapped basis
functions or a lost 1 / du moves the result by the noise.  No fixture carries a fragile pair, asserted on the CPU before a kernel
runs; no case is left out.

With a module (pairMLP) the reference is the float64 module itself on the reference pair set, and the table's interpolation
error enters the bound: allowed = (number of pairs) x max |phi~ - phi| measured in float64 on a dense grid from the same float32
nodes, plus MARGIN x floor.  For the gradient with respect to the module parameters the same with dphi/dtheta_k in the place of
phi (the node gradient meets the Jacobian of the tabulation, so the kernel interpolates dphi/dtheta_k from its nodes) and the
floor of dU/dnodes carried through |Jacobian|.

(Every case prints floor, allowed and the kernel's figure per quantity; MDG_TEST_REPORT=<file> collects them.)"""
import copy

import numpy as np
import pytest
import torch

import energy_table_ref as ER
import pair_forms_ref as PF
from test_energy_frames_host import _report, frames_108, mk_system
from test_energy_table_host import interpolation_error, small_mlp
from test_gpu_pressure import liquid as sized_liquid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 10.0
CUT = 2.5


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run_gpu(xyz, cell, tab, u0, du, cutoff, mask, gU, positions=True, nodes=True):
    """(U, dL/dq or None, dL/dnodes or None, route, n_below) of L = sum_f gU_f U_f through ops.EnergyTableFn"""
    from mdgrad_amd import _lib, ops
    q = T(xyz).requires_grad_(positions)
    tb = T(tab).requires_grad_(nodes)
    mk = None if mask is None else T(np.asarray(mask, np.uint8))
    U = ops.EnergyTableFn.apply(q, tb, _lib.make_cell(np.asarray(cell, np.float64)), len(tab) // 2, u0, du, cutoff, mk)
    below = int(ops.EnergyTableFn.last_below)
    ops.EnergyTableFn.last_route = None
    want = ([q] if positions else []) + ([tb] if nodes else [])
    grads = list(torch.autograd.grad((U * T(np.asarray(gU, np.float32))).sum(), want))
    gq = grads.pop(0) if positions else None
    gT = grads.pop(0) if nodes else None
    return U.detach(), gq, gT, ops.EnergyTableFn.last_route, below


def reference_frames(xyz, cell, tab, u0, du, cutoff, mask=None):
    """per frame (float64 Result, floors, float32 Result); no frame may carry a fragile pair"""
    out = []
    for x in xyz:
        assert len(ER.fragile(x, cell, cutoff, mask)) == 0, "the fixture has a fragile pair at this cutoff"
        member = PF.membership(x, cell, [ER.carrier(cutoff, mask)])[0]
        ref = ER.evaluate(x, cell, tab, u0, du, cutoff, mask, member=member)
        r32 = ER.evaluate(x, cell, tab, u0, du, cutoff, mask, np.float32, member)
        out.append((ref, ER.floors(ref, r32), r32))
    return out


def check(what, out, refs, gU):
    U, gq, gT, _, below = out
    gU = np.asarray(gU, np.float64)
    figs = []
    for f, (ref, fl, _) in enumerate(refs):
        figs.append(("U[%d]" % f, PF.error(float(U[f]), ref, "U"), fl["U"]))
        if gq is not None and gU[f] != 0:
            figs.append(("dq[%d]" % f, PF.error(gq[f].cpu().numpy().astype(np.float64) / gU[f], ref, "dq"), fl["dq"]))
    if gT is not None:
        want = sum(gU[f] * ref.dT for f, (ref, _, _) in enumerate(refs))
        scale = sum(abs(gU[f]) * ref.sdT for f, (ref, _, _) in enumerate(refs))
        floor = sum(abs(gU[f]) * ref.sdT * fl["dT"] for f, (ref, fl, _) in enumerate(refs))            # absolute, per entry
        got = gT.cpu().numpy().astype(np.float64)
        live = scale > 0
        assert (got[~live] == 0).all(), "a node no pair touches must get an exact zero"
        k = int(np.argmax(np.abs(got - want)[live] / floor[live]))                                    # the worst entry by its own floor
        figs.append(("dnodes[%d]" % np.nonzero(live)[0][k], float((np.abs(got - want)[live] / scale[live])[k]),
                     float((floor[live] / scale[live])[k])))
        # ... and all entries together, every entry with its OWN floor (a pair that the float32 grid coordinate puts into the
        # neighbouring cell moves a few entries by a basis value; the entry-wise maximum above is then theirs alone)
        own = sum(abs(gU[f]) * np.maximum(np.abs(r32.dT - ref.dT), PF.EPS * ref.sdT) for f, (ref, _, r32) in enumerate(refs))
        figs.append(("dnodes sum", float(np.abs(got - want).sum() / scale.sum()), float(own.sum() / scale.sum())))
    assert below == sum(ref.n_below for ref, _, _ in refs)
    bad = []
    for q, v, floor in figs:
        allowed = MARGIN * floor
        _report("%-44s %-10s floor %.3e  allowed %.3e  kernel %.3e%s" % (what, q, floor, allowed, v, "" if v <= allowed else "   <-- FAILS"))
        if not v <= allowed:
            bad.append((q, v, allowed))
    assert not bad, "%s: %s" % (what, bad)


def clean_frames(n, frames, cutoff, mask=None):
    """`frames` frames of n atoms without a fragile pair, drawn as tests/test_gpu_energy_frames.py::test_sizes draws them"""
    if n <= 6:
        cell = np.array([4.0, 4.0, 4.0], dtype=np.float32)
        xyz = np.random.default_rng(n).uniform(1.2, 2.6, (frames + 9, n, 3)).astype(np.float32)
    else:
        xyz, cell = sized_liquid(n, seed=n, frames=frames + 9)
    clean = [x for x in xyz if len(ER.fragile(x, cell, cutoff, mask)) == 0][:frames]
    assert len(clean) == frames
    return np.stack(clean), cell


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n,frames,p", [(5, 5, 64), (6, 5, 64), (108, 5, 2048), (129, 3, 4096), (1100, 3, 257), (1331, 3, 2048)])
def test_sizes(n, frames, p):
    """A wave per frame with odd and even N (the k = N / 2 half shell) and a partly live last workgroup of four, the workload's
    108, a workgroup per frame just past the wave boundary (with 4 096 nodes: the 108 KB of LDS), tiles with an odd (5) and an
    even (6: the k = nb / 2 shell) number of blocks.  U, dL/dq and dL/dnodes with a random upstream gU, both routes."""
    if n == 108:
        fx, two = frames_108()
        xyz, cell = np.stack([two[k % 2] for k in range(frames)]), fx.cell
    else:
        xyz, cell = clean_frames(n, frames, min(CUT, 0.49 * (4.0 if n <= 6 else (n / 0.8) ** (1 / 3))))
    cutoff = min(CUT, 0.49 * float(cell[0]))
    u0, du = ER.grid(cutoff, p, 0.2)
    tab = ER.lj_energy_table(u0, du, p, seed=n, noise=0.04)
    refs = reference_frames(xyz[:2], cell, tab, u0, du, cutoff) * 3 if n == 108 else reference_frames(xyz, cell, tab, u0, du, cutoff)
    refs = refs[:frames]
    gU = np.random.default_rng(1).uniform(0.5, 1.5, frames).astype(np.float32) * np.where(np.arange(frames) % 2, -1, 1)
    full = run_gpu(xyz, cell, tab, u0, du, cutoff, None, gU)
    check("N=%d F=%d p=%d full rows" % (n, frames, p), full, refs, gU)
    only = run_gpu(xyz, cell, tab, u0, du, cutoff, None, gU, positions=False)
    check("N=%d F=%d p=%d nodes only" % (n, frames, p), only, refs, gU)
    assert full[3] == "full" and only[3] == "nodes" and torch.equal(only[0], full[0])
    assert torch.equal(only[2], full[2]), "both routes add the same integers per pair"


def test_masked():
    """an index_tuple plus ex_pairs selection at N = 108"""
    fx, two = frames_108()
    A, B = PF.species(108)
    mask = PF.select_mask(108, index_tuple=(A, B), ex_pairs=PF.excluded_list(108))
    p = 300
    u0, du = ER.grid(CUT, p, 0.2)
    tab = ER.lj_energy_table(u0, du, p, seed=9, noise=0.04)
    refs = reference_frames(two, fx.cell, tab, u0, du, CUT, mask)
    gU = [0.8, -1.3]
    full = run_gpu(two, fx.cell, tab, u0, du, CUT, mask, gU)
    check("masked full rows", full, refs, gU)
    only = run_gpu(two, fx.cell, tab, u0, du, CUT, mask, gU, positions=False)
    check("masked nodes only", only, refs, gU)
    free = run_gpu(two, fx.cell, tab, u0, du, CUT, None, gU, positions=False)
    assert not torch.equal(free[0], only[0])


def test_routes():
    """detached frames take the nodes-only sweep, frames that need a gradient the full rows; the node gradient is the same bits
    (both add fx64(gU_f scale basis) once per visit; the full rows visit twice and the final kernel halves)"""
    fx, two = frames_108()
    p = 512
    u0, du = ER.grid(CUT, p, 0.2)
    tab = ER.lj_energy_table(u0, du, p, seed=2, noise=0.04)
    gU = [1.7, -0.3]
    full = run_gpu(two, fx.cell, tab, u0, du, CUT, None, gU)
    only = run_gpu(two, fx.cell, tab, u0, du, CUT, None, gU, positions=False)
    rows = run_gpu(two, fx.cell, tab, u0, du, CUT, None, gU, nodes=False)
    assert (full[3], only[3], rows[3]) == ("full", "nodes", "full")
    assert torch.equal(full[2], only[2]) and torch.equal(full[1], rows[1]) and float(full[2].abs().max()) > 0


@pytest.mark.parametrize("n,frames,p", [(108, 7, 2048), (300, 4, 128), (1100, 2, 128)])
def test_bitwise_repeatable_and_frame_order(n, frames, p):
    """two launches give the same bits; permuting the frames (gU alike) permutes U bitwise and leaves dL/dnodes bitwise
    unchanged (integer sums); gU = 0 gives exact zeros"""
    if n == 108:
        fx, two = frames_108()
        rng = np.random.default_rng(3)
        xyz, cell = np.stack([two[k % 2] + rng.normal(0, 1e-3, two[0].shape).astype(np.float32) for k in range(frames)]), fx.cell
    else:
        xyz, cell = sized_liquid(n, seed=7, frames=frames)
    cutoff = min(CUT, 0.49 * float(cell[0]))
    u0, du = ER.grid(cutoff, p, 0.2)
    tab = ER.lj_energy_table(u0, du, p, seed=4, noise=0.04)
    gU = np.linspace(0.5, 1.5, frames).astype(np.float32)
    perm = np.random.default_rng(0).permutation(frames)
    for positions in (True, False):
        a = run_gpu(xyz, cell, tab, u0, du, cutoff, None, gU, positions)
        b = run_gpu(xyz, cell, tab, u0, du, cutoff, None, gU, positions)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and (not positions or torch.equal(a[1], b[1]))
        c = run_gpu(xyz[perm], cell, tab, u0, du, cutoff, None, gU[perm], positions)
        assert torch.equal(c[0], a[0][T(perm)]) and torch.equal(c[2], a[2]) and (not positions or torch.equal(c[1], a[1][T(perm)]))
        z = run_gpu(xyz, cell, tab, u0, du, cutoff, None, np.zeros(frames, np.float32), positions)
        assert torch.equal(z[2], torch.zeros_like(z[2])) and (not positions or torch.equal(z[1], torch.zeros_like(z[1])))


# ---------------------------------------------------------------------------------------------- the class
def test_range_rule():
    from mdgrad_amd.thermo import TabulatedEnergy
    fx = PF.liquid(108)
    x = fx.x.copy()
    x[1] = x[0] + np.float32([0.3, 0.0, 0.0])                   # r = 0.3 < 0.2 * 2.5
    assert len(ER.fragile(x, fx.cell, CUT)) == 0
    xyz = np.stack([fx.x, x])
    mlp = small_mlp()
    system = mk_system(fx.x, fx.cell, DEV)
    with pytest.raises(RuntimeError, match="r_min"):
        TabulatedEnergy.from_terms(system, [(mlp, CUT)], nodes=256)(T(xyz))
    obs = TabulatedEnergy.from_terms(system, [(mlp, CUT)], nodes=256, check_range=False)
    U = obs(T(xyz))
    u0, du, _ = obs.grid()
    tab = obs.tabulate().detach().cpu().numpy()
    refs = reference_frames(xyz, fx.cell, tab, u0, du, CUT)
    assert int(obs.last_below) == sum(r.n_below for r, _, _ in refs) == 1
    for f, (ref, fl, _) in enumerate(refs):
        err = PF.error(float(U[f].detach()), ref, "U")
        _report("range rule U[%d]  floor %.3e  allowed %.3e  kernel %.3e" % (f, fl["U"], MARGIN * fl["U"], err))
        assert err <= MARGIN * fl["U"]
    # the pair below the first node carries no force: atoms 0 and 1 get what the reference gives them
    q = T(xyz).requires_grad_(True)
    (gq,) = torch.autograd.grad(obs(q)[1], q)
    assert PF.error(gq[1].cpu().numpy(), refs[1][0], "dq") <= MARGIN * refs[1][1]["dq"]


class EndToEnd:
    """Stack(pairMLP + ExcludedVolume) on five frames of 108 atoms, and its float64 reference"""

    def __init__(self):
        from mdgrad_amd import potentials as P
        from mdgrad_amd.interface import PairPotentials, Stack
        from mdgrad_amd.thermo import TabulatedEnergy
        fx, two = frames_108()
        rng = np.random.default_rng(5)
        cand = [two[0], two[1]] + [(two[0] + rng.normal(0, 0.02, two[0].shape)).astype(np.float32) for _ in range(12)]
        self.cell = fx.cell
        self.xyz = np.stack([x for x in cand if len(ER.fragile(x, fx.cell, CUT)) == 0][:5])
        assert len(self.xyz) == 5
        self.system = mk_system(fx.x, fx.cell, DEV)
        self.mlp = small_mlp(seed=11).to(DEV)
        self.prior = P.ExcludedVolume(sigma=0.9, epsilon=1.0, power=12)
        for p_ in self.prior.parameters():
            p_.requires_grad_(False)
        self.model = Stack({"pairnn": PairPotentials(self.system, self.mlp, cutoff=CUT),
                            "pair": PairPotentials(self.system, self.prior, cutoff=CUT)})
        self.nodes = 512
        self.obs = TabulatedEnergy(self.system, self.model, nodes=self.nodes)
        self.u0, self.du, _ = self.obs.grid()
        self.q = T(self.xyz)
        # reference pair set and float64 distances per frame
        self.r = []
        for x in self.xyz:
            member = PF.membership(x, fx.cell, [ER.carrier(CUT)])[0]
            _, _, d2 = PF._images(x, fx.cell, np.dtype(np.float64))
            self.r.append(torch.as_tensor(np.sqrt(d2[np.triu(member, 1)])))
        self.prior_term = [PF.Term("exvol12", CUT, theta=(0.9, 1.0))]

    def mlp64(self):
        return copy.deepcopy(self.mlp).cpu().double()

    def reference(self, module64, gU=None):
        """float64: U_f of the modules on the reference pair set (module part, prior part), and d(sum_f gU_f U_f)/dtheta"""
        Um = torch.stack([module64(r[:, None]).sum() for r in self.r])
        Up = np.array([PF.evaluate(x, np.zeros_like(x), self.cell, self.prior_term).U for x in self.xyz])
        g = None
        if gU is not None:
            g = torch.autograd.grad((Um * torch.as_tensor(np.asarray(gU, np.float64))).sum(), list(module64.parameters()))
        return Um.detach().numpy(), Up, g

    def allowed_U(self, module64):
        """per frame: (number of pairs) x the interpolation error of this table + MARGIN x floor (tabulated and exact part)"""
        tab = self.obs.tabulate().detach().cpu().numpy()
        err, _ = interpolation_error(tab, self.u0, self.du, module64, CUT)
        out = []
        for x in self.xyz:
            ref, fl, _ = reference_frames([x], self.cell, tab, self.u0, self.du, CUT)[0]
            pr = PF.evaluate(x, np.zeros_like(x), self.cell, self.prior_term)
            flp = PF.floors(x, np.zeros_like(x), self.cell, self.prior_term, pr)["U"]
            out.append(ref.n_pairs * err + MARGIN * (fl["U"] * float(ref.sU) + flp * float(pr.sU)))
        return np.array(out), err

    def allowed_dtheta(self, gU):
        """per parameter entry: sum_f |gU_f| pairs_f x max_u |interpolated dphi/dtheta_k - dphi/dtheta_k| (the float32 Jacobian of
        the tabulation on the CPU against float64 autograd on a dense grid) + MARGIN x the floor of dL/dnodes through |Jacobian|"""
        from mdgrad_amd.thermo import TabulatedEnergy
        gU = np.abs(np.asarray(gU, np.float64))
        key = tuple(float(p_.detach().double().sum()) for p_ in self.mlp.parameters())
        if getattr(self, "_dth", (None,))[0] != key:
            self._dth = (key,) + self._dtheta_parts()
        _, E, J, frames = self._dth
        pairs = sum(g * n for g, (n, _) in zip(gU, frames))
        node_floor = sum(g * fl for g, (_, fl) in zip(gU, frames))
        return pairs * E + MARGIN * (np.abs(J) * node_floor[:, None]).sum(0)

    def _dtheta_parts(self):
        from mdgrad_amd.thermo import TabulatedEnergy
        m32, m64 = copy.deepcopy(self.mlp).cpu(), self.mlp64()
        host = TabulatedEnergy.from_terms(mk_system(self.xyz[0], self.cell), [(m32, CUT)], nodes=self.nodes)
        tab = host.tabulate()
        ps = list(m32.parameters())
        J = [torch.autograd.grad(tab[k], ps, retain_graph=True, allow_unused=True) for k in range(2 * self.nodes)]
        J = np.stack([np.concatenate([(torch.zeros_like(p_) if g is None else g).reshape(-1).numpy() for g, p_ in zip(row, ps)])
                      for row in J]).astype(np.float64)                                              # [2 p, P]
        u = self.u0 + self.du * (np.arange((self.nodes - 1) * 2 + 1, dtype=np.float64) / 2)
        u = u[u < CUT * CUT]
        g_, b, _ = ER.basis(u, self.u0, self.du, self.nodes, np.dtype(np.float64))
        interp = sum(b[k][:, None] * J[2 * g_ + k] for k in range(4))                                # [M, P]
        ps64 = list(m64.parameters())
        truth = []
        for uu in u:
            g = torch.autograd.grad(m64(torch.as_tensor([[np.sqrt(uu)]])).sum(), ps64, allow_unused=True)
            truth.append(np.concatenate([(torch.zeros_like(p_) if x is None else x).reshape(-1).numpy() for x, p_ in zip(g, ps64)]))
        E = np.abs(interp - np.stack(truth)).max(0)                                                  # [P]
        tabn = tab.detach().numpy()
        frames = []
        for x in self.xyz:
            ref, fl, _ = reference_frames([x], self.cell, tabn, self.u0, self.du, CUT)[0]
            frames.append((ref.n_pairs, ref.sdT * fl["dT"]))
        return E, J, frames

    def gpu_dtheta(self, gU):
        ps = list(self.mlp.parameters())
        U = self.obs(self.q)
        g = torch.autograd.grad((U * T(np.asarray(gU, np.float32))).sum(), ps, allow_unused=True)
        return np.concatenate([(torch.zeros_like(p_) if x is None else x).reshape(-1).cpu().numpy() for x, p_ in zip(g, ps)]).astype(np.float64)


_E2E = []


def e2e():
    if not _E2E:
        _E2E.append(EndToEnd())
    return _E2E[0]


def compare_dtheta(what, E, gU):
    from mdgrad_amd import ops
    got = E.gpu_dtheta(gU)
    assert ops.EnergyTableFn.last_route == "nodes"
    _, _, g = E.reference(E.mlp64(), gU)
    want = np.concatenate([x.reshape(-1).numpy() for x in g])
    allowed = E.allowed_dtheta(gU)
    err = np.abs(got - want)
    k = int(np.argmax(err - allowed))
    _report("%-40s dtheta: worst entry %d  |err| %.3e  allowed %.3e  (largest |dtheta| %.3e)" % (what, k, err[k], allowed[k], np.abs(want).max()))
    assert (err <= allowed).all() and np.abs(want).max() > 0


def test_end_to_end_with_a_module():
    E = e2e()
    m64 = E.mlp64()
    Um, Up, _ = E.reference(m64)
    allowed, ierr = E.allowed_U(m64)
    U = E.obs(E.q).detach().cpu().numpy().astype(np.float64)
    for f in range(5):
        err = abs(U[f] - (Um[f] + Up[f]))
        _report("end to end U[%d]: interpolation error %.3e  allowed %.3e  kernel %.3e" % (f, ierr, allowed[f], err))
        assert err <= allowed[f]
    # the class gives what the model gives frame by frame (its neighbour-list route evaluates the module per pair)
    E.model._reset_topology(E.q[0])
    assert abs(float(E.model(E.q[0])) - (Um[0] + Up[0])) <= allowed[0]
    compare_dtheta("end to end", E, [0.7, -1.1, 0.4, 1.3, -0.6])


def test_reweighting():
    from mdgrad_amd.observable import rdf
    from mdgrad_amd.reweight import Reweighting
    E = e2e()
    kT = 1.0
    state = copy.deepcopy(E.mlp.state_dict())
    try:
        rw = Reweighting(E.obs, kT, E.q)
        w0 = rw.weights()
        assert torch.equal(w0.detach(), torch.full_like(w0, 1.0 / 5)), "the weights at theta_ref are exactly 1 / F"
        # d <O> / d theta at theta_ref = the covariance identity: sum_f gU_f dU_f/dtheta, gU_f = -(O_f - <O>) / (F kT)
        obs = rdf(E.system, nbins=20, r_range=(0.75, 2.5))
        with torch.no_grad():
            rows = obs.per_frame(E.q)
        c = T(np.random.default_rng(2).standard_normal(rows.shape[-1]).astype(np.float32))
        O = (rows * c).sum(-1).double().cpu().numpy()
        gU = -(O - O.mean()) / (5 * kT)
        ps = list(E.mlp.parameters())
        g = torch.autograd.grad((rw.average(rows) * c).sum(), ps, allow_unused=True)
        got = np.concatenate([(torch.zeros_like(p_) if x is None else x).reshape(-1).cpu().numpy() for x, p_ in zip(g, ps)]).astype(np.float64)
        _, _, gr = E.reference(E.mlp64(), gU)
        want = np.concatenate([x.reshape(-1).numpy() for x in gr])
        # (rw.average rounds its float64 sum to the rows' float32: 2^-24 of |c . <rows>| through the same chain is far below)
        allowed = E.allowed_dtheta(gU)
        err = np.abs(got - want)
        k = int(np.argmax(err - allowed))
        _report("covariance identity: worst entry %d  |err| %.3e  allowed %.3e  (largest %.3e)" % (k, err[k], allowed[k], np.abs(want).max()))
        assert (err <= allowed).all() and np.abs(want).max() > 0
        # a small step of the MLP weights
        old64 = E.mlp64()
        a_old, _ = E.allowed_U(old64)
        with torch.no_grad():
            for p_ in E.mlp.parameters():
                p_.add_(0.01 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).to(DEV))
        new64 = E.mlp64()
        a_new, _ = E.allowed_U(new64)
        dU = E.reference(new64)[0] - E.reference(old64)[0]                 # (the exact prior cancels bit for bit)
        lw_ref = -dU / kT - np.log(np.exp(-dU / kT).sum())
        lw = torch.log(rw.weights().detach()).cpu().numpy()
        tol = 2 * float((a_old + a_new).max()) / kT
        _report("reweighting ln w: max |err| %.3e  allowed %.3e  (spread of ln w %.3e)" % (np.abs(lw - lw_ref).max(), tol, np.ptp(lw_ref)))
        assert np.abs(lw - lw_ref).max() <= tol and np.ptp(lw_ref) > 0
    finally:
        E.mlp.load_state_dict(state)


def test_refusals_on_the_device():
    from mdgrad_amd import potentials as P
    from mdgrad_amd.interface import GNNPotentials, PairPotentials, Stack, TPairPotentials
    from mdgrad_amd.nn import get_model
    from mdgrad_amd.thermo import TabulatedEnergy
    fx, two = frames_108()
    system = mk_system(fx.x, fx.cell, DEV)
    mlp = PairPotentials(system, small_mlp(), cutoff=CUT)
    gnn = GNNPotentials(system, get_model({"n_atom_basis": 16, "n_filters": 16, "n_gaussians": 8, "n_convolutions": 1,
                                           "cutoff": 2.5}), cutoff=2.5)
    with pytest.raises(NotImplementedError, match="GNN, bonded, many-body and charge"):
        TabulatedEnergy(system, Stack({"pair": mlp, "gnn": gnn}))
    tmlp = P.TpairMLP(n_gauss=8, r_start=0.3, r_end=2.5, n_layers=1, n_width=8, nonlinear="ELU")
    with pytest.raises(NotImplementedError, match="TpairMLP"):
        TabulatedEnergy(system, TPairPotentials(system, tmlp, T=1.0, cutoff=CUT))
    with pytest.raises(NotImplementedError, match="PotentialEnergy"):
        TabulatedEnergy(system, PairPotentials(system, P.LennardJones(1.0, 1.0), cutoff=CUT))
    obs = TabulatedEnergy(system, mlp, nodes=128)
    q = T(two).requires_grad_(True)
    (gq,) = torch.autograd.grad(obs(q).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.pow(2).sum().backward()
    # float64 device positions take the torch restatement, not the kernels
    U64 = obs(T(two).double())
    assert U64.dtype == torch.float64 and torch.allclose(U64.float(), obs(T(two)), rtol=1e-5, atol=1e-5)


def test_example_runs():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fit_rdf_reweight_pairmlp.py")
    spec = importlib.util.spec_from_file_location("fit_rdf_reweight_pairmlp", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.main(["--replicas", "8", "--epochs", "2"])
    assert len(hist) == 2 and all(np.isfinite(h[0]) for h in hist)
