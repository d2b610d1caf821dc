"""The built-in pair forms of every trajectory kernel family and of pair_ell -- one evaluation per kernel variant -- against the
float64 reference of tests/pair_forms_ref.py (pinned on the CPU by tests/test_pair_forms_ref_host.py, which also checks every
fixture used here), and one short float64 trajectory check per family.

How one evaluation is read from a trajectory kernel (all NVE; the thermostat algebra has its own oracle tests)

  force     a two-frame launch with v0 = 0 and t = [0, 2^-20].  NVE has no 1/m: q1 = q0 + (v0 + F dt / 2) dt, v1 = v0 +
            F(q0) dt / 2 + F(q1) dt / 2.  Every coordinate is at least 0.25 in magnitude and |F| < 2^15, so the displacement is
            below half an ulp: q_t[:, 1] == q0 bitwise (asserted), and F = v_t[:, 1] 2^20 exactly.  The ring kernels also hand
            out f_t[:, 1] (mdg_traj_fwd_small_ft): the same bits (asserted).
  adjoint   stored frames 0 and 1 are the fixture, the stored velocity of frame 1 is -F / 2, g_v[:, 1] = w, nothing else
            incoming, t = [0, 1].  The backward branch of verlet_update (sovlers.py:42-101; the same lines in traj_small.hip,
            traj_ring.hpp and traj_large.hip -- "vhalf = v - 0.5 (-f) h", ":71", ":72", ":82,101") then evaluates at frame 1
            first: adj_v0 = w + dq / 2 and adj_theta = d(w.F)/dtheta of that evaluation alone; with v = -F / 2 its half-step
            velocity is zero, so the interval's second evaluation (which only feeds adj_q0, not read here) stays at the fixture
            instead of a point half a force away.  On the ring both adjoints run: the one that reads the forward's forces (_ft)
            and the one that rebuilds them; on the large path both the adjoint over the stored lists (block = 0) and the one
            that searches at every evaluation (block = -1).  Handing dq out as w + dq / 2 rounds it to the float32 grid of
            that sum: the measurement's own error, 2^-23 |w + dq / 2| per entry, is taken off before the comparison
            (pair_forms_ref.error, `slack`); pair_ell returns H.w directly and gets none.
  pair_ell  ops.pair_eval(ell, x, term, theta, w, energy, theta_grads): U, dU/dx = -F, H.w = -dq, dU/dtheta, -d(w.F)/dtheta.

Measure: |gpu - float64| / scale per atom and component (per entry for theta, over sum |phi| for U), scale = the sum of the
absolute summands (pair_forms_ref); an atom with scale 0 must hold exact zeros (the pair at exactly rc of `cutoff_pair`, atoms
of a species no term selects).  allowed = MARGIN x floor, MARGIN = 10 as for the bonded, pressure and RDF kernels (fused
multiply-adds, v_rsq_f32 and v_exp_f32 at 1 ulp where the CPU uses libm, another summation order); floor = the float32
restatement of the same formulas against float64 on the CPU, for that fixture, form and quantity, at least 2^-24.  Nothing
comes from the kernel under test.  Every case asserts its route first: mdg_traj_ring_taken, spec.large,
the forced block and the lanes per atom it implies (pick_tpa_log2 restated), the fused-image multiplier on the ring, inside or
outside the [-0.24, 1.24] window, that the large path kept its candidate lists (so the adjoint over them runs), and for
pair_ell the lanes per atom (pick_lpa restated, and the library's own workgroup count from mdg_pair_partial_size).

pair_ell_kernel<LPA, LEVEL>: LPA = 64 for every fixture below 4 096 atoms; 32, 16 and 8 run on 6 000, 9 000 and 18 000 atoms
that are exact periodic copies of a 500-atom fixture (pair_forms_ref.supercell), whose reference is the 500-atom one tiled;
every pair_ell case runs LEVEL 2, 1 and 0.

Cases the dispatch tables do not have (asserted as refusals, test_routes_the_ring_refuses): a masked term that is not of the LJ
family, and a stack whose members are not all LJ-family terms of one kind with at least one mask, do not run on the ring
(ring_form); they run on the workgroup kernels' generic loop, which is covered.  Morse has no parameters: its theta rows are empty.
The selection masks are symmetric by contract (ops.build_mask), so no supported input can show a transposed read of a mask;
test_one_sided_mask_is_read_from_the_row_of_the_atom_it_updates feeds the kernels that keep a row per atom one that is not.

Floors (CPU, tests/test_pair_forms_ref_host.py::test_print_the_float32_floors; liquid108 and, the smallest system, liquid2):

    form        liquid108: U   F        dq       dth      dU         liquid2: U   F        dq       dth      dU
    lj          6.0e-8   2.9e-6   2.4e-6   1.8e-7   8.0e-8           6.0e-8   2.3e-7   8.8e-7   6.3e-7   3.4e-7
    ljfam_8_4   1.3e-7   1.4e-6   1.6e-6   6.7e-8   6.0e-8           8.6e-8   2.2e-7   2.3e-6   1.2e-6   2.8e-7
    lj69        6.0e-8   2.4e-6   2.3e-6   1.4e-7   6.0e-8           6.0e-8   6.4e-7   3.5e-6   1.8e-6   6.7e-7
    exvol12     6.0e-8   1.6e-6   1.9e-6   9.4e-8   6.0e-8           6.9e-7   8.3e-7   8.2e-7   7.7e-7   6.9e-7
    exvol10     6.0e-8   1.5e-6   1.3e-6   6.0e-8   6.0e-8           2.3e-7   3.6e-7   3.6e-7   2.8e-7   2.1e-7
    morse_pos   6.0e-8   4.4e-7   9.4e-7   -        -                8.7e-8   1.1e-7   4.2e-7   -        -
    morse_neg   6.0e-8   4.1e-7   1.2e-6   -        -                1.2e-7   1.1e-7   3.0e-7   -        -
    buck        7.8e-8   4.1e-7   2.4e-7   6.0e-8   6.0e-8           4.0e-7   4.6e-7   5.0e-7   3.5e-7   3.8e-7
    yukawa      6.0e-8   2.0e-7   1.8e-7   6.0e-8   6.0e-8           6.7e-8   6.0e-8   6.0e-8   9.9e-8   6.0e-8

What the MI355X showed: every case within its allowance, the kernels at 0.0 .. 4.7 x the floor (allowed: 10); nothing had to
be fixed and no term had to be added to the floor model.  The largest multiples are where the floor is the bare 2^-24: Yukawa
on two atoms on the ring (F 3.2, dq 4.7), dU/dtheta of the LJ forms on pair_ell (3.0).  The largest kernel figure over the cases
of a family and form, in brackets as a multiple of that case's floor:

    lj                pair_ell           F 4.0e-06 (1.0)  dq 3.8e-06 (1.0)  dth 2.2e-07 (1.7)  U 1.1e-07 (1.9)  dU 1.9e-07 (3.0)
                      pair_ell<32|16|8>  F 1.6e-06 (0.8)  dq 1.7e-06 (1.0)  dth 3.2e-08 (0.5)  U 6.0e-08 (1.0)  dU 1.0e-07 (1.7)
                      workgroup          F 2.7e-06 (1.3)  dq 3.0e-06 (1.1)  dth 2.4e-07 (1.8)
                      ring               F 2.7e-06 (1.3)  dq 2.8e-06 (1.0)  dth 2.4e-07 (1.0)
                      large              F 4.2e-06 (0.9)  dq 3.8e-06 (1.0)  dth 2.2e-07 (1.8)
    ljfam_8_4         pair_ell           F 2.5e-06 (1.0)  dq 1.8e-06 (1.1)  dth 6.3e-08 (0.9)  U 6.6e-08 (0.9)  dU 1.1e-07 (1.8)
                      workgroup          F 1.3e-06 (0.9)  dq 1.7e-06 (1.1)  dth 1.2e-08 (0.2)
                      ring               F 1.8e-06 (1.3)  dq 1.8e-06 (1.1)  dth 1.1e-08 (0.2)
    lj69              pair_ell           F 2.2e-06 (0.9)  dq 2.2e-06 (1.0)  dth 6.4e-08 (1.0)  U 5.8e-08 (1.0)  dU 1.8e-07 (3.0)
                      workgroup          F 1.8e-06 (0.7)  dq 2.1e-06 (0.9)  dth 5.7e-08 (0.4)
                      ring               F 2.5e-06 (1.0)  dq 2.2e-06 (1.0)  dth 5.7e-08 (0.4)
    exvol12           pair_ell           F 2.3e-06 (1.2)  dq 2.0e-06 (1.0)  dth 7.0e-08 (0.7)  U 1.4e-07 (2.3)  dU 1.4e-07 (2.3)
                      workgroup          F 1.5e-06 (0.9)  dq 1.6e-06 (0.9)  dth 6.0e-08 (0.6)
                      ring               F 1.5e-06 (0.9)  dq 1.7e-06 (0.9)  dth 6.6e-08 (0.7)
    exvol10           pair_ell           F 1.7e-06 (1.0)  dq 1.3e-06 (1.0)  dth 3.0e-08 (0.4)  U 7.8e-08 (1.3)  dU 1.0e-07 (1.7)
                      workgroup          F 1.2e-06 (0.8)  dq 1.1e-06 (0.9)  dth 3.7e-08 (0.6)
                      ring               F 1.4e-06 (1.0)  dq 1.2e-06 (0.9)  dth 4.0e-08 (0.7)
    morse_pos         pair_ell           F 5.2e-07 (1.1)  dq 1.2e-06 (1.8)  U 4.4e-08 (0.7)
                      workgroup          F 4.4e-07 (1.0)  dq 7.3e-07 (0.8)
                      ring               F 6.7e-07 (0.9)  dq 9.4e-07 (1.0)
    morse_neg         pair_ell           F 8.1e-07 (1.0)  dq 2.3e-06 (0.9)  U 9.5e-08 (1.6)
                      pair_ell<32|16|8>  F 2.5e-07 (0.6)  dq 7.2e-07 (0.9)  U 9.3e-08 (1.6)
                      workgroup          F 7.5e-07 (1.7)  dq 1.7e-06 (2.7)
                      ring               F 7.5e-07 (0.8)  dq 1.3e-06 (1.1)
                      large              F 8.1e-07 (1.0)  dq 2.3e-06 (1.2)
    buck              pair_ell           F 3.9e-07 (1.0)  dq 3.0e-07 (1.0)  dth 5.8e-08 (0.7)  U 7.6e-08 (1.1)  dU 1.0e-07 (1.7)
                      workgroup          F 4.3e-07 (0.7)  dq 3.0e-07 (1.1)  dth 3.3e-08 (0.6)
                      ring               F 3.6e-07 (0.9)  dq 3.1e-07 (1.2)  dth 2.4e-08 (0.4)
    yukawa            pair_ell           F 2.4e-07 (0.8)  dq 2.8e-07 (1.7)  dth 1.0e-08 (0.2)  U 3.1e-08 (0.5)  dU 4.1e-08 (0.7)
                      pair_ell<32|16|8>  F 1.0e-07 (0.5)  dq 1.5e-07 (0.8)  dth 2.0e-09 (0.0)  U 2.4e-09 (0.0)  dU 2.4e-08 (0.4)
                      workgroup          F 2.6e-07 (1.0)  dq 2.5e-07 (1.1)  dth 1.5e-08 (0.2)
                      ring               F 2.5e-07 (3.2)  dq 2.8e-07 (4.7)  dth 2.2e-07 (2.2)
                      large              F 3.1e-07 (1.0)  dq 2.9e-07 (1.2)  dth 1.1e-08 (0.2)
    two_species       pair_ell           F 3.4e-06 (1.0)  dq 2.3e-06 (0.9)  dth 1.9e-07 (0.9)  U 5.9e-08 (1.0)  dU 1.6e-07 (1.0)
                      workgroup          F 3.4e-06 (1.0)  dq 2.3e-06 (0.9)  dth 1.9e-07 (0.9)
                      ring               F 2.9e-06 (0.9)  dq 2.5e-06 (1.0)  dth 2.1e-07 (0.9)
    excluded_pairs    pair_ell           F 1.3e-06 (0.8)  dq 1.9e-06 (1.2)  dth 1.5e-08 (0.2)  U 2.4e-08 (0.4)  dU 5.0e-08 (0.8)
                      workgroup          F 1.4e-06 (0.9)  dq 1.7e-06 (1.1)  dth 2.5e-08 (0.4)
                      ring               F 1.8e-06 (1.2)  dq 1.8e-06 (1.1)  dth 2.4e-08 (0.4)
    excluded_pairs_lj ring               F 2.9e-06 (1.0)  dq 2.4e-06 (1.0)  dth 9.8e-08 (0.5)
    three_term        workgroup          F 2.3e-06 (1.0)  dq 3.1e-06 (1.0)  dth 1.2e-07 (0.6)
                      ring               F 2.4e-06 (1.0)  dq 2.6e-06 (0.8)  dth 1.9e-07 (0.8)
                      large              F 1.8e-06 (0.8)  dq 3.0e-06 (0.9)  dth 3.8e-07 (1.5)
    three_term_ljfam  ring               F 1.2e-06 (0.9)  dq 1.9e-06 (1.1)  dth 4.0e-08 (0.4)
    two_term          workgroup          F 1.3e-06 (0.8)  dq 1.5e-06 (0.8)  dth 7.7e-08 (0.6)
                      ring               F 1.5e-06 (0.9)  dq 1.5e-06 (0.8)  dth 6.8e-08 (0.6)
    two_cutoffs       workgroup          F 1.9e-06 (1.0)  dq 2.8e-06 (0.9)  dth 1.2e-07 (1.3)
                      ring               F 2.6e-06 (1.4)  dq 2.5e-06 (0.8)  dth 2.2e-07 (0.9)
                      large              F 4.4e-06 (1.0)  dq 4.4e-06 (0.9)  dth 1.9e-08 (0.3)
    one_sided         pair_ell           F 2.1e-06 (0.7)  dq 2.2e-06 (0.9)
                      workgroup          F 2.3e-06 (0.8)  dq 2.3e-06 (0.9)
                      large              F 2.0e-06 (0.7)  dq 2.3e-06 (0.9)

    short trajectories (test_short_trajectory_and_adjoint_vs_float64_oracle): every quantity within 0.1 .. 1.6 x the
    difference between the float32 and the float64 oracle of the same run (allowed: 10), e.g. dtheta, T = 4, NVE: workgroup /
    Buckingham 4.5e-10 against 3.0e-8, ring / masked LJFamily 2.3e-7 against 2.3e-7, large / Yukawa 8.7e-11 against 2.6e-10.

(Every case prints floor, allowed and the kernel's figure per quantity; MDG_TEST_REPORT=<file> collects them.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle as O
import pair_forms_ref as R
from test_gpu_parity import T, mk_system, DEV

pytestmark = pytest.mark.gpu
MARGIN = 10.0
DT = 2.0 ** -20
EDGE_FORMS = ("lj", "morse_neg", "yukawa")


def _report(line):
    print(line)
    if os.environ.get("MDG_TEST_REPORT"):
        with open(os.environ["MDG_TEST_REPORT"], "a") as fh:
            fh.write(line + "\n")


# ------------------------------------------------------------------------------------------------ fixtures and references
def fixture(name):
    if name.startswith("liquid"):
        n, _, cell = name[6:].partition("@")
        return R.liquid(int(n), float(cell) if cell else None)
    return {"contact": R.contact, "cutoff_pair": R.cutoff_pair, "unwrapped": R.unwrapped, "triclinic": R.triclinic,
            "base500": R.base500}[name]()


def members_of(what, n):
    """a form name -> one unmasked term with cutoff 2.5; a stack name of pair_forms_ref.stack -> its members"""
    return [(what, None, 2.5, None)] if what in R.FORMS else R.stack(what, n)


_REF = {}


def reference(fx_name, what):
    """(fixture, members, terms, w, Result64, floors): computed once per fixture and term list"""
    key = (fx_name, what)
    if key not in _REF:
        fx = fixture(fx_name)
        n = len(fx.x)
        members = members_of(what, n)
        terms = R.terms_of(members, n)
        w = R.direction(n)
        ref, fl, _ = R.reference(fx, terms, w)
        _REF[key] = (fx, members, terms, w, ref, fl)
    return _REF[key]


def judge(case, ref, fl, got, slack=None):
    """got: {quantity: array or list of arrays}; prints and collects every figure, then asserts them all"""
    bad = []
    for q, v in got.items():
        fig = R.error(v, ref, q, slack if q == "dq" else None)
        allowed = MARGIN * fl[q]
        _report("%-52s %-4s floor %.3e  allowed %.3e  kernel %.3e%s" % (case, q, fl[q], allowed, fig,
                                                                      "" if fig <= allowed else "   <-- FAILS"))
        assert np.isfinite(R._flat(v)).all(), (case, q)
        if not fig <= allowed:
            bad.append((q, fig, allowed))
    assert not bad, "%s: %s" % (case, bad)


# ------------------------------------------------------------------------------------------------ the trajectory kernels
def pick_tpa_log2(n_atoms, block):
    """lanes per atom of the workgroup kernels, as csrc/traj_small.hip: the largest 2^l <= 64 with n_atoms 2^l <= block (a
    restatement: the cases with a "tpa" expectation say which width they mean to hit; it does not follow the library if its
    rule changes)"""
    lg = 0
    while lg < 6 and (n_atoms << (lg + 1)) <= block:
        lg += 1
    return lg


def integrator(fx, members, large):
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE
    system = mk_system(fx.x, fx.cell)
    mods = []
    for form, theta, rc, sel in members:
        kw = {}
        if sel is not None:
            kw = {k: (torch.as_tensor(np.asarray(v)) if k == "ex_pairs" else v) for k, v in sel.items()}
        mods.append(PairPotentials(system, R.module(form, theta), cutoff=rc, **kw))
    integ = NVE(Stack({"t%d" % k: m for k, m in enumerate(mods)}), system).to(DEV)
    integ.fused_large = bool(large)
    return integ


def route(spec, family, block, n_rep=2):
    """forces the block and asserts the family the launch will take; returns (ring taken, lib)"""
    from mdgrad_amd import _lib
    lib = _lib.load()
    assert spec is not None, "fused_spec refused the case"
    assert bool(spec.large) == (family == "large")
    if spec.large:
        return False, lib
    spec.block = block
    prm = spec.params(n_rep, 2)
    ring = bool(lib.mdg_traj_ring_taken(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)))
    assert ring == (family == "ring"), "ring taken: %s" % ring
    assert (block == 64) == (family == "ring")
    return ring, lib


def one_evaluation(spec, lib, ring, x, ws_):
    """F [R, N, 3] and, per adjoint variant, (dq [R, N, 3], adj_theta [R, K], adj_v0) of one evaluation at x with the
    directions ws_ [R, N, 3] (see the module docstring)"""
    from mdgrad_amd import _lib
    P, ptr, st = C.byref, _lib.ptr, _lib.stream_ptr(DEV)
    n_rep, n = len(ws_), spec.n_atoms
    prm, cs, terms = spec.params(n_rep, 2), spec.cell_struct, spec.terms
    theta = spec.flat_params().detach().contiguous()
    th = ptr(theta) if theta.numel() else None
    q0 = T(np.broadcast_to(x, (n_rep,) + x.shape).copy(), DEV).contiguous()
    v0 = torch.zeros_like(q0)
    shape = (n_rep, 2, n, 3)
    v_t, q_t = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    f_t = torch.zeros(shape, device=DEV) if ring else None
    t_fwd = torch.tensor([0.0, DT], device=DEV)
    head = (P(prm), P(cs), P(terms), th, ptr(spec.mass))
    if spec.large:
        ws = torch.empty(int(lib.mdg_traj_large_workspace(n_rep, n, 2, spec.n_theta_total)), device=DEV)
        flags = torch.zeros(8, dtype=torch.int32, device=DEV)
        _lib.check(lib.mdg_traj_fwd_large(*head, ptr(t_fwd), ptr(v0), ptr(q0), None, ptr(v_t), ptr(q_t), None, ptr(ws), ptr(flags),
                                          st), "fwd_large")
        fl = flags.tolist()
        assert fl[0] == 0 and fl[1] == 0 and fl[3] == 0, fl
        assert not fl[4], "a candidate row overflowed: the adjoint over the stored lists (large_adj_listed) would not run"
        builds = torch.empty(n_rep, 2, dtype=torch.int32, device=DEV)
        rc = lib.mdg_traj_large_list_builds(ptr(ws), n_rep, n, 2, spec.n_theta_total, ptr(builds), st)
        builds = builds.tolist() if rc == 0 else None
    else:
        bad = torch.zeros(n_rep, dtype=torch.int32, device=DEV)
        _lib.check(lib.mdg_traj_fwd_small_ft(*head, ptr(t_fwd), ptr(v0), ptr(q0), None, ptr(v_t), ptr(q_t), None, ptr(f_t), ptr(bad),
                                             st), "fwd_small_ft")
        assert int(bad.abs().sum()) == 0
        builds = None
    torch.cuda.synchronize()
    assert torch.equal(q_t[:, 0], q0) and torch.equal(q_t[:, 1], q0), "the atoms moved: F is not v_t 2^20"
    F = v_t[:, 1] * (1.0 / DT)
    assert float(F.abs().max()) < 2.0 ** 15
    if ring:
        assert torch.equal(f_t[:, 1], F), "f_t[:, 1] and the velocity reading differ"
    # ---- the adjoint of one interval of length 1 from frame 1
    w = T(ws_, DEV).contiguous()
    g_v = torch.zeros(shape, device=DEV)
    g_v[:, 1] = w
    g_q = torch.zeros(shape, device=DEV)
    v_s = torch.zeros(shape, device=DEV)
    v_s[:, 1] = -0.5 * F
    t_adj = torch.tensor([0.0, 1.0], device=DEV)
    out = {}

    def adjoint(name, call):
        adj_v0, adj_q0 = torch.empty(n_rep, n, 3, device=DEV), torch.empty(n_rep, n, 3, device=DEV)
        adj_th = torch.zeros(n_rep, max(spec.n_theta_total, 1), device=DEV)
        call(adj_v0, adj_q0, adj_th)
        torch.cuda.synchronize()
        a64 = adj_v0.cpu().numpy().astype(np.float64)
        out[name] = (2.0 * (a64 - ws_.astype(np.float64)), adj_th.cpu().numpy().astype(np.float64), a64)

    if spec.large:
        for name, blk in (("listed", 0), ("search", -1)):
            pl = type(prm).from_buffer_copy(prm)
            pl.block = blk

            def call(av, aq, ath, pl=pl):
                flags = torch.zeros(8, dtype=torch.int32, device=DEV)
                _lib.check(lib.mdg_traj_adj_large(P(pl), P(cs), P(terms), th, ptr(spec.mass), ptr(t_adj), ptr(v_s), ptr(q_t), None,
                                                  ptr(g_v), ptr(g_q), None, ptr(av), ptr(aq), None, ptr(ath), ptr(ws), ptr(flags),
                                                  st), "adj_large")
                f = flags.tolist()
                assert f[0] == 0 and f[1] == 0 and (pl.block == -1 or f[5] == 0), f
            adjoint(name, call)
    else:
        for name, ft in ((("ft", f_t), ("rebuild", None)) if ring else (("plain", None),)):
            def call(av, aq, ath, ft=ft):
                _lib.check(lib.mdg_traj_adj_small_ft(*head, ptr(t_adj), ptr(v_s), ptr(q_t), None, ptr(ft), ptr(g_v), ptr(g_q), None,
                                                     ptr(av), ptr(aq), None, ptr(ath), st), "adj_small_ft")
            adjoint(name, call)
    return F.cpu().numpy().astype(np.float64), out, builds


def _window(fx):
    s = fx.x @ np.linalg.inv(np.asarray(fx.cell, np.float64)) if fx.cell.ndim == 2 else fx.x / fx.cell
    return bool(s.min() > -0.24 and s.max() < 1.24)


def run_trajectory_case(family, block, fx_name, what, expect=None):
    expect = expect or {}
    fx, members, terms, w, ref, fl = reference(fx_name, what)
    n = len(fx.x)
    case = "%s/%s %s %s" % (family, block, fx_name, what)
    integ = integrator(fx, members, family == "large")
    spec = integ.fused_spec("verlet")
    ring, lib = route(spec, family, block)
    if fx_name != "triclinic":
        assert _window(fx) == (fx_name != "unwrapped"), "window"
    assert bool(spec.cell_struct.diag) == (fx_name != "triclinic")
    if family == "workgroup":
        assert pick_tpa_log2(n, block) == expect.get("tpa", pick_tpa_log2(n, block)), pick_tpa_log2(n, block)
    if "fused_image" in expect:
        prm = spec.params(2, 2)
        fused = bool(lib.mdg_traj_ring_fused_image(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)))
        assert fused == expect["fused_image"], fused
    ws_ = np.stack([w, -2.0 * w]).astype(np.float32)            # (replica 1: the same evaluation, scaled exactly)
    F, adj, builds = one_evaluation(spec, lib, ring, fx.x, ws_)
    if "reuse" in expect:
        assert builds is not None and all(row == [0, 0] for row in builds), "the second evaluation did not reuse the list: %s" % builds
    assert np.array_equal(F[0], F[1]), "two replicas of one configuration differ"
    judge(case, ref, fl, {"F": F[0]})
    offs = [(spec.terms.t[k].theta_off, spec.terms.t[k].n_theta) for k in range(len(terms))]
    assert [c for _, c in offs] == [t.n_theta for t in terms]
    for name, (dq, ath, a64) in adj.items():
        for r, s in ((0, 1.0), (1, -2.0)):
            got = {"dq": dq[r] / s, "dth": [ath[r, o:o + c] / s for o, c in offs]}
            judge("%s [%s adjoint, replica %d]" % (case, name, r), ref, fl, got, slack=2.0 ** -23 * np.abs(a64[r] / s))
    return spec


WORKGROUP = (
    [(256, "liquid108", f, {"tpa": 1}) for f in R.FORMS] +
    [(128, "liquid108", "lj", {"tpa": 0}), (128, "liquid107", "lj", {"tpa": 0}), (128, "unwrapped", "lj", {"tpa": 0}),
     (256, "liquid130", "lj", {"tpa": 0}), (256, "liquid131", "lj", {"tpa": 0}), (256, "liquid256", "lj", {"tpa": 0}),
     (1024, "liquid256", "lj", {"tpa": 2}), (256, "liquid131", "buck", {"tpa": 0}), (1024, "liquid131", "yukawa", {"tpa": 2})] +
    [(1024, "liquid%d" % n, f, {"tpa": t}) for n, t in ((2, 6), (3, 6), (31, 5)) for f in ("lj", "morse_neg")] +
    [(b, "liquid108", s, {}) for b in (128, 256) for s in ("two_species", "excluded_pairs", "three_term", "two_term",
                                                          "two_cutoffs")] +
    [(256, "liquid107", "three_term", {}), (256, "triclinic", "lj", {}), (256, "triclinic", "yukawa", {}),
     (128, "triclinic", "two_cutoffs", {})] +
    [(256, fxn, f, {}) for fxn in ("contact", "cutoff_pair") for f in EDGE_FORMS] + [(256, "contact", "buck", {})])


@pytest.mark.parametrize("block,fx_name,what,expect", WORKGROUP, ids=["%d-%s-%s" % c[:3] for c in WORKGROUP])
def test_workgroup_kernels_one_evaluation(block, fx_name, what, expect):
    """the one-workgroup-per-replica kernels: every form at N = 108; LJ 12-6 packed with the near image (108), the clamped
    image (107: odd; unwrapped), LD = N (130, 131, 256); a non-LJ form at 131; 64, 64 and 32 lanes per atom (N = 2, 3, 31 at
    block 1024); the generic multi-term loop with masks, three terms and two cutoffs; the triclinic cell; the edge fixtures."""
    run_trajectory_case("workgroup", block, fx_name, what, expect)


RING = (
    [("liquid%d" % n, f, {}) for n in (108, 107) for f in R.FORMS] +
    [("liquid%d" % n, f, {}) for n in (2, 3, 31, 54) for f in ("lj", "yukawa")] +
    [("liquid108", "lj", {"fused_image": True}), ("liquid108@6.4", "lj", {"fused_image": False}), ("unwrapped", "lj", {}),
     ("liquid108@6.4", "buck", {}), ("unwrapped", "morse_pos", {})] +
    [("liquid%d" % n, s, {}) for n in (108, 107) for s in ("two_species", "excluded_pairs", "excluded_pairs_lj", "three_term",
                                                          "three_term_ljfam",
                                                          "two_term", "two_cutoffs")] +
    [(fxn, f, {}) for fxn in ("contact", "cutoff_pair") for f in EDGE_FORMS])
RING = list(dict.fromkeys((a, b, tuple(sorted(c.items()))) for a, b, c in RING))


@pytest.mark.parametrize("fx_name,what,expect", RING, ids=["%s-%s%s" % (c[0], c[1], "-image" if c[2] else "") for c in RING])
def test_ring_kernels_one_evaluation(fx_name, what, expect):
    """the wave-per-replica kernels (block = 64): every form at N = 108 and 107; LJ 12-6 and a pair_eval form at N = 2, 3, 31,
    54; the full sweep with the fused image (4.8), the window sweep (6.4: no multiplier), the clamped sweep (unwrapped); a
    masked term of LJ 12-6 and of the LJ family; two and three terms, also with cutoffs 2.5 and 1.8; the edge fixtures."""
    run_trajectory_case("ring", 64, fx_name, what, dict(expect))


LARGE = ([("liquid108", f, {}) for f in EDGE_FORMS] + [("liquid1000", f, {"reuse": True}) for f in EDGE_FORMS] +
         [("liquid1000", "two_cutoffs", {"reuse": True}), ("liquid108", "three_term", {}), ("triclinic", "lj", {}),
          ("triclinic", "morse_neg", {})] +
         [(fxn, f, {}) for fxn in ("contact", "cutoff_pair") for f in EDGE_FORMS])


@pytest.mark.parametrize("fx_name,what,expect", LARGE, ids=["%s-%s" % c[:2] for c in LARGE])
def test_large_path_kernels_one_evaluation(fx_name, what, expect):
    """the multi-launch kernels (fused_large): the all-atom scan at N = 108, the binned search and -- second evaluation of
    the forward, adjoint over the stored lists -- the listed kernels at N = 1 000, a masked two-term stack there, the
    triclinic cell, the edge fixtures; each adjoint both over the stored lists and with fresh searches."""
    spec = run_trajectory_case("large", 0, fx_name, what, expect)
    assert spec.large


def test_routes_the_ring_refuses():
    """what MDG_RING_LAUNCH / ring_form do not have: a masked term outside the LJ family, a stack with a member outside it, an
    unmasked stack, the triclinic cell -- the launch goes to the workgroup kernels (whose generic loop is covered above)"""
    from mdgrad_amd import _lib
    lib = _lib.load()
    n = 108
    A, B = R.species(n)
    sel = dict(index_tuple=(A, B))
    for fx_name, members in (("liquid108", [("yukawa", None, 2.5, sel)]), ("liquid108", [("morse_neg", None, 2.5, sel)]),
                             ("liquid108", [("buck", None, 2.5, dict(ex_pairs=R.excluded_list(n)))]),
                             ("liquid108", [("lj", None, 2.5, sel), ("yukawa", None, 2.5, None)]),
                             ("liquid108", [("lj", None, 2.5, sel), ("ljfam_8_4", None, 2.5, None)]),
                             ("liquid108", [("lj", None, 2.5, None), ("lj", (0.9, 0.8), 1.8, None)]),
                             ("triclinic", [("lj", None, 2.5, None)])):
        spec = integrator(fixture(fx_name), members, False).fused_spec("verlet")
        assert spec is not None and not spec.large
        spec.block = 64
        prm = spec.params(2, 2)
        assert not lib.mdg_traj_ring_taken(C.byref(prm), C.byref(spec.cell_struct), C.byref(spec.terms)), (fx_name, members)


# ------------------------------------------------------------------------------------------------ pair_ell
def pick_lpa(n_atoms):
    """lanes per atom of pair_ell_kernel<LPA, LEVEL>, as csrc/pair_ell.hip states the rule: 64, halved while n_atoms lpa / 2
    reaches 131 072 -- 64 below 4 096 atoms, 32 below 8 192, 16 below 16 384, 8 from there (a restatement: it says which
    instantiation a case means to hit and does not follow the library if its rule changes)"""
    lpa = 64
    while lpa > 8 and n_atoms * lpa // 2 >= 131072:
        lpa //= 2
    return lpa


def pair_ell_case(case, fx, member_counts, form, theta, rc, sel, n_theta, w, ref, fl, lpa):
    """LEVEL 2 (w given: U, dU/dx, H.w and both theta sums), LEVEL 1 (no w: U, dU/dx, dU/dtheta) and LEVEL 0 (U alone) of
    pair_ell_kernel<lpa, LEVEL> on one neighbour list"""
    from mdgrad_amd import _lib, ops
    n = len(fx.x)
    assert pick_lpa(n) == lpa, "the case runs pair_ell_kernel<%d, .>, not <%d, .>" % (pick_lpa(n), lpa)
    # ... and the library's own launch geometry: its partial sums are per workgroup of 256 / lpa atoms (mdg_pair_partial_size)
    size = _lib.load().mdg_pair_partial_size
    assert int(size(n)) == int(size(1)) * ((n + 256 // lpa - 1) // (256 // lpa)), "the library takes another lanes-per-atom"
    mod = R.module(form, theta)
    mask = ops.build_mask(n, device=DEV, **sel) if sel is not None else None
    x = T(fx.x, DEV)
    pr = [p.detach().reshape(-1) for p in mod.mdg_params()]
    th = torch.cat(pr).to(DEV) if pr else None
    term = ops.make_term(mod.mdg_term(), rc, 0, n_theta, mask)
    ell = ops.build_ell(x, _lib.make_cell(fx.cell), rc, mask=mask)
    assert ell.cnt.cpu().numpy().tolist() == list(member_counts), "the neighbour list is not the reference's pair set"
    f64 = lambda v: v.cpu().numpy().astype(np.float64)             # noqa: E731
    o = ops.pair_eval(ell, x, term, th, w=T(w, DEV), energy=True, theta_grads=True)
    got = {"U": f64(o["energy"]).reshape(()), "F": -f64(o["grad"]), "dq": -f64(o["hw"])}
    if n_theta:
        got["dth"], got["dU"] = [-f64(o["gtheta_w"])], [f64(o["gtheta"])]
    else:
        assert o["gtheta"] is None and o["gtheta_w"] is None
    judge(case + " [level 2]", ref, fl, got)
    o = ops.pair_eval(ell, x, term, th, w=None, energy=True, theta_grads=True)
    assert o["hw"] is None
    got = {"U": f64(o["energy"]).reshape(()), "F": -f64(o["grad"])}
    if n_theta:
        got["dU"] = [f64(o["gtheta"])]
    judge(case + " [level 1]", ref, fl, got)
    o = ops.pair_eval(ell, x, term, th, w=None, energy=True, grad=False)
    assert o["grad"] is None and o["gtheta"] is None
    judge(case + " [level 0]", ref, fl, {"U": f64(o["energy"]).reshape(())})


PAIR_ELL = ([(fxn, f) for fxn in ("liquid108", "contact", "cutoff_pair") for f in R.FORMS] +
            [("liquid1000", f) for f in EDGE_FORMS] +
            [("liquid108", "two_species"), ("liquid107", "excluded_pairs"), ("triclinic", "lj"), ("unwrapped", "buck")])


@pytest.mark.parametrize("fx_name,what", PAIR_ELL, ids=["%s-%s" % c for c in PAIR_ELL])
def test_pair_ell_one_evaluation(fx_name, what):
    """the generic path, 64 lanes per atom (every system below 4 096 atoms): the neighbour list of ops.build_ell and the three
    levels of pair_ell_kernel<64, LEVEL> for every form on liquid(108), contact and cutoff_pair, N = 1 000 (the cell-list
    builder), masks, the triclinic cell, unwrapped atoms"""
    fx, members, terms, w, ref, fl = reference(fx_name, what)
    assert len(members) == 1
    form, theta, rc, sel = members[0]
    counts = R.membership(fx.x, fx.cell, terms)[0].sum(1).tolist()
    pair_ell_case("pair_ell %s %s" % (fx_name, what), fx, counts, form, theta, rc, sel, terms[0].n_theta, w, ref, fl, 64)


PAIR_ELL_LPA = [((2, 2, 3), 32), ((3, 3, 2), 16), ((3, 3, 4), 8)]


@pytest.mark.parametrize("form", EDGE_FORMS)
@pytest.mark.parametrize("reps,lpa", PAIR_ELL_LPA, ids=["lpa%d" % c[1] for c in PAIR_ELL_LPA])
def test_pair_ell_other_lanes_per_atom(reps, lpa, form):
    """pair_ell_kernel<32 | 16 | 8, LEVEL>: 6 000, 9 000 and 18 000 atoms -- exact periodic copies of the 500-atom fixture
    (pair_forms_ref.supercell: every minimum-image vector is, bit for bit, one of the original's), so the float64 reference
    and the float32 floor are those of the 500 atoms, tiled; tests/test_pair_forms_ref_host.py checks that on a dense
    1 000-atom supercell"""
    base, members, terms, w, ref, fl = reference("base500", form)
    k = reps[0] * reps[1] * reps[2]
    fx = R.supercell(reps)
    counts = np.tile(R.membership(base.x, base.cell, terms)[0].sum(1), k).tolist()
    pair_ell_case("pair_ell %s %s" % (fx.name, form), fx, counts, form, None, 2.5, None, terms[0].n_theta, np.tile(w, (k, 1)),
                  R.tile(ref, k), fl, lpa)


@pytest.mark.parametrize("family,block", [("workgroup", 128), ("workgroup", 1024), ("large", 0), ("pair_ell", 0)])
def test_one_sided_mask_is_read_from_the_row_of_the_atom_it_updates(family, block):
    """Masks are symmetric by contract, and under a symmetric mask a transposed read (mask[j, i] for the sums of atom i) changes
    nothing.  So that such a read fails a test, the kernels that give every atom its own row get one mask with bits cleared
    on one side only (pair_forms_ref.one_sided_mask): F_i and dq_i lose the pair, F_j and dq_j keep it.  The ring kernels
    evaluate a pair once for both atoms and are left out: a one-sided mask means nothing there."""
    from mdgrad_amd import _lib, ops
    fx = fixture("liquid108")
    n = 108
    w = R.direction(n)
    m1 = R.one_sided_mask(n)
    assert (m1 != m1.T).sum() == 2 * len(R.excluded_list(n))
    terms = [R.Term("lj", 2.5, m1, one_sided=True)]
    ref, fl, member = R.reference(fx, terms, w)
    sym = R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, m1 & m1.T)])
    flip = R.evaluate(fx.x, w, fx.cell, [R.Term("lj", 2.5, m1.T, one_sided=True)])
    assert R.error(sym.F, ref, "F") > 1e-3 and R.error(flip.F, ref, "F") > 1e-3 and R.error(flip.dq, ref, "dq") > 1e-3
    case = "%s/%s liquid108 one-sided mask" % (family, block)
    if family == "pair_ell":
        mask = T(m1.astype(np.uint8), DEV).contiguous()
        mod = R.module("lj")
        x = T(fx.x, DEV)
        th = torch.cat([p.detach().reshape(-1) for p in mod.mdg_params()]).to(DEV)
        ell = ops.build_ell(x, _lib.make_cell(fx.cell), 2.5, mask=mask)
        assert ell.cnt.cpu().numpy().tolist() == member[0].sum(1).tolist()
        o = ops.pair_eval(ell, x, ops.make_term(mod.mdg_term(), 2.5, 0, 2, mask), th, w=T(w, DEV), energy=False, theta_grads=False)
        judge(case, ref, fl, {"F": -o["grad"].cpu().numpy().astype(np.float64), "dq": -o["hw"].cpu().numpy().astype(np.float64)})
        return
    integ = integrator(fx, [("lj", None, 2.5, dict(ex_pairs=R.excluded_list(n)))], family == "large")
    spec = integ.fused_spec("verlet")
    ring, lib = route(spec, family, block)
    mk = spec.masks[0]
    assert mk.data_ptr() == spec.terms.t[0].mask and tuple(mk.shape) == (n, n)
    assert np.array_equal(mk.cpu().numpy().astype(bool), m1 & m1.T)
    mk.copy_(T(m1.astype(np.uint8), DEV))                         # (in place: the launch reads this buffer)
    ws_ = np.stack([w, -2.0 * w]).astype(np.float32)
    F, adj, _ = one_evaluation(spec, lib, ring, fx.x, ws_)
    judge(case, ref, fl, {"F": F[0]})
    for name, (dq, _, a64) in adj.items():
        judge("%s [%s adjoint]" % (case, name), ref, fl, {"dq": dq[0]}, slack=2.0 ** -23 * np.abs(a64[0]))


# ------------------------------------------------------------------------------------------------ short trajectories
def _loss(L):
    v, q = L[0], L[1]
    out = q[1:].pow(2).sum() / q[1:].numel() + v[-1].pow(2).sum() / v[-1].numel()
    return out + 1e-2 * L[2][-1].sum() if len(L) == 3 else out


def _oracle_run(dtype, fx, members, mass, vel, nhc, t):
    terms = []
    for form, theta, rc, sel in members:
        kind, consts, th = R.FORMS[form]
        terms.append(O.PairTerm(kind, torch.tensor(R.Term(form, rc, None, theta).theta, dtype=dtype), rc,
                                torch.tensor(np.asarray(fx.cell, np.float64), dtype=dtype), **(sel or {}), **consts))
    model = O.ModelOracle(terms)
    eom = O.NHCOracle(model, torch.tensor(mass, dtype=dtype), 1.0, 30.0, 3) if nhc else O.NVEOracle(model)
    y0 = (torch.tensor(vel, dtype=dtype), torch.tensor(fx.x, dtype=dtype)) + ((torch.zeros(3, dtype=dtype),) if nhc else ())
    traj = O.odeint_oracle(eom, y0, t.to(dtype))
    leaves = [x.clone().requires_grad_(True) for x in traj]
    _loss(leaves).backward()
    lam, gth = O.adjoint_oracle(eom, traj, [x.grad for x in leaves], t.to(dtype))
    return [x.detach().double().numpy() for x in traj], [x.double().numpy() for x in lam], gth.double().numpy()


TRAJ = [("workgroup", 256, "liquid108", "buck"), ("ring", 64, "liquid107", "excluded_pairs"), ("large", 0, "liquid108", "yukawa")]


@pytest.mark.parametrize("nT", [2, 4])
@pytest.mark.parametrize("ensemble", ["nhc", "nve"])
@pytest.mark.parametrize("family,block,fx_name,what", TRAJ, ids=[c[0] for c in TRAJ])
def test_short_trajectory_and_adjoint_vs_float64_oracle(family, block, fx_name, what, ensemble, nT):
    """What one evaluation does not see -- lambda_q, the second evaluation, the theta sums over an interval: one interval and
    a run of four frames (dt 0.004) with Buckingham on the workgroup kernels, a masked LJFamily 8-4 on the ring (N = 107) and
    Yukawa on the large path, NoseHooverChain and NVE, against oracle.odeint_oracle / adjoint_oracle in float64.  Allowed per
    quantity: MARGIN x the largest difference between the float32 oracle and the float64 oracle of the same run, at least
    2^-24 of the quantity's largest entry -- computed here on the CPU, printed with the kernel's figure."""
    from mdgrad_amd import ops
    from mdgrad_amd.interface import PairPotentials, Stack
    from mdgrad_amd.md import NVE, NoseHooverChain
    fx = fixture(fx_name)
    n = len(fx.x)
    members = members_of(what, n)
    nhc = ensemble == "nhc"
    vel = np.random.default_rng(5).normal(0, 0.5, fx.x.shape).astype(np.float32)
    mass = np.full(n, 1.008, np.float32)
    system = mk_system(fx.x, fx.cell, vel, mass)
    mods = []
    for form, theta, rc, sel in members:
        kw = {k: (torch.as_tensor(np.asarray(v)) if k == "ex_pairs" else v) for k, v in (sel or {}).items()}
        mods.append(PairPotentials(system, R.module(form, theta), cutoff=rc, **kw))
    stack = Stack({"t%d" % k: m for k, m in enumerate(mods)})
    integ = (NoseHooverChain(stack, system, T=1.0, num_chains=3, Q=30.0) if nhc else NVE(stack, system)).to(DEV)
    integ.fused_large = family == "large"
    spec = integ.fused_spec("NH_verlet" if nhc else "verlet")
    route(spec, family, block, n_rep=1)
    t = torch.tensor([0.004 * k for k in range(nT)], dtype=torch.float32)
    v0, q0 = T(vel, DEV).requires_grad_(True), T(fx.x, DEV).requires_grad_(True)
    pv0 = torch.zeros(3, device=DEV, requires_grad=True) if nhc else None
    theta = spec.flat_params()
    out = ops.FusedTrajFn.apply(v0, q0, pv0, t.to(DEV), theta, spec)
    params = [p for m in mods for p in m.model.mdg_params()]
    for p in params:
        p.grad = None
    _loss(out).backward()
    gth = np.concatenate([p.grad.detach().cpu().numpy().reshape(-1) for p in params]).astype(np.float64)
    t64, l64, g64 = _oracle_run(torch.float64, fx, members, mass, vel, nhc, t)
    t32, l32, g32 = _oracle_run(torch.float32, fx, members, mass, vel, nhc, t)
    got = ([("v_t", out[0]), ("q_t", out[1])] + ([("pv_t", out[2])] if nhc else []) +
           [("adj_v0", v0.grad), ("adj_q0", q0.grad)] + ([("adj_pv0", pv0.grad)] if nhc else []))
    refs64, refs32 = t64 + l64, t32 + l32
    bad = []
    case = "%s %s %s %s T=%d" % (family, fx_name, what, ensemble, nT)
    for (nm, g), a, b in list(zip(got, refs64, refs32)) + [(("dtheta", gth), g64, g32)]:
        g = g.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(g) else g
        top = float(np.abs(a).max())
        floor = max(float(np.abs(a - b).max()), 2.0 ** -24 * top)
        fig = float(np.abs(g - a).max())
        _report("%-52s %-7s |f32 - f64 oracle| %.3e  allowed %.3e  kernel %.3e  (largest entry %.3e)%s" % (
            case, nm, floor, MARGIN * floor, fig, top, "" if fig <= MARGIN * floor else "   <-- FAILS"))
        if not fig <= MARGIN * floor:
            bad.append((nm, fig, MARGIN * floor))
    assert not bad, "%s: %s" % (case, bad)
