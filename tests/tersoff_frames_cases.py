"""The inputs of the K38 tests (thermo.TersoffEnergy, csrc/tersoff_frames.hip): frames of one box with a Tersoff parameter set
(one species: tests/tersoff_ref.py) or a table set and one frame's species (tests/tersoff_multi_ref.py), the modules built on
them and the float64 references per frame, computed once per Case and parameter state.

tests/test_tersoff_frames_host.py checks every fixture's conditions on the CPU: the cutoff below half the box and the longest
row of the float64 list against the kernel's row cap."""
import numpy as np
import torch

import tersoff_multi_ref as RM
import tersoff_ref as R1

F32 = np.float32
SIC_SEED, S3_SEED = RM.SEEDS["sic_alloy64"], RM.SEEDS["s3_64"]


class Case:
    """frames [F, N, 3] of one box; params = a one-species set, or tab + types = a table set and one frame's species"""

    def __init__(self, name, frames, cell, params=None, tab=None, types=None):
        self.name = name
        self.frames, self.cell = np.ascontiguousarray(frames, dtype=F32), np.asarray(cell, dtype=F32)
        self.F, self.N = self.frames.shape[0], self.frames.shape[1]
        self.params, self.tab, self.types = params, tab, types
        self.multi = tab is not None
        self._ref = {}

    @property
    def cutoff(self):
        return RM.rc_max(self.tab) if self.multi else float(self.params["R"] + self.params["D"])

    def modules(self, system):
        """(model, TersoffEnergy) on `system` (one frame of this case on the device under test)"""
        from mdgrad_amd.interface import Tersoff, TersoffMulti
        from mdgrad_amd.thermo import TersoffEnergy
        if self.multi:
            pair, centre = RM.pair_centre(self.tab)
            model = TersoffMulti.from_tables(system, self.types, pair, centre)
        else:
            model = Tersoff(system, **self.params)
        return model, TersoffEnergy(system, model)

    def theta(self, model):
        """the module's float32 (A, B, h) as the float64 reference takes them: [3] or [2 S^2 + S]"""
        return np.concatenate([p.detach().cpu().double().numpy().reshape(-1) for p in (model.A, model.B, model.h)])

    def lists(self, f):
        key = ("list", f)
        if key not in self._ref:
            self._ref[key] = R1.bonds_and_triplets(self.frames[f], self.cell, self.cutoff)
        return self._ref[key]

    def energy64(self, model, f):
        """U of frame f in float64 at the module's parameters (the definition alone, no scales)"""
        th, x = torch.as_tensor(self.theta(model)), torch.tensor(self.frames[f]).double()
        if self.multi:
            return float(RM.energy(x, self.types, self.tab, self.lists(f), self.cell, theta=th))
        return float(R1.energy(x, th, self.lists(f), self.cell, R1.consts(**self.params)))

    def reference(self, model, n=None):
        """dict of stacked float64 arrays (U, A_U, dth, A_dth, grad, A_grad) for the first n frames at the module's float32
        parameters, and the row lengths of every frame"""
        th = self.theta(model)
        key, n = tuple(th.tolist()), self.F if n is None else n
        for f in range(n):
            if (key, f) not in self._ref:
                if self.multi:
                    self._ref[(key, f)] = RM.evaluate(self.frames[f], self.types, self.tab, self.lists(f), self.cell, theta=th)
                else:
                    self._ref[(key, f)] = R1.evaluate(self.frames[f], th, self.lists(f), self.cell, R1.consts(**self.params))
        refs = [self._ref[(key, f)] for f in range(n)]
        out = {k: torch.stack([r[k] for r in refs]) for k in ("U", "A_U", "dth", "A_dth", "grad", "A_grad")}
        out["rows"] = [self.lists(f)["rows"] for f in range(n)]
        return out

    def longest_row(self, f):
        """the longest row of frame f inside the support of its directed pairs, by a float64 all-pairs count"""
        x = self.frames[f].astype(np.float64)
        d = x[None, :, :] - x[:, None, :]
        d -= np.rint(d / self.cell) * self.cell
        r = np.sqrt((d ** 2).sum(-1))
        if self.multi:
            ty = np.asarray(self.types)
            rc = (self.tab["R"] + self.tab["D"])[ty[:, None], ty[None, :]]
        else:
            rc = self.cutoff
        return int(((r < rc) & (r > 0)).sum(1).max())


def _diamond(n, cells, a0, jit, seed):
    xs = [R1.jittered_diamond(cells, a0, jit, seed + s) for s in range(n)]
    return np.stack([x for x, _ in xs]), xs[0][1]


def si_frames(n):
    return Case("si_frames", *_diamond(n, 2, 5.432, 0.3, 64), params=R1.SILICON)


def si216():
    """216 atoms: a workgroup per frame"""
    return Case("si216", *_diamond(2, 3, 5.432, 0.3, 216), params=R1.SILICON)


def gas37():
    """tersoff_ref.gas37 (hub with a row of 18, an atom without a neighbour, a dimer with zeta = 0, a trimer) and the same with
    atom 4 moved onto atom 3 (r = 0: skipped)"""
    x, cell = R1.gas37(R1.SEEDS["gas37"])
    twin = x.copy()
    twin[4] = twin[3]
    return Case("gas37", np.stack([x, twin]), cell, params=R1.SILICON)


def long_rows():
    """R + D = 5.0 on the 64-atom box (half box 5.432): rows of 27 - 30"""
    return Case("long_rows", *_diamond(2, 2, 5.432, 0.15, 64), params=dict(R1.SILICON, R=4.85, D=0.15))


def lam3():
    return Case("lam3", *_diamond(2, 2, 5.432, 0.3, 64), params=R1.LAM3)


def c64():
    return Case("c64", *_diamond(2, 2, 3.566, 0.15, 257), params=R1.CARBON)


def sic_frames(n):
    return Case("sic_frames", *_diamond(n, 2, 4.6, 0.25, SIC_SEED), tab=RM.sic(), types=RM.species_split(64, 2, SIC_SEED))


def sic_asym():
    """SiC with the outer radius of the directed pair (Si, C) 0.2 A beyond that of (C, Si)"""
    tab = RM.sic()
    tab["R"] = tab["R"].copy()
    tab["R"][0, 1] += 0.2
    return Case("sic_asym", *_diamond(2, 2, 4.6, 0.25, SIC_SEED), tab=tab, types=RM.species_split(64, 2, SIC_SEED))


def s3_frames():
    return Case("s3_frames", *_diamond(2, 2, 4.9, 0.25, S3_SEED), tab=RM.sicge(), types=RM.species_split(64, 3, S3_SEED))


def overflow(multi=False):
    """128 atoms (two shifted copies of the 64-atom frame): in the middle frame 70 of them sit in a ball of sigma = 0.5 A, so
    their rows run far beyond the cap.  The outer frames are equal."""
    rng = np.random.default_rng(3)
    x, cell = R1.jittered_diamond(2, 5.432, 0.3, 64)
    ok = np.concatenate([x, np.mod(x + 1.1, cell)]).astype(F32)
    bad = ok.copy()
    bad[:70] = (np.array([5.0, 5.0, 5.0]) + rng.normal(0, 0.5, (70, 3))).astype(F32)
    frames = np.stack([ok, bad, ok])
    if multi:
        return Case("overflow_sige", frames, cell, tab=RM.sige(), types=RM.species_split(128, 2, 3))
    return Case("overflow", frames, cell, params=R1.SILICON)


def all_cases():
    """every fixture the GPU tests evaluate, at the number of frames they use"""
    return [si_frames(6), si216(), gas37(), long_rows(), lam3(), c64(), sic_frames(6), sic_asym(), s3_frames()]
