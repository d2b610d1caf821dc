"""Trajectory reweighting (Thaler and Zavadlav, "Learning neural network potentials from experimental data via Differentiable
Trajectory Reweighting", 2021): the gradient of an ensemble average with respect to the potential's parameters WITHOUT a
backward pass through the dynamics.  Frames x_f sampled at the reference parameters theta_ref are re-used at nearby theta with
the weights

    w_f = exp(-(U_theta(x_f) - U_ref(x_f)) / kT) / sum_g exp(-(U_theta(x_g) - U_ref(x_g)) / kT)

so <O>_theta ~ sum_f w_f O(x_f), and d<O>/dtheta flows through the weights alone: at theta = theta_ref it is the covariance
identity  d<O>/dtheta = -(<O dU/dtheta> - <O><dU/dtheta>) / kT.  The sampler (any thermostat, the stochastic one included)
runs under torch.no_grad(); when the effective sample size drops, new frames are drawn at the current parameters."""
import torch


class Reweighting:
    """rw = Reweighting(energy, kT, q_ref)

    energy   callable q -> U per frame with the leading shape of q's frames: a thermo.PotentialEnergy (built-in pair forms: one
             batched HIP launch, and ONE parameters-only launch for the whole backward pass), a thermo.TabulatedEnergy (learned
             pair modules, pairMLP ...: their energy tabulated at every call, one launch per table, and ONE nodes-only launch
             whose node gradient autograd carries into the module), or any torch function of the user's own (many-body ...
             models)
    kT       temperature in energy units
    q_ref    frames sampled at the current parameters, [..., N, 3]; stored detached, with u_ref = energy(q_ref).detach()

    weights()   softmax over ALL frames (leading dimensions flattened) of -(energy(q_ref) - u_ref) / kT, in float64 with the
                maximum subtracted; differentiable with respect to the parameters behind `energy`.  At theta = theta_ref the
                same kernel on the same input gives the same bits, every difference is 0 and the weights are exactly 1 / F.
    n_eff()     exp(-sum_f w_f ln w_f), between 1 and F (DiffTRe's effective sample size)
    stale()     n_eff < fraction * F: time to resample
    average(v)  sum_f w_f v[f] for v [F.., ...] (leading shape = that of the frames), cast back to v.dtype
    resample(q) new reference frames at the current parameters

    Frames of stacked replicas ([..., k N, 3] handed to a PotentialEnergy of the k-replica system, or an [R, T, N, 3] batch) are
    pooled into one set: the replicas sample one ensemble.
    U is float32 when it comes from the HIP kernels: its absolute error -- about 1e-7 of the sum of |phi| over the pairs of a
    frame, growing with N -- bounds the error of ln w = -(U - U_ref) / kT.  It cancels exactly at theta_ref and stays far
    below the statistical error for the parameter steps between two resamples; for thousands of atoms and small kT hand in a
    float64 callable."""

    def __init__(self, energy, kT, q_ref):
        self.energy = energy
        self.kT = float(kT)
        if not self.kT > 0:
            raise ValueError("Reweighting: kT must be positive, got %r" % (kT,))
        self.resample(q_ref)

    def resample(self, q_ref):
        """New reference frames (sampled at the current parameters): the weights are uniform again."""
        self.q_ref = q_ref.detach()
        with torch.no_grad():
            self.u_ref = self.energy(self.q_ref).detach()
        self.shape = tuple(self.u_ref.shape)
        self.n_frames = self.u_ref.numel()
        if self.n_frames < 1:
            raise ValueError("Reweighting: no frames")
        return self

    def weights(self):
        """w [F..] in float64 (the leading shape of the frames), summing to 1."""
        du = (self.energy(self.q_ref) - self.u_ref).to(torch.float64).reshape(-1)
        a = -du / self.kT
        a = a - a.detach().max()
        e = torch.exp(a)
        return (e / e.sum()).reshape(self.shape)

    def n_eff(self, w=None):
        """exp(-sum w ln w): F for uniform weights, 1 when one frame carries everything."""
        w = (self.weights() if w is None else w).detach().reshape(-1)
        return float(torch.exp(-torch.special.xlogy(w, w).sum()))

    def stale(self, fraction=0.9, w=None):
        return self.n_eff(w) < fraction * self.n_frames

    def average(self, values, w=None):
        """sum_f w_f values[f]; values [F.., ...]: the frames' leading shape first, any trailing shape."""
        w = self.weights() if w is None else w
        nd = len(self.shape)
        if tuple(values.shape[:nd]) != self.shape:
            raise ValueError("Reweighting.average: values must lead with the frames' shape %s, got %s"
                             % (self.shape, tuple(values.shape)))
        v = values.reshape(self.n_frames, -1).to(torch.float64)
        # (a product and a column sum, not a [1, F] x [F, K] matrix product: with one output row a GEMM runs its whole inner
        #  dimension, the frames, on a handful of workgroups)
        out = (w.reshape(-1, 1).to(v.device) * v).sum(0)
        return out.reshape(tuple(values.shape[nd:])).to(values.dtype)
