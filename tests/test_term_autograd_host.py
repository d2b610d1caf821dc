"""The shared Python layer of the interaction terms, without a GPU: the generic autograd pair (ops.TermEnergyFn ->
ops.TermGradFn) on a toy term written in torch, the device mirror of host-visible parameters (interface._DeviceMirror) on CPU
tensors, the no-accum branches of the two parameter tails of force_vjp, and the flat tail on three one-element parameters
against the three-scalar tail it replaced (the reductions it queues, run here by a host stand-in of GradJobs.run).

Tolerance: torch.equal where the hand formula and autograd do the same operations; otherwise 1e-12 of the largest entry --
float64 round-off on numbers of order one, not a measured quantity."""
import pytest
import torch

from mdgrad_amd import interface, ops

F64 = torch.float64


def close(got, want, what):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(want.shape))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), what


def energy(x, a, b):
    return (a * x.pow(4).sum() + (b * x.pow(2)).sum()).reshape(())


class Toy:
    """U(x, a, b) = a sum(x^4) + sum(b x^2), first and second order by hand; `packed` = (dU/da, dU/db)."""

    noun = "dU/d(a, b) of the toy term"

    def __init__(self, a, b):
        self.a, self.b = a.detach().reshape(()), b.detach()
        self.calls = {"first": 0, "second": 0}

    def first_order(self, xyz, energy):
        self.calls["first"] += 1
        e = self.a * xyz.pow(4).sum() + (self.b * xyz.pow(2)).sum() if energy else None
        packed = torch.cat([xyz.pow(4).sum().reshape(1), xyz.pow(2).sum(0)])
        return e, 4.0 * self.a * xyz.pow(3) + 2.0 * self.b * xyz, packed

    def second_order(self, xyz, w):
        self.calls["second"] += 1
        hw = (12.0 * self.a * xyz.pow(2) + 2.0 * self.b) * w
        return hw, torch.cat([(4.0 * xyz.pow(3) * w).sum().reshape(1), (2.0 * xyz * w).sum(0)])


def _inputs(a_shape=(1,)):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(5, 3, generator=g, dtype=F64).requires_grad_(True)
    a = torch.full(a_shape, 0.7, dtype=F64).requires_grad_(True)
    b = (0.5 + torch.rand(3, generator=g, dtype=F64)).requires_grad_(True)
    return x, a, b, torch.randn(5, 3, generator=g, dtype=F64)


# ------------------------------------------------------------------------------------------------ 1: the autograd pair
@pytest.mark.parametrize("a_shape", [(1,), ()], ids=["a[1]", "a[]"])
def test_backward_equals_plain_autograd_and_parameters_keep_their_shape(a_shape):
    x, a, b, _ = _inputs(a_shape)
    toy = Toy(a, b)
    U = ops.TermEnergyFn.apply(x, toy, a, b)
    assert U.shape == () and torch.equal(U.detach(), energy(x, a, b).detach())
    got = torch.autograd.grad(U, (x, a, b))
    want = torch.autograd.grad(energy(x, a, b), (x, a, b))
    assert [t.shape for t in got] == [x.shape, a.shape, b.shape]
    for t, r, name in zip(got, want, ("dU/dx", "dU/da", "dU/db")):
        close(t, r, name)
    assert toy.calls == {"first": 1, "second": 0}, "backward uses the cache of the forward evaluation"
    # a weight on U reaches every gradient once
    got3 = torch.autograd.grad(3.0 * ops.TermEnergyFn.apply(x, toy, a, b), (x, a, b))
    for t, r in zip(got3, got):
        assert torch.equal(t, 3.0 * r)


@pytest.mark.parametrize("a_shape", [(1,), ()], ids=["a[1]", "a[]"])
def test_double_backward_equals_plain_autograd_hessian_vector_and_mixed_derivatives(a_shape):
    x, a, b, w = _inputs(a_shape)
    toy = Toy(a, b)
    g, ga, gb = torch.autograd.grad(ops.TermEnergyFn.apply(x, toy, a, b), (x, a, b), create_graph=True)
    got = torch.autograd.grad((g * w).sum(), (x, a, b))
    (r,) = torch.autograd.grad(energy(x, a, b), x, create_graph=True)
    want = torch.autograd.grad((r * w).sum(), (x, a, b))
    assert [t.shape for t in got] == [x.shape, a.shape, b.shape]
    for t, v, name in zip(got, want, ("H w", "d(w.dU/dx)/da", "d(w.dU/dx)/db")):
        close(t, v, name)
    assert toy.calls == {"first": 1, "second": 1}
    # without a cache (TermGradFn on its own) the first-order evaluation runs there
    g2, packed = ops.TermGradFn.apply(x, toy, None, a, b)
    assert torch.equal(g2, g.detach()) and packed.shape == (4,) and toy.calls["first"] == 2


def test_cotangent_on_the_parameter_gradient_is_refused_naming_the_term():
    x, a, b, _ = _inputs()
    toy = Toy(a, b)
    (ga,) = torch.autograd.grad(ops.TermEnergyFn.apply(x, toy, a, b), a, create_graph=True)
    with pytest.raises(NotImplementedError, match=r"dU/d\(a, b\) of the toy term"):
        torch.autograd.grad(ga.sum(), x)
    assert toy.calls["second"] == 0


class _Drop(torch.autograd.Function):
    """Identity whose backward hands no gradient on."""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def test_unused_position_gradient_returns_without_a_second_order_evaluation():
    x, a, b, _ = _inputs()
    toy = Toy(a, b)
    (g,) = torch.autograd.grad(ops.TermEnergyFn.apply(x, toy, a, b), x, create_graph=True)
    got = torch.autograd.grad(_Drop.apply(g).sum(), (x, a, b), allow_unused=True)
    assert got == (None, None, None) and toy.calls["second"] == 0


# ------------------------------------------------------------------------------------------------ 2: the device mirror
def _mirror(ps):
    calls = []

    def pack(srcs, out=None):
        calls.append(1)
        return torch.cat([p.detach().reshape(-1).to(torch.float32) for p in srcs], out=out)
    return interface._DeviceMirror(lambda: ps, pack), calls


def test_device_mirror_packs_once_and_repacks_when_a_source_changes():
    ps = [torch.nn.Parameter(torch.tensor([1.5])), torch.nn.Parameter(torch.tensor([2.5, 3.5]))]
    m, calls = _mirror(ps)
    buf = m.get()
    assert buf.dtype == torch.float32 and buf.tolist() == [1.5, 2.5, 3.5] and len(calls) == 1
    again = m.get()
    assert again.data_ptr() == buf.data_ptr() and len(calls) == 1, "nothing changed: the same storage, no pack"
    with torch.no_grad():
        ps[0].add_(1.0)                                    # (in place: bumps the version counter)
    assert m.get().data_ptr() == buf.data_ptr() and buf.tolist() == [2.5, 2.5, 3.5] and len(calls) == 2
    with torch.no_grad():
        ps[1].add_(1.0)
    assert m.get().tolist() == [2.5, 3.5, 4.5] and len(calls) == 3
    assert m.get() is not None and len(calls) == 3
    old = ps[0]                                            # (kept alive: the new tensor gets another address)
    ps[0] = torch.nn.Parameter(torch.tensor([9.0]))
    assert m.get().data_ptr() == buf.data_ptr() and buf.tolist() == [9.0, 3.5, 4.5] and len(calls) == 4
    assert old is not ps[0]


def test_device_mirror_reallocates_when_the_size_changes():
    ps = [torch.nn.Parameter(torch.tensor([1.0, 2.0]))]
    m, calls = _mirror(ps)
    buf = m.get()
    ps[0] = torch.nn.Parameter(torch.tensor([1.0, 2.0, 3.0]))
    new = m.get()
    assert new.tolist() == [1.0, 2.0, 3.0] and buf.tolist() == [1.0, 2.0] and len(calls) == 2


# ------------------------------------------------------------------------------------------------ 3: the parameter tails
def test_single_parameter_tail_without_accum():
    p = torch.nn.Parameter(torch.zeros(2, 3))
    gw = torch.arange(6.0)
    assert interface._param_tail(gw, p, -2.5, False, None) is None
    assert interface._param_tail(None, p, -2.5, True, None) == []                  # (no trainable parameter)
    assert interface._param_tail(None, p, -2.5, True, ops.ThetaAccum([p])) is None
    (out,) = interface._param_tail(gw, p, -2.5, True, None)
    assert out.shape == p.shape and torch.equal(out, (-2.5) * gw.reshape(2, 3))
    (out,) = interface._param_tail(gw, p, -1.0, True, None)
    assert out.shape == p.shape and torch.equal(out, -gw.reshape(2, 3))


def test_three_scalar_tail_without_accum():
    th = [torch.nn.Parameter(torch.ones(1)) for _ in range(3)]
    pthw = torch.ones(4, 3)
    assert interface._theta_flat_tail(pthw, th, False, None) is None
    frozen = [t.detach() for t in th]
    assert interface._theta_flat_tail(None, frozen, True, None) == []
    assert interface._theta_flat_tail(None, frozen, True, ops.ThetaAccum(th)) is None
    assert interface._theta_flat_tail(pthw, th, False, ops.ThetaAccum(th)) is None


def _three_scalar_tail(pthw, thetas, want_theta, accum):
    """The tail that StillingerWeber, SuttonChen and Tersoff used before they took _theta_flat_tail, restated: the reference of
    the test below."""
    if not want_theta:
        return None
    if pthw is None:
        return [] if accum is None else None
    trainable = [isinstance(p, torch.nn.Parameter) for p in thetas]
    if accum is not None:
        jobs = ops.GradJobs()
        offs = [accum.off.get(id(p)) for p, t in zip(thetas, trainable) if t]
        if len(offs) == 3 and None not in offs and offs[1] == offs[0] + 1 and offs[2] == offs[0] + 2:
            jobs.colsum(offs[0], pthw)
        else:
            for col, (p, t) in enumerate(zip(thetas, trainable)):
                if t and accum.off.get(id(p)) is not None:
                    jobs.colsum(accum.off[id(p)], pthw[:, col:col + 1])
        jobs.run(accum, alpha=-1.0, accumulate=True)
        return None
    gw = ops.theta_sum(pthw, alpha=-1.0)
    return [gw[k:k + 1].reshape(p.shape) for k, (p, t) in enumerate(zip(thetas, trainable)) if t]


def _tail_cases():
    """name -> (thetas, parameters of the accumulator or None), three one-element parameters each."""
    def three():
        return [torch.nn.Parameter(torch.tensor([float(k + 1)])) for k in range(3)]
    cases = {}
    th = three()
    cases["adjacent"] = (th, list(th))
    th = three()
    cases["scattered"] = (th, [th[0], torch.nn.Parameter(torch.zeros(2)), th[2], th[1]])
    th = three()
    cases["adjacent elsewhere"] = (th, [torch.nn.Parameter(torch.zeros(2, 2))] + list(th))
    th = three()
    th[1] = th[1].detach()
    cases["partly frozen"] = (th, [th[0], th[2]])
    th = three()
    cases["one parameter not in the accumulator"] = (th, [th[2], th[0]])
    th = three()
    cases["no accumulator"] = (th, None)
    th = three()
    th[0] = th[0].detach()
    cases["no accumulator, partly frozen"] = (th, None)
    return cases


@pytest.mark.parametrize("case", sorted(_tail_cases()))
def test_flat_tail_on_three_scalars_queues_and_returns_what_the_three_scalar_tail_did(case, monkeypatch):
    log = []

    def run(self, acc, alpha=1.0, accumulate=True):                 # GradJobs.run on the host: column sums only
        for kind, off, rows, m, n, ts, row_map in self.jobs:
            assert kind == ops._lib.GRAD_COLSUM and ts[1:] == [None, None, None] and row_map is None
            log.append((off, rows, m, n, ts[0].clone(), float(alpha), bool(accumulate)))
            add = alpha * ts[0].sum(0)
            acc.flat[off:off + m] = acc.flat[off:off + m] + add if accumulate else add
    monkeypatch.setattr(ops.GradJobs, "run", run)
    pthw = torch.tensor([[1.0, -2.0, 4.0], [0.5, 8.0, -16.0], [32.0, 0.25, 64.0], [-128.0, 256.0, 0.125]])
    thetas, params = _tail_cases()[case]
    out = []
    for tail in (_three_scalar_tail, interface._theta_flat_tail):
        del log[:]
        accum = None
        if params is not None:
            accum = ops.ThetaAccum(params)
            accum.flat.copy_(torch.arange(accum.n, dtype=torch.float32) + 0.5)     # (something to accumulate onto)
        got = tail(pthw, thetas, True, accum)
        out.append((list(log), got, None if accum is None else accum.flat.clone()))
    (jobs_a, got_a, flat_a), (jobs_b, got_b, flat_b) = out
    assert len(jobs_a) == len(jobs_b) and len(jobs_a) >= 1
    for a, b in zip(jobs_a, jobs_b):
        assert a[:4] == b[:4] and a[5:] == b[5:], "offset, rows, width, alpha, accumulate"
        assert a[4].shape == b[4].shape and torch.equal(a[4], b[4])
    if params is None:
        assert len(got_a) == len(got_b) == sum(isinstance(p, torch.nn.Parameter) for p in thetas)
        for a, b in zip(got_a, got_b):
            assert a.shape == b.shape == (1,) and torch.equal(a, b)
        assert flat_a is None and flat_b is None
    else:
        assert got_a is None and got_b is None and torch.equal(flat_a, flat_b)
        assert not torch.equal(flat_a, torch.arange(flat_a.numel(), dtype=torch.float32) + 0.5)
