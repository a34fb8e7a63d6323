"""Reuse of the prologue product P0 = A Z0 across forward calls (include/dladmm.h
DLADMM_F_P0_SAVE / DLADMM_F_P0_REUSE, ops.PrologueCache, the models' `reuse_prologue`): the
load-P0 form of the fused kernel (csrc/dladmm_fused_kernel.h P0LOAD) reads a product formed once
by the fused kernel's own MFMA sequence, so every output of a filling call (p0_reused False) and
of the calls after it (p0_reused True) equals the uncached run's BIT FOR BIT.

The yardstick is always the same model with reuse_prologue = False: the compute form, the code
path of every call before the cache existed.  The batches here would take the row-split paths 5 /
6 by default, so everything runs under plan_flags(no_rowsplit=True): path 1.

Left out for spilling (DESIGN, the load form's census): no instantiation -- reuse must apply to
every variant at every shape."""
from importlib import import_module

import numpy as np
import pytest
import torch

import problems as P
from conftest import load_golden
from test_gpu_backward import make_train_net
from test_gpu_parity import check_golden, make_net

pytestmark = pytest.mark.gpu

# (variant, shape) pairs whose load form is not built (they would fall back to the compute form on
# the second call): none
LEFT_OUT = set()
SHAPES = [(12, 24), (64, 256), (250, 500)]   # one per instantiation: padded, exact, padded
VARIANTS = ["v1", "v2", "v3", "v4", "v5", "v6", "v7", "v7t"]   # v7 / v7t: V4's / V5's kernels
NAMES = ("Z", "E", "L", "T", "loss_sums", "P")


def _net(dl, variant, m, n, B, K, seed, reuse=True, train=False):
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=seed, perturb=0.2,
             wscale=0.4 if variant in ("v1", "v2") else P.VARIANT_SPECS[variant]["wscale"])
    inp, sd = P.build_problem(d)
    mk = make_train_net if train else make_net
    net = mk(dl, variant, inp, sd, K, **P.ctor_extra(d)).cuda()
    net.reuse_prologue = reuse
    # the problems' E0 = L0 = 0 would hide a wrong E0 / L0 read of the up-front rows
    g = torch.Generator().manual_seed(seed)
    net.E0 = (0.05 * torch.randn(net.E0.shape, generator=g)).cuda()
    net.L0 = (0.05 * torch.randn(net.L0.shape, generator=g)).cuda()
    return net, torch.from_numpy(inp["X"]).cuda()


def _fwd(dl, net, X, keep_all=True, lk=0, want_P=False):
    """What net.run does, plus the training form's saved products (want_P)."""
    with torch.no_grad(), dl.ops.plan_flags(no_rowsplit=True):
        r = dl.ops.dladmm_forward(net.VARIANT, X, net.A, [w.detach() for w in net._weights()],
                                  net.Z0, net.E0, net.L0, keep_all=keep_all, want_T=True,
                                  loss_kind=lk, want_P=want_P, precision=net.precision,
                                  p0_cache=net._p0_cache(), **net._tables(X.device))
    torch.cuda.synchronize()
    assert r.path == 1
    return r


def _same(a, b, tag):
    for nm in NAMES:
        x, y = getattr(a, nm), getattr(b, nm)
        assert (x is None) == (y is None), (tag, nm)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), (tag, nm)


def _run(dl, net, X, **kw):
    with dl.ops.plan_flags(no_rowsplit=True):
        r = net.run(X, **kw)
    torch.cuda.synchronize()
    assert r.path == 1
    return r


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_fill_and_reuse_bit_equal_to_uncached(variant, shape, dl):
    m, n = shape
    expect = (variant, shape) not in LEFT_OUT
    assert ("v4", (250, 500)) not in LEFT_OUT
    for B in (64, 70):          # 70: a partial 64-column tile
        for K in (1, 3):
            net, X = _net(dl, variant, m, n, B, K, 7300 + B + K)
            for keep_all in (True, False):
                for lk in (0, dl._lib.LOSS_L1L1):
                    want_P = keep_all   # the saved-product (training) form where it applies
                    tag = (variant, shape, B, K, keep_all, lk)
                    net.reuse_prologue = False
                    ref = _fwd(dl, net, X, keep_all, lk, want_P)
                    assert not ref.p0_reused
                    net.reuse_prologue = True
                    net.invalidate_cache()
                    fill = _fwd(dl, net, X, keep_all, lk, want_P)
                    again = _fwd(dl, net, X, keep_all, lk, want_P)
                    third = _fwd(dl, net, X, keep_all, lk, want_P)
                    assert not fill.p0_reused, tag
                    assert again.p0_reused == expect and third.p0_reused == expect, tag
                    assert (ref.P is not None) == want_P, tag
                    _same(fill, ref, tag + ("fill",))
                    _same(again, ref, tag + ("reuse",))
                    _same(third, again, tag + ("determinism",))


def _record(monkeypatch):
    mod = import_module("d-ladmm_amd.model")
    orig, seen = mod.dladmm_forward, []

    def wrap(*a, **k):
        r = orig(*a, **k)
        seen.append(r)
        return r
    monkeypatch.setattr(mod, "dladmm_forward", wrap)
    return seen


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_golden_fixtures_second_call(name, dl, monkeypatch):
    """Every forward fixture on its default plan (tests/test_gpu_parity.py): the second call reuses
    P0 exactly where the plan is path 1 with fp32, is bit-equal to the first and meets the
    fixture's bars."""
    seen = _record(monkeypatch)
    g, meta = load_golden(name)
    d = meta["defn"]
    inp, sd = P.build_problem(d)
    net = make_net(dl, d["variant"], inp, sd, d["K"], **P.ctor_extra(d))
    X = torch.from_numpy(inp["X"]).cuda()
    with torch.no_grad():
        first = net(X)
        second = net(X)
    torch.cuda.synchronize()
    r1, r2 = seen[0], seen[1]
    assert not r1.p0_reused
    assert r2.p0_reused == (r2.path == 1), (name, r2.path)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert torch.equal(x, y), name
    check_golden(name, g, meta, net, X, second)


def test_invalidation(dl):
    m, n, B, K = 64, 256, 70, 3
    net, X = _net(dl, "v4", m, n, B, K, 7401)

    def fresh():
        net.reuse_prologue = False
        r = _run(dl, net, X)
        net.reuse_prologue = True
        return r

    def expect_refill(tag, stale=None):
        r = _run(dl, net, X)
        assert not r.p0_reused, tag
        _same(r, fresh(), tag)
        if stale is not None:
            assert not torch.equal(r.Z, stale.Z), tag
        r2 = _run(dl, net, X)
        assert r2.p0_reused, tag
        _same(r2, r, tag)
        return r2

    r0 = _run(dl, net, X)
    assert not r0.p0_reused and _run(dl, net, X).p0_reused
    net.Z0 = torch.randn_like(net.Z0) * 0.1
    r = expect_refill("new Z0", r0)
    net.Z0.mul_(2)
    r = expect_refill("Z0.mul_", r)
    net.A.add_(0.01 * torch.randn_like(net.A))
    r = expect_refill("A.add_", r)
    net.invalidate_cache()
    r = expect_refill("invalidate_cache")
    # an edit through .data is not seen (documented): invalidate_cache() makes it so
    net.Z0.data.mul_(0.5)
    net.invalidate_cache()
    r = expect_refill("data edit + invalidate_cache", r)
    net.precision = "f32_split"   # path 4: the flags do not act
    with dl.ops.plan_flags(no_rowsplit=True):
        assert not net.run(X).p0_reused and not net.run(X).p0_reused
    net.precision = "f32"
    # another batch: the model's own column span after shard_batch_
    net.shard_batch_(0, 2)
    Xs = X[:, : net.Z0.shape[1]].contiguous()
    rs = _run(dl, net, Xs)
    assert not rs.p0_reused
    net.reuse_prologue = False
    _same(rs, _run(dl, net, Xs), "shard_batch_")
    net.reuse_prologue = True
    assert _run(dl, net, Xs).p0_reused


def test_changing_weights_keeps_the_cache(dl):
    m, n, B, K = 64, 256, 70, 3
    net, X = _net(dl, "v4", m, n, B, K, 7402, train=True)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    r0 = _run(dl, net, X)
    with dl.ops.plan_flags(no_rowsplit=True):
        tot, _ = net.training_loss(X, 0.01)
        tot.backward()
    opt.step()
    r1 = _run(dl, net, X)
    assert r1.p0_reused and not torch.equal(r1.Z, r0.Z)
    sd = {k: v.clone() * (0.9 if k.startswith("fc") else 1.0) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    r2 = _run(dl, net, X)
    assert r2.p0_reused and not torch.equal(r2.Z, r1.Z)
    net.reuse_prologue = False
    _same(r2, _run(dl, net, X), "after optimizer step and load_state_dict")


def test_two_models_alternating_and_two_streams(dl):
    m, n, B, K = 12, 24, 70, 3
    a, X = _net(dl, "v4", m, n, B, K, 7403)
    b, _ = _net(dl, "v4", m, n, B, K, 7403)
    b.Z0 = torch.randn_like(b.Z0) * 0.1
    refs = []
    for net in (a, b):
        net.reuse_prologue = False
        refs.append(_run(dl, net, X, loss_kind=dl._lib.LOSS_L1L1))
        net.reuse_prologue = True
    assert not torch.equal(refs[0].Z, refs[1].Z)
    for it in range(3):
        for net, ref in zip((a, b), refs):
            r = _run(dl, net, X, loss_kind=dl._lib.LOSS_L1L1)
            assert r.p0_reused == (it > 0)
            _same(r, ref, ("two models", it))
    # one model, two more streams: each fills its own workspace, then reuses it
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for it in range(2):
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                r = _run(dl, a, X, loss_kind=dl._lib.LOSS_L1L1)
            assert r.p0_reused == (it > 0)
            _same(r, refs[0], ("two streams", it))
    assert _run(dl, a, X, loss_kind=dl._lib.LOSS_L1L1).p0_reused   # the first stream's slot stays


@pytest.mark.parametrize("name", ["grad_v4_med", "grad_v1_med"])
def test_training_forward_reuses_and_gradients_equal(name, dl, monkeypatch):
    """A training forward (saved products) after a cache fill reuses P0; its gradients equal the
    uncached forward's bit for bit."""
    seen = _record(monkeypatch)
    grads = {}
    for reuse in (False, True):
        g, meta = load_golden(name)
        d = meta["defn"]
        inp, sd = P.build_problem(d)
        net = make_train_net(dl, d["variant"], inp, sd, d["K"], **P.ctor_extra(d))
        net.reuse_prologue = reuse
        X = torch.from_numpy(inp["X"]).cuda()
        with dl.ops.plan_flags(no_rowsplit=True):
            for it in range(2):
                net.zero_grad(set_to_none=True)
                del seen[:]
                tot, _ = net.training_loss(X, 0.01)
                tot.backward()
                assert seen[0].path == 1 and seen[0].p0_reused == (reuse and it == 1), (name, it)
        torch.cuda.synchronize()
        grads[reuse] = {k: p.grad.clone() for k, p in net.named_parameters()
                        if p.grad is not None}
    assert grads[True].keys() == grads[False].keys() and grads[True]
    for k in grads[True]:
        assert torch.equal(grads[True][k], grads[False][k]), (name, k)


def test_graph_capture_does_not_reuse(dl):
    m, n, B, K = 64, 256, 640, 3
    net, X = _net(dl, "v4", m, n, B, K, 7404)
    x = X.clone()
    with dl.ops.plan_flags(no_rowsplit=True):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            assert not net.run(x).p0_reused
            assert net.run(x).p0_reused        # the cache is filled
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            out = net.run(x)
        assert not out.p0_reused and out.path == 1
        x.copy_(X * 0.5)
        g.replay()
        torch.cuda.synchronize()
        net.reuse_prologue = False
        ref = net.run(x)
    torch.cuda.synchronize()
    for nm in ("Z", "E", "L"):
        assert torch.equal(getattr(out, nm), getattr(ref, nm)), nm
