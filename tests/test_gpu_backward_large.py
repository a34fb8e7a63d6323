"""The backward on its natural plan past the register-resident shapes (m > 256 or n > 512): the
per-layer kernels BK1 / BK2 / BK3 / WG (csrc/dladmm_backward.hip) with more than one m-slice
(blockIdx.y > 0, ib0 > 0), padded m- and n-slices, more parameter-partial slots than one slice
fills, weight-gradient tilings past 512 x 256 and split-K chunks of more than one step with a
ragged tail -- none of which a shape within 256 x 512 reaches, flags or not.

Every case asserts that the forward ran the per-layer kernels (path 2) and the backward the
per-layer phases (dladmm_bwd_path 0) with no plan flag set, so a case another path serves cannot
pass silently.  The shapes, their geometry and the seeds are tests/bwd_large_cases.py's; the
references are the fp64 oracle (oracle/dladmm_oracle_grad.py) at the bar of
tests/test_gpu_backward.py, max(GTOL, 3 x gap), where the seeds keep gap <= GTOL / 3
(tests/test_backward_large_cases.py), so the bar is GTOL on every key.
"""
from importlib import import_module

import numpy as np
import pytest
import torch

import bwd_large_cases as C
import parity
import problems as P
from test_gpu_backward import GTOL, make_train_net, nrel, record_paths, total_loss

pytestmark = pytest.mark.gpu


def record_bwd_paths(monkeypatch, **override):
    """dladmm_bwd_path of every backward the model runs (BackwardResult.path), in call order;
    override: extra keyword arguments for ops.dladmm_backward (wgrad_split)."""
    mod = import_module("d-ladmm_amd.model")
    orig, paths = mod.dladmm_backward, []

    def wrap(*a, **k):
        r = orig(*a, **dict(k, **override))
        paths.append(r.path)
        return r
    monkeypatch.setattr(mod, "dladmm_backward", wrap)
    return paths


def build(dl, shape, variant, precision="f32"):
    d, inp, sd, up = C.problem(shape, variant)
    net = make_train_net(dl, variant, inp, sd, d["K"], precision=precision, **P.ctor_extra(d))
    X = torch.from_numpy(inp["X"]).cuda()
    A = torch.from_numpy(inp["A"]).cuda()
    return d, net, X, A, up


def run_full_loss(dl, shape, variant):
    """Forward + backward of the torch-op training loss plus the seeded cotangents."""
    d, net, X, A, up = build(dl, shape, variant)
    loss = total_loss(net(X), X, A, up, C.loss_kind(variant), d["K"])
    loss.backward()
    torch.cuda.synchronize()
    return d, net


def check_vs_oracle(case, shape, variant, loss, net, path="per_layer"):
    """Every gradient against the fp64 oracle at max(GTOL, 3 x gap); returns the worst error."""
    ref, gap = C.reference(shape, variant, loss)
    none = C.unreachable(variant, C.SHAPES[shape][3], loss)
    worst = 0.0
    for key, p in net.named_parameters():
        assert (p.grad is None) == (key in none), key
        if p.grad is None:
            assert not np.any(ref[key]), key
            continue
        e = nrel(p.grad.cpu().numpy(), ref[key])
        print(f"{case} {shape} {variant} {key}: err {e:.3e} gap {gap[key]:.3e}")
        parity.check(f"{case} {shape} {variant}", path, key, e, max(GTOL, 3.0 * gap[key]),
                     gap[key])
        worst = max(worst, e)
    return worst


def grads_of(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("shape,variant", C.ORACLE_CASES)
def test_large_grads_match_oracle(shape, variant, dl, monkeypatch):
    """The reference training loss built with torch ops on the outputs plus seeded cotangents on
    Z, E, L (and T where the variant returns it), which the kernels of the second m-slice read
    too, against the fp64 backward oracle."""
    fwd, bwd = record_paths(monkeypatch), record_bwd_paths(monkeypatch)
    d, net = run_full_loss(dl, shape, variant)
    assert fwd == [2] and bwd == [0], (fwd, bwd)
    check_vs_oracle("large grads vs oracle64", shape, variant, "full", net)


@pytest.mark.parametrize("shape,variant", C.FUSED_CASES)
def test_large_fused_training_loss(shape, variant, dl, monkeypatch):
    """net.training_loss: the objective's value against the torch-op loss (rtol 1e-5) and its
    gradients, injected in the BK1 / BK2 epilogues of every m- and n-slice, against the oracle."""
    fwd, bwd = record_paths(monkeypatch), record_bwd_paths(monkeypatch)
    d, net, X, A, _ = build(dl, shape, variant)
    K, kind = d["K"], C.loss_kind(variant)
    total, per_layer = net.training_loss(X, P.GRAD_ALPHA, P.loss_coeffs(K), kind)
    total.backward()
    torch.cuda.synchronize()
    assert fwd == [2] and bwd == [0], (fwd, bwd)
    assert per_layer.shape == (K,)
    zero = {nm: np.zeros((K, 1, 1), np.float32) for nm in ("Gz", "Ge", "Gl")}
    with torch.no_grad():
        ref_total = total_loss(net(X), X, A, zero, kind, K)
    np.testing.assert_allclose(float(total), float(ref_total), rtol=1e-5)
    check_vs_oracle("large fused objective vs oracle64", shape, variant, "train", net)


@pytest.mark.parametrize("shape,variant", C.SHARD_CASES)
def test_large_column_shards_sum(shape, variant, dl, monkeypatch):
    """Column shards [0, 333) and [333, 1000) through training_loss(batch=B, cols=...): their
    accumulated gradients equal the full batch's within 1e-5 and the losses at rtol 1e-5.  A
    column's forward state does not depend on its neighbours, so no shrink mask can differ
    between the runs: what differs is the split-K chunking (32-column chunks with a 16-column
    tail at B = 1,000; 21 and 42 one-step chunks on the shards) and the column-group slots."""
    fwd, bwd = record_paths(monkeypatch), record_bwd_paths(monkeypatch)
    d, full, X, _, _ = build(dl, shape, variant)
    K, B, kind = d["K"], d["B"], C.loss_kind(variant)
    coeffs = P.loss_coeffs(K)
    tf, pf = full.training_loss(X, P.GRAD_ALPHA, coeffs, kind)
    tf.backward()
    shard = build(dl, shape, variant)[1]
    tot, per = 0.0, 0.0
    for c0, c1 in ((0, 333), (333, B)):
        t, pl = shard.training_loss(X[:, c0:c1], P.GRAD_ALPHA, coeffs, kind, batch=B,
                                    cols=(c0, c1))
        t.backward()   # .grad accumulates over the shards
        tot, per = tot + float(t), per + pl.double().cpu().numpy()
    torch.cuda.synchronize()
    assert fwd == [2, 2, 2] and bwd == [0, 0, 0], (fwd, bwd)
    np.testing.assert_allclose(tot, float(tf), rtol=1e-5)
    np.testing.assert_allclose(per, pf.double().cpu().numpy(), rtol=1e-5)
    ps = dict(shard.named_parameters())
    for key, p in full.named_parameters():
        if p.grad is None:
            assert ps[key].grad is None, key
            continue
        e = nrel(ps[key].grad.cpu().numpy(), p.grad.cpu().numpy())
        print(f"shards {shape} {variant} {key}: {e:.3e}")
        parity.check(f"large column shards {shape} {variant}", "per_layer", key, e, 1e-5)


@pytest.mark.parametrize("shape,variant", C.SPLIT_WGRAD_CASES)
def test_large_split_wgrad(shape, variant, dl, flags, monkeypatch):
    """The split-f16 weight gradient on the per-layer backward (make_bwd_plan's x3w && !rev:
    16-column steps) at a 5 x 3 tiling: with the plan flag wgrad_f32 and without, every non-fc
    gradient bit-equal, fc* within 1e-5 and not bitwise equal (the f16 kernel ran), and the split
    run within the oracle's bar.

    Two facts of the code shape this case.  (1) The split kernel takes a launch only when the
    padded batch and the chunk are whole 32-column sub-chunks (wgrad_x3_fits; otherwise the whole
    launch is the fp32 kernel's, not single chunks): at B = 1,000 the padded batch is 1,008 =
    31.5 sub-chunks, so no launch takes it.  B = 561 (Bpad 576, 36 steps, 18 chunks of 32
    columns) is the smallest batch at this tiling where it does.  (2) The modules request the
    split weight gradient only after a split-f16 forward (ops.dladmm_backward: saved.path == 4),
    and past 256 x 512 the forward under "f32_split" is the fp32 per-layer one (path 2,
    test_split_falls_back_where_unsupported), so through the module alone both runs are the fp32
    kernel's, bit for bit -- asserted first.  The library's path is then driven by passing
    wgrad_split=True to ops.dladmm_backward under the module's autograd function."""
    d, net, X, _, _ = build(dl, shape, variant, precision="f32_split")
    K, kind = d["K"], C.loss_kind(variant)
    coeffs = P.loss_coeffs(K)

    def run(**override):
        with monkeypatch.context() as mp:
            fwd, bwd = record_paths(mp), record_bwd_paths(mp, **override)
            net = build(dl, shape, variant, precision="f32_split")[1]
            tot, _ = net.training_loss(X, P.GRAD_ALPHA, coeffs, kind)
            tot.backward()
            torch.cuda.synchronize()
            assert fwd == [2] and bwd == [0], (fwd, bwd)
        return net

    plain = grads_of(run())
    split_net = run(wgrad_split=True)
    split = grads_of(split_net)
    flags.set(wgrad_f32=True)
    f32 = grads_of(run(wgrad_split=True))
    flags.set(wgrad_f32=False)
    assert plain.keys() == split.keys() == f32.keys()
    wkeys = [k for k in f32 if k.startswith("fc")]
    assert len(wkeys) == K
    for k in f32:
        assert torch.equal(plain[k], f32[k]), k   # the module alone: the fp32 kernel
        a, b = split[k].double(), f32[k].double()
        if k in wkeys:
            assert not torch.equal(split[k], f32[k]), k
            e = float((a - b).norm() / b.norm())
            print(f"split wgrad {shape} {variant} {k}: {e:.3e}")
            parity.check(f"large split wgrad vs fp32 wgrad {shape} {variant}", "per_layer x3w", k,
                         e, 1e-5)
        else:
            assert torch.equal(split[k], f32[k]), k
    check_vs_oracle("large split wgrad vs oracle64", shape, variant, "train", split_net,
                    path="per_layer x3w")


@pytest.mark.parametrize("shape,variant", C.DETERMINISM_CASES)
def test_large_grads_deterministic(shape, variant, dl):
    a = grads_of(run_full_loss(dl, shape, variant)[1])
    b = grads_of(run_full_loss(dl, shape, variant)[1])
    assert a.keys() == b.keys() and a
    for k in a:
        assert torch.equal(a[k], b[k]), k
