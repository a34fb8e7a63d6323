"""The backward's results do not depend on what its workspace held: with every cached workspace
buffer (ops._WS, one per device and stream, shared by the forward and backward of every model)
set to 0x00 bytes and to 0xFF bytes -- NaN as fp32 and as fp64 -- between the forward and
loss.backward(), the gradients are bit-equal and finite, on every backward path.

The forward tests of this kind are tests/test_gpu_poison.py; the backward has the larger
workspace and the claims that rest on reading the code: the reverse sweeps zero only their
parameter partials (and hand-off counters) and the weight gradient's padding rows, and never the
V2 / V3 per-row partials (every entry the reduction reads is written by the
wave that owns the row); the per-layer phases zero their adjoint buffers and partials but not the
packed operands or the weight-gradient partials; bwd path 3 stores NaN on purpose after a
timed-out hand-off, into a buffer the next call on the stream gets back.  In a training loop over
one model the stale bytes are the previous step's identical values, so a missing zero-fill shows
only when shapes or models alternate -- or here.

The fill sits between forward and backward so the forward's own leftovers are replaced too:
nothing the forward saves for the backward lives in the workspace.
"""
import pytest
import torch

import bwd_large_cases as C
import problems as P
from test_gpu_backward import make_train_net, record_paths, total_loss
from test_gpu_backward_large import record_bwd_paths

pytestmark = pytest.mark.gpu


def case(variant, m, n, B, K, want, precision="f32", shape=None, **plan):
    tag = "-".join([variant, f"{m}x{n}", f"b{B}", precision] + sorted(plan) + [f"path{want}"])
    return pytest.param(dict(variant=variant, m=m, n=n, B=B, K=K, want=want, precision=precision,
                             shape=shape, plan=plan), id=tag)


CASES = []
# bwd path 1, the 64-column reverse sweep.  The scalar variants take the row-split forward at
# this batch by default (paths 5 / 6, whose backward is path 2 / 3: below), so their sweep is
# selected with no_rowsplit; V2 / V3 (default plan) and the split-f16 forward (B = 72, a
# multiple of 4) run it unasked.  V2 / V3: the never-zeroed per-row partials, at a row stride
# (120 / 500) below the kernel's padded rows; f32_split: the split weight gradient's operand
# columns padded to 32.
CASES += [case(v, 96, 200, 70, 4, 1, no_rowsplit=True) for v in ("v4", "v1", "v5", "v6")]
CASES += [case(v, m, n, B, 3, 1) for v in ("v2", "v3") for m, n, B in ((100, 120, 70),
                                                                       (250, 500, 77))]
CASES += [case("v4", 96, 200, 72, 4, 1, precision="f32_split")]
# bwd path 3 (after the four-workgroup forward, as planned) and 2 (no_xsplit); V2 / V3 take the
# row-split kernels under rowsplit_rows
for B in (20, 300):
    CASES += [case(v, 250, 500, B, 3, 3) for v in ("v4", "v1")]
    CASES += [case(v, 250, 500, B, 3, 2, no_xsplit=True) for v in ("v4", "v1")]
    CASES += [case(v, 250, 500, B, 3, 3, rowsplit_rows=True) for v in ("v2", "v3")]
    CASES += [case(v, 250, 500, B, 3, 2, rowsplit_rows=True, no_xsplit=True) for v in ("v2", "v3")]
# bwd path 0, the per-layer phases: forced where the sweep would run (with the forward's saved
# products: BK1 fused into BK3's launch, both partial buffers), and on the natural plan past
# 256 x 512 (tests/bwd_large_cases.py)
CASES += [case(v, 96, 200, 70, 4, 0, bwd_per_layer=True) for v in ("v4", "v3")]
CASES += [case(v, 300, 530, 333, 3, 0, shape="300x530_b333") for v in ("v4", "v3", "v1")]


def problem(c):
    if c["shape"] is not None:
        d, inp, sd, up = C.problem(c["shape"], c["variant"])
        return d, inp, sd, up
    d = dict(variant=c["variant"], m=c["m"], n=c["n"], B=c["B"], K=c["K"], seed=9800,
             perturb=0.1)
    if c["variant"] in ("v1", "v2"):
        d["wscale"] = 0.4
    inp, sd = P.build_problem(d)
    return d, inp, sd, P.make_upstream(d, P.VARIANT_SPECS[c["variant"]]["ret_t"])


@pytest.mark.parametrize("mode", ["cotangents", "training_loss"])
@pytest.mark.parametrize("c", CASES)
def test_backward_from_poisoned_workspace(c, mode, dl, flags, monkeypatch):
    d, inp, sd, up = problem(c)
    K, variant = d["K"], c["variant"]
    kind = C.loss_kind(variant)
    flags.set(**c["plan"])
    fwd, bwd = record_paths(monkeypatch), record_bwd_paths(monkeypatch)
    net = make_train_net(dl, variant, inp, sd, K, precision=c["precision"])
    X = torch.from_numpy(inp["X"]).cuda()
    A = torch.from_numpy(inp["A"]).cuda()

    def step(fill):
        net.zero_grad(set_to_none=True)
        if mode == "training_loss":
            loss = net.training_loss(X, P.GRAD_ALPHA, P.loss_coeffs(K), kind)[0]
        else:
            loss = total_loss(net(X), X, A, up, kind, K)
        held = None
        if fill is not None:
            assert dl.ops._WS, "no cached workspace"
            for buf in dl.ops._WS.values():
                buf.fill_(fill)
            held = {k: (b.data_ptr(), b.numel()) for k, b in dl.ops._WS.items()}
        loss.backward()
        torch.cuda.synchronize()
        if held is not None:   # the backward ran in the buffers that were filled
            assert {k: (b.data_ptr(), b.numel()) for k, b in dl.ops._WS.items()} == held
        return {k: p.grad.detach().clone() for k, p in net.named_parameters()
                if p.grad is not None}

    first = step(None)   # sizes the cached workspace
    g00, gff = step(0x00), step(0xFF)
    assert bwd == [c["want"]] * 3, (fwd, bwd)
    if c["want"] == 0 and not c["plan"]:
        assert fwd == [2] * 3, fwd
    assert first and first.keys() == g00.keys() == gff.keys()
    for k in g00:
        assert torch.isfinite(gff[k]).all() and torch.isfinite(g00[k]).all(), k
        assert torch.equal(gff[k], g00[k]), f"{k}: differs between a 0x00 and a 0xFF workspace"
        assert torch.equal(first[k], g00[k]), f"{k}: differs from the first run"
