"""The fused kernel's weight ring (csrc/dladmm_fused_kernel.h, csrc/dladmm_ring_windows.h) on the
device: every instantiation's ring shape, with the counted windows and the piece schedule the
library was built with.  tests/test_ring_windows.py proves the counts on the host; a count that is
wrong all the same, or a piece issued into a slot that is still read, shows here as a result that
changes from run to run, that depends on what the buffers held before, or that differs from an
independent computation.

Problem sizes per ring shape: (20, 24) one chunk per GEMM and pieces of a chunk shorter than 16
fragments; (64, 256) and (50, 200) 64 fragments per GEMM (four chunks of 16, or two of 32 in the
two-slot ring); (256, 512) and (200, 500) 512 fragments (thirty-two chunks, or sixteen).  K = 1 ends on the filler stream; B = 1 .. 130 covers a ragged last tile and more than
one workgroup.  Everything runs on path 1 (plan flag no_rowsplit).

Checked: three runs are equal bit for bit; a run whose outputs and workspace come from NaN-filled
memory equals them; the second call, which reads the cached prologue product (the load form),
equals them; at the 256 x 512 instantiation V1 / V4 / V5 / V6 equal path 5 (the row-split kernel,
whose source this ring does not touch) bit for bit; every other variant and shape is held to the
fp32 parity bar against the oracle (parity.check_f32)."""
import pytest
import torch

import problems as P
from test_gpu_news_lskm import E_SLOTS, make as make_news, t as to_t
from test_gpu_p0_reuse import _fwd, _net, _same
from test_gpu_parity import _compare, _oracle_case, make_net
from test_gpu_poison import poison

pytestmark = pytest.mark.gpu

SMALL, MID, MIDP, BIG, BIGP = (20, 24), (64, 256), (50, 200), (256, 512), (200, 500)
# V1 .. V6 on the middle shape; V4, and V1 with its counted beta loads, on every shape
CASES = [(v, MID) for v in ("v1", "v2", "v3", "v4", "v5", "v6")] + \
        [(v, s) for v in ("v1", "v4") for s in (SMALL, MIDP, BIG, BIGP)] + \
        [("v5", BIG), ("v6", BIGP), ("v3", BIG)]
KS = (1, 2, 5)
BS = (1, 16, 65, 130)


def _poisoned(dl, K, m, n, B):
    dl.ops._WS.clear()  # a fresh workspace too
    poison([(K, n, B), (K, m, B), (K, m, B), (K + 1, m, B)], 64 << 20)


@pytest.mark.parametrize("variant,shape", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_repeatable_poisoned_cached(variant, shape, dl):
    m, n = shape
    for K in KS:
        for B in BS:
            net, X = _net(dl, variant, m, n, B, K, 8100 + 7 * B + K, reuse=False)
            # keep_all with the saved products (the training forward) and the fused objective;
            # lean without either; and the two mixed
            for keep_all, lk, want_P in ((True, dl._lib.LOSS_L1L1, True), (False, 0, False),
                                         (True, 0, False), (False, dl._lib.LOSS_L1L1, False)):
                tag = (variant, shape, K, B, keep_all, lk)
                net.reuse_prologue = False
                ref = _fwd(dl, net, X, keep_all, lk, want_P)
                for rep in range(2):
                    _same(_fwd(dl, net, X, keep_all, lk, want_P), ref, tag + ("repeat", rep))
                _poisoned(dl, K, m, n, B)
                _same(_fwd(dl, net, X, keep_all, lk, want_P), ref, tag + ("poisoned",))
                net.reuse_prologue = True
                net.invalidate_cache()
                fill = _fwd(dl, net, X, keep_all, lk, want_P)
                again = _fwd(dl, net, X, keep_all, lk, want_P)
                assert not fill.p0_reused and again.p0_reused, tag
                _same(fill, ref, tag + ("fill",))
                _same(again, ref, tag + ("load form",))
                _poisoned(dl, K, m, n, B)
                net.invalidate_cache()
                _fwd(dl, net, X, keep_all, lk, want_P)
                _same(_fwd(dl, net, X, keep_all, lk, want_P), ref, tag + ("load form poisoned",))


@pytest.mark.parametrize("variant", ["v1", "v4", "v5", "v6"])
@pytest.mark.parametrize("shape", [BIG, BIGP], ids=str)
def test_big_shape_bit_equal_to_path5(variant, shape, dl):
    m, n = shape
    for K in KS:
        for B in BS:
            net, X = _net(dl, variant, m, n, B, K, 8200 + 7 * B + K, reuse=True)
            kw = dict(keep_all=True, want_T=True, want_P=True, loss_kind=dl._lib.LOSS_L1L1,
                      **net._tables(X.device))
            args = (net.VARIANT, X, net.A, [w.detach() for w in net._weights()], net.Z0, net.E0,
                    net.L0)
            with torch.no_grad():
                with dl.ops.plan_flags(no_xsplit=True):
                    rs = dl.ops.dladmm_forward(*args, **kw)
                fu = [_fwd(dl, net, X, True, dl._lib.LOSS_L1L1, True) for _ in range(2)]
            torch.cuda.synchronize()
            assert rs.path == 5 and not fu[0].p0_reused and fu[1].p0_reused
            for r in fu:
                for nm in ("Z", "E", "L", "T", "P"):
                    assert torch.equal(getattr(r, nm), getattr(rs, nm)), (variant, shape, K, B, nm)


ORACLE = [(v, s) for v in ("v1", "v2", "v3", "v4", "v5", "v6") for s in (MID,)] + \
         [(v, s) for v in ("v1", "v4") for s in (SMALL, MIDP)] + [("v2", BIGP), ("v3", BIG)]


@pytest.mark.parametrize("variant,shape", ORACLE, ids=lambda c: str(c).replace(" ", ""))
def test_vs_oracle(variant, shape, dl, oracle):
    m, n = shape
    for K, B in ((5, 130), (1, 65), (2, 16)):
        inp, sd, ref = _oracle_case(oracle, variant, m, n, B, K, seed=8300 + B,
                                    wscale=0.4 if variant in ("v1", "v2") else None)
        net = make_net(dl, variant, inp, sd, K).cuda()
        X = torch.from_numpy(inp["X"]).cuda()
        for call in ("compute form", "load form"):
            r = _fwd(dl, net, X)
            assert bool(r.p0_reused) == (call == "load form")
            # the outputs the reference returns (V1 .. V3 return no T)
            out = tuple(list(getattr(r, nm)) for nm in "ZELT" if nm in ref["r64"])
            _compare(out, ref, tag=f"ring {variant} {shape} K={K} B={B} {call}")


@pytest.mark.parametrize("shape", [SMALL, MID, BIGP], ids=str)
def test_news_elz_units(shape, dl, flags):
    """The ELZ instantiations (the newS loop's entry, V4 and V7): steps E, L, Z from (Z_0, E0, L0)
    equal the plain fused run's layers bit for bit, repeatably and from poisoned memory."""
    m, n = shape
    B, K = 65, 5
    lib = dl._lib
    defn = dict(variant="v7", m=m, n=n, B=B, K=K, seed=8400, perturb=0.2, wscale=0.9)
    inp, sd = P.build_problem(defn)
    case = dict(script="news", defn=defn, layers=K, alpha=0.01, delta=-99.0, mu="None",
                mu_param=0.0)
    net = make_news(dl, case, inp, sd)
    X = to_t(inp["X"]).cuda()
    flags.set(no_rowsplit=True)
    ptab = net._tables(X.device)["scalar_params"]
    W = [w.detach() for w in net._weights()]
    etab = ptab.clone()
    etab[1:, E_SLOTS] = ptab[:-1, E_SLOTS]
    km = net._km_table(K)
    At = [net.A.t().contiguous()] * K
    with torch.no_grad():
        for v, tab, etb, Ws in ((lib.V4_SCALAR, ptab, etab, W), (lib.V7_SCALAR_V1E, km, km, At)):
            z = dl.dladmm_forward(v, X, net.A, Ws, net.Z0, net.E0, net.L0, scalar_params=tab,
                                  keep_all=True, want_T=True)
            for trial in range(3):
                if trial == 2:
                    _poisoned(dl, K, m, n, B)
                e = net._elz(v, X, z.Z[0], net.E0, net.L0, Ws[1:], etb[1:].contiguous(),
                             want_T=True)
                et = net._elz(v, X, z.Z[0], net.E0, net.L0, Ws[1:], etb[1:].contiguous(),
                              tail=True)
                torch.cuda.synchronize()
                assert e.path == 1 and et.path == 1
                assert torch.equal(e.Z, z.Z[1:]), (shape, v, trial, "Z")
                assert torch.equal(e.E, z.E[:K - 1]), (shape, v, trial, "E")
                assert torch.equal(e.L, z.L[:K - 1]), (shape, v, trial, "L")
                assert torch.equal(e.T[:K - 1], z.T[1:K]), (shape, v, trial, "T")
                assert torch.equal(et.Z, e.Z) and torch.equal(et.E, e.E) and \
                    torch.equal(et.L, e.L), (shape, v, trial, "tail")
                assert torch.equal((et.P[:K - 1] + et.E) - X, e.T[:K - 1]), (shape, v, trial, "P")
