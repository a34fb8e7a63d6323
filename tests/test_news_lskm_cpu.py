"""The newS test classes (d-ladmm_amd/lskm_news.py) without a device: the fp64 restatement
tests/news_lskm_ref.py pinned to the reference class's fixtures, construction / state_dict /
argument errors of the three product classes, and descriptor validation of the new C entry
points (variant V7, DLADMM_F_ELZ, dladmm_safeguard_news_f32)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import news_lskm_ref as R
import parity
import problems_news as PN
from test_capi import _desc


def ref_forward(case, inp, sd, **kw):
    d = case["defn"]
    return R.forward(inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, case["layers"],
                     case["learned"], case["safeguard"], case["continued"], case["K"],
                     case["alpha"], delta=case["delta"], mu_method=case["mu"],
                     mu_param=case["mu_param"], fc=PN.FC[case["script"]],
                     interval=d.get("interval", 1), **kw)


def outputs(case, inp, r):
    """Z / E / L lists as the script returns them (_Acols: the initial triple in front)."""
    pre = case["script"] != "news"
    return [([inp[nm + "0"]] if pre else []) + r[nm] for nm in "ZEL"]


@pytest.mark.parametrize("name", sorted(PN.NEWS_LSKM_FIXTURES))
def test_restatement_matches_reference_fixture(name):
    g, meta = load_golden(name)
    case = meta["case"]
    assert case == PN.NEWS_LSKM_FIXTURES[name]
    inp, sd = PN.build_problem(case["defn"])
    r = ref_forward(case, inp, sd)
    out = outputs(case, inp, r)
    assert len(out[0]) == int(g["n_out"])
    for i, j in enumerate(g["layers_kept"]):
        for c, nm in enumerate("ZEL"):
            gap = float(g["gap_" + nm][i])
            parity.check(name, "ref64", f"{nm}[{int(j)}]", parity.nrel(out[c][j], g[nm][i]),
                         parity.tol(gap), gap)
    if "sg_count" in g.files:
        np.testing.assert_array_equal(r["sg_count"], g["sg_count"])
        assert float(g["min_margin"]) >= PN.MIN_MARGIN
        np.testing.assert_allclose(np.stack(r["snorm"]), g["snorm64"], rtol=1e-9)
        np.testing.assert_allclose(np.stack(r["margin"]), g["margin"], rtol=1e-6, atol=1e-12)


def build(dl, script, m=16, n=32, B=8, layers=4, **kw):
    g = torch.Generator().manual_seed(5)
    A = torch.randn(m, n, generator=g)
    A = A / A.norm(dim=0, keepdim=True)
    extra = {"interval": 2} if script == "ptied" else {}
    cls = getattr(dl, PN.CLASSES[script])
    return cls(m=m, n=0, d=n, batch_size=B, A=A, Z0=torch.zeros(n, B), E0=torch.zeros(m, B),
               L0=torch.zeros(m, B), layers=layers, **extra, **kw)


TRAIN = {"news": "DLADMMNetNewS", "tied": "DLADMMNetTiedNewS", "ptied": "DLADMMNetPTiedNewS"}


@pytest.mark.parametrize("script", ["news", "tied", "ptied"])
def test_construction_and_checkpoint(script, dl):
    net = build(dl, script, alpha=0.02, delta=0.05, mu_k_method="EMA", mu_k_param=0.5)
    assert (net.alpha, net.delta, net.mu_k_method, net.num_iter) == (0.02, 0.05, "EMA", 200)
    assert net.prepend_init == (script != "news")
    assert net.name() == ("DLADMMNet_scalar_ptied2_newS_layerwise" if script == "ptied"
                          else "DLADMMNet")
    # the test scripts' init: thresholds 0.2 / 0.8, fc = A^T + 1e-3 N(0, 1) (no 0.4 scale)
    assert float(net.active_para[0]) == pytest.approx(0.2)
    assert float(net.active_para1[0]) == pytest.approx(0.8)
    fc0 = net.fc.weight if script == "tied" else net.fc[0].weight
    assert float((fc0.detach().cpu() - net.A.t().cpu()).abs().max()) < 1e-2
    # same keys, same order as the newS training model; its checkpoint loads strictly
    extra = {"interval": 2} if script == "ptied" else {}
    train = getattr(dl, TRAIN[script])(m=16, n=0, d=32, batch_size=8, A=net.A.cpu(),
                                       Z0=torch.zeros(32, 8), E0=torch.zeros(16, 8),
                                       L0=torch.zeros(16, 8), layers=4, **extra)
    sd = train.state_dict()
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k


@pytest.mark.parametrize("name", ["news_lskm_sg_ema_small", "news_lskm_tied_sg_ema",
                                  "news_lskm_ptied_sg_ema"])
def test_reference_key_order(name, dl):
    _g, meta = load_golden(name)
    net = build(dl, meta["case"]["script"], layers=6)
    assert list(net.state_dict().keys()) == meta["keys"]


def test_argument_errors(dl):
    with pytest.raises(NotImplementedError):
        build(dl, "news", mu_k_method="RM")
    with pytest.raises(ValueError):
        build(dl, "tied", mu_k_method="XX")
    net = build(dl, "news")
    x = torch.zeros(16, 8)
    with pytest.raises(AssertionError):
        net(x, False, True, False)
    with pytest.raises(IndexError):
        net(x, True, False, False, K=5)
    with pytest.raises(IndexError):
        net(x, True, True, False, K=5)


# ------------------------------------------------------------------ C ABI (host-only calls)
def test_v7_plan_and_refusals(dl):
    L, lib = dl._lib.lib(), dl._lib
    d, _k = _desc(dl, variant=lib.V7_SCALAR_V1E, batch=20, loss_kind=0, loss_sums=None)
    assert L.dladmm_fwd_path(ctypes.byref(d)) == 6
    d.flags = lib.F_NO_XSPLIT
    assert L.dladmm_fwd_path(ctypes.byref(d)) == 5
    d.flags = lib.F_NO_ROWSPLIT
    assert L.dladmm_fwd_path(ctypes.byref(d)) == 1
    assert L.dladmm_fwd_workspace_bytes(ctypes.byref(d)) > 0
    for kw in (dict(flags=lib.F_PER_LAYER), dict(precision=lib.PREC_F32_SPLIT),
               dict(precision=lib.PREC_BF16), dict(P=1 << 40), dict(m=300, ld_w=300), dict(n=600, ld_a=600)):
        bad, _k2 = _desc(dl, variant=lib.V7_SCALAR_V1E, batch=20, loss_kind=0, loss_sums=None,
                         **kw)
        assert L.dladmm_fwd_path(ctypes.byref(bad)) == -7, kw
        assert L.dladmm_fwd_workspace_bytes(ctypes.byref(bad)) == 0
        assert L.dladmm_fwd_f32(ctypes.byref(bad), None) == -7
    d, _k = _desc(dl, variant=8)
    assert L.dladmm_fwd_path(ctypes.byref(d)) == -2
    # no backward
    b = lib.BwdDesc()
    f, _k3 = _desc(dl, variant=lib.V7_SCALAR_V1E, batch=20, loss_kind=0, loss_sums=None)
    ctypes.memmove(ctypes.byref(b.fwd), ctypes.byref(f), ctypes.sizeof(f))
    b.gW, b.ld_gw = 1 << 40, 256
    assert L.dladmm_bwd_path(ctypes.byref(b)) == -7
    assert L.dladmm_bwd_workspace_bytes(ctypes.byref(b)) == 0


def test_elz_plan_and_refusals(dl):
    L, lib = dl._lib.lib(), dl._lib
    base = dict(batch=20, loss_kind=0, loss_sums=None)
    for v in (lib.V4_SCALAR, lib.V5_TIED, lib.V7_SCALAR_V1E):
        d, _k = _desc(dl, variant=v, flags=lib.F_ELZ, **base)
        assert L.dladmm_fwd_path(ctypes.byref(d)) == 5      # never the four-workgroup split
        d.flags = lib.F_ELZ | lib.F_NO_ROWSPLIT
        assert L.dladmm_fwd_path(ctypes.byref(d)) == 1
        d.flags = lib.F_ELZ | lib.F_ELZ_TAIL
        assert L.dladmm_fwd_path(ctypes.byref(d)) == -7     # the tail needs P
        d.P = 1 << 40
        assert L.dladmm_fwd_path(ctypes.byref(d)) == 5
    # the P0 flags do not act on an ELZ call: same workspace
    d, _k = _desc(dl, flags=lib.F_ELZ | lib.F_NO_ROWSPLIT, **base)
    ws = L.dladmm_fwd_workspace_bytes(ctypes.byref(d))
    d.flags |= lib.F_P0_SAVE
    assert L.dladmm_fwd_workspace_bytes(ctypes.byref(d)) == ws > 0
    for kw in (dict(variant=lib.V6_LASSO), dict(keep_all=0),
               dict(loss_kind=1, loss_sums=1 << 40), dict(precision=lib.PREC_F32_SPLIT),
               dict(m=300, ld_w=300), dict(flags=lib.F_ELZ | lib.F_PER_LAYER)):
        args = dict(base, flags=lib.F_ELZ)
        args.update(kw)
        bad, _k2 = _desc(dl, **args)
        assert L.dladmm_fwd_path(ctypes.byref(bad)) == -7, kw
    d, _k = _desc(dl, flags=lib.F_ELZ_TAIL, P=1 << 40, **base)
    assert L.dladmm_fwd_path(ctypes.byref(d)) == -7         # the tail without the ELZ entry


def _sg_desc(dl, **kw):
    d = dl._lib.SafeguardNewsDesc()
    d.abi_version = dl._lib.ABI_VERSION
    d.m, d.n, d.batch, d.ld = 16, 32, 8, 8
    for f in ("X", "Zl", "El", "Ll", "Zk", "Ek", "Lk", "En", "Znn", "Pn", "Pnn", "Zo", "Eo",
              "Lo", "mu", "count", "inv_bs"):
        setattr(d, f, 1 << 40)   # never dereferenced: every case below fails validation
    d.updater = dl._lib.MU_EMA
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("field,value,code", [
    ("abi_version", 5, -1), ("m", 0, -3), ("batch", 0, -3), ("ld", 7, -3), ("updater", 4, -7),
    ("updater", -1, -7), ("X", None, -5), ("Pnn", None, -5), ("inv_bs", None, -5),
    ("mu", None, -5), ("Ek", None, -5), ("count", None, -5), ("Lo", None, -5),
])
def test_safeguard_news_validation(dl, field, value, code):
    L = dl._lib.lib()
    assert L.dladmm_safeguard_news_f32(ctypes.byref(_sg_desc(dl, **{field: value})), None) == code
    assert L.dladmm_safeguard_news_f32(None, None) == -5
