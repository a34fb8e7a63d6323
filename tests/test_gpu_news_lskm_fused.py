"""The newS safeguarded LSKM forward as one launch (dladmm_lskm_news_f32,
csrc/dladmm_lskm_news_fused.hip) against the fp64 restatement (tests/news_lskm_ref.py), the
reference class's fixtures and, bit for bit, the multi-launch path."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import parity
import problems as P
import problems_news as PN
from test_gpu_news_lskm import make, t
from test_news_lskm_cpu import ref_forward

pytestmark = pytest.mark.gpu


def case_of(script, variant, B, layers, seed, mu, param, delta, **extra):
    d = dict(variant=variant, m=250, n=500, B=B, K=layers, seed=seed, perturb=0.2, wscale=0.9,
             **extra)
    return dict(script=script, defn=d, layers=layers, alpha=0.01, delta=delta, mu=mu,
                mu_param=param, learned=True, safeguard=True, continued=False, K=layers)


CASES = {
    "ema20": case_of("news", "v7", 20, 5, 2210, "EMA", 0.5, 0.05),
    "gs20": case_of("news", "v7", 20, 5, 2210, "GS", 0.1, 0.0),
    "rt20": case_of("news", "v7", 20, 5, 2210, "RT", 0.0, 0.1),
    "none20": case_of("news", "v7", 20, 5, 2210, "None", 0.0, 0.0),
    "ema300": case_of("news", "v7", 300, 5, 2490, "EMA", 0.5, 0.05),
    "ema1037": case_of("news", "v7", 1037, 5, 3227, "EMA", 0.5, 0.05),
    "tied": case_of("tied", "v7t", 20, 6, 2250, "EMA", 0.5, 0.05),
    "ptied": case_of("ptied", "v7p", 20, 6, 2251, "EMA", 0.5, 0.05, interval=2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_matches_restatement_and_multi_launch(name, dl):
    """m = 250, n = 500: padded rows of the 256 x 512 shape.  B = 20: two workgroups, the second
    with 4 valid columns; 300 / 1,037: many workgroups and a ragged tail.  A column whose fp64
    decision margin is below 1e-4 at some layer is left out from that layer on: at most 1 %."""
    case = CASES[name]
    inp, sd = P.build_problem(case["defn"])
    B, nl = inp["X"].shape[1], case["layers"]
    net = make(dl, case, inp, sd)
    net.prepend_init = False   # the layers' triples alone
    X = t(inp["X"]).cuda()
    Z, E, L, cnt = net(X, True, True, fused_safeguard=True)
    mask = net.sg_mask.cpu().numpy()
    ref = ref_forward(case, inp, sd)
    assert len(Z) == len(E) == len(L) == nl and cnt.dtype == np.float64
    ok = np.ones(B, bool)
    oks = []
    for k in range(nl):
        ok &= ref["margin"][k] >= 1e-4
        oks.append(ok.copy())
        assert ok.sum() >= 0.99 * B, (k, int(ok.sum()))
        np.testing.assert_array_equal(mask[k][ok] != 0, ref["keep"][k][ok])
        for got, nm in ((Z, "Z"), (E, "E"), (L, "L")):
            assert parity.nrel(got[k].cpu().numpy()[:, ok], ref[nm][k][:, ok]) <= 1e-5, (nm, k)
    if ok.all():
        np.testing.assert_array_equal(cnt, ref["sg_count"])
    if case["mu"] == "EMA":
        assert 0 < cnt.sum() < nl * B   # both branches ran
    Z2, E2, L2, cnt2 = net(X, True, True, fused_safeguard=False)
    mask2 = net.sg_mask.cpu().numpy()
    for k in range(nl):
        okc = torch.from_numpy(oks[k]).cuda()
        np.testing.assert_array_equal(mask[k][oks[k]], mask2[k][oks[k]])
        for a, b in ((Z[k], Z2[k]), (E[k], E2[k]), (L[k], L2[k])):
            assert torch.equal(a[:, okc], b[:, okc]), k


@pytest.mark.parametrize("name", ["news_lskm_sg_ema_small", "news_lskm_acols_sg_ema",
                                  "news_lskm_tied_sg_ema", "news_lskm_ptied_sg_gs"])
def test_fused_matches_reference_fixture(name, dl):
    """16 x 32 zero-padded to the 256 x 512 shape (exact): the k - 1 / k parameter rows, layer 0,
    the tied scaling and the partially tied weight index against values the reference produced."""
    g, meta = load_golden(name)
    case = meta["case"]
    inp, sd = PN.build_problem(case["defn"])
    net = make(dl, case, inp, sd, fused_safeguard=True)
    out = net(t(inp["X"]).cuda(), True, True, False, K=case["K"])
    assert len(out) == 4
    assert len(out[0]) == len(out[1]) == len(out[2]) == int(g["n_out"])
    np.testing.assert_array_equal(out[3], g["sg_count"])
    for i, j in enumerate(g["layers_kept"]):
        for c, nm in enumerate("ZEL"):
            gap = float(g["gap_" + nm][i])
            parity.check(name, "f32", f"{nm}[{int(j)}]",
                         parity.nrel(out[c][j].cpu().numpy(), g[nm][i]), parity.tol(gap), gap)


@pytest.mark.parametrize("delta,learned", [(-99.0, True), (2.0, False)])
def test_fused_delta_ends(delta, learned, dl):
    """delta = -99 keeps every learned step: the learned newS forward.  delta = 2 makes the
    threshold negative: every valid column is safeguarded in every layer (count == B: none of the
    12 padding columns of the second workgroup is counted) and the run is the pure KM iteration."""
    case = dict(CASES["ema20"], delta=delta)
    inp, sd = P.build_problem(case["defn"])
    net = make(dl, case, inp, sd)
    X = t(inp["X"]).cuda()
    Z, E, L, cnt = net(X, True, True, fused_safeguard=True)
    np.testing.assert_array_equal(cnt, np.full(5, 0.0 if learned else 20.0))
    ref = net(X, learned, False, K=5)
    for a, b in zip(Z + E + L, ref[0] + ref[1] + ref[2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("field,value,code", [
    ("X", None, "NULL"), ("count", None, "NULL"), ("workspace", None, "NULL"),
    ("m", 257, "UNSUPPORTED"), ("n", 513, "UNSUPPORTED"), ("abi_version", 1, "ABI_VERSION")])
def test_descriptor_validation(field, value, code, dl):
    lib = dl._lib
    d = lib.LskmNewsDesc()
    d.abi_version = lib.ABI_VERSION
    d.m, d.n, d.batch, d.layers = 250, 500, 20, 2
    fake = 1 << 40  # never dereferenced: validation only
    for f in ("X", "A", "Z0", "E0", "L0", "scalar_params", "km_params", "inv_bs", "Z", "E", "L",
              "count", "workspace"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = 20
    d.ld_a, d.ld_w = 500, 250
    w = lib.ptr_array([fake, fake])
    d.W = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    d.workspace_bytes = 1 << 30
    setattr(d, field, value)
    codes = dict(NULL=-5, UNSUPPORTED=-7, ABI_VERSION=-1)   # include/dladmm.h DLADMM_E_*
    assert lib.lib().dladmm_lskm_news_f32(ctypes.byref(d), None) == codes[code]


def test_fused_required_past_register_shape(dl):
    case = dict(CASES["ema20"], defn=dict(CASES["ema20"]["defn"], m=512, n=2048, B=4))
    inp, sd = P.build_problem(case["defn"])
    net = make(dl, case, inp, sd, fused_safeguard=True)
    with pytest.raises(ValueError):
        net(t(inp["X"]).cuda(), True, True)
