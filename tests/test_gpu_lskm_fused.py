"""The learned + safeguarded KM forward as one launch (dladmm_lskm_f32, csrc/dladmm_lskm_fused.hip)
against the fp64-norm oracle (oracle/dladmm_oracle_lskm.py) and, bit for bit, against the
multi-launch path, at the test script's m = 250, n = 500 (padded rows of the 256 x 512 shape)."""
import ctypes

import numpy as np
import pytest
import torch

import problems as P

pytestmark = pytest.mark.gpu


def nrel(a, b):
    a = np.asarray(a.cpu().numpy(), np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make(dl, B, mu="None", mu_param=0.0, delta=-99.0, m=250, n=500, fused=None):
    d = dict(variant="v4", m=m, n=n, B=B, K=5, seed=1190 + B, perturb=0.2, wscale=0.9)
    inp, sd = P.build_problem(d)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    net = dl.DLADMMNetLSKM(m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]),
                           E0=t(inp["E0"]), L0=t(inp["L0"]), layers=5, alpha=0.01, delta=delta,
                           mu_k_method=mu, mu_k_param=mu_param, fused_safeguard=fused)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net, inp, sd, torch.from_numpy(inp["X"]).cuda()


@pytest.mark.parametrize("mu,param,delta,B", [
    ("EMA", 0.5, 0.05, 20), ("GS", 0.2, 0.0, 20), ("RT", 0.0, 0.0, 20), ("None", 0.0, 0.0, 20),
    ("EMA", 0.5, 0.05, 300), ("EMA", 0.5, 0.05, 1037)])
def test_fused_matches_oracle_and_multi_launch(mu, param, delta, B, dl):
    """B = 20: two groups, the second with 4 columns; 300 / 1037: many workgroups and a ragged
    tail.  Every decision of these cases is at least 5.6e-4 (relative) from its threshold, fp32
    GEMM-order effects are ~1e-6: the counts are exact and the two paths agree in every bit."""
    from oracle import dladmm_oracle_lskm as ol
    net, inp, sd, X = make(dl, B, mu, param, delta)
    Z, E, L, T, cnt = net(X, True, True, fused_safeguard=True)
    ref = ol.lskm_forward(inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, 5, True,
                          True, False, 5, 0.01, delta=delta, mu_method=mu, mu_param=param)
    np.testing.assert_array_equal(cnt, ref["sg_count"])
    if mu != "None":
        assert 0 < cnt.sum() < 5 * B   # both branches taken
    assert len(Z) == len(E) == len(L) == 5 and len(T) == 6 and cnt.dtype == np.float64
    for k in range(5):
        for got, want in ((Z[k], ref["Z"][k]), (E[k], ref["E"][k]), (L[k], ref["L"][k]),
                          (T[k + 1], ref["T"][k + 1])):
            assert nrel(got, want) <= 1e-5, k
    Z2, E2, L2, T2, cnt2 = net(X, True, True, fused_safeguard=False)
    np.testing.assert_array_equal(cnt, cnt2)
    for a, b in zip(Z + E + L + T, Z2 + E2 + L2 + T2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("delta,learned", [(-99.0, True), (2.0, False)])
def test_fused_delta_ends(delta, learned, dl):
    """delta = -99 keeps every learned step: the V4 forward.  delta = 2 makes the threshold
    negative: every valid column is safeguarded in every layer (count == B: none of the 12
    padding columns of the second group is counted) and the run is the pure KM iteration."""
    B = 20
    net, _, _, X = make(dl, B, "EMA", 0.5, delta)
    Z, E, L, T, cnt = net(X, True, True, fused_safeguard=True)
    np.testing.assert_array_equal(cnt, np.full(5, 0.0 if learned else B))
    ref = net(X, learned, False, K=5)
    for a, b in zip(Z + E + L + T, ref[0] + ref[1] + ref[2] + ref[3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("field,value,code", [
    ("X", None, "NULL"), ("count", None, "NULL"), ("workspace", None, "NULL"),
    ("m", 257, "UNSUPPORTED"), ("n", 513, "UNSUPPORTED"), ("abi_version", 1, "ABI_VERSION")])
def test_descriptor_validation(field, value, code, dl):
    lib = dl._lib
    d = lib.LskmDesc()
    d.abi_version = lib.ABI_VERSION
    d.m, d.n, d.batch, d.layers = 250, 500, 20, 2
    fake = 1 << 40  # never dereferenced: validation only
    for f in ("X", "A", "Z0", "E0", "L0", "scalar_params", "km_params", "Z", "E", "L", "T",
              "count", "workspace"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = 20
    d.ld_a, d.ld_w = 500, 250
    w = lib.ptr_array([fake, fake])
    d.W = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    d.workspace_bytes = 1 << 30
    setattr(d, field, value)
    codes = dict(NULL=-5, UNSUPPORTED=-7, ABI_VERSION=-1)   # include/dladmm.h DLADMM_E_*
    assert lib.lib().dladmm_lskm_f32(ctypes.byref(d), None) == codes[code]


def test_fused_required_past_register_shape(dl):
    net, _, _, X = make(dl, 4, m=512, n=2048, fused=True)
    with pytest.raises(ValueError):
        net(X, True, True)
