"""DLADMMNetLenaLSKM (test_lena_lskm.py's V1 class): the one-launch safeguarded forward
(dladmm_lskm_lena_f32, csrc/dladmm_lskm_lena_fused.hip) against a plain numpy restatement of
test_lena_lskm.py:91-188 in fp64 and, bit for bit, against the multi-launch path, at m = 250,
n = 500 (padded rows of the 256 x 512 shape; B = 20: a second group with 4 valid columns)."""
import ctypes

import numpy as np
import pytest
import torch

import parity
import problems as P

pytestmark = pytest.mark.gpu
K = 6


def ref_lskm(inp, sd, K, alpha, delta, mu, param, dtype=np.float64):
    """test_lena_lskm.py:91-188 with use_learned = use_safeguard = True; mu_updater.py's step."""
    f = dtype
    X, A, Z, E, L = (np.asarray(inp[k], f) for k in ("X", "A", "Z0", "E0", "L0"))
    A32 = np.asarray(inp["A"], np.float32)
    lip = np.float32(np.linalg.norm(A32.T @ A32, ord=2))             # :56, fp32 in every dtype
    ss1 = f(1.0) / np.sqrt(f(lip))
    act = lambda x, th: np.maximum(x - th, 0) - np.maximum(-x - th, 0)  # noqa: E731

    def S(Zk, Ek, Lk, Tk):                                           # :91-106
        Zn = act(Zk - ss1 * (A.T @ (Lk + ss1 * Tk)), ss1 * f(alpha))
        En = act(Ek - f(0.5) * (Lk + ss1 * (A @ Zn + Ek - X)), f(0.5))
        Tn = A @ Zn + En - X
        return Zn, En, Tn, Lk + ss1 * Tn

    T = A @ Z + E - X
    mu_k = np.sqrt((S(Z, E, L, T)[2] ** 2).sum(0))                   # :120
    out = dict(Z=[], E=[], L=[], cnt=np.zeros(K), margin=np.inf)
    for k in range(K):
        b1, b2 = (np.asarray(sd[f"beta{i}.{k}"], f) for i in (1, 2))
        Zk, Ek, Tk, Lk = S(Z, E, L, T)
        Zl = act(Z - np.asarray(sd[f"fc.{k}.weight"], f) @ (L + b1 * T), f(0.025))
        El = act(X - A @ Zl - b2 * L, f(0.06))
        Tl = A @ Zl + El - X
        Ll = L + b1 * Tl
        nrm = np.sqrt((S(Zl, El, Ll, Tl)[2] ** 2).sum(0))            # :151-152
        thr = f(1.0 - delta) * mu_k
        keep = nrm < thr                                             # :156
        out["margin"] = min(out["margin"], float(np.min(np.abs(nrm - thr) / np.abs(thr))))
        upd = dict(EMA=f(param) * nrm + f(1 - param) * mu_k, GS=f(1 - param) * mu_k, RT=nrm)
        mu_k = np.where(keep, upd[mu], mu_k) if mu in upd else np.full_like(nrm, 1e10)
        Z, E, L, T = (np.where(keep[None, :], a, b)
                      for a, b in ((Zl, Zk), (El, Ek), (Ll, Lk), (Tl, Tk)))
        out["cnt"][k] = (~keep).sum()
        for nm, v in (("Z", Z), ("E", E), ("L", L)):
            out[nm].append(v)
    return out


def make(dl, B, mu="EMA", param=0.3, delta=0.3, m=250, n=500, K=K, seed=None, fused=None):
    d = dict(variant="v1", m=m, n=n, B=B, K=K, seed=1290 + B if seed is None else seed,
             perturb=0.2, wscale=0.9)
    inp, sd = P.build_problem(d)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    net = dl.DLADMMNetLenaLSKM(m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]),
                               E0=t(inp["E0"]), L0=t(inp["L0"]), layers=K, alpha=0.01,
                               delta=delta, mu_k_method=mu, mu_k_param=param,
                               fused_safeguard=fused)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net, inp, sd, torch.from_numpy(inp["X"]).cuda()


def check_against(case, got, r64, r32):
    for nm, seq in zip("ZEL", got[:3]):
        for k, g in enumerate(seq):
            g = g.cpu().numpy()
            e64 = parity.nrel(g, r64[nm][k])
            e32, gap = parity.nrel(g, r32[nm][k]), parity.nrel(r32[nm][k], r64[nm][k])
            parity.check_f32(case, "lskm_lena_fused", f"{nm}[{k}]", e32, e64, gap)


@pytest.mark.parametrize("mu,param,delta,B", [
    ("EMA", 0.3, 0.5, 20), ("GS", 0.2, 0.2, 20), ("RT", 0.0, 0.2, 20), ("None", 0.0, 0.0, 20),
    ("EMA", 0.3, 0.3, 300), ("EMA", 0.3, 0.3, 1037)])
def test_fused_matches_reference_and_multi_launch(mu, param, delta, B, dl):
    """Every decision of these cases is at least 3.0e-4 (relative) from its threshold in fp64,
    fp32 GEMM-order effects are ~1e-6: the counts are exact.  Both branches are taken (counts,
    EMA delta = 0.5 B = 20: [20, 20, 15, 4, 5, 16]; "None": [15, 0, 0, 0, 0, 0])."""
    net, inp, sd, X = make(dl, B, mu, param, delta)
    out = net(X, fused_safeguard=True)
    r64 = ref_lskm(inp, sd, K, 0.01, delta, mu, param)
    r32 = ref_lskm(inp, sd, K, 0.01, delta, mu, param, np.float32)  # the reference's fp32 gap
    assert r64["margin"] >= 3.0e-4
    assert 0 < r64["cnt"].sum() < K * B
    assert len(out) == 4 and out[3].dtype == np.float64
    np.testing.assert_array_equal(out[3], r64["cnt"])
    check_against(f"lena_lskm_{mu}_{B}", out, r64, r32)
    out2 = net(X, fused_safeguard=False)
    np.testing.assert_array_equal(out[3], out2[3])
    for a, b in zip(out[0] + out[1] + out[2], out2[0] + out2[1] + out2[2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("delta,learned", [(-99.0, True), (2.0, False)])
def test_fused_delta_ends(delta, learned, dl):
    """delta = -99 keeps every learned step: the V1 forward.  delta = 2 makes the threshold
    negative: every valid column is safeguarded in every layer (count == B: none of the 12
    padding columns of the second group is counted) and the run is the pure KM iteration."""
    B = 20
    net, _, _, X = make(dl, B, delta=delta)
    Z, E, L, cnt = net(X, fused_safeguard=True)
    np.testing.assert_array_equal(cnt, np.full(K, 0.0 if learned else B))
    ref = net(X, learned, False, K=K)
    assert len(ref) == 3
    for a, b in zip(Z + E + L, ref[0] + ref[1] + ref[2]):
        assert torch.equal(a, b)


def test_small_shape_through_padding(dl):
    """16 x 32 runs in the 256 x 512 instantiation: 15 of 16 row blocks are padding.  Seed 1298
    (= 1290 + B, the file's rule): the minimum fp64 decision margin, asserted here, is >= 1e-4,
    so the counts are compared."""
    net, inp, sd, X = make(dl, 8, m=16, n=32, K=3)
    out = net(X, fused_safeguard=True)
    r64 = ref_lskm(inp, sd, 3, 0.01, 0.3, "EMA", 0.3)
    assert r64["margin"] >= 1e-4
    np.testing.assert_array_equal(out[3], r64["cnt"])
    check_against("lena_lskm_16x32", out, r64, ref_lskm(inp, sd, 3, 0.01, 0.3, "EMA", 0.3,
                                                         np.float32))


@pytest.mark.parametrize("field,value,code", [
    ("X", None, "NULL"), ("count", None, "NULL"), ("workspace", None, "NULL"),
    ("beta1_elem", None, "NULL"), ("m", 257, "UNSUPPORTED"), ("n", 513, "UNSUPPORTED"),
    ("abi_version", 1, "ABI_VERSION")])
def test_descriptor_validation(field, value, code, dl):
    lib = dl._lib
    d = lib.LskmLenaDesc()
    d.abi_version = lib.ABI_VERSION
    d.m, d.n, d.batch, d.layers = 250, 500, 20, 2
    fake = 1 << 40  # never dereferenced: validation only
    for f in ("X", "A", "Z0", "E0", "L0", "scalar_params", "km_params", "Z", "E", "L", "count",
              "workspace"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = d.ld_beta = 20
    d.ld_a, d.ld_w = 500, 250
    w = lib.ptr_array([fake, fake])
    d.W = d.beta1_elem = d.beta2_elem = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    d.workspace_bytes = 1 << 30
    setattr(d, field, value)
    codes = dict(NULL=-5, UNSUPPORTED=-7, ABI_VERSION=-1)   # include/dladmm.h DLADMM_E_*
    assert lib.lib().dladmm_lskm_lena_f32(ctypes.byref(d), None) == codes[code]


def test_python_errors(dl):
    net, _, _, X = make(dl, 4, m=512, n=2048, K=1, fused=True)
    with pytest.raises(ValueError):
        net(X)
    with pytest.raises(ValueError):
        net(X[:, :3].contiguous(), fused_safeguard=False)
