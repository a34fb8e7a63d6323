"""DLADMMNetLThetaLSKM / DLADMMNetGtLThetaLSKM / DLADMMNetFullLSKM (the per-row test-script
classes): the one-launch safeguarded forward (dladmm_lskm_rowp_f32,
csrc/dladmm_lskm_rowp_fused.hip) against a plain numpy restatement of the three scripts' KM / S /
forward in fp64 and, bit for bit, against the multi-launch path, at m = 250, n = 500 (padded rows
of the 256 x 512 shape; B = 20: a second group with 4 valid columns)."""
import ctypes
from math import sqrt

import numpy as np
import pytest
import torch

import parity
import problems as P

pytestmark = pytest.mark.gpu
K = 6
ALPHA = 0.01
CLASSES = dict(ltheta=("DLADMMNetLThetaLSKM", "v2"), gt=("DLADMMNetGtLThetaLSKM", "v2"),
               full=("DLADMMNetFullLSKM", "v3"))


def consts(cls, lip):
    """(beta, ss1, ss2, c) in fp32, as the script of `cls` forms them (lip: fp32 ||A^T A||_2)."""
    f = np.float32
    if cls == "gt":                                # test_syn_gt_ltheta.py:96-98, :119-121
        beta = f(1.0) / np.sqrt(lip)
        c1 = beta * f(0.5)
        return beta, beta, f(0.5), np.sqrt(c1 / (f(1) - c1))
    if cls == "ltheta":                            # test_syn_l1l1_ltheta.py:147-154
        return f(1.0), f(0.999) / lip, f(0.999), f(sqrt(0.999 / (1 - 0.999)))
    return f(1.0), f(0.5) / lip, f(0.3), f(sqrt(0.3 / (1 - 0.3)))   # test_syn_l1l1_full.py:154-165


def ref_lskm(cls, inp, sd, K, delta, mu, param, dtype=np.float64):
    """The scripts' forward with use_learned = use_safeguard = True; mu_updater.py's step."""
    f = dtype
    X, A, Z, E, L = (np.asarray(inp[k], f) for k in ("X", "A", "Z0", "E0", "L0"))
    A32 = np.asarray(inp["A"], np.float32)
    lip = np.float32(np.linalg.norm(A32.T @ A32, ord=2))
    beta32, ss1_32, ss2, c = consts(cls, lip)
    beta, ss1, thz = f(beta32), f(ss1_32), f(np.float32(ss1_32 * np.float32(ALPHA)))
    ss2, c = f(ss2), f(c)
    act = lambda x, th: np.maximum(x - th, 0) - np.maximum(-x - th, 0)  # noqa: E731
    p = lambda nm, k: np.asarray(sd[f"{nm}.{k}"], f)                    # noqa: E731

    def KM(Zk, Ek, Lk, Tk):
        Zn = act(Zk - ss1 * (A.T @ (Lk + beta * Tk)), thz)
        En = act(Ek - ss2 * (Lk + beta * (A @ Zn + Ek - X)), ss2)
        Tn = A @ Zn + En - X
        return Zn, En, Tn, Lk + beta * Tn

    def S_norm(Zk, Ek, Lk, Tk, Ep):
        _, En, Tn, _ = KM(Zk, Ek, Lk, Tk)
        return np.sqrt(((beta * Tn) ** 2).sum(0) + ((c * (En - 2 * Ek + Ep)) ** 2).sum(0))

    T = A @ Z + E - X
    mu_k = S_norm(Z, E, L, T, E)
    out = dict(Z=[], E=[], L=[], T=[T], cnt=np.zeros(K), margin=np.inf)
    for k in range(K):
        Zk, Ek, Tk, Lk = KM(Z, E, L, T)
        Zl = act(Z - np.asarray(sd[f"fc.{k}.weight"], f) @ (L + p("beta1", k) * T),
                 p("active_para", k))
        if cls == "full":                          # test_syn_l1l1_full.py:218-225
            VVar = L + p("beta2", k) * (A @ Zl + E - X)
            El = act(E - p("ss2", k) * VVar, p("active_para1", k))
            Tl = A @ Zl + El - X
            Ll = L + p("beta3", k) * Tl
        else:                                      # test_syn_l1l1_ltheta.py:197-201
            El = act(X - A @ Zl - p("beta2", k) * L, p("active_para1", k))
            Tl = A @ Zl + El - X
            Ll = L + p("beta1", k) * Tl
        nrm = S_norm(Zl, El, Ll, Tl, E)
        thr = f(1.0 - delta) * mu_k
        keep = nrm < thr
        out["margin"] = min(out["margin"], float(np.min(np.abs(nrm - thr) / np.abs(thr))))
        upd = dict(EMA=f(param) * nrm + f(1 - param) * mu_k, GS=f(1 - param) * mu_k, RT=nrm)
        mu_k = np.where(keep, upd[mu], mu_k) if mu in upd else np.full_like(nrm, 1e10)
        Z, E, L, T = (np.where(keep[None, :], a, b)
                      for a, b in ((Zl, Zk), (El, Ek), (Ll, Lk), (Tl, Tk)))
        out["cnt"][k] = (~keep).sum()
        for nm, v in (("Z", Z), ("E", E), ("L", L), ("T", T)):
            out[nm].append(v)
    return out


def problem(cls, B, m=250, n=500, K=K, seed=None, negrows=False, wscale=0.9):
    d = dict(variant=CLASSES[cls][1], m=m, n=n, B=B, K=K, seed=2300 + B if seed is None else seed,
             perturb=0.2, wscale=wscale)
    inp, sd = P.build_problem(d)
    if negrows:   # every third row of both thresholds negative: the per-row sign of the clamp form
        for k in range(K):
            for nm in ("active_para", "active_para1"):
                sd[f"{nm}.{k}"][::3] *= -0.25
    return inp, sd


def make(dl, cls, B, mu="EMA", param=0.5, delta=0.05, fused=None, **kw):
    inp, sd = problem(cls, B, **kw)
    m, n = inp["A"].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    net = getattr(dl, CLASSES[cls][0])(
        m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]), E0=t(inp["E0"]),
        L0=t(inp["L0"]), layers=kw.get("K", K), alpha=ALPHA, delta=delta, mu_k_method=mu,
        mu_k_param=param, fused_safeguard=fused)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net, inp, sd, torch.from_numpy(inp["X"]).cuda()


def check_against(case, got, r64, r32):
    for nm, seq in zip("ZELT", got[:4]):
        assert len(seq) == len(r64[nm])
        for k, g in enumerate(seq):
            g = g.cpu().numpy()
            e64 = parity.nrel(g, r64[nm][k])
            e32, gap = parity.nrel(g, r32[nm][k]), parity.nrel(r32[nm][k], r64[nm][k])
            parity.check_f32(case, "lskm_rowp_fused", f"{nm}[{k}]", e32, e64, gap)


def same(out, out2):
    for a, b in zip(sum(out[:4], []), sum(out2[:4], [])):
        assert torch.equal(a, b)


def fused_vs_reference(dl, cls, B, mu, param, delta, min_margin, **kw):
    """The fused run against the fp64 reference (whose decisions are asserted to be min_margin
    clear of their thresholds, so the counts are exact) and against the multi-launch run."""
    net, inp, sd, X = make(dl, cls, B, mu, param, delta, **kw)
    nl = kw.get("K", K)
    r64 = ref_lskm(cls, inp, sd, nl, delta, mu, param)
    r32 = ref_lskm(cls, inp, sd, nl, delta, mu, param, np.float32)  # the reference's fp32 gap
    print(f"{cls} {mu} B={B}: margin {r64['margin']:.3e}, counts {r64['cnt']}")
    assert r64["margin"] >= min_margin
    assert 0 < r64["cnt"].sum() < nl * B
    out = net(X, fused_safeguard=True)
    assert len(out) == 5 and out[4].dtype == np.float64 and len(out[3]) == nl + 1
    np.testing.assert_array_equal(out[4], r64["cnt"])
    check_against(f"rowp_lskm_{cls}_{mu}_{B}", out, r64, r32)
    out2 = net(X, fused_safeguard=False)
    np.testing.assert_array_equal(out[4], out2[4])
    same(out, out2)


@pytest.mark.parametrize("cls,mu,param,delta,B", [
    ("ltheta", "EMA", 0.5, -8.0, 20), ("gt", "EMA", 0.5, -5.0, 20), ("full", "EMA", 0.5, 0.05, 20),
    ("full", "GS", 0.2, 0.05, 20), ("full", "RT", 0.0, 0.05, 20), ("full", "None", 0.0, 0.4, 20),
    ("ltheta", "EMA", 0.5, -8.0, 1037)])
def test_fused_matches_reference_and_multi_launch(cls, mu, param, delta, B, dl):
    """Every decision of these cases is at least 1e-4 (relative) from its threshold in fp64 (the
    smallest margins: 6.0e-4 at B = 1,037, 7.9e-4 with GS); fp32 summation-order effects are
    ~1e-6, so the counts are exact.  Both branches are taken: the untrained V2 step (W ~ A^T, no
    step size) has a large residual, so its deltas are negative (ltheta, delta = -8:
    [20, 20, 15, 14, 14, 14]; gt, -5: [2, 0, ...]; full EMA: [0, 20, 20, 20, 20, 4])."""
    fused_vs_reference(dl, cls, B, mu, param, delta, 1e-4)


@pytest.mark.parametrize("cls", ["ltheta", "full"])
@pytest.mark.parametrize("delta,learned", [(-99.0, True), (2.0, False)])
def test_fused_delta_ends(cls, delta, learned, dl):
    """delta = -99 keeps every learned step: the parent's forward.  delta = 2 makes the threshold
    negative: every valid column is safeguarded in every layer (count == B: none of the 12
    padding columns of the second group is counted) and the run is the pure KM iteration.
    W = 0.4 A^T (the V2 fixtures' scale): at 0.9 the untrained V2 step's residual passes 100 mu
    in one column, which the reference safeguards too."""
    B = 20
    net, _, _, X = make(dl, cls, B, delta=delta, wscale=0.4)
    out = net(X, fused_safeguard=True)
    np.testing.assert_array_equal(out[4], np.full(K, 0.0 if learned else B))
    ref = net(X, learned, False, K=K)
    assert len(ref) == 4
    same(out, ref)


def test_row_stride_under_padding(dl):
    """(100, 120): the table's row stride is 120 under 256 padded rows of every slot."""
    fused_vs_reference(dl, "full", 8, "EMA", 0.5, 0.05, 1e-4, m=100, n=120)


def test_mixed_sign_thresholds(dl):
    """16 x 32 through zero padding, every third row of theta_z and theta_e negative.  The fp64
    margin, asserted, is 2.7e-2 (counts [5, 7, 8]), so the counts are compared."""
    fused_vs_reference(dl, "full", 8, "EMA", 0.5, -0.5, 1e-4, m=16, n=32, K=3, negrows=True)


@pytest.mark.parametrize("field,value,code", [
    ("X", None, "NULL"), ("count", None, "NULL"), ("workspace", None, "NULL"),
    ("row_params", None, "NULL"), ("m", 257, "UNSUPPORTED"), ("n", 513, "UNSUPPORTED"),
    ("abi_version", 1, "ABI_VERSION")])
def test_descriptor_validation(field, value, code, dl):
    lib = dl._lib
    d = lib.LskmRowpDesc()
    d.abi_version = lib.ABI_VERSION
    d.m, d.n, d.batch, d.layers, d.emode = 250, 500, 20, 2, lib.V3_FULL
    fake = 1 << 40  # never dereferenced: validation only
    for f in ("X", "A", "Z0", "E0", "L0", "row_params", "km_params", "Z", "E", "L", "T", "count",
              "workspace"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = 20
    d.ld_a, d.ld_w, d.row_stride = 500, 250, 513
    w = lib.ptr_array([fake, fake])
    d.W = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    d.workspace_bytes = 1 << 30
    setattr(d, field, value)
    codes = dict(NULL=-5, UNSUPPORTED=-7, ABI_VERSION=-1)   # include/dladmm.h DLADMM_E_*
    assert lib.lib().dladmm_lskm_rowp_f32(ctypes.byref(d), None) == codes[code]


def test_python_errors(dl):
    net, _, _, X = make(dl, "ltheta", 4, m=512, n=2048, K=1, fused=True)
    with pytest.raises(ValueError):
        net(X)
    with pytest.raises(ValueError):
        net(X[:, :3].contiguous(), fused_safeguard=False)
