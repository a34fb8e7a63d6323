"""The newS test classes on the HIP kernels (d-ladmm_amd/lskm_news.py): the reference class's
fixtures (tests/golden/make_golden_news_lskm.py), bit-equality of the ELZ entry with the plain
fused run, the K = 1,000 KM depth, many 16-column safeguard workgroups, poisoned buffers."""
import importlib

import numpy as np
import pytest
import torch

from conftest import load_golden
import news_lskm_ref as R
import parity
import problems as P
import problems_news as PN
from test_gpu_poison import poison
from test_news_lskm_cpu import ref_forward

pytestmark = pytest.mark.gpu

E_SLOTS = [1, 2, 3, 4, 5]   # beta2, beta3, ss2, ss2b, theta_e: the E / L half of a table row


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def make(dl, case, inp, sd, **kw):
    m, n = inp["A"].shape
    B = inp["X"].shape[1]
    cls = getattr(dl, PN.CLASSES[case["script"]])
    net = cls(m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]), E0=t(inp["E0"]),
              L0=t(inp["L0"]), layers=case["layers"], alpha=case["alpha"], delta=case["delta"],
              mu_k_method=case["mu"], mu_k_param=case["mu_param"],
              prepend_init=True if case["script"] == "acols" else None,
              **P.ctor_extra(case["defn"]), **kw)
    net.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
    return net


# ------------------------------------------------------------------ 1. fixture parity
@pytest.mark.parametrize("name", sorted(PN.NEWS_LSKM_FIXTURES))
def test_matches_reference_fixture(name, dl):
    g, meta = load_golden(name)
    case = meta["case"]
    inp, sd = PN.build_problem(case["defn"])
    net = make(dl, case, inp, sd)
    assert net.prepend_init == (case["script"] != "news")
    X = t(inp["X"]).cuda()
    out = net(X, case["learned"], case["safeguard"], case["continued"], K=case["K"])
    assert len(out) == (4 if case["learned"] and case["safeguard"] else 3)
    assert len(out[0]) == len(out[1]) == len(out[2]) == int(g["n_out"])
    for i, j in enumerate(g["layers_kept"]):
        for c, nm in enumerate("ZEL"):
            gap = float(g["gap_" + nm][i])
            parity.check(name, "f32", f"{nm}[{int(j)}]",
                         parity.nrel(out[c][j].cpu().numpy(), g[nm][i]), parity.tol(gap), gap)
    if "sg_count" in g.files:
        np.testing.assert_array_equal(out[3], g["sg_count"])
        nl = min(case["K"], case["layers"])
        assert tuple(net.sg_mask.shape) == (case["layers"], X.shape[1])
        np.testing.assert_array_equal((net.sg_mask[:nl] == 0).sum(1).cpu().numpy(),
                                      g["sg_count"][:nl])
    s0 = net.Snorm_ELZ(net.E0, net.L0, net.Z0, X).cpu().numpy()
    gap = float(g["gap_snorm0"])
    parity.check(name, "f32", "Snorm_ELZ(E0, L0, Z0)", parity.nrel(s0, g["snorm0"]),
                 parity.tol(gap), gap)


# ------------------------------------------------------------------ 2. entry-mode bit-equality
SHAPES = {"s0": (16, 32), "s1": (64, 256), "s2": (250, 500)}
PLANS = {"default": {}, "no_xsplit": dict(no_xsplit=True), "no_rowsplit": dict(no_rowsplit=True)}


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_elz_entry_bit_equal(shape, plan, dl, flags):
    m, n = SHAPES[shape]
    B, K = 24, 4
    lib = dl._lib
    defn = dict(variant="v7", m=m, n=n, B=B, K=K, seed=2150, perturb=0.2, wscale=0.9)
    inp, sd = P.build_problem(defn)
    case = dict(script="news", defn=defn, layers=K, alpha=0.01, delta=-99.0, mu="None",
                mu_param=0.0)
    net = make(dl, case, inp, sd)
    X = t(inp["X"]).cuda()
    flags.set(**PLANS[plan])
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
            e = net._elz(v, X, z.Z[0], net.E0, net.L0, Ws[1:], etb[1:].contiguous(), want_T=True)
            assert e.path == (1 if shape != "s2" or plan == "no_rowsplit" else 5)
            assert torch.equal(e.Z, z.Z[1:]), (shape, plan, v, "Z")
            assert torch.equal(e.E, z.E[:K - 1]), (shape, plan, v, "E")
            assert torch.equal(e.L, z.L[:K - 1]), (shape, plan, v, "L")
            assert torch.equal(e.T[:K - 1], z.T[1:K]), (shape, plan, v, "T")
            # the tail's saved products: P[j] + E[j] - X is T[j]; P[steps] = A Z_last
            et = net._elz(v, X, z.Z[0], net.E0, net.L0, Ws[1:], etb[1:].contiguous(), tail=True)
            assert torch.equal(et.Z, e.Z) and torch.equal(et.E, e.E) and torch.equal(et.L, e.L)
            assert torch.equal((et.P[:K - 1] + et.E) - X, e.T[:K - 1])
            ref = net.A.double() @ et.Z[-1].double()
            assert parity.nrel(et.P[K - 1].cpu().numpy(), ref.cpu().numpy()) <= parity.REL
        # never safeguarded (delta = -99): the pure learned newS forward, bit for bit
        Zl, El, Ll = dl.DLADMMNetNewS.forward(net, X)
        Zs, Es, Ls, cnt = net(X, True, True, False)
        assert np.array_equal(cnt, np.zeros(K))
        assert bool((net.sg_mask == 1).all())
        for k in range(K):
            assert torch.equal(Zs[k], Zl[k]) and torch.equal(Es[k], El[k]) and \
                torch.equal(Ls[k], Ll[k]), (shape, plan, k)
        # always safeguarded (delta = 2: Snorm < -mu never holds): the pure KM run, bit for bit
        net.delta = 2.0
        Zk, Ek, Lk = net(X, False, False, False, K=K)
        Zs, Es, Ls, cnt = net(X, True, True, False)
        assert np.array_equal(cnt, np.full(K, float(B)))
        assert bool((net.sg_mask == 0).all())
        for k in range(K):
            assert torch.equal(Zs[k], Zk[k]) and torch.equal(Es[k], Ek[k]) and \
                torch.equal(Ls[k], Lk[k]), (shape, plan, k)


# ------------------------------------------------------------------ 3. KM depth, paths
def test_km_depth_1000(dl):
    """K = 1,000 KM iterations (the newS scripts' km1000 ground truth) in one launch against the
    fp64 restatement, at the bar of test_gpu_lskm.test_km_ground_truth_depth."""
    d = dict(variant="v7", m=64, n=128, B=40, K=3, seed=2160, perturb=0.1)
    inp, sd = P.build_problem(d)
    case = dict(script="news", defn=d, layers=3, alpha=0.01, delta=-99.0, mu="None",
                mu_param=0.0, learned=False, safeguard=False, continued=False, K=1000)
    net = make(dl, case, inp, sd)
    X = t(inp["X"]).cuda()
    Z, E, L = net(X, False, False, False, K=1000)
    assert len(Z) == len(E) == len(L) == 1000
    ref = ref_forward(case, inp, sd)
    for k in (0, 9, 99, 999):
        assert parity.nrel(Z[k].cpu().numpy(), ref["Z"][k]) <= 1e-4, k
        assert parity.nrel(E[k].cpu().numpy(), ref["E"][k]) <= 1e-4, k
        assert parity.nrel(L[k].cpu().numpy(), ref["L"][k]) <= 1e-4, k


def test_v7_paths(dl, flags):
    """The new variant at 256 x 512, B = 20: path 6, path 5 under no_xsplit, path 1 under
    no_rowsplit -- the same bits on all three."""
    m, n, B, K = 256, 512, 20, 5
    inp = P.make_inputs(m, n, B, 2170)
    A, X = t(inp["A"]).cuda(), t(inp["X"]).cuda()
    Z0, E0, L0 = (t(inp[k]).cuda() for k in ("Z0", "E0", "L0"))
    tab = torch.zeros((K, 8), device="cuda")
    tab[:, [0, 1, 2, 5]] = 1.0
    tab[:, 6], tab[:, 7] = 0.0015, 0.15
    W = [A.t().contiguous()] * K
    outs = {}
    for want, opts in ((6, {}), (5, dict(no_xsplit=True)), (1, dict(no_rowsplit=True))):
        flags.set(no_xsplit=False, no_rowsplit=False)
        flags.set(**opts)
        r = dl.dladmm_forward(dl._lib.V7_SCALAR_V1E, X, A, W, Z0, E0, L0, scalar_params=tab)
        assert r.path == want
        outs[want] = r
    for p in (5, 6):
        for nm in "ZELT":
            assert torch.equal(getattr(outs[p], nm), getattr(outs[1], nm)), (p, nm)
    # against the fp64 recurrence
    Ad, Xd = A.double(), X.double()
    Z, E, Lm = Z0.double(), E0.double(), L0.double()
    sh = lambda x, th: torch.relu(x - th) - torch.relu(-x - th)  # noqa: E731
    T = Ad @ Z + E - Xd
    for k in range(K):
        Z = sh(Z - float(tab[k, 7]) * (Ad.t() @ (Lm + T)), float(tab[k, 6]))
        E = sh(Xd - Ad @ Z - Lm, 1.0)
        T = Ad @ Z + E - Xd
        Lm = Lm + T
    assert parity.nrel(outs[1].Z[-1].cpu().numpy(), Z.cpu().numpy()) <= 1e-5
    assert parity.nrel(outs[1].E[-1].cpu().numpy(), E.cpu().numpy()) <= 1e-5


# ------------------------------------------------------------------ 4. many columns
@pytest.mark.parametrize("B", [300, 1037])
def test_safeguard_many_columns(B, dl):
    """Several 16-column safeguard workgroups and a ragged last one at the test scripts' m = 250,
    n = 500, against the fp64 restatement.  A column whose fp64 decision margin is below 1e-4 at
    some layer is left out from that layer on (its path may legitimately differ): at most 1 %."""
    d = dict(variant="v7", m=250, n=500, B=B, K=5, seed=2190 + B, perturb=0.2, wscale=0.9)
    inp, sd = P.build_problem(d)
    case = dict(script="news", defn=d, layers=5, alpha=0.01, delta=0.05, mu="EMA", mu_param=0.5,
                learned=True, safeguard=True, continued=False, K=5)
    net = make(dl, case, inp, sd)
    X = t(inp["X"]).cuda()
    Z, E, L, cnt = net(X, True, True, False)
    ref = ref_forward(case, inp, sd)
    assert 0 < ref["sg_count"].sum() < 5 * B   # both branches taken
    mask = net.sg_mask.cpu().numpy()
    ok = np.ones(B, bool)
    for k in range(5):
        ok &= ref["margin"][k] >= 1e-4
        assert ok.sum() >= 0.99 * B, (k, int(ok.sum()))
        np.testing.assert_array_equal(mask[k][ok] != 0, ref["keep"][k][ok])
        for got, nm in ((Z, "Z"), (E, "E"), (L, "L")):
            assert parity.nrel(got[k].cpu().numpy()[:, ok], ref[nm][k][:, ok]) <= 1e-5, (nm, k)
    if ok.all():
        np.testing.assert_array_equal(cnt, ref["sg_count"])


# ------------------------------------------------------------------ 5. poisoned buffers
@pytest.mark.parametrize("B", [24, 640])
def test_outputs_from_poisoned_memory(B, dl):
    m, n, K = 256, 512, 4
    ops = importlib.import_module("d-ladmm_amd.ops")
    d = dict(variant="v7", m=m, n=n, B=B, K=K, seed=7310, perturb=0.1, wscale=0.9)
    inp, sd = P.build_problem(d)
    inp2 = P.make_inputs(m, n, B, 7311)
    case = dict(script="news", defn=d, layers=K, alpha=0.01, delta=0.05, mu="EMA", mu_param=0.5)
    net = make(dl, case, inp, sd)
    x1, x2 = t(inp["X"]).cuda(), t(inp2["X"]).cuda()

    def run(x):
        Z, E, L, cnt = net(x, True, True, False)
        r = net._km_steps(x, Z[-1], E[-1], L[-1], 3, want_T=True)
        return ([a.clone() for a in Z + E + L] + [r.Z.clone(), r.E.clone(), r.L.clone(),
                                                  r.T[:3].clone(), net.sg_mask.clone()], cnt)

    ref, rc = run(x1)
    run(x2)   # leave the other input's results in the freed blocks
    shapes = [(K, n, B), (K, m, B), (K, m, B), (2, m, B), (1, n, B), (1, m, B), (3, n, B),
              (3, m, B), (4, m, B), (B,)]
    for trial in range(2):
        if trial == 1:
            ops._WS.clear()   # fresh workspace too
            poison(shapes, 64 << 20)
        got, gc = run(x1)
        torch.cuda.synchronize()
        assert np.array_equal(gc, rc)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), f"B={B} trial {trial}: output {i} differs"
            assert not torch.isnan(a.float()).any()
