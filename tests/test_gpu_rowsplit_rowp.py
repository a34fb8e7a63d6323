"""V2 / V3 (per-row parameters) on the small-batch row-split forms, plan flag rowsplit_rows
(include/dladmm.h DLADMM_F_ROWSPLIT_ROWP): forward paths 5 and 6
(csrc/dladmm_fused_rs_kernel.h, MEM = 1 / 4), backward paths 2 and 3
(csrc/dladmm_reverse_rs_kernel.h).  Split "xs" = the flag alone (path 6 where its grid fits one workgroup per CU), "rs" = the flag plus
no_xsplit (path 5).  Without the flag V2 / V3 keep path 1 (tests/test_gpu_rowsplit.py).

The forward performs the fused kernel's PK_ROW arithmetic operation for operation: every layer's
Z, E, L, T and the saved products equal path 1's (plan flag no_rowsplit) BIT FOR BIT.  The reverse
sweep forms gU_k and Var_k bit for bit as the 64-column sweep does, so the weight gradients are
equal; the per-row parameter gradients are the same fp32 partials -- one per (layer, slot, row,
16-column group), row16_sum of the same 16 columns as the 64-column sweep's wave of that index --
reduced in the same fp64 order: 1e-12, the bar tests/test_gpu_reverse.py check_equal_row gives
identical partials in identical order.  No slot needed the regrouped-sum bar.  Independent of
path 1: the reference's golden outputs and gradients (V3) and the oracle (V2)."""
import numpy as np
import pytest
import torch

import problems as P
from conftest import load_golden
from test_gpu_backward import (GTOL, check_against_golden, make_train_net, nrel, record_paths,
                               run_grads, total_loss)
from test_gpu_parity import _compare, _oracle_case, check_golden, make_net
from test_gpu_reverse import _cotangents
from test_gpu_rowsplit import _cus, _run, _split, _xs_grid

pytestmark = pytest.mark.gpu


def _flag_split(dl, split, B):
    """(plan flags, expected forward path) of a row-split flavour of V2 / V3 at batch B."""
    fl, want = _split(dl, split, B)
    return fl | dl._lib.F_ROWSPLIT_ROWP, want


def _mixed(sd, K):
    """theta_z of every other ROW negative in every layer (test_gpu_reverse._zmask_ab)."""
    for k in range(K):
        v = sd[f"active_para.{k}"].copy()
        v[1::2] = -0.3 * np.abs(v[1::2])
        sd[f"active_para.{k}"] = v
    return sd


def test_rowp_plan_scope(dl):
    """V2 / V3 take paths 6 / 5 (backward 3 / 2) only under the flag, within the row-split plan's
    other limits (256 x 512 instantiation, fp32; no_rowsplit / no_xsplit win); the flag changes
    nothing for another variant."""
    L = dl._lib
    ops = dl.ops
    K = 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def paths(variant, flags, mn=(250, 500), B=64, precision="f32"):
        d = dict(variant=variant, m=mn[0], n=mn[1], B=B, K=K, seed=5500, perturb=0.1)
        inp, sd = P.build_problem(d)
        net = make_train_net(dl, variant, inp, sd, K).cuda()
        with torch.no_grad():
            tables = net._tables(net.A.device)
        args = (net.VARIANT, t(inp["X"]), net.A, [w.detach() for w in net._weights()], net.Z0,
                net.E0, net.L0)
        with torch.no_grad():
            r = ops.dladmm_forward(*args, keep_all=True, want_T=True, want_P=True,
                                   loss_kind=L.LOSS_L1L1, flags=flags, precision=precision,
                                   **tables)
        coef = torch.tensor([[1e-2, 1.0]] * K, device="cuda")
        b = ops.dladmm_backward(*args, r, loss_kind=L.LOSS_L1L1, loss_coef=coef, **tables)
        return r.path, b.path

    F = L.F_ROWSPLIT_ROWP
    assert _xs_grid(64) <= _cus()
    for v in ("v2", "v3"):
        assert paths(v, 0) == (1, 1)
        assert paths(v, F) == (6, 3)
        assert paths(v, F | L.F_NO_XSPLIT) == (5, 2)
        assert paths(v, F | L.F_NO_ROWSPLIT) == (1, 1)
        assert paths(v, F, precision="f32_split")[0] == paths(v, 0, precision="f32_split")[0]
        assert paths(v, F, mn=(64, 128)) == (1, 1)
    assert paths("v4", F) == paths("v4", 0) == (6, 3)
    assert paths("v4", F | L.F_NO_XSPLIT) == paths("v4", L.F_NO_XSPLIT) == (5, 2)


def _assert_fwd_equal(rs, fu, names=("Z", "E", "L", "T"), tag=None):
    for nm in names:
        a, b = getattr(rs, nm), getattr(fu, nm)
        assert a.shape == b.shape, (tag, nm)
        assert torch.equal(a, b), (tag, nm, float((a - b).abs().max()))


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("B", [1, 20, 77, 300])
def test_rowp_bit_equal_to_fused(variant, B, split, dl):
    m, n, K = 250, 500, 5
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=6100 + B, perturb=0.2,
             wscale=0.4 if variant == "v2" else P.VARIANT_SPECS[variant]["wscale"])
    inp, sd = P.build_problem(d)
    fl, want = _flag_split(dl, split, B)
    rs = _run(dl, variant, inp, sd, K, flags=fl)
    fu = _run(dl, variant, inp, sd, K, flags=dl._lib.F_NO_ROWSPLIT)
    assert rs.path == want and fu.path == 1
    _assert_fwd_equal(rs, fu)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("shape", [(65, 257), (100, 120)])
def test_rowp_ragged_shapes_and_lean_mode(variant, shape, split, dl):
    """Ragged m / n inside the 256 x 512 instantiation -- (100, 120): a row table narrower than
    the kernel's padded rows, which read 0 past each slot's rows and stay zero -- keep_all and
    lean (last layer only)."""
    m, n = shape
    K, B = 4, 45
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=6200 + m, perturb=0.2, wscale=0.4)
    inp, sd = P.build_problem(d)
    fl, want = _flag_split(dl, split, B)
    for keep_all in (True, False):
        rs = _run(dl, variant, inp, sd, K, keep_all=keep_all, flags=fl)
        fu = _run(dl, variant, inp, sd, K, keep_all=keep_all, flags=dl._lib.F_NO_ROWSPLIT)
        assert rs.path == want and fu.path == 1
        _assert_fwd_equal(rs, fu, tag=keep_all)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("neg", ["mixed", "negtheta"])
def test_rowp_negative_thresholds(variant, neg, split, dl):
    """theta_z < 0 on every other row (mixed), or theta_z and theta_e < 0 on every other layer
    (negtheta): Z in the clamp form, E in the literal one, as the fused kernel."""
    m, n, K, B = 250, 500, 5, 20
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=6250, perturb=0.2, wscale=0.4,
             negtheta=neg == "negtheta")
    inp, sd = P.build_problem(d)
    if neg == "mixed":
        sd = _mixed(sd, K)
    fl, want = _flag_split(dl, split, B)
    rs = _run(dl, variant, inp, sd, K, flags=fl)
    fu = _run(dl, variant, inp, sd, K, flags=dl._lib.F_NO_ROWSPLIT)
    assert rs.path == want and fu.path == 1
    _assert_fwd_equal(rs, fu)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("B", [20, 25])
def test_rowp_training_forward(variant, B, split, dl):
    """The saved products bit for bit with path 1's; the fused objective's sums and per-column
    terms to fp32 rounding (the waves' row partials summed in another order), the bar of
    test_gpu_rowsplit.test_rowsplit_training_forward."""
    m, n, K = 250, 500, 5
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=6150 + B, perturb=0.2,
             wscale=0.4 if variant == "v2" else P.VARIANT_SPECS[variant]["wscale"])
    inp, sd = P.build_problem(d)
    L = dl._lib
    kw = dict(want_P=True, loss_kind=L.LOSS_L1L1, want_col_loss=True)
    fl, want = _flag_split(dl, split, B)
    rs = _run(dl, variant, inp, sd, K, flags=fl, **kw)
    fu = _run(dl, variant, inp, sd, K, flags=L.F_NO_ROWSPLIT, **kw)
    assert rs.path == want and fu.path == 1
    assert rs.P is not None and fu.P is not None
    _assert_fwd_equal(rs, fu, names=("Z", "E", "L", "T", "P"))
    np.testing.assert_allclose(rs.loss_sums.cpu().numpy(), fu.loss_sums.cpu().numpy(),
                               rtol=1e-5)
    np.testing.assert_allclose(rs.col_loss.cpu().numpy(), fu.col_loss.cpu().numpy(),
                               rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------ against the pinned reference
@pytest.mark.parametrize("split", ["xs", "rs"])
def test_rowp_v3_forward_matches_reference_golden(split, dl, flags, monkeypatch):
    """The reference's own outputs of v3_med_pert (256 x 512, B = 12, K = 15) at the parity bar
    test_gpu_parity applies to the fixture."""
    name = "v3_med_pert"
    g, meta = load_golden(name)
    d = meta["defn"]
    inp, sd = P.build_problem(d)
    net = make_net(dl, d["variant"], inp, sd, d["K"], **P.ctor_extra(d))
    X = torch.from_numpy(inp["X"]).cuda()
    paths = record_paths(monkeypatch)
    flags.set(rowsplit_rows=True, no_xsplit=split == "rs")
    with torch.no_grad():
        out = net(X)
    torch.cuda.synchronize()
    assert paths and paths[0] == _split(dl, split, d["B"])[1], paths
    check_golden(name, g, meta, net, X, out)


@pytest.mark.parametrize("split", ["xs", "rs"])
def test_rowp_v3_grads_match_reference_autograd(split, dl, flags, monkeypatch):
    """grad_v3_med: the reference autograd's gradients through forward path 6 / 5 and backward
    path 3 / 2, at check_against_golden's own bar."""
    paths = record_paths(monkeypatch)
    flags.set(rowsplit_rows=True, no_xsplit=split == "rs")
    g, meta, net, loss = run_grads(dl, "grad_v3_med")
    assert paths and paths[0] == _split(dl, split, meta["defn"]["B"])[1], paths
    np.testing.assert_allclose(loss, g["loss"][0], rtol=1e-4)
    check_against_golden(g, meta, net)


@pytest.mark.parametrize("split", ["xs", "rs"])
def test_rowp_v2_forward_vs_oracle(split, dl, oracle):
    """V2 has no golden fixture at this shape: the oracle at the fp32 bar, m=250 n=500 K=15,
    B=100 (as test_gpu_rowsplit.test_rowsplit_vs_oracle)."""
    m, n, K, B = 250, 500, 15, 100
    inp, sd, ref = _oracle_case(oracle, "v2", m, n, B, K, seed=6300)
    fl, want = _flag_split(dl, split, B)
    r = _run(dl, "v2", inp, sd, K, flags=fl)
    assert r.path == want
    # (the reference's V2 forward returns no T: Z, E, L)
    assert "T" not in ref["r64"]
    _compare((list(r.Z), list(r.E), list(r.L)), ref, tag=f"rowsplit {split} v2 B=100", path="f32")


@pytest.mark.parametrize("split", ["xs", "rs"])
def test_rowp_v2_grads_match_oracle(split, dl, flags, monkeypatch):
    """V2 at m=250, n=500, B=20 against the backward oracle, the tolerance of
    test_gpu_backward.test_grads_match_oracle_larger_batch."""
    from oracle import dladmm_oracle as fwd
    from oracle import dladmm_oracle_grad as og
    variant = "v2"
    m, n, B, K = 250, 500, 20, 4
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=6400, perturb=0.1, wscale=0.4)
    inp, sd = P.build_problem(d)
    up = P.make_upstream(d, P.VARIANT_SPECS[variant]["ret_t"])
    net = make_train_net(dl, variant, inp, sd, K)
    X = torch.from_numpy(inp["X"]).cuda()
    A = torch.from_numpy(inp["A"]).cuda()
    paths = record_paths(monkeypatch)
    flags.set(rowsplit_rows=True, no_xsplit=split == "rs")
    loss = total_loss(net(X), X, A, up, "l1l1", K)
    loss.backward()
    torch.cuda.synchronize()
    assert paths and paths[0] == _split(dl, split, B)[1], paths
    ref = {}
    for dt in (np.float32, np.float64):
        o = fwd.forward(variant, inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, K,
                        dtype=dt)
        gz = og.train_loss_grads(o["Z"], inp["X"], inp["A"], P.GRAD_ALPHA, P.loss_coeffs(K),
                                 "l1l1", dtype=dt)
        gz = [a + b for a, b in zip(gz, up["Gz"])]
        ref[dt] = og.vjp(variant, inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, K,
                         gZ=gz, gE=list(up["Ge"]), gL=list(up["Gl"]),
                         gT=list(up["Gt"]) if "Gt" in up else None, dtype=dt)
    for key, p in net.named_parameters():
        gap = nrel(ref[np.float32][key], ref[np.float64][key])
        e = nrel(p.grad.cpu().numpy(), ref[np.float64][key])
        assert e <= max(GTOL, 3.0 * gap), (key, e, gap)


# ------------------------------------------------------------ reverse sweep vs the 64-column one
def _sweep_ab(dl, variant, m, n, B, K, split, cot, seed, mixed=False, twice=False):
    """The same saved-state construction on a row-split forward (the flag) and on path 1
    (no_rowsplit), the backward of each: fused L1L1 objective with random coefficients plus the
    upstream cotangents named in cot (subset of "ZELT")."""
    ops, L = dl.ops, dl._lib
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=seed, perturb=0.1)
    inp, sd = P.build_problem(d)
    if mixed:
        sd = _mixed(sd, K)
    net = make_train_net(dl, variant, inp, sd, K).cuda()
    X = torch.from_numpy(inp["X"]).cuda()
    with torch.no_grad():
        tables = net._tables(X.device)
    W = [w.detach() for w in net._weights()]
    args = (net.VARIANT, X, net.A, W, net.Z0, net.E0, net.L0)
    lk = L.LOSS_L1L1
    g = torch.Generator(device="cuda").manual_seed(seed)
    coef = (torch.rand(K, 2, device="cuda", generator=g) *
            torch.tensor([1e-2, 1.0], device="cuda")).contiguous()
    c = _cotangents(m, n, B, K, seed + 1, cot)
    # of the size of the objective's own cotangents (gradients of column means)
    cots = tuple(None if c[nm] is None else [None if t is None else t / B for t in c[nm]]
                 for nm in "ZELT")
    xf, want = _flag_split(dl, split, B)
    out = []
    for fl in (xf, L.F_NO_ROWSPLIT):
        with torch.no_grad():
            r = ops.dladmm_forward(*args, keep_all=True, want_T=True, want_P=True, loss_kind=lk,
                                   flags=fl, **tables)
        runs = [ops.dladmm_backward(*args, r, *cots, loss_kind=lk, loss_coef=coef, **tables)
                for _ in range(2 if twice and fl == xf else 1)]
        out.append((r, runs))
    (fr, rs), (f1, cl) = out
    assert fr.path == want and f1.path == 1
    assert all(b.path == want - 3 for b in rs) and cl[0].path == 1
    return rs, cl[0]


def _check_sweep(dl, rs, cl, m, n, K, variant):
    L = dl._lib
    assert torch.equal(rs.gW, cl.gW)
    gr, gc = rs.g_row.cpu().numpy(), cl.g_row.cpu().numpy()
    assert gr.shape == gc.shape
    for k in range(K):
        e = nrel(gr[k], gc[k])
        print(f"{variant} layer {k}: g_row nrel {e:.3e}")
        assert e <= 1e-12, (k, e)
    mask = {L.P_THETA_Z, L.P_BETA1, L.P_BETA2, L.P_BETA3, L.P_THETA_E}
    if variant == "v3":
        mask.add(L.P_SS2)
    for slot in range(L.NSCALAR):
        rows = 0 if slot not in mask else (n if slot == L.P_THETA_Z else m)
        assert not gr[:, slot, rows:].any(), slot
        if slot in mask:
            assert gr[:, slot, :rows].any(), slot


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("B", [20, 25, 300])
@pytest.mark.parametrize("gz", [False, True])
def test_rowp_reverse_sweep(variant, B, gz, split, dl):
    m, n, K = 250, 500, 4
    rs, cl = _sweep_ab(dl, variant, m, n, B, K, split, "Z" if gz else "", 6600 + B)
    _check_sweep(dl, rs[0], cl, m, n, K, variant)


@pytest.mark.parametrize("variant", ["v2", "v3"])
@pytest.mark.parametrize("split,cot,B", [("xs", "ELT", 20), ("rs", "ZELT", 25),
                                         ("xs", "ZELT", 300), ("rs", "ELT", 300)])
def test_rowp_reverse_sweep_cotangents(variant, split, cot, B, dl):
    m, n, K = 250, 500, 4
    rs, cl = _sweep_ab(dl, variant, m, n, B, K, split, cot, 6700 + B)
    _check_sweep(dl, rs[0], cl, m, n, K, variant)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_rowp_reverse_sweep_ragged_shape(variant, split, dl):
    """(100, 120) at B = 45: a row table (stride 120) narrower than the kernel's padded rows."""
    m, n, K, B = 100, 120, 4, 45
    rs, cl = _sweep_ab(dl, variant, m, n, B, K, split, "", 6800)
    _check_sweep(dl, rs[0], cl, m, n, K, variant)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_rowp_reverse_sweep_mixed_negative_theta(variant, split, dl):
    """theta_z < 0 on every other row: each row's own mask bound 2 |theta_z|."""
    m, n, K, B = 250, 500, 4, 25
    rs, cl = _sweep_ab(dl, variant, m, n, B, K, split, "Z", 6900, mixed=True)
    _check_sweep(dl, rs[0], cl, m, n, K, variant)


@pytest.mark.parametrize("split", ["xs", "rs"])
@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_rowp_reverse_sweep_deterministic(variant, split, dl):
    m, n, K, B = 250, 500, 4, 25
    (a, b), _ = _sweep_ab(dl, variant, m, n, B, K, split, "Z", 6950, twice=True)
    assert torch.equal(a.gW, b.gW) and torch.equal(a.g_row, b.g_row)
