"""The one-launch register-resident bf16 forward (precision="bf16" with plan flag bf16_fused,
forward path 7) against the oracle's bf16 restatement, at the bar of tests/test_gpu_bf16.py: with
s_k = nrel(oracle bf16, oracle fp32), within max(1e-5, 0.25 s_k) of the restatement and within
1e-5 + 1.25 s_k of the fp32 reference, every layer of every returned output."""
import numpy as np
import pytest
import torch

import problems as P

pytestmark = pytest.mark.gpu


def nrel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def build(dl, variant, m, n, B, K, seed):
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=seed, perturb=0.1,
             wscale=0.4 if variant in ("v1", "v2") else None)
    inp, sd = P.build_problem(d)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    net = dl.VARIANTS[variant](m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]),
                               E0=t(inp["E0"]), L0=t(inp["L0"]), layers=K)
    net.load_state_dict({k: t(v) for k, v in sd.items()})
    net.requires_grad_(False)
    net.cuda()
    net.precision = "bf16"
    return inp, sd, net, t(inp["X"]).cuda()


def check_bar(oracle, variant, inp, sd, K, out):
    args = (variant, inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, K)
    rb = oracle.forward(*args, gemm="bf16")
    r32 = oracle.forward(*args)
    for nm, layers in out.items():
        for k, got in enumerate(layers):
            got = got.cpu().numpy()
            s = nrel(rb[nm][k], r32[nm][k])
            assert nrel(got, rb[nm][k]) <= max(1e-5, 0.25 * s), (nm, k, s)
            assert nrel(got, r32[nm][k]) <= 1e-5 + 1.25 * s, (nm, k, s)


@pytest.mark.parametrize("variant,m,n,B,K,seed", [
    ("v4", 96, 200, 68, 6, 9400), ("v5", 96, 200, 68, 6, 9400), ("v6", 96, 200, 68, 6, 9400),
    ("v1", 96, 200, 68, 6, 9400),   # ragged rows in both GEMMs, a second workgroup of 4 columns
    ("v4", 16, 32, 4, 2, 9401),     # the smallest shape on instantiation 1: one k-step
    ("v4", 64, 256, 64, 3, 9402),   # instantiation 1 exactly full
    ("v4", 256, 512, 132, 3, 9403), ("v1", 256, 512, 132, 3, 9403),  # instantiation 2, 3 workgroups
    ("v6", 250, 500, 20, 4, 9404),  # the scripts' shape and batch
])
def test_fused_bf16_tracks_bf16_restatement(variant, m, n, B, K, seed, dl, oracle, flags):
    flags.set(bf16_fused=True)
    inp, sd, net, X = build(dl, variant, m, n, B, K, seed)
    r = net.run(X)
    assert r.path == 7
    out = dict(Z=r.Z, E=r.E, L=r.L)
    if r.T is not None:
        out["T"] = r.T
    check_bar(oracle, variant, inp, sd, K, out)


def test_fused_bf16_news_class(dl, oracle, flags):
    """The tied newS class runs as its V5 plan: path 7, its own (re-indexed) outputs at the bar."""
    flags.set(bf16_fused=True)
    m, n, B, K = 96, 200, 68, 4
    inp, sd, net, X = build(dl, "v7t", m, n, B, K, 9405)
    assert net.run(X).path == 7
    with torch.no_grad():
        Z, E, L = net(X)
    check_bar(oracle, "v7t", inp, sd, K, dict(Z=Z, E=E, L=L))


def test_fused_bf16_lean_sums_and_determinism(dl, flags):
    flags.set(bf16_fused=True)
    m, n, B, K = 96, 200, 68, 4
    _inp, _sd, net, X = build(dl, "v4", m, n, B, K, 9406)
    full = net.run(X, keep_all=True, loss_kind=1)
    full2 = net.run(X, keep_all=True, loss_kind=1)
    lean = net.run(X, keep_all=False, loss_kind=1)
    assert full.path == 7 and lean.path == 7
    for a, b in ((full.Z, full2.Z), (full.E, full2.E), (full.L, full2.L), (full.T, full2.T),
                 (full.loss_sums, full2.loss_sums)):
        assert torch.equal(a, b)
    for a, b in ((lean.Z[0], full.Z[-1]), (lean.E[0], full.E[-1]), (lean.L[0], full.L[-1]),
                 (lean.T[0], full.T[-1]), (lean.loss_sums, full.loss_sums)):
        assert torch.equal(a, b)
    ls = full.loss_sums.cpu().numpy()
    for k in range(K):
        z = full.Z[k].double().cpu().numpy()
        res = (full.E[k] - full.T[k + 1]).double().cpu().numpy()   # X - A Z_k = E_k - T_{k+1}
        assert abs(ls[k, 0] - np.abs(z).sum()) <= 1e-6 * np.abs(z).sum(), k
        assert abs(ls[k, 1] - np.abs(res).sum()) <= 1e-4 * np.abs(res).sum(), k


@pytest.mark.parametrize("variant,m,n,K", [("v3", 96, 200, 3), ("v4", 300, 530, 2)])
def test_fused_bf16_flag_falls_back_to_tiles(variant, m, n, K, dl, flags):
    """A variant or shape the kernel does not take keeps path 3, bit for bit, flag or no flag."""
    _inp, _sd, net, X = build(dl, variant, m, n, 68, K, 9407)
    plain = net.run(X)
    flags.set(bf16_fused=True)
    flagged = net.run(X)
    assert plain.path == 3 and flagged.path == 3
    for a, b in ((plain.Z, flagged.Z), (plain.E, flagged.E), (plain.L, flagged.L)):
        assert torch.equal(a, b)
