"""The one-launch bf16 forward (path 7) for the per-row models V2 / V3 (plan flags bf16_fused +
bf16_fused_rows) against the oracle's bf16 restatement, at the bar of tests/test_gpu_bf16_fused.py
(its build / check_bar): with s_k = nrel(oracle bf16, oracle fp32), within max(1e-5, 0.25 s_k) of
the restatement and within 1e-5 + 1.25 s_k of the fp32 reference, every layer of Z, E, L.  At
perturb = 0.1 a row table read one row off misses that bar 17 to 740 times over at every case
(DESIGN section 27)."""
import numpy as np
import pytest
import torch

from test_gpu_bf16_fused import build, check_bar

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,m,n,B,K,seed", [
    ("v2", 96, 200, 68, 6, 9500), ("v3", 96, 200, 68, 6, 9500),    # ragged rows, m != n, 2 workgroups
    ("v2", 16, 32, 4, 2, 9501), ("v3", 16, 32, 4, 2, 9501),        # one k-step; the last layer's clamp
    ("v3", 64, 256, 64, 3, 9502),                                  # instantiation 1 exactly full
    ("v2", 30, 50, 8, 3, 9505), ("v3", 30, 50, 8, 3, 9505),        # row stride 50: no multiple of 4
    ("v2", 256, 512, 132, 3, 9503), ("v3", 256, 512, 132, 3, 9503),  # instantiation 2
    ("v2", 250, 500, 20, 4, 9504), ("v3", 250, 500, 20, 4, 9504),  # the scripts' shape, padded rows
])
def test_fused_bf16_rows_tracks_bf16_restatement(variant, m, n, B, K, seed, dl, oracle, flags):
    flags.set(bf16_fused=True, bf16_fused_rows=True)
    inp, sd, net, X = build(dl, variant, m, n, B, K, seed)
    r = net.run(X)
    assert r.path == 7
    check_bar(oracle, variant, inp, sd, K, dict(Z=r.Z, E=r.E, L=r.L))


@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_fused_bf16_rows_lean_sums_and_determinism(variant, dl, flags):
    flags.set(bf16_fused=True, bf16_fused_rows=True)
    m, n, B, K = 96, 200, 68, 4
    inp, _sd, net, X = build(dl, variant, m, n, B, K, 9506)
    full = net.run(X, keep_all=True, loss_kind=1)
    full2 = net.run(X, keep_all=True, loss_kind=1)
    lean = net.run(X, keep_all=False, loss_kind=1)
    assert full.path == 7 and lean.path == 7
    for a, b in ((full.Z, full2.Z), (full.E, full2.E), (full.L, full2.L),
                 (full.loss_sums, full2.loss_sums)):
        assert torch.equal(a, b)
    for a, b in ((lean.Z[0], full.Z[-1]), (lean.E[0], full.E[-1]), (lean.L[0], full.L[-1]),
                 (lean.loss_sums, full.loss_sums)):
        assert torch.equal(a, b)
    if variant == "v3":
        # the sums against fp64; V3 returns no T (X - A Z_k = E_k - T_{k+1}), so the fit term is
        # recomputed from the bf16-rounded operands the kernel multiplies
        ls = full.loss_sums.cpu().numpy()
        bf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).bfloat16().double().numpy()  # noqa: E731
        for k in range(K):
            z = full.Z[k].double().cpu().numpy()
            res = inp["X"].astype(np.float64) - bf(inp["A"]) @ bf(full.Z[k].cpu().numpy())
            assert abs(ls[k, 0] - np.abs(z).sum()) <= 1e-6 * np.abs(z).sum(), k
            assert abs(ls[k, 1] - np.abs(res).sum()) <= 1e-4 * np.abs(res).sum(), k
