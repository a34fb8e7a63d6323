"""A/B timing of the per-row models' (V2 / V3) safeguarded LSKM forward: the one-launch kernel
(fused_safeguard=True, csrc/dladmm_lskm_rowp_fused.hip) against the multi-launch path
(fused_safeguard=False) at the test scripts' workload (m = 250, d = 500, 20 layers, EMA 0.5,
delta = 0.05) at B = 20 and B = 1,000, for DLADMMNetLThetaLSKM and DLADMMNetFullLSKM, in ONE
process, the two alternated call by call, HIP events around each call, after warm-up
(tools/bench_news_lskm.py's `timed`).

The yardstick is the multi-launch path of the same session and the margin is that path's own
spread (p90 - p10 of its per-call times): `fused_faster` holds where the fused median is below the
multi-launch median by more than that spread; `default_fused` holds only if it does at every batch
for both classes.  Also recorded: the safeguarded columns per layer of both
settings and whether every output tensor of the two settings is bit-equal.

    python tools/bench_rowp_lskm.py [--batches 20,1000] [--calls 50] [--out profiles/rowp_lskm_fused_ab.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from bench_news_lskm import stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="20,1000")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--delta", type=float, default=0.05)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    dev = torch.device("cuda", 0)
    M, N = 250, 500
    Bs = [int(b) for b in a.batches.split(",")]
    A, X, Z0, E0, L0 = bench.synth(M, N, max(Bs), 0, dev)
    res = {"config": dict(m=M, n=N, layers=a.layers, calls=a.calls, warm=a.warm, updater="EMA",
                          mu_param=0.5, delta=a.delta, alpha=0.01)}
    for name in ("DLADMMNetLThetaLSKM", "DLADMMNetFullLSKM"):
        for B in Bs:
            torch.manual_seed(0)
            net = getattr(dl, name)(m=M, n=0, d=N, batch_size=B, A=A, Z0=Z0[:, :B].contiguous(),
                                    E0=E0[:, :B].contiguous(), L0=L0[:, :B].contiguous(),
                                    layers=a.layers, delta=a.delta, mu_k_method="EMA",
                                    mu_k_param=0.5).cuda()
            xb = X[:, :B].contiguous()
            t = timed({"multi_launch": lambda: net(xb, fused_safeguard=False),
                       "fused": lambda: net(xb, fused_safeguard=True)}, a.calls, a.warm)
            r = {k: stats(v) for k, v in t.items()}
            of, om = net(xb, fused_safeguard=True), net(xb, fused_safeguard=False)
            spread = r["multi_launch"]["p90_ms"] - r["multi_launch"]["p10_ms"]
            r["spread_ms"] = spread
            r["ratio"] = r["fused"]["median_ms"] / r["multi_launch"]["median_ms"]
            r["fused_faster"] = bool(
                r["fused"]["median_ms"] < r["multi_launch"]["median_ms"] - spread)
            r["sg_count_fused"] = [float(c) for c in of[4]]
            r["sg_count_multi_launch"] = [float(c) for c in om[4]]
            r["outputs_bit_equal"] = bool(all(
                torch.equal(x, y) for c in range(4) for x, y in zip(of[c], om[c])))
            res[f"{name}_B{B}"] = r
    res["default_fused"] = bool(all(v["fused_faster"] for k, v in res.items()
                                    if isinstance(v, dict) and "fused_faster" in v))
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
