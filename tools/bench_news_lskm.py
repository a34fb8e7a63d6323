"""Timing of the newS test class (DLADMMNetNewSLSKM) against the test_syn_l1l1_scalar.py class
(DLADMMNetLSKM) at the test scripts' workload (m = 250, d = 500), in ONE process, the two
alternated call by call, HIP events around each call, after warm-up:

  * pure KM, K = 1,000: the V7 form against the existing V5-form `_km` run (same two GEMMs per
    iteration, a cheaper E-step);
  * safeguarded, 20 layers, EMA 0.5, delta 0.05: per-call time of both classes, and the number of
    kernel launches per safeguarded layer of the newS class (counted from its call structure:
    every forward call packs A and the weight, then runs one fused kernel; the select is one --
    constants of the call structure, not counted here: a kernel trace of tools/prof_news_lskm.py
    counts them).

The spread is the old class's own run-to-run spread, p90 - p10 of its per-call times (a single
outlier call does not widen it); the expectations the tool records: KM no slower than V5 plus
that spread, safeguarded at most 7/6 of the old class plus that spread.  Neither gates a test.

    python tools/bench_news_lskm.py [--batches 20,1000] [--calls 50] [--out profiles/news_lskm.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def timed(fns, calls, warm):
    """Per-call ms of each callable, alternated: {name: [ms]}."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {k: [] for k in fns}
    for rep in range(warm + calls):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            ev0.record()
            r = fn()
            ev1.record()
            torch.cuda.synchronize()
            del r
            if rep >= warm:
                out[k].append(ev0.elapsed_time(ev1))
    return out


def stats(t):
    t = np.asarray(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="20,1000")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    dev = torch.device("cuda", 0)
    M, N = 250, 500
    Bs = [int(b) for b in a.batches.split(",")]
    A, X, Z0, E0, L0 = bench.synth(M, N, max(Bs), 0, dev)
    res = {"config": dict(m=M, n=N, K=a.K, layers=a.layers, calls=a.calls, warm=a.warm,
                          updater="EMA", mu_param=0.5, delta=0.05)}
    for B in Bs:
        kw = dict(m=M, n=0, d=N, batch_size=B, A=A, Z0=Z0[:, :B].contiguous(),
                  E0=E0[:, :B].contiguous(), L0=L0[:, :B].contiguous(), layers=a.layers,
                  alpha=0.01, delta=0.05, mu_k_method="EMA", mu_k_param=0.5)
        torch.manual_seed(0)
        old = dl.DLADMMNetLSKM(**kw).cuda()
        torch.manual_seed(0)
        new = dl.DLADMMNetNewSLSKM(**kw).cuda()
        xb = X[:, :B].contiguous()
        km = timed({"v5_km": lambda: old(xb, False, False, False, K=a.K),
                    "v7_km": lambda: new(xb, False, False, False, K=a.K)}, a.calls, a.warm)
        sg = timed({"lskm": lambda: old(xb, True, True, False),
                    "news_lskm": lambda: new(xb, True, True, False)}, a.calls, a.warm)
        r = {k: stats(v) for k, v in {**km, **sg}.items()}
        sp_km = r["v5_km"]["p90_ms"] - r["v5_km"]["p10_ms"]
        sp_sg = r["lskm"]["p90_ms"] - r["lskm"]["p10_ms"]
        r["km"] = dict(spread_ms=sp_km, ratio=r["v7_km"]["median_ms"] / r["v5_km"]["median_ms"],
                       expectation_met=bool(r["v7_km"]["median_ms"]
                                            <= r["v5_km"]["median_ms"] + sp_km))
        r["safeguarded"] = dict(
            spread_ms=sp_sg, ratio=r["news_lskm"]["median_ms"] / r["lskm"]["median_ms"],
            expectation_met=bool(r["news_lskm"]["median_ms"]
                                 <= 7.0 / 6.0 * r["lskm"]["median_ms"] + sp_sg),
            sg_count=[float(c) for c in new(xb, True, True, False)[3]],
            # per layer: KM candidate, L2O candidate, KM step from the L2O candidate (each: pack A,
            # pack the weight, the fused kernel) and the select
            by_construction=dict(launches_per_layer=dict(fused=3, pack_frags_kernel=6, select=1,
                                                         total=10), gemm_passes_per_layer=7))
        res[f"B{B}"] = r
    txt = json.dumps(res, indent=1)
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
