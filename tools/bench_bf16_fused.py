"""A/B timing of the bf16 forward's kernel paths in ONE process: (a) precision "bf16" on the
per-layer tile kernels (path 3, the default), (b) the same call with the plan flag bf16_fused (the
one-launch register-resident kernel, path 7), (c) precision "f32_split" (path 4).  Inputs stay
resident; the forms alternate call by call after a warm-up; each call is timed with HIP events
around the whole dladmm_forward call (weight packing included) and, with the descriptor's kernel
events, around the layer kernels alone.  Workloads: V4 with every layer written, V4 lean (last
layer only), V1 with every layer written, at m x n, K layers, batch B.  Prints one JSON line with
the median and the 10th / 90th percentiles (ms), the path that ran, and for path 7 the achieved
output-store bandwidth and bf16 MFMA rate over the kernel-event time.

    python tools/bench_bf16_fused.py [--batch 65536] [--reps 20] [--warmup 3]
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


def pct(t):
    return dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)),
                p90_ms=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bf16_fused: no GPU (timings are taken on the device only)")
    dl = importlib.import_module("d-ladmm_amd")
    ops = importlib.import_module("d-ladmm_amd.ops")
    dev = torch.device("cuda", 0)
    m, n, B, K = a.m, a.n, a.batch, a.layers
    A, X, Z0, E0, L0 = bench.synth(m, n, B, 0, dev)
    forms = (("bf16_tiles", "bf16", False), ("bf16_fused", "bf16", True),
             ("f32_split", "f32_split", False))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in ev:
        e.record()  # torch creates the hipEvent lazily; make the handles exist
    torch.cuda.synchronize()
    res = {"config": dict(m=m, n=n, K=K, B=B, reps=a.reps, warmup=a.warmup)}
    for wl, variant, keep_all in (("v4_keep_all", "v4", True), ("v4_lean", "v4", False),
                                  ("v1_keep_all", "v1", True)):
        net = dl.VARIANTS[variant](m=m, n=0, d=n, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0,
                                   layers=K).cuda().requires_grad_(False)
        call, kern, path = ({f[0]: [] for f in forms} for _ in range(3))
        for rep in range(a.warmup + a.reps):
            for name, prec, fused in forms:
                net.precision = prec
                with ops.plan_flags(bf16_fused=fused):
                    torch.cuda.synchronize()
                    ev[0].record()
                    r = net.run(X, keep_all=keep_all, kernel_events=(ev[2], ev[3]))
                    ev[1].record()
                    torch.cuda.synchronize()
                path[name] = r.path
                del r
                if rep >= a.warmup:
                    call[name].append(ev[0].elapsed_time(ev[1]))
                    kern[name].append(ev[2].elapsed_time(ev[3]))
        out = {}
        for name, _p, _f in forms:
            out[name] = dict(path=path[name], call=pct(call[name]), kernels=pct(kern[name]))
        # what path 7 must move and multiply: the returned layers (Z, E, L and T) and 2 K + 1
        # products of m x n x B
        nl = K if keep_all else 1
        out_bytes = 4.0 * B * (nl * (n + 2 * m) + (nl + (1 if keep_all else 0)) * m)
        flops = 2.0 * m * n * B * (2 * K + 1)
        t = out["bf16_fused"]["kernels"]["median_ms"] * 1e-3
        out["bf16_fused"]["store_GBps"] = out_bytes / t / 1e9
        out["bf16_fused"]["mfma_TFLOPs"] = flops / t / 1e12
        res[wl] = out
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
