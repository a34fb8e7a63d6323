"""A/B timing of the per-row models' (V2 / V3) bf16 forward in ONE process, as
tools/bench_bf16_fused.py does for the other variants: (a) precision "bf16" on the per-layer tile
kernels (path 3, the default), (b) the same call under plan_flags(bf16_fused, bf16_fused_rows) (the
one-launch register-resident kernel, path 7), (c) precision "f32" (path 1).  Inputs stay
resident; the forms alternate call by call after a warm-up; each call is timed with HIP events
around the whole dladmm_forward call (weight packing included) and, with the descriptor's kernel
events, around the layer kernels alone.  Workloads: V2 and V3, every layer written and lean.
Prints one JSON line with the median and the 10th / 90th percentiles (ms), the path that ran, and
whether path 7's median beats path 3's by more than path 3's own p90 - p10.

    python tools/bench_bf16_fused_rowp.py [--batch 65536] [--reps 20] [--warmup 3]
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
import bench  # noqa: E402
from tools.bench_bf16_fused import pct  # noqa: E402


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
        raise SystemExit("bench_bf16_fused_rowp: no GPU (timings are taken on the device only)")
    dl = importlib.import_module("d-ladmm_amd")
    ops = importlib.import_module("d-ladmm_amd.ops")
    dev = torch.device("cuda", 0)
    m, n, B, K = a.m, a.n, a.batch, a.layers
    A, X, Z0, E0, L0 = bench.synth(m, n, B, 0, dev)
    forms = (("bf16_tiles", "bf16", False, 3), ("bf16_fused", "bf16", True, 7),
             ("f32", "f32", False, 1))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in ev:
        e.record()  # torch creates the hipEvent lazily; make the handles exist
    torch.cuda.synchronize()
    res = {"config": dict(m=m, n=n, K=K, B=B, reps=a.reps, warmup=a.warmup)}
    for variant in ("v2", "v3"):
        net = dl.VARIANTS[variant](m=m, n=0, d=n, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0,
                                   layers=K).cuda().requires_grad_(False)
        for keep_all in (True, False):
            call, kern = ({f[0]: [] for f in forms} for _ in range(2))
            for rep in range(a.warmup + a.reps):
                for name, prec, fused, want in forms:
                    net.precision = prec
                    with ops.plan_flags(bf16_fused=fused, bf16_fused_rows=fused):
                        torch.cuda.synchronize()
                        ev[0].record()
                        r = net.run(X, keep_all=keep_all, kernel_events=(ev[2], ev[3]))
                        ev[1].record()
                        torch.cuda.synchronize()
                    if r.path != want:
                        raise SystemExit(f"{variant} {name}: path {r.path}, expected {want}")
                    del r
                    if rep >= a.warmup:
                        call[name].append(ev[0].elapsed_time(ev[1]))
                        kern[name].append(ev[2].elapsed_time(ev[3]))
            out = {f[0]: dict(path=f[3], call=pct(call[f[0]]), kernels=pct(kern[f[0]]))
                   for f in forms}
            t3, t7 = out["bf16_tiles"]["call"], out["bf16_fused"]["call"]
            out["fused_beats_tiles_by_more_than_tiles_spread"] = bool(
                t3["median_ms"] - t7["median_ms"] > t3["p90_ms"] - t3["p10_ms"])
            res[f"{variant}_{'keep_all' if keep_all else 'lean'}"] = out
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
