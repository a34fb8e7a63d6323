"""A/B timing of the prologue-product reuse in ONE process: the same model with reuse_prologue
False (every call packs A and forms A Z0) and True (the load-P0 form after the first call),
interleaved per repetition, HIP events around each net.run -- the fused L1L1 objective, every
layer written, on the default plan.  Prints one JSON line per (variant, batch): median ms of
either mode, the kernel path and whether the timed calls reused P0.

    python tools/bench_p0_ab.py --variants v4,v1 --batches 65536,20 [--reps 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="v4")
    ap.add_argument("--batches", default="65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--layers", type=int, default=15)
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    L = importlib.import_module("d-ladmm_amd._lib")
    dev = torch.device("cuda", 0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for variant in a.variants.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            torch.manual_seed(1126)
            A, X, Z0, E0, L0 = bench.synth(a.m, a.n, B, 0, dev)
            net = dl.VARIANTS[variant](m=a.m, n=0, d=a.n, batch_size=B, A=A, Z0=Z0, E0=E0,
                                       L0=L0, layers=a.layers).cuda().requires_grad_(False)
            times = {False: [], True: []}
            reused = {False: set(), True: set()}
            path = 0
            for rep in range(a.reps + 2):
                for mode in (False, True):
                    net.reuse_prologue = mode
                    torch.cuda.synchronize()
                    ev0.record()
                    r = net.run(X, loss_kind=L.LOSS_L1L1)
                    ev1.record()
                    torch.cuda.synchronize()
                    if rep >= 2:   # warm-up, and the call that fills the cache
                        times[mode].append(ev0.elapsed_time(ev1))
                        reused[mode].add(bool(r.p0_reused))
                    path = r.path
                    del r
            print(json.dumps({
                "variant": variant, "B": B, "path": path, "reps": a.reps,
                "ms_compute": float(np.median(times[False])),
                "ms_reuse": float(np.median(times[True])),
                "range_compute": [min(times[False]), max(times[False])],
                "range_reuse": [min(times[True]), max(times[True])],
                "p0_reused": {"compute": sorted(reused[False]), "reuse": sorted(reused[True])}}),
                flush=True)
            del net, A, X, Z0, E0, L0
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
