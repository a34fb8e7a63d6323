"""A/B timing of the plan flag rowsplit_rows (include/dladmm.h DLADMM_F_ROWSPLIT_ROWP): V2 / V3
(per-row parameters) on the small-batch row-split kernels (forward path 6 / 5, backward path 3 / 2)
against their default plan (path 1, the 64-column reverse sweep), in ONE process: a warm-up round,
then interleaved repetitions, each call timed with HIP events on the current stream.

    python tools/bench_rowp_ab.py [--variants v2,v3] [--batches 20,1000] [--reps 30]
                                  [--commit HASH] [--out profiles/rowsplit_rowp_ab.json]

Three legs per (variant, batch), m = 250, n = 500, K = 15:
  forward   a training forward (keep_all, T, saved products, fused L1L1 objective);
  backward  dladmm_bwd_f32 on that forward's saved state (fused objective);
  step      a whole tools/bench_train.py step (--fused-loss: forward, backward, Adam), the two
            settings in alternating runs.
The outputs of the two settings are compared at the timed sizes (Z, E, L, T, P, gW bit for bit;
the per-row gradients to 1e-12).  Prints one JSON line and writes it to --out.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402  (synthetic inputs)
import bench_train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="v2,v3")
    ap.add_argument("--batches", default="20,1000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--m", type=int, default=250)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--commit", default="", help="recorded in the result")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    ops = importlib.import_module("d-ladmm_amd.ops")
    L = importlib.import_module("d-ladmm_amd._lib")
    dev = torch.device("cuda", 0)
    m, n, K = a.m, a.n, a.layers
    legs = {"off": 0, "on": L.F_ROWSPLIT_ROWP}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    med = lambda v: float(np.median(v))  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        ev0.record()
        r = fn()
        ev1.record()
        torch.cuda.synchronize()
        return r, ev0.elapsed_time(ev1)

    res = {"config": dict(m=m, n=n, K=K, reps=a.reps, step_rounds=a.step_rounds, commit=a.commit,
                          device=torch.cuda.get_device_name(0),
                          timing="HIP events around each call, median of interleaved "
                                 "repetitions after one warm-up round; step: host clock around "
                                 "a synchronised tools/bench_train.py --fused-loss step"),
           "cases": []}
    for variant in a.variants.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            torch.manual_seed(1126)
            A, X, Z0, E0, L0 = bench.synth(m, n, B, 0, dev)
            net = dl.VARIANTS[variant](m=m, n=0, d=n, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0,
                                       layers=K).cuda()
            with torch.no_grad():
                tables = net._tables(dev)
            W = [w.detach() for w in net._weights()]
            args = (net.VARIANT, X, net.A, W, net.Z0, net.E0, net.L0)
            coef = torch.tensor([[1e-3 / B, 1.0 / B]] * K, device=dev)
            fkw = dict(keep_all=True, want_T=True, want_P=True, loss_kind=L.LOSS_L1L1, **tables)
            bkw = dict(loss_kind=L.LOSS_L1L1, loss_coef=coef, **tables)
            tf = {k: [] for k in legs}
            tb = {k: [] for k in legs}
            fwd, bwd = {}, {}
            for rep in range(a.reps + 1):
                for k, fl in legs.items():
                    with torch.no_grad():
                        fwd[k], t = timed(lambda: ops.dladmm_forward(*args, flags=fl, **fkw))
                    if rep:
                        tf[k].append(t)
            for rep in range(a.reps + 1):
                for k in legs:
                    bwd[k], t = timed(lambda: ops.dladmm_backward(*args, fwd[k], **bkw))
                    if rep:
                        tb[k].append(t)
            same_f = all(torch.equal(getattr(fwd["on"], nm), getattr(fwd["off"], nm))
                         for nm in ("Z", "E", "L", "T", "P"))
            same_w = torch.equal(bwd["on"].gW, bwd["off"].gW)
            gr, gc = bwd["on"].g_row.double(), bwd["off"].g_row.double()
            row_err = float((gr - gc).norm() / gc.norm())
            # whole steps, the settings in alternating runs
            steps = {k: [] for k in legs}
            for _ in range(a.step_rounds):
                for k in legs:
                    sa = bench_train.parser().parse_args(
                        ["--variant", variant, "--batch", str(B), "--m", str(m), "--n", str(n),
                         "--layers", str(K), "--fused-loss", "--steps", "20", "--warmup", "3"] +
                        (["--plan-flags", "rowsplit_rows"] if k == "on" else []))
                    steps[k].append(bench_train.run(sa))
            case = dict(variant=variant, B=B,
                        fwd_path={k: fwd[k].path for k in legs},
                        bwd_path={k: bwd[k].path for k in legs},
                        outputs_bit_equal=bool(same_f), gW_bit_equal=bool(same_w),
                        g_row_nrel=row_err)
            for k in legs:
                case[k] = dict(forward_ms=med(tf[k]), forward_min_ms=float(np.min(tf[k])),
                               backward_ms=med(tb[k]), backward_min_ms=float(np.min(tb[k])),
                               step_ms=med([s["step_ms"] for s in steps[k]]),
                               step_forward_ms=med([s["forward_ms"] for s in steps[k]]),
                               step_backward_ms=med([s["backward_ms"] for s in steps[k]]),
                               step_ms_runs=[s["step_ms"] for s in steps[k]])
            case["speedup"] = {q: case["off"][q] / case["on"][q]
                               for q in ("forward_ms", "backward_ms", "step_ms")}
            res["cases"].append(case)
            del net, fwd, bwd
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
