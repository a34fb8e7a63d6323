"""Workload for a kernel trace of the safeguarded newS forward: `--calls` calls of
`DLADMMNetNewSLSKM` (or, with --old, of `DLADMMNetLSKM`) at m = 250, d = 500, 20 layers, EMA 0.5,
delta 0.05, after warm-up.  Also prints the host-side issue time against the wall time of one call.

    rocprofv3 --kernel-trace --stats -d <dir> -o news -- python tools/prof_news_lskm.py --batch 1000
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--old", action="store_true")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    dev = torch.device("cuda", 0)
    A, X, Z0, E0, L0 = bench.synth(250, 500, a.batch, 0, dev)
    cls = dl.DLADMMNetLSKM if a.old else dl.DLADMMNetNewSLSKM
    torch.manual_seed(0)
    net = cls(m=250, n=0, d=500, batch_size=a.batch, A=A, Z0=Z0, E0=E0, L0=L0, layers=20,
              alpha=0.01, delta=0.05, mu_k_method="EMA", mu_k_param=0.5).cuda()
    for _ in range(3):
        net(X, True, True, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        net(X, True, True, False)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"{cls.__name__} B={a.batch}: host issue {(t1 - t0) * 1e3 / a.calls:.3f} ms per call, "
          f"wall {(t2 - t0) * 1e3 / a.calls:.3f} ms per call")


if __name__ == "__main__":
    main()
