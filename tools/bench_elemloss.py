"""A/B timing of one training step on the supervised (main_syn_gt_ltheta.py:243-246) and the
reweighted (main_syn_l1l1_rw_ltheta.py:236-238) objectives at the scripts' workload (V2, m = 250,
d = 500, 20 layers, B = 20), in ONE process, the forms alternated call by call, HIP events around
forward + backward(), after warm-up (tools/bench_news_lskm.py):

  gt / rw              training_loss(kind=...) + backward(): sums and seeds in dladmm_elemloss_f32
  gt_torch / rw_torch  the differentiable forward(), then the script's loss lines in torch ops,
                       autograd through both
  l1l1                 training_loss(kind="l1l1") + backward(): the floor

`beats_spread` holds where the torch-op form's median exceeds the fused one's by more than the
torch-op form's own spread (p90 - p10).  --large also records one reading of the same three gt /
rw forms at V4, B = 65,536, K = 15 (no criterion).

    python tools/bench_elemloss.py [--calls 50] [--large] [--out profiles/elemloss_train_ab.json]
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


def measure(dl, cls, B, K, calls, warm):
    dev = torch.device("cuda", 0)
    M, N, alpha = 250, 500, 0.5   # the scripts' alpha
    A, X, Z0, E0, L0 = bench.synth(M, N, B, 0, dev)
    g = torch.Generator(device=dev).manual_seed(7)
    zs, es = ((torch.rand(r, B, generator=g, device=dev) < 0.1) *
              torch.randn(r, B, generator=g, device=dev) for r in (N, M))
    torch.manual_seed(0)
    net = getattr(dl, cls)(m=M, n=0, d=N, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0,
                           layers=K).cuda()
    rw_c = [0.05 * (k + 1) for k in range(K)]

    def step(loss):
        net.zero_grad(set_to_none=True)
        total = loss()
        total.backward()
        return total.detach()

    def gt_torch():
        Z, E = net(X)[:2]
        return sum(torch.sum((Z[k] - zs) ** 2.0) + torch.sum((E[k] - es) ** 2.0)
                   for k in range(K))

    def rw_torch():
        Z, E = net(X)[:2]
        return sum(rw_c[k] * (alpha * torch.mean(torch.abs(Z[k])) + torch.mean(torch.abs(E[k])))
                   for k in range(K))

    forms = {
        "gt": lambda: step(lambda: net.training_loss(X, alpha, kind="gt", z_label=zs,
                                                     e_label=es)[0]),
        "gt_torch": lambda: step(gt_torch),
        "rw": lambda: step(lambda: net.training_loss(X, alpha, rw_c, kind="rw")[0]),
        "rw_torch": lambda: step(rw_torch),
        "l1l1": lambda: step(lambda: net.training_loss(X, alpha, kind="l1l1")[0])}
    r = {name: stats(v) for name, v in timed(forms, calls, warm).items()}
    res = {"config": dict(model=cls, m=M, n=N, layers=K, batch=B, alpha=alpha, calls=calls,
                          warm=warm), **r}
    for kind in ("gt", "rw"):
        t = r[kind + "_torch"]
        res[kind + "_torch_spread_ms"] = t["p90_ms"] - t["p10_ms"]
        res[kind + "_beats_spread"] = bool(t["median_ms"] - r[kind]["median_ms"] >
                                           t["p90_ms"] - t["p10_ms"])
        tot = {name: float(forms[name]()) for name in (kind, kind + "_torch")}
        res[kind + "_totals"] = tot
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    res = {"scripts": measure(dl, "DLADMMNetLTheta", 20, 20, a.calls, a.warm)}
    if a.large:
        res["large"] = measure(dl, "DLADMMNetScalar", 65536, 15, 5, 2)
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
