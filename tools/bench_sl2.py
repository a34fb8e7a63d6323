"""A/B timing of one training step on the S-L2 objective of main_syn_l1l1-sl2_scalar.py
(:255-280) at the script's workload (m = 250, d = 500, 20 layers, B = 20, alpha = 0.001,
lam = 1e-4), in ONE process, the forms alternated call by call, HIP events around each call, after
warm-up (tools/bench_news_lskm.py):

  fused     training_loss(kind="sl2") + backward(): the term and its adjoint in dladmm_sl2_f32
  torch_ops the same objective without that kernel: the differentiable forward(), then the L1L1
            loss and the script's KM / S lines in torch ops, autograd through both
  l1l1      training_loss(kind="l1l1") + backward(): the step without the term

What the term costs is fused - l1l1 against torch_ops - l1l1; `term_saving_exceeds_spread` holds
where the difference of the two medians is larger than the torch-op form's own spread (p90 - p10).
Also recorded: the two forms' totals and the norm-relative distance of their gradients.

    python tools/bench_sl2.py [--calls 50] [--out profiles/sl2_train_ab.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
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
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    dev = torch.device("cuda", 0)
    M, N, B, K = 250, 500, a.batch, a.layers
    alpha, lam = 0.001, 1e-4
    A, X, Z0, E0, L0 = bench.synth(M, N, B, 0, dev)
    torch.manual_seed(0)
    net = dl.DLADMMNetScalarSl2(m=M, n=0, d=N, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0,
                                layers=K).cuda()
    coeffs = [0.6] * (K - 1) + [1.0]
    k = net._sl2_consts()
    ss1, ss2, c = k["ss1"], k["ss2"], math.sqrt(0.3 / 0.7)
    act = lambda x, th: torch.relu(x - th) - torch.relu(-1.0 * x - th)  # noqa: E731

    def step(loss):
        net.zero_grad(set_to_none=True)
        total = loss()
        total.backward()
        return total.detach()

    def torch_ops():
        Z, E, L, T = net(X)
        total = 0
        for j in range(K):
            lj = alpha * Z[j].abs().sum(0).mean() + (X - A @ Z[j]).abs().sum(0).mean()
            if j == K - 1:   # model.S(Z[k], E[k], L[k], T[k+1], X, Ep), :117-157
                Ep = E[j - 1] if j > 0 else E0
                Zn = act(Z[j] - ss1 * (A.t() @ (L[j] + T[j + 1])), ss1 * alpha)
                En = act(E[j] - ss2 * (L[j] + (A @ Zn + E[j] - X)), ss2)
                Sn = torch.cat([A @ Zn + En - X, c * (En - 2 * E[j] + Ep)])
                lj = lj + lam * (Sn ** 2).sum(0).mean()
            total = total + coeffs[j] * lj
        return total

    forms = {"fused": lambda: step(lambda: net.training_loss(X, alpha, coeffs, kind="sl2",
                                                             lam=lam)[0]),
             "torch_ops": lambda: step(torch_ops),
             "l1l1": lambda: step(lambda: net.training_loss(X, alpha, coeffs, kind="l1l1")[0])}
    t = timed(forms, a.calls, a.warm)
    r = {name: stats(v) for name, v in t.items()}
    tot = {}
    grads = {}
    for name in ("fused", "torch_ops"):
        tot[name] = float(forms[name]())
        grads[name] = torch.cat([p.grad.double().flatten() for p in net.parameters()])
    spread = r["torch_ops"]["p90_ms"] - r["torch_ops"]["p10_ms"]
    term_f = r["fused"]["median_ms"] - r["l1l1"]["median_ms"]
    term_t = r["torch_ops"]["median_ms"] - r["l1l1"]["median_ms"]
    res = {"config": dict(m=M, n=N, layers=K, batch=B, alpha=alpha, lam=lam, calls=a.calls,
                          warm=a.warm),
           **r, "torch_ops_spread_ms": spread, "term_fused_ms": term_f, "term_torch_ops_ms": term_t,
           "term_saving_exceeds_spread": bool(term_t - term_f > spread),
           "totals": tot,
           "grad_nrel_fused_vs_torch_ops": float((grads["fused"] - grads["torch_ops"]).norm() /
                                                 grads["torch_ops"].norm())}
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
