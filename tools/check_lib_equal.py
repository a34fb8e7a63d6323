"""Bit-for-bit comparison of two builds of the library on the row-split paths, in ONE process
(the libraries loaded as tools/bench_fwd_ab.py loads them, --libs; the first is the baseline).

For every variant (V2 / V3 under the plan flag rowsplit_rows; V7 runs on V5's tables), B in
--batches, forward paths 5 (no_xsplit) and 6 (default plan) at m = 250, n = 500:
  * forward: keep_all on / off x objective none / l1l1 / lasso, the saved product P with
    keep_all (V7 keeps no product) -- every output, loss sum and per-column term
    `torch.equal`;
  * the ELZ entry (V4 / V5 / V7, path 5), with and without the tail product;
  * backward (V1 .. V6, bwd paths 2 and 3): once with the fused objective, once with cotangents
    of Z / E / L / T -- every gradient `torch.equal`.
Prints one JSON line; --out also writes it.  Exit status 1 if anything differs.

    python tools/check_lib_equal.py --libs d-ladmm_amd/lib/abl/parent/libdladmm_hip.so,main \
        [--batches 20,77] [--out profiles/rowsplit_merge_equal.json]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import problems as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--batches", default="20,77")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dl = importlib.import_module("d-ladmm_amd")
    ops = importlib.import_module("d-ladmm_amd.ops")
    L = importlib.import_module("d-ladmm_amd._lib")
    specs = a.libs.split(",")
    assert len(specs) == 2, "--libs takes the baseline and the build under test"
    libs = []
    for spec in specs:
        L._LIB = None
        L.LIB_PATH = os.path.join(ROOT, "d-ladmm_amd", "lib", "libdladmm_hip.so") \
            if spec == "main" else os.path.join(ROOT, spec)
        libs.append(L.lib())
    m, n, K = 250, 500, a.layers
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    cases, diffs, paths, refused = 0, [], set(), []

    def both(tag, want_paths, fn):
        """fn() under each library: a dict of tensors (or lists of them); all must be equal."""
        nonlocal cases
        res = []
        for lib in libs:
            L._LIB = lib
            try:
                r = fn()
            except Exception as e:  # e.g. a configuration the C ABI refuses: both must
                r = dict(path=f"{type(e).__name__}: {e}")
            torch.cuda.synchronize()
            res.append(r)
        if isinstance(res[0]["path"], str) or isinstance(res[1]["path"], str):
            if res[0]["path"] != res[1]["path"]:
                diffs.append((tag, "refused", res[0]["path"], res[1]["path"]))
            refused.append(tag)
            return
        cases += 1
        p0, p1 = res[0].pop("path"), res[1].pop("path")
        paths.add(p1)
        if p0 != p1 or p1 not in want_paths:
            diffs.append((tag, "path", p0, p1))
        for k in res[0]:
            x, y = res[0][k], res[1][k]
            xs, ys = (x, y) if isinstance(x, (list, tuple)) else ([x], [y])
            for i, (u, v) in enumerate(zip(xs, ys)):
                if (u is None) != (v is None) or (u is not None and not torch.equal(u, v)) or \
                        (u is not None and not bool(torch.isfinite(u).all())):
                    diffs.append((tag, k, i))

    for B in [int(b) for b in a.batches.split(",")]:
        for vi, variant in enumerate(("v1", "v2", "v3", "v4", "v5", "v6", "v7")):
            base = "v5" if variant == "v7" else variant
            vid = L.V7_SCALAR_V1E if variant == "v7" else None
            d = dict(variant=base, m=m, n=n, B=B, K=K, seed=7000 + 10 * B + vi, perturb=0.1,
                     wscale=0.4 if base in ("v1", "v2") else P.VARIANT_SPECS[base].get("wscale"))
            inp, sd = P.build_problem(d)
            net = dl.VARIANTS[base](m=m, n=0, d=n, batch_size=B, A=t(inp["A"]), Z0=t(inp["Z0"]),
                                    E0=t(inp["E0"]), L0=t(inp["L0"]), layers=K)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            net.cuda().requires_grad_(False)
            X = t(inp["X"])
            with torch.no_grad():
                tables = net._tables(X.device)
            W = [w.detach() for w in net._weights()]
            args = (vid or net.VARIANT, X, net.A, W, net.Z0, net.E0, net.L0)
            rowp = L.F_ROWSPLIT_ROWP if variant in ("v2", "v3") else 0
            for split, fl, fpath in (("rs", L.F_NO_XSPLIT | rowp, 5), ("xs", rowp, 6)):
                for keep_all in (True, False):
                    for lk in (L.LOSS_NONE, L.LOSS_L1L1, L.LOSS_LASSO):
                        def fwd():
                            r = ops.dladmm_forward(*args, keep_all=keep_all, want_T=True,
                                                   want_P=keep_all and variant != "v7",
                                                   loss_kind=lk, want_col_loss=bool(lk),
                                                   flags=fl, **tables)
                            return dict(path=r.path, Z=r.Z, E=r.E, L=r.L, T=r.T, P=r.P,
                                        loss_sums=r.loss_sums, col_loss=r.col_loss)
                        both(f"fwd {variant} B={B} {split} keep_all={keep_all} loss={lk}",
                             (fpath,), fwd)
                if variant in ("v4", "v5", "v7") and split == "rs":
                    for tail in (False, True):
                        def elz():
                            new = lambda *sh: torch.empty(sh, device="cuda")  # noqa: E731
                            out = ops.ForwardResult(new(K, n, B), new(K, m, B), new(K, m, B),
                                                    None, None)
                            if tail:
                                out.P = new(K + 1, m, B)
                            r = ops.dladmm_forward(
                                *args, keep_all=True, want_T=False, out=out,
                                flags=fl | L.F_ELZ | (L.F_ELZ_TAIL if tail else 0), **tables)
                            return dict(path=r.path, Z=r.Z, E=r.E, L=r.L, P=r.P)
                        both(f"elz {variant} B={B} tail={tail}", (5,), elz)
                if variant == "v7":
                    continue
                lk = L.LOSS_LASSO if variant == "v6" else L.LOSS_L1L1
                for cot in (False, True):
                    def bwd():
                        g = torch.Generator(device="cuda").manual_seed(B)
                        with torch.no_grad():
                            r = ops.dladmm_forward(*args, keep_all=True, want_T=True, want_P=True,
                                                   loss_kind=lk, flags=fl, **tables)
                        rnd = lambda rows, cnt: [  # noqa: E731
                            torch.randn(rows, B, generator=g, device="cuda") / B for _ in range(cnt)]
                        if cot:
                            kw = dict(gZ=rnd(n, K), gE=rnd(m, K), gL=rnd(m, K), gT=rnd(m, K + 1))
                        else:
                            coef = (torch.rand(K, 2, device="cuda", generator=g) *
                                    torch.tensor([1e-2, 1.0], device="cuda")).contiguous()
                            kw = dict(loss_kind=lk, loss_coef=coef)
                        b = ops.dladmm_backward(*args, r, **kw, **tables)
                        return dict(path=10 * r.path + b.path, gW=b.gW, g_scalar=b.g_scalar,
                                    g_row=b.g_row, g_beta1=b.g_beta1, g_beta2=b.g_beta2)
                    both(f"bwd {variant} B={B} {split} cotangents={cot}",
                         (10 * fpath + fpath - 3,), bwd)
    res = dict(libs=specs, batches=a.batches, m=m, n=n, K=K, cases=cases,
               paths_seen=sorted(paths), refused_by_both=refused,
               differing=[list(map(str, x)) for x in diffs], all_equal=not diffs and cases > 0)
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if res["all_equal"] else 1)


if __name__ == "__main__":
    main()
