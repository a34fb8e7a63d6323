"""Bit-for-bit comparison of two builds of the library, in ONE process (the libraries loaded as
tools/bench_fwd_ab.py loads them, --libs; the first is the baseline).  --paths picks the groups
of cases (comma-separated, or `all`); every output, loss sum, per-column term and gradient must
be `torch.equal` and finite.

rowsplit (the default), at m, n = 250, 500: for every variant (V2 / V3 under the plan flag
rowsplit_rows; V7 runs on V5's tables), B in --batches, forward paths 5 (no_xsplit) and 6
(default plan):
  * forward: keep_all on / off x objective none / l1l1 / lasso, the saved product P with
    keep_all (V7 keeps no product);
  * the ELZ entry (V4 / V5 / V7, path 5), with and without the tail product;
  * backward (V1 .. V6, bwd paths 2 and 3): once with the fused objective, once with cotangents
    of Z / E / L / T.
The other groups run at the three register-resident shapes with ragged rows (m, n = 20, 30;
50, 200; 250, 500), B in --batches:
  * no_rowsplit: path 1, V1 .. V7 with the fused objective, with and without the saved product,
    and the ELZ entry (V4 / V5 / V7) with and without the tail;
  * f32_split: path 4, V1 / V4 / V5 / V6 (the batch rounded down to a multiple of 4);
  * per_layer, bf16: paths 2 and 3, one variant per E-step form (V1, V4, V6);
  * bwd1: the reverse sweep after a path-1 forward, V1 .. V6, with the fused objective and with
    cotangents;
  * and per group, at the largest shape, V4 with theta_z and theta_e negated and (the groups that
    hold it) V3 with its per-row ones negated: the other shrink form.
Prints one JSON line; --out also writes it.  Exit status 1 if anything differs.

    python tools/check_lib_equal.py --libs d-ladmm_amd/lib/abl/parent/libdladmm_hip.so,main \
        [--paths all] [--batches 20,77] [--out profiles/step_math_equal.json]
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

GROUPS = ("rowsplit", "no_rowsplit", "f32_split", "per_layer", "bf16", "bwd1")
SHAPES = ((20, 30), (50, 200), (250, 500))  # the register-resident shapes, ragged rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--batches", default="20,77")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--paths", default="rowsplit",
                    help="comma-separated groups of " + ",".join(GROUPS) + ", or all")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    groups = GROUPS if a.paths == "all" else tuple(a.paths.split(","))
    assert set(groups) <= set(GROUPS), f"--paths: groups of {GROUPS}"
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
    K = a.layers
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

    def problem(variant, vi, m, n, B, negate=False):
        """The variant's seeded problem at (m, n, B): forward arguments and parameter tables;
        negate: theta_z and theta_e of the scalar (V2 / V3: the row) table negated."""
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
        if negate:
            key = "row_params" if tables.get("row_params") is not None else "scalar_params"
            tab = tables[key].clone()
            tab[:, [L.P_THETA_Z, L.P_THETA_E]] *= -1.0
            tables = {**tables, key: tab}
        W = [w.detach() for w in net._weights()]
        return (vid or net.VARIANT, X, net.A, W, net.Z0, net.E0, net.L0), tables

    def elz_case(args, tables, m, n, B, fl, tail):
        new = lambda *sh: torch.empty(sh, device="cuda")  # noqa: E731
        out = ops.ForwardResult(new(K, n, B), new(K, m, B), new(K, m, B), None, None)
        if tail:
            out.P = new(K + 1, m, B)
        r = ops.dladmm_forward(*args, keep_all=True, want_T=False, out=out,
                               flags=fl | L.F_ELZ | (L.F_ELZ_TAIL if tail else 0), **tables)
        return dict(path=r.path, Z=r.Z, E=r.E, L=r.L, P=r.P)

    def bwd_case(args, tables, m, n, B, fl, lk, cot):
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

    def fwd_case(args, tables, fl, keep_all, lk, want_P, precision="f32"):
        r = ops.dladmm_forward(*args, keep_all=keep_all, want_T=True, want_P=want_P,
                               loss_kind=lk, want_col_loss=bool(lk), flags=fl,
                               precision=precision, **tables)
        return dict(path=r.path, Z=r.Z, E=r.E, L=r.L, T=r.T, P=r.P,
                    loss_sums=r.loss_sums, col_loss=r.col_loss)

    ALL = ("v1", "v2", "v3", "v4", "v5", "v6", "v7")
    lk_of = lambda v: L.LOSS_LASSO if v == "v6" else L.LOSS_L1L1  # noqa: E731
    # (group, variants, forward plan flags, precision, forward path)
    plans = (("no_rowsplit", ALL, L.F_NO_ROWSPLIT, "f32", 1),
             ("f32_split", ("v1", "v4", "v5", "v6"), 0, "f32_split", 4),
             ("per_layer", ("v1", "v4", "v6"), L.F_PER_LAYER, "f32", 2),
             ("bf16", ("v1", "v4", "v6"), 0, "bf16", 3),
             ("bwd1", ALL[:6], L.F_NO_ROWSPLIT, "f32", 1))
    for B0 in [int(b) for b in a.batches.split(",")]:
        for grp, variants, fl, prec, fpath in plans:
            if grp not in groups:
                continue
            # path 4 takes whole dwordx4 rows only (batch % 4 == 0; any other batch runs path 1)
            B = B0 - B0 % 4 if grp == "f32_split" else B0
            cases_of = [(v, m, n, False) for m, n in SHAPES for v in variants]
            cases_of += [(v, *SHAPES[-1], True) for v in ("v4", "v3") if v in variants]
            for variant, m, n, neg in cases_of:
                args, tables = problem(variant, ALL.index(variant), m, n, B, neg)
                tag = f"{grp} {variant} {m}x{n} B={B}" + (" negated thetas" if neg else "")
                lk = lk_of(variant)
                if grp == "bwd1":
                    for cot in (False, True):
                        both(f"{tag} cotangents={cot}", (11,),
                             lambda: bwd_case(args, tables, m, n, B, fl, lk, cot))
                    continue
                for want_P in ((False, True) if grp == "no_rowsplit" else (False,)):
                    both(f"{tag} keep_all loss={lk} P={want_P}", (fpath,),
                         lambda: fwd_case(args, tables, fl, True, lk,
                                          want_P and variant != "v7", prec))
                both(f"{tag} last layer", (fpath,),
                     lambda: fwd_case(args, tables, fl, False, L.LOSS_NONE, False, prec))
                if grp == "no_rowsplit" and variant in ("v4", "v5", "v7"):
                    for tail in (False, True):
                        both(f"{tag} elz tail={tail}", (1,),
                             lambda: elz_case(args, tables, m, n, B, fl, tail))
        if "rowsplit" not in groups:
            continue
        m, n, B = 250, 500, B0
        for vi, variant in enumerate(ALL):
            args, tables = problem(variant, vi, m, n, B)
            rowp = L.F_ROWSPLIT_ROWP if variant in ("v2", "v3") else 0
            for split, fl, fpath in (("rs", L.F_NO_XSPLIT | rowp, 5), ("xs", rowp, 6)):
                for keep_all in (True, False):
                    for lk in (L.LOSS_NONE, L.LOSS_L1L1, L.LOSS_LASSO):
                        fwd = lambda: fwd_case(args, tables, fl, keep_all, lk,  # noqa: E731
                                               keep_all and variant != "v7")
                        both(f"fwd {variant} B={B} {split} keep_all={keep_all} loss={lk}",
                             (fpath,), fwd)
                if variant in ("v4", "v5", "v7") and split == "rs":
                    for tail in (False, True):
                        elz = lambda: elz_case(args, tables, m, n, B, fl, tail)  # noqa: E731
                        both(f"elz {variant} B={B} tail={tail}", (5,), elz)
                if variant == "v7":
                    continue
                lk = lk_of(variant)
                for cot in (False, True):
                    bwd = lambda: bwd_case(args, tables, m, n, B, fl, lk, cot)  # noqa: E731
                    both(f"bwd {variant} B={B} {split} cotangents={cot}",
                         (10 * fpath + fpath - 3,), bwd)
    res = dict(libs=specs, paths=list(groups), batches=a.batches, K=K, cases=cases,
               paths_seen=sorted(paths), refused_by_both=refused,
               differing=[list(map(str, x)) for x in diffs], all_equal=not diffs and cases > 0)
    print(json.dumps(res))
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if res["all_equal"] else 1)


if __name__ == "__main__":
    main()
