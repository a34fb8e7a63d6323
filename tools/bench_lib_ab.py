"""A/B of builds of the library on the headline workload: bench.py run as a fresh process per
run, the arms alternated within each round (arm 0, arm 1, ..., arm 0, ...), DLADMM_LIB choosing
the build.  Prints one JSON object: every run's ms per step and kernel ms, per-arm median and
run-to-run range, and for every arm after the first (the baseline) the project's rule -- the
drop of the medians counts as a gain only if it is at least 3 x the larger range of the two arms.

    python tools/bench_lib_ab.py base=LIB0.so name1=LIB1.so ... [--runs 3] [--steps 200]
                                 [--warmup 3] [--out FILE] [-- extra bench.py arguments]
"""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        i = argv.index("--")
        argv, extra = argv[:i], argv[i + 1:]
    opt = {"--runs": 3, "--steps": 200, "--warmup": 3, "--out": ""}
    arms = []
    it = iter(argv)
    for a in it:
        if a in opt:
            v = next(it)
            opt[a] = v if a == "--out" else int(v)
        else:
            name, _, path = a.partition("=")
            arms.append((name, os.path.abspath(path)))
    runs = {name: [] for name, _ in arms}
    for rnd in range(opt["--runs"]):
        for name, path in arms:
            env = dict(os.environ, DLADMM_LIB=path)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                "--steps", str(opt["--steps"]), "--warmup", str(opt["--warmup"])]
                               + extra, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
                raise SystemExit(f"bench.py failed for arm {name} (exit {p.returncode})")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            run = {k: res.get(k) for k in ("ms_per_step", "value", "objective_last_layer")}
            run["kernel_ms"] = res.get("roofline", {}).get("kernel_ms")
            runs[name].append(run)
            print(f"[ab] round {rnd} {name}: {run['ms_per_step']:.4f} ms/step, kernel "
                  f"{run['kernel_ms']}", file=sys.stderr, flush=True)
    out = {"steps": opt["--steps"], "warmup": opt["--warmup"], "bench_args": extra,
           "rule": "gain iff median drop >= 3 x the larger run-to-run range of the two arms",
           "arms": {}}
    for name, path in arms:
        ms = [r["ms_per_step"] for r in runs[name]]
        out["arms"][name] = {"lib": os.path.relpath(path, ROOT), "runs": runs[name],
                             "median_ms": statistics.median(ms), "range_ms": max(ms) - min(ms)}
    base = arms[0][0]
    for name, _ in arms[1:]:
        a, b = out["arms"][base], out["arms"][name]
        drop = a["median_ms"] - b["median_ms"]
        rng = max(a["range_ms"], b["range_ms"])
        b["vs_" + base] = {"drop_ms": drop, "drop_frac": drop / a["median_ms"],
                           "larger_range_ms": rng, "gain": bool(drop >= 3 * rng and drop > 0)}
    s = json.dumps(out, indent=1)
    print(s)
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
