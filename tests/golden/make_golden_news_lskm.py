"""Generate tests/golden/news_lskm_*.npz from the REFERENCE newS test-script classes (classic KM
/ learned + safeguarded KM of test_syn_l1l1_newS.py, test_syn_l1l1_newS_Acols.py,
test_syn_scalar_tied_newS_Acols.py and test_syn_scalar_ptied_newS_Acols.py).

Build container only (reads the reference checkout).  As make_golden_lskm.py: only `class
DLADMMNet` of the script -- parsed with `ast` -- and the updater classes of mu_updater.py are
executed, in a namespace that supplies the module globals the class reads (alpha, delta,
mu_k_method, mu_k_param, mu_updater_dict, args.continued, layers, K); the script's module level
never runs.  Each case runs on CPU in fp32 and fp64.  Stored: values only -- Z/E/L at selected
layers, sg_count, the fp64 run's Snorm of every Snorm_ELZ call, the decision margins, the
fp32-vs-fp64 gaps, Snorm_ELZ(E0, L0, Z0, X).

Every safeguarded fixture must have equal fp32 / fp64 counts and every fp64 decision at least
problems_news.MIN_MARGIN (relative) away from its threshold: asserted here, stored in the file.

Usage:  python tests/golden/make_golden_news_lskm.py [--ref /root/reference] [names ...]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problems  # noqa: E402
import problems_news as PN  # noqa: E402
from make_golden import nrel  # noqa: E402
from make_golden_lskm import load_classes  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def ref_class(ref_root, case, calls):
    ns = dict(torch=torch, nn=nn, F=F, np=np, sqrt=math.sqrt, print=lambda *a, **k: None)
    load_classes(os.path.join(ref_root, "mu_updater.py"),
                 {"EMAUpdater", "GSUpdater", "RTUpdater", "RMUpdater", "BlankUpdater"}, ns)
    ns["mu_updater_dict"] = {"EMA": ns["EMAUpdater"], "GS": ns["GSUpdater"],
                             "RT": ns["RTUpdater"], "RM": ns["RMUpdater"],
                             "None": ns["BlankUpdater"]}
    ns.update(alpha=case["alpha"], delta=case["delta"], mu_k_method=case["mu"],
              mu_k_param=case["mu_param"], layers=case["layers"], K=case["K"],
              args=types.SimpleNamespace(continued=case["continued"]))
    load_classes(os.path.join(ref_root, PN.SCRIPTS[case["script"]]), {"DLADMMNet"}, ns)
    base = ns["DLADMMNet"]

    class Recorded(base):   # keeps what every Snorm_ELZ call returned
        def Snorm_ELZ(self, *a, **k):
            s = base.Snorm_ELZ(self, *a, **k)
            calls.append(s.detach().double().numpy().copy())
            return s
    return Recorded


def run(ref_root, case, dtype):
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    d = case["defn"]
    inp, sd = problems.build_problem(d)
    calls = []
    cls = ref_class(ref_root, case, calls)
    conv = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    m, n = inp["A"].shape
    B = inp["X"].shape[1]
    net = cls(m=m, n=0, d=n, batch_size=B, A=conv(inp["A"]), Z0=conv(inp["Z0"]),
              E0=conv(inp["E0"]), L0=conv(inp["L0"]), layers=case["layers"],
              **problems.ctor_extra(d))
    net.load_state_dict({k: conv(v) for k, v in sd.items()}, strict=True)
    net = net.to(dtype)
    net.L = net.L.to(dtype)
    with torch.no_grad():
        out = net(conv(inp["X"]), case["learned"], case["safeguard"], case["continued"])
        calls_fwd = list(calls)
        s0 = net.Snorm_ELZ(net.E0, net.L0, net.Z0, conv(inp["X"])).double().numpy()
    return out, calls_fwd, s0, list(net.state_dict().keys())


def margins(case, snorm):
    """Re-run the mu updater (mu_updater.py) on the fp64 run's norms: per decision the relative
    distance |Snorm - (1 - delta) mu| / ((1 - delta) mu), and the safeguarded counts."""
    mu = snorm[0]
    mg, cnt = [], []
    p = case["mu_param"]
    for s in snorm[1:]:
        thr = (1.0 - case["delta"]) * mu
        keep = s < thr
        mg.append(np.abs(s - thr) / thr)
        cnt.append(float((~keep).sum()))
        if case["mu"] == "None":
            mu = np.full_like(s, 1e10)
        else:
            upd = {"EMA": p * s + (1 - p) * mu, "GS": (1 - p) * mu, "RT": s}[case["mu"]]
            mu = np.where(keep, upd, mu)
    return np.array(mg), np.array(cnt)


def make_one(name, case, ref_root):
    o32, _c32, s0_32, keys = run(ref_root, case, torch.float32)
    o64, c64, s0_64, _ = run(ref_root, case, torch.float64)
    n = len(o32[0])   # K, or K + 1 for the _Acols scripts (initial triple in front)
    pick = sorted({0, 1, n // 2, n - 1})
    rec = {"layers_kept": np.array(pick), "n_out": np.array(n)}
    for i, nm in enumerate("ZEL"):
        rec[nm] = np.stack([o32[i][j].numpy() for j in pick]).astype(np.float32)
        rec["gap_" + nm] = np.array([nrel(o32[i][j].numpy(), o64[i][j].numpy()) for j in pick])
    rec["snorm0"] = s0_64
    rec["gap_snorm0"] = np.array(nrel(s0_32, s0_64))
    if len(o32) == 4:
        rec["sg_count"] = np.asarray(o32[3], np.float64)
        rec["sg_count64"] = np.asarray(o64[3], np.float64)
        rec["snorm64"] = np.stack(c64)
        mg, cnt = margins(case, c64)
        nl = len(cnt)
        assert np.array_equal(rec["sg_count"], rec["sg_count64"]), (name, "fp32/fp64 counts")
        assert np.array_equal(cnt, rec["sg_count64"][:nl]), (name, "updater re-run")
        rec["margin"] = mg
        rec["min_margin"] = np.array(mg.min())
        assert mg.min() >= PN.MIN_MARGIN, (name, float(mg.min()))
    rec["meta"] = np.array(json.dumps(dict(name=name, case=case, keys=keys,
                                           torch=torch.__version__,
                                           source=PN.SCRIPTS[case["script"]])))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **rec)
    sg = rec.get("sg_count")
    print(f"{name:28s} {os.path.getsize(path)/1e3:7.1f} kB  max gap "
          f"{max(float(np.max(rec['gap_' + k])) for k in 'ZEL'):.2e}  sg_count "
          f"{None if sg is None else sg.tolist()}  min margin "
          f"{float(rec['min_margin']) if sg is not None else float('nan'):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    torch.set_num_threads(8)
    for nm in a.names or list(PN.NEWS_LSKM_FIXTURES):
        make_one(nm, PN.NEWS_LSKM_FIXTURES[nm], a.ref)


if __name__ == "__main__":
    main()
