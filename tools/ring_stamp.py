"""The fused fp32 kernel's chunk-boundary step in parts, from its DLADMM_STAMP=2 diagnostic build.

    python tools/ablate.py --unit dladmm_fused_p0.hip stamp2=-DDLADMM_STAMP=2
    (and dladmm_capi.hip with -DX3_STAMP=1, which makes the library read DLADMM_DBG_PTR)
    DLADMM_LIB=d-ladmm_amd/lib/abl/stamp2/libdladmm_hip.so python tools/ring_stamp.py [OUT.json]

The tool cannot read the ring's chunk size from the library: it counts the boundary steps per
class for RING_CHUNK fragments per chunk (environment, default 32: the headline kernel's two-slot
ring; set RING_CHUNK=16 for a build with -DDLADMM_RING2=0).

Runs the headline workload (V4, m=256, n=512, K=15, B=65536, all layers written, the load-P0
form after the first call) and prints, as the mean over waves: total cycles, the G1 / G2 passes,
and per class of boundary step (G1 | G2 pass, with | without an epilogue row) the cycles of the
vmcnt wait, the s_barrier, barrier exit to the end of the DMA issue, and the rest of the step;
with the spread form, the issue of the pieces in the other steps.  Read the shares, not the
absolute time: every stamp drains the wave's LDS reads.
"""
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, M, N, K = 65536, 256, 512, 15
MB, NB = M // 16, N // 16
PARTS = ("vmcnt_wait", "s_barrier", "dma_issue", "rest_of_step")
CLASSES = ("g1_norow", "g1_row", "g2_norow", "g2_row")


def boundary_steps(chunk):
    """Boundary steps per forward and class (rows at step (i * SP) / 8 of a pair of SP steps)."""
    spc = chunk // 2
    cnt = dict.fromkeys(CLASSES, 0)
    for s in range((NB // 2) * MB):
        if s % spc == spc - 1:
            cnt["g1_row" if any((i * MB) // 8 == s % MB for i in range(8)) else "g1_norow"] += K
    for s in range((MB // 2) * NB):
        if s % spc == spc - 1:
            cnt["g2_row" if any((i * NB) // 8 == s % NB for i in range(8)) else "g2_norow"] += K
    return cnt


def main():
    dev = torch.device("cuda", 0)
    dbg = torch.zeros(B // 16 * 32, dtype=torch.int64, device=dev)
    os.environ["DLADMM_DBG_PTR"] = str(dbg.data_ptr())
    import bench
    dl = importlib.import_module("d-ladmm_amd")
    A, X, Z0, E0, L0 = bench.synth(M, N, B, 0, dev)
    net = dl.DLADMMNetScalar(m=M, n=0, d=N, batch_size=B, A=A, Z0=Z0, E0=E0, L0=L0, layers=K)
    net.requires_grad_(False)
    with torch.no_grad():
        for _ in range(3):
            r = net.run(X, keep_all=True, loss_kind=dl._lib.LOSS_L1L1)
            reused = bool(r.p0_reused)
            del r
    torch.cuda.synchronize()
    v = dbg.view(-1, 32).double().mean(0).tolist()
    chunk = int(os.environ.get("RING_CHUNK", "32"))
    steps = boundary_steps(chunk)
    out = {"p0_reused": reused, "chunk": chunk, "total": v[0], "g1_passes": v[1],
           "g2_passes": v[2], "ring_vmcnt": v[4], "ring_barrier": v[5], "boundary": {},
           "spread_piece_issue": {"g1": v[24], "g2": v[25]}}
    for c, cls in enumerate(CLASSES):
        d = {p: v[8 + 4 * c + i] for i, p in enumerate(PARTS)}
        d["steps"] = steps[cls]
        d["cycles_per_step"] = sum(d[p] for p in PARTS) / max(1, steps[cls])
        out["boundary"][cls] = d
    bsum = sum(out["boundary"][c][p] for c in CLASSES for p in PARTS)
    out["boundary_share_of_total"] = bsum / v[0]
    for p in PARTS:
        out["share_" + p] = sum(out["boundary"][c][p] for c in CLASSES) / v[0]
    # a step that holds no barrier, per pass kind: what a boundary step would cost without one
    for g, key, nsteps in (("g1", "g1_passes", (NB // 2) * MB), ("g2", "g2_passes", (MB // 2) * NB)):
        bs = sum(sum(out["boundary"][c][p] for p in PARTS) for c in CLASSES if c.startswith(g))
        nb = sum(steps[c] for c in CLASSES if c.startswith(g))
        out[g + "_plain_step_cycles"] = (out[key] - bs) / (K * nsteps - nb)
    s = json.dumps(out, indent=1)
    print(s)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
