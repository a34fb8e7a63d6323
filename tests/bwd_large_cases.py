"""The case table of the backward tests past the register-resident shapes (m > 256 or n > 512:
the per-layer backward kernels BK1 / BK2 / BK3 / WG of csrc/dladmm_backward.hip on their natural
plan) and the fp32 / fp64 oracle references those tests share.

tests/test_gpu_backward_large.py runs the cases on the GPU; tests/test_backward_large_cases.py
pins, on the CPU, the condition the seeds were chosen for: at these sizes a shrink mask that flips
on a near-threshold element moves a gradient by far more than rounding, which would show as a
large fp32-vs-fp64 `gap` of the oracle itself and widen the bar max(GTOL, 3 x gap) enough to hide
a real error.  Every case's seed keeps gap <= GTOL / 3 on every key, so the bar is GTOL everywhere,
and keeps every input of a kink (shrink thresholds, the l1 residual's sign) away from it (SEEDS
below).

Geometry (csrc/dladmm_capi.hip make_bwd_plan; MB / NB = 16-row blocks of m / n, 16-block
m-slices, 16-block n-slices, 128 x 128 weight-gradient tiles over the rows padded to 128, 64
columns per workgroup, split-K chunks of whole 16-column steps, ceil(512 / tiles) of them wanted):

  (257, 513, 70)    MB 17 -> 2 m-slices (the second: one block, one valid row); NB 33 -> padded
                    to 64 blocks = 4 n-slices, two of them pure padding; 3 x 5 = 15 tiles;
                    Bpad 80: 5 chunks of one step
  (264, 200, 1)     only m past the limit: 2 m-slices (second: one block, 8 valid rows), 2
                    n-slices; 3 x 2 = 6 tiles; Bpad 16: one chunk of one step
  (100, 600, 77)    only n past the limit: 1 m-slice, NB 38 -> 4 n-slices (third: 6 blocks, fourth
                    padding); 1 x 5 = 5 tiles; Bpad 80: 5 chunks
  (300, 530, 333)   MB 19 -> 2 m-slices (second: 3 blocks, last with 12 valid rows), NB 34 -> 4
                    n-slices; 3 x 5 = 15 tiles; six 64-column groups; Bpad 336: 21 one-step chunks
  (300, 530, 1000)  as above with Bpad 1008 = 63 steps, 35 chunks wanted -> 32-column chunks, 32
                    of them, the last 16 columns
  (300, 530, 561)   Bpad 576 = 36 steps -> 18 chunks of 32 columns: the smallest batch at this
                    tiling whose chunks and padded batch are whole 32-column sub-chunks, which the
                    split-f16 weight gradient needs (wgrad_x3_fits)
  (512, 2048, 70)   BASELINE config 4's m and n: 2 full m-slices, 8 n-slices, 4 x 16 = 64 tiles;
                    Bpad 80: 5 chunks
"""
from __future__ import annotations

import functools

import numpy as np

import problems as P

GTOL = 1e-4          # tests/test_gpu_backward.py
GAP_MAX = GTOL / 3   # the oracle's own fp32-vs-fp64 distance every case's seed must keep

# (m, n, B, K) by name
SHAPES = {
    "257x513_b70": (257, 513, 70, 3),
    "264x200_b1": (264, 200, 1, 3),
    "100x600_b77": (100, 600, 77, 3),
    "300x530_b333": (300, 530, 333, 3),
    "300x530_b1000": (300, 530, 1000, 3),
    "300x530_b561": (300, 530, 561, 3),
    "512x2048_b70": (512, 2048, 70, 2),
}

# The seed of every (shape, variant) the tests run: the first of 9700, 9701, ... that meets both
# conditions tests/test_backward_large_cases.py pins, for the losses the case is used with --
#   (a) the oracle's fp32-vs-fp64 gap stays under GAP_MAX on every key (in fact under 1e-5);
#   (b) no input of a kink of the fp64 forward or loss -- a shrink input against its threshold,
#       the l1l1 residual X - A Z_k against 0 -- lies within MARGIN_SIGMAS x sigma of the kink,
#       sigma being the rms fp32-vs-fp64 deviation of those inputs (kink_margin).
# (a) alone says only that numpy's fp32 rounding flipped no mask.  The GPU (and torch's own mm
# under a torch-op loss) sums its GEMMs in another order, so it draws its own rounding errors of
# about the same sigma (1e-7 here; measured 1.0-1.5 x numpy's) and flips what sits closer to its
# kink than that.  Both were seen on the MI355X with seeds that met (a):
#   V4 at B = 1,000, seed 9700 (gap 2.6e-6): an E-step input 1.9e-8 = 0.2 sigma from its
#     threshold flipped; beta2.1 8.4e-4, fc.1.weight 5.8e-4, beta2.0 1.1e-4 from the oracle;
#     without that one column of the batch the worst key is 7.4e-6.
#   V2 at B = 333, seed 9703: no shrink mask differs, but a residual 1.5e-7 = 1.2 sigma from 0
#     changed sign in the torch-op loss; beta1.0 / active_para.0 / fc.0.weight 1.9e-4 - 2.3e-4,
#     all of it in that column's share of gU_0 (the layer's E-step keys stayed at 5e-7).
# V1 at B = 1,000 (3.4 million kink inputs, thresholds 0.025 / 0.06) reaches 1.72 sigma at best
# in 300 seeds: its columns are drawn from a pool (POOL below).
MARGIN_SIGMAS = 3.0
SEEDS = {
    "257x513_b70": dict(v4=9702, v6=9700, v1=9702, v3=9700),
    "264x200_b1": dict(v4=9700, v6=9700, v1=9700, v3=9700),
    "100x600_b77": dict(v4=9700, v6=9700, v1=9701, v3=9702),
    "300x530_b333": dict(v1=9703, v2=9716, v3=9709, v4=9701, v5=9729, v6=9700, v7=9700,
                         v7t=9705, v7p=9711),
    "300x530_b1000": dict(v4=9849, v6=9701, v1=9744, v3=9701),
    "300x530_b561": dict(v4=9714, v6=9702),
    "512x2048_b70": dict(v4=9700, v6=9700, v1=9709, v3=9700),
}

BASE_VARIANTS = ("v4", "v6", "v1", "v3")
ALL_VARIANTS = ("v1", "v2", "v3", "v4", "v5", "v6", "v7", "v7t", "v7p")

# test_large_grads_match_oracle: the torch-op training loss plus seeded cotangents on Z, E, L (T)
ORACLE_CASES = [(s, v) for s in ("257x513_b70", "264x200_b1", "100x600_b77") for v in BASE_VARIANTS] \
    + [("300x530_b333", v) for v in ALL_VARIANTS] \
    + [(s, v) for s in ("300x530_b1000", "512x2048_b70") for v in BASE_VARIANTS]
# test_large_fused_training_loss: net.training_loss
FUSED_CASES = [(s, v) for s in ("257x513_b70", "300x530_b333", "512x2048_b70")
               for v in ("v4", "v6")]
# test_large_column_shards_sum (no oracle), test_large_split_wgrad (fused objective), determinism
SHARD_CASES = [("300x530_b1000", v) for v in ("v4", "v1", "v6")]
SPLIT_WGRAD_CASES = [("300x530_b561", v) for v in ("v4", "v6")]
DETERMINISM_CASES = [("300x530_b333", v) for v in ("v4", "v3")]

# every (shape, variant, loss) whose oracle reference a GPU test applies the bar to:
# loss "full" = training loss + cotangents, "train" = the bare training loss (fused objective)
REFERENCE_CASES = [(s, v, "full") for s, v in ORACLE_CASES] + \
    [(s, v, "train") for s, v in FUSED_CASES + SPLIT_WGRAD_CASES]

# parameters only the E- / L-step of a layer reads: the last layer's are outside the graph of a
# loss that cannot reach E_{K-1} / L_{K-1} (reference autograd leaves their .grad None)
EL_ONLY = ("beta2", "beta3", "ss2", "ss2_1", "ss2_2", "active_para1")


def loss_kind(variant: str) -> str:
    return "lasso" if variant == "v6" else "l1l1"


def defn(shape: str, variant: str) -> dict:
    m, n, B, K = SHAPES[shape]
    d = dict(variant=variant, m=m, n=n, B=B, K=K, seed=SEEDS[shape][variant], perturb=0.1)
    if variant in ("v1", "v2"):
        d["wscale"] = 0.4   # V1 / V2 at W = 0.4 A^T: their default init is ill-conditioned
    if variant == "v7p":
        d["interval"] = 1   # K = 3 layers: one weight per layer, each scaled by ss1_k
    return d


def unreachable(variant: str, K: int, loss: str):
    """state_dict keys no cotangent of the loss reaches.  The bare training loss reads Z only; the
    newS schedules return E[k] = V4 E_{k-1}, L[k] = V4 L_{k-1}, never the last layer's."""
    if loss == "full" and variant not in ("v7", "v7t", "v7p"):
        return set()
    names = [nm for nm, _, _ in P.VARIANT_SPECS[variant]["params"]]
    return {f"{nm}.{K - 1}" for nm in names if nm in EL_ONLY}


@functools.lru_cache(maxsize=None)
def problem(shape: str, variant: str):
    """(definition, inputs, state_dict, upstream cotangents) of a case.  E0 and L0 are seeded
    N(0, 0.1^2) here, not the reference's zeros (main_lena.py:182-183): with L0 = 0 the gradient
    of layer 0's L_{k-1} coefficient (V1 / V2 beta2.0, V6 ss2_2.0) is identically zero whatever
    the kernel reads there, and a wrong row offset into E0 / L0 in the second m-slice would read
    the same zeros as the right one."""
    d = defn(shape, variant)
    pool = POOL.get((shape, variant))
    dp = dict(d, B=pool) if pool else d
    inp, sd = P.build_problem(dp)
    rng = np.random.default_rng(d["seed"] + 15485863)
    inp = dict(inp, E0=(0.1 * rng.standard_normal(inp["E0"].shape)).astype(np.float32),
               L0=(0.1 * rng.standard_normal(inp["L0"].shape)).astype(np.float32))
    up = P.make_upstream(dp, P.VARIANT_SPECS[variant]["ret_t"])
    if pool:
        inp, sd, up = _clear_columns(d, pool, inp, sd, up)
    return d, inp, sd, up


# Cases drawn from a pool of columns: where no seed keeps all B columns MARGIN_SIGMAS away from
# every kink (V1 at B = 1,000: 1.72 sigma at best in 300 seeds, and at that seed the GPU took the
# other branch of one: beta1.0 5.0e-4 from the oracle), the seed generates `pool` columns and the
# case is the first B of them whose own kink inputs all lie POOL_SIGMAS x sigma away, judged on
# the fp64 oracle alone.  A column's forward state does not depend on its neighbours, so the
# choice of columns changes no column's margins.
POOL = {("300x530_b1000", "v1"): 1100}
POOL_SIGMAS = 4.0


def _clear_columns(d, pool, inp, sd, up):
    from oracle import dladmm_oracle_grad as og
    variant, K, B = d["variant"], d["K"], d["B"]
    kept = {}
    for dt in (np.float32, np.float64):
        kept[dt] = {}
        og.vjp(variant, inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, K, dtype=dt,
               keep=kept[dt])
    _, sigma, col = _kink_margin(kept[np.float32], kept[np.float64], inp["X"],
                                 loss_kind(variant))
    cols = np.flatnonzero(col >= POOL_SIGMAS * sigma)[:B]
    assert len(cols) == B, f"pool of {pool} columns has only {len(cols)} clear ones"
    cut = lambda a: np.ascontiguousarray(a[..., cols]) if a.shape[-1] == pool else a  # noqa: E731
    return ({k: cut(v) for k, v in inp.items()}, type(sd)((k, cut(v)) for k, v in sd.items()),
            {k: cut(v) for k, v in up.items()})


@functools.lru_cache(maxsize=None)
def reference(shape: str, variant: str, loss: str):
    """(ref64, gap): the fp64 oracle's gradients by state_dict key and the fp32 oracle's
    norm-relative distance from them.  Computed once per case and shared: treat as read-only."""
    from oracle import dladmm_oracle as fwd
    from oracle import dladmm_oracle_grad as og
    d, inp, sd, up = problem(shape, variant)
    K, kind = d["K"], loss_kind(variant)
    res, kept = {}, {np.float32: {}, np.float64: {}}
    for dt in (np.float32, np.float64):
        args = (variant, inp["X"], inp["A"], inp["Z0"], inp["E0"], inp["L0"], sd, K)
        o = fwd.forward(*args, dtype=dt)
        gz = og.train_loss_grads(o["Z"], inp["X"], inp["A"], P.GRAD_ALPHA, P.loss_coeffs(K), kind,
                                 dtype=dt)
        if loss == "train":
            res[dt] = og.vjp(*args, gZ=gz, dtype=dt, keep=kept[dt])
        else:
            gz = [a + b for a, b in zip(gz, up["Gz"])]
            res[dt] = og.vjp(*args, gZ=gz, gE=list(up["Ge"]), gL=list(up["Gl"]),
                             gT=list(up["Gt"]) if "Gt" in up else None, dtype=dt,
                             keep=kept[dt])
    gap = {k: nrel(res[np.float32][k], res[np.float64][k]) for k in res[np.float64]}
    _MARGINS[(shape, variant)] = _kink_margin(kept[np.float32], kept[np.float64], inp["X"],
                                               kind)[:2]
    return res[np.float64], gap


_MARGINS: dict = {}


def _kink_margin(k32, k64, X, kind):
    """(margin, sigma, per-column margin) over every input of a kink of the forward and the loss: U_k of the Z-step's
    shrink, the E-step's input where it has a shrink, and, under the l1l1 loss, the residual
    X - A Z_k whose sign is the fit term's gradient.  margin = the smallest distance of an fp64
    input from its kink (| |u| - |theta| |, |X - A Z_k|), sigma = the rms fp32-vs-fp64 deviation
    of those inputs."""
    col, sq, cnt = None, 0.0, 0
    K = len(k64["U"])
    kinks = [(k32["U"], k64["U"], k64["thz"]), (k32["Eh"], k64["Eh"], k64["the"])]
    if kind == "l1l1":
        X = np.asarray(X, np.float64)
        kinks.append(([X - np.asarray(p, np.float64) for p in k32["P"]],
                      [X - p for p in k64["P"]], [0.0] * K))
    for a32, a64, ths in kinks:
        for u32, u64, t in zip(a32, a64, ths):
            if u64 is None:
                continue
            c = np.min(np.abs(np.abs(u64) - np.abs(t)), axis=0)
            col = c if col is None else np.minimum(col, c)
            sq += float(np.sum((np.asarray(u32, np.float64) - u64) ** 2))
            cnt += u64.size
    return float(col.min()), float(np.sqrt(sq / cnt)), col


def kink_margin(shape: str, variant: str):
    """(margin, sigma) of a case's forward (_kink_margin); any loss: the forward is the same."""
    if (shape, variant) not in _MARGINS:
        loss = next(l for s, v, l in REFERENCE_CASES if (s, v) == (shape, variant))
        reference(shape, variant, loss)
    return _MARGINS[(shape, variant)]


def nrel(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a))
