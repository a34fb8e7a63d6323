"""The element-wise training terms (ops.dladmm_elemloss -> dladmm_elemloss_f32,
csrc/dladmm_elemloss.hip) and training_loss(kind="gt" | "rw") against a torch fp64 restatement
of the reference forwards (main_syn_gt.py:57-98, main_syn_gt_ltheta.py:59-98,
main_syn_l1l1_scalar.py:74-131) and loss lines (main_syn_gt.py:243-248,
main_syn_l1l1_rw_ltheta.py:236-238), differentiated by autograd.

Bars: sums, totals and per-layer losses within 1e-5 relative (tests/test_gpu_lena.py's bar for
fused losses); cotangents within 1e-6 norm-relative (two fp32 roundings per element, ~1.2e-7);
parameter gradients within GTOL = 1e-4 norm-relative (tests/test_gpu_backward.py), no element
excluded; column shards' fp64 sums within 1e-9 relative of the whole batch's.
"""
import functools

import pytest
import torch

GTOL = 1e-4
ALPHA = 0.5  # the scripts' alpha (main_syn_gt.py:157, main_syn_l1l1_rw_ltheta.py:163)

#        id           model             m    n    K  B     seed cols
CASES = [("v2_script", "DLADMMNetLTheta", 250, 500, 3, 20, 21, None),  # ragged column tile; a
         # slab ending inside n and one straddling the Z / E boundary
         ("v1_script", "DLADMMNet", 250, 500, 2, 20, 22, None),        # per-sample betas
         ("v4_tiny", "DLADMMNetScalar", 16, 32, 2, 5, 23, None),       # heavy padding
         ("v4_two_tiles", "DLADMMNetScalar", 100, 120, 3, 70, 24, None),  # second tile ragged
         ("v2_K1", "DLADMMNetLTheta", 250, 500, 1, 20, 25, None),      # a single layer
         ("v4_cols", "DLADMMNetScalar", 100, 120, 3, 56, 26, (8, 48)),  # ld > column count
         # the two sides of the tile switch (csrc/dladmm_elemloss.h kElWideBatch = 2048)
         ("v4_narrow_max", "DLADMMNetScalar", 100, 120, 2, 2047, 27, None),
         ("v4_wide", "DLADMMNetScalar", 100, 120, 2, 2050, 28, None),
         # n no multiple of the narrow access's 4 rows; a second launch past 64 layers
         ("v4_n30_K65", "DLADMMNetScalar", 16, 30, 65, 5, 29, None)]
IDS = [c[0] for c in CASES]
DEFAULTS = {"DLADMMNet": dict(beta1=1.0, beta2=1.0),
            "DLADMMNetLTheta": dict(beta1=1.0, beta2=1.0, active_para=0.025, active_para1=0.06),
            "DLADMMNetScalar": dict(beta1=1.0, beta2=1.0, beta3=1.0, ss2=1.0, active_para=0.2,
                                    active_para1=0.8)}


def rel(a, b):
    """Largest element-wise relative error; a reference of exactly 0 asks for exactly 0."""
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    nb = float(b.norm())
    return float((a - b).norm()) / nb if nb > 0 else float(a.norm())


@functools.lru_cache(maxsize=None)
def problem(case):
    """gen_syn_data.py's distribution with its sparse zs / es as the labels, the scripts' Z0 /
    E0 / L0, and the models' parameters perturbed by 10 % with 0.4 * (A^T + 1e-3 N) weights; fp32
    CPU tensors, never modified."""
    _, cls, m, n, K, B, seed, _ = case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    A = rn(m, n)
    A = A / A.pow(2).sum(0, keepdim=True).sqrt()
    zs = (torch.rand(n, B, generator=g) < 0.1) * rn(n, B)
    es = (torch.rand(m, B, generator=g) < 0.1) * rn(m, B)
    inp = dict(A=A.float(), X=(A @ zs + es).float(), zs=zs.float(), es=es.float(),
               Z0=(torch.rand(n, B, generator=g) / n).float(),
               E0=torch.zeros(m, B), L0=torch.zeros(m, B))
    sd = {}
    for k in range(K):
        for nm, val in DEFAULTS[cls].items():
            rows = n if nm == "active_para" else m
            shape = {"DLADMMNet": (m, B), "DLADMMNetLTheta": (rows, 1)}.get(cls, (1, 1))
            sd[f"{nm}.{k}"] = (val * (1.0 + 0.1 * rn(*shape))).float()
        sd[f"fc.{k}.weight"] = (0.4 * (inp["A"].t() + 1e-3 * rn(n, m))).float().contiguous()
    return inp, sd


def make_net(dl, case):
    _, cls, m, n, K, B, _, _ = case
    inp, sd = problem(case)
    net = getattr(dl, cls)(m=m, n=0, d=n, batch_size=B, A=inp["A"], Z0=inp["Z0"], E0=inp["E0"],
                           L0=inp["L0"], layers=K)
    net.load_state_dict(sd, strict=True)
    return net.cuda(), inp


def shard(case, t):
    """The case's columns of a (rows, B) tensor: a view with the whole batch's row stride."""
    return t if case[7] is None else t[:, case[7][0]:case[7][1]]


# ---- the restatement (fp64) -------------------------------------------------------------------
def shrink(x, th):
    return torch.relu(x - th) - torch.relu(-1.0 * x - th)


def forward64(cls, p, X, A, Z, E, L, K):
    Zs, Es = [], []
    T = A @ Z + E - X
    for k in range(K):
        b1 = p[f"beta1.{k}"]
        if cls == "DLADMMNetScalar":                            # main_syn_l1l1_scalar.py:74-131
            Z = shrink(Z - p[f"fc.{k}.weight"] @ (L + b1 * T), p[f"active_para.{k}"])
            VVar = L + p[f"beta2.{k}"] * (A @ Z + E - X)
            E = shrink(E - p[f"ss2.{k}"] * VVar, p[f"active_para1.{k}"])
            b3 = p[f"beta3.{k}"]
        else:                                                   # main_syn_gt.py:68-89
            thz, the = (0.025, 0.06) if cls == "DLADMMNet" else \
                (p[f"active_para.{k}"], p[f"active_para1.{k}"])
            Z = shrink(Z - p[f"fc.{k}.weight"] @ (L + b1 * T), thz)
            E = shrink(X - A @ Z - p[f"beta2.{k}"] * L, the)
            b3 = b1
        T = A @ Z + E - X
        L = L + b3 * T
        Zs.append(Z), Es.append(E)
    return Zs, Es


def layer_loss(kind, Z, E, zs, es, denom):
    if kind == "gt":                                            # main_syn_gt.py:243-248
        return (((Z - zs) ** 2.0).sum() + ((E - es) ** 2.0).sum()) / denom
    return ALPHA * Z.abs().mean() + E.abs().mean()              # main_syn_l1l1_rw_ltheta.py:237


@functools.lru_cache(maxsize=None)
def objective64(case, kind, coeffs, denom):
    """total, per-layer losses and parameter gradients (None where autograd gives None), fp64."""
    cls, K = case[1], case[4]
    inp, sd = problem(case)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    X, Z0, E0, L0, zs, es = (shard(case, inp[k].double()) for k in
                             ("X", "Z0", "E0", "L0", "zs", "es"))
    Z, E = forward64(cls, p, X, inp["A"].double(), Z0, E0, L0, K)
    per = [layer_loss(kind, Z[k], E[k], zs, es, denom) for k in range(K)]
    total = sum(c * v for c, v in zip(coeffs, per) if c != 0.0)
    total.backward()
    return total.detach(), torch.stack(per).detach(), {k: v.grad for k, v in p.items()}


# ---- the op at the GPU forward's own outputs ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("power", [2, 1], ids=["square", "abs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_elemloss_op_vs_fp64(dl, case, power):
    K = case[4]
    net, inp = make_net(dl, case)
    X = shard(case, inp["X"]).contiguous().cuda()
    with torch.no_grad():
        r = net._run_shard(X, case[7], want_T=False)
    zs, es = shard(case, inp["zs"].cuda()), shard(case, inp["es"].cuda())
    if power == 1:
        zs = es = None          # the reweighted loss has no reference: exact zeros of E_k count
    w = torch.linspace(0.3, 0.7, K, device="cuda")
    tot = torch.empty((K, 2), device="cuda", dtype=torch.float64)
    run = lambda **o: dl.ops.dladmm_elemloss(r.Z, r.E, zs, es, power=power, **o)  # noqa: E731
    s0 = run(total=tot)
    out = run(coef=w)
    again = run(coef=w)
    last = run(coef=w, want=[False] * (K - 1) + [True])

    for t, (V, ref, g) in enumerate(((r.Z, zs, out[1]), (r.E, es, out[2]))):
        d = V.double() - (0.0 if ref is None else ref.double())
        term = d ** 2 if power == 2 else d.abs()
        cs = term.sum(1)
        g64 = w.double()[:, None, None] * (2 * d if power == 2 else torch.sign(d))
        serr, terr = rel(s0[:, t], cs), rel(tot[:, t], cs.sum(1))
        print(f"{case[0]} power {power} {'ZE'[t]}: colsum {serr:.3g} total {terr:.3g} "
              f"cotangent {nrel(g, g64):.3g}")
        assert serr <= 1e-5 and terr <= 1e-5
        assert nrel(g, g64) <= 1e-6
        if power == 1:
            assert not bool(g[V == 0].any())                   # sgn(0) = 0, exactly
            assert t == 0 or bool((V == 0).any())              # E_k does hold exact zeros
    assert torch.equal(s0, out[0])                             # sums only == adjoint form
    for a, b in zip(out, again):                               # repeatable, bit for bit
        assert torch.equal(a, b)
    assert torch.equal(last[0], out[0])
    assert torch.equal(last[1][K - 1], out[1][K - 1]) and torch.equal(last[2][K - 1],
                                                                      out[2][K - 1])
    # two column shards (views: row stride > columns) sum to the whole batch, in fp64
    B = X.shape[1]
    parts = []
    for c0, c1 in ((0, B // 3), (B // 3, B)):
        cut = lambda t: None if t is None else t[..., c0:c1]  # noqa: E731
        pt = torch.empty_like(tot)
        dl.ops.dladmm_elemloss(cut(r.Z), cut(r.E), cut(zs), cut(es), power=power, total=pt)
        parts.append(pt)
    assert rel(parts[0] + parts[1], tot) <= 1e-9


# ---- the whole path -----------------------------------------------------------------------------
def scripts_coeffs(kind, K):
    return tuple(0.05 * (k + 1) for k in range(K)) if kind == "rw" else (1.0,) * K


WHOLE = [(c, kind, scripts_coeffs(kind, c[4]), "sum") for c in CASES[:6] for kind in ("gt", "rw")]
# the layerwise scripts' form: the last layer only, the column mean
WHOLE.append((CASES[3], "gt", (0.0, 0.0, 1.0), "mean"))
WIDS = [f"{c[0]}-{kind}" for c, kind, _, _ in WHOLE[:-1]] + ["v4_two_tiles-gt-layerwise"]


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind,coeffs,reduction", WHOLE, ids=WIDS)
def test_training_loss_vs_fp64_autograd(dl, case, kind, coeffs, reduction):
    net, inp = make_net(dl, case)
    net.requires_grad_(True)
    cols = case[7]
    X = shard(case, inp["X"]).contiguous().cuda()
    B = X.shape[1]
    kw = dict(kind=kind, cols=cols)
    if kind == "gt":   # the shard's columns of the labels, as views
        kw.update(z_label=shard(case, inp["zs"].cuda()), e_label=shard(case, inp["es"].cuda()),
                  reduction=reduction)
    total, per = net.training_loss(X, ALPHA, coeffs, **kw)
    total.backward()
    g1 = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    total2, _ = net.training_loss(X, ALPHA, coeffs, **kw)
    (2 * total2).backward()
    with torch.no_grad():
        ev, per_ev = net.training_loss(X, ALPHA, coeffs, **kw)

    tot64, per64, g64 = objective64(case, kind, coeffs, float(B) if reduction == "mean" else 1.0)
    errs = {}
    for k, g in g64.items():
        if g is None:
            assert g1[k] is None, k                            # no cotangent reaches it
        else:
            errs[k] = nrel(g1[k], g)
    worst = max(errs, key=errs.get)
    print(f"{case[0]} {kind}: total {float(total.detach()):.8g} vs {float(tot64):.8g}; "
          f"worst gradient {worst} {errs[worst]:.3g}; {len(g64) - len(errs)} unreached")
    assert abs(float(total) - float(tot64)) <= 1e-5 * abs(float(tot64))
    assert nrel(per, per64) <= 1e-5
    for k, e in errs.items():
        assert e <= GTOL, (k, e)
    if coeffs[0] == 0.0:
        assert len(errs) < len(g64)                            # the last layer's L step
    for k, p in net.named_parameters():                        # the upstream gradient scales exactly
        assert (p.grad is None and g1[k] is None) or torch.equal(p.grad, 2 * g1[k]), k
    # evaluation (the sums-only form, the inference forward) gives the training forward's values
    assert abs(float(ev) - float(total)) <= 1e-6 * abs(float(total)) and nrel(per_ev, per) <= 1e-6
    # a retained graph backed through twice: the second backward forms the cotangents again
    net.zero_grad(set_to_none=True)
    total3, _ = net.training_loss(X, ALPHA, coeffs, **kw)
    total3.backward(retain_graph=True)
    total3.backward()
    for k, p in net.named_parameters():
        assert (p.grad is None and g1[k] is None) or nrel(p.grad, 2 * g1[k]) <= 1e-6, k
