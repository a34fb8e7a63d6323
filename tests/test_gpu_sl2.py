"""The fused S-L2 training term (ops.dladmm_sl2 -> dladmm_sl2_f32, csrc/dladmm_sl2.hip) and
training_loss(kind="sl2") against a torch fp64 restatement of main_syn_l1l1-sl2_scalar.py's KM
(:117-143), S (:146-157) and loss lines (:255-278), differentiated by autograd.  The V3 script
(main_syn_l1l1-sl2_full.py) has the same lines on (m, 1) / (d, 1) parameters.

Bars: per-column sums within 1e-5 relative (the bar of tests/test_gpu_lena.py's losses); every
cotangent and parameter gradient within GTOL = 1e-4 norm-relative (tests/test_gpu_backward.py:
GEMM summation order moves fp32 gradients by more than rounding).  The op is compared at the GPU
forward's own outputs, where the KM step's shrink arguments must stay clear of their thresholds
(asserted on the fp64 side, no element excluded).
"""
import functools
import math

import numpy as np
import pytest
import torch

GTOL = 1e-4
ALPHA = 0.001  # the scripts' alpha
SS2 = float(np.float32(0.3))
C = float(np.float32(math.sqrt(0.3 / 0.7)))

#        id             model               m    n    K  B   seed
CASES = [("v4_script", "DLADMMNetScalarSl2", 250, 500, 3, 20, 11),  # padded rows, 4-column group
         ("v3_script", "DLADMMNetFull", 250, 500, 3, 20, 12),       # the per-row model
         ("v4_tiny", "DLADMMNetScalar", 16, 32, 2, 5, 13),          # heavy padding
         ("v4_K1", "DLADMMNetScalarZ0", 250, 500, 1, 20, 14),       # Ep = E0, NULL gEp
         ("v4_ld", "DLADMMNetScalar", 100, 120, 3, 8, 15)]          # leading dimensions
IDS = [c[0] for c in CASES]


def nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    nb = float(b.norm())
    return float((a - b).norm()) / nb if nb > 0 else float(a.norm())


@functools.lru_cache(maxsize=None)
def problem(case):
    """gen_syn_data.py's distribution, the scripts' Z0 / E0 / L0, and the scripts' parameters
    perturbed by 10 % with 0.4 * (A^T + 1e-3 N) weights; fp32 CPU tensors, never modified."""
    _, _, m, n, K, B, seed = case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    A = rn(m, n)
    A = A / A.pow(2).sum(0, keepdim=True).sqrt()
    zs = (torch.rand(n, B, generator=g) < 0.1) * rn(n, B)
    es = (torch.rand(m, B, generator=g) < 0.1) * rn(m, B)
    inp = dict(A=A.float(), X=(A @ zs + es).float(),
               Z0=(torch.rand(n, B, generator=g) / n).float(),
               E0=torch.zeros(m, B), L0=torch.zeros(m, B))
    v3 = case[1] == "DLADMMNetFull"
    sd = {}
    for k in range(K):
        for nm, val in (("beta1", 1.0), ("beta2", 1.0), ("beta3", 1.0), ("ss2", 1.0),
                        ("active_para", 0.2), ("active_para1", 0.8)):
            rows = (n if nm == "active_para" else m) if v3 else 1
            sd[f"{nm}.{k}"] = (val * (1.0 + 0.1 * rn(rows, 1))).float()
        sd[f"fc.{k}.weight"] = (0.4 * (inp["A"].t() + 1e-3 * rn(n, m))).float().contiguous()
    return inp, sd


def make_net(dl, case):
    _, cls, m, n, K, B, _ = case
    inp, sd = problem(case)
    net = getattr(dl, cls)(m=m, n=0, d=n, batch_size=B, A=inp["A"], Z0=inp["Z0"], E0=inp["E0"],
                           L0=inp["L0"], layers=K)
    net.load_state_dict(sd, strict=True)
    return net.cuda(), inp, sd


# ---- the restatement (fp64) -------------------------------------------------------------------
def shrink(x, th):
    return torch.relu(x - th) - torch.relu(-1.0 * x - th)


def forward64(p, X, A, Z0, E0, L0, K):                      # DLADMMNet.forward, :63-110
    Z, E, L, T = [Z0], [E0], [L0], [A @ Z0 + E0 - X]
    for k in range(K):
        Var = L[-1] + p[f"beta1.{k}"] * T[-1]
        Zk = shrink(Z[-1] - p[f"fc.{k}.weight"] @ Var, p[f"active_para.{k}"])
        VVar = L[-1] + p[f"beta2.{k}"] * (A @ Zk + E[-1] - X)
        Ek = shrink(E[-1] - p[f"ss2.{k}"] * VVar, p[f"active_para1.{k}"])
        Tk = A @ Zk + Ek - X
        Z.append(Zk), E.append(Ek), L.append(L[-1] + p[f"beta3.{k}"] * Tk), T.append(Tk)
    return Z[1:], E[1:], L[1:], T                           # T[0 .. K]


def s_colsum(A, ss1, Z, E, L, T, X, Ep):
    """squared_two_norm(S(Z, E, L, T, X, Ep)) per column (:117-161, beta = 1), and the two
    shrink arguments' distances to their thresholds."""
    thz = float(torch.tensor(ss1, dtype=torch.float32) * ALPHA)  # fp32 tensor * scalar, :129
    U = Z - ss1 * (A.t() @ (L + 1.0 * T))
    Zn = shrink(U, thz)
    TTn = A @ Zn + E - X
    V = E - SS2 * (L + 1.0 * TTn)
    En = shrink(V, SS2)
    Tn = A @ Zn + En - X
    Sn = torch.cat([1.0 * Tn, C * (En - 2 * E + Ep)])
    with torch.no_grad():
        margin = min(float(((U.abs() - thz).abs() / thz).min()),
                     float(((V.abs() - SS2).abs() / SS2).min()))
    return (Sn ** 2).sum(0), margin


def ss1_of(A32):                                            # 0.5 / self.L, :31 and :119
    a = A32.numpy()
    return float(np.float32(0.5) / np.float32(np.linalg.norm(np.matmul(a.transpose(), a), ord=2)))


def objective64(case, coeffs, lam):
    """total, per-layer losses and parameter gradients of the scripts' loop (:255-280), fp64."""
    K = case[4]
    inp, sd = problem(case)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    X, A, Z0, E0, L0 = (inp[k].double() for k in ("X", "A", "Z0", "E0", "L0"))
    Z, E, L, T = forward64(p, X, A, Z0, E0, L0, K)
    per = [ALPHA * Z[k].abs().sum(0).mean() + (X - A @ Z[k]).abs().sum(0).mean() for k in range(K)]
    Ep = E[K - 2] if K > 1 else E0
    per[K - 1] = per[K - 1] + lam * s_colsum(A, ss1_of(inp["A"]), Z[K - 1], E[K - 1], L[K - 1],
                                             T[K], X, Ep)[0].mean()
    total = sum(c * v for c, v in zip(coeffs, per))
    total.backward()
    return total.detach(), torch.stack(per).detach(), {k: v.grad for k, v in p.items()}


# ---- the op at the GPU forward's own outputs ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sl2_op_vs_fp64_autograd(dl, case):
    K = case[4]
    net, inp, _ = make_net(dl, case)
    X = inp["X"].cuda()
    with torch.no_grad():
        r = net._run_shard(X, None, want_T=True)   # run() keeps no T for V3
    Ep = r.E[K - 2] if K > 1 else net.E0
    state = (r.Z[K - 1], r.E[K - 1], r.L[K - 1], r.T[K])
    kw = dict(alpha=ALPHA, **net._sl2_consts())
    w = torch.tensor([0.37], device="cuda")
    run = lambda **o: dl.ops.dladmm_sl2(X, net.A, *state, Ep, **kw, **o)  # noqa: E731
    s0 = run()
    out = run(coef=w, want_gEp=K > 1)
    again = run(coef=w, want_gEp=K > 1)

    A64, ss1 = inp["A"].double(), ss1_of(inp["A"])
    assert kw["ss1"] == ss1 and kw["beta"] == 1.0 and float(np.float32(kw["ss2"])) == SS2
    leaves = [t.double().cpu().requires_grad_(K > 1 or i < 4)
              for i, t in enumerate(state + (Ep,))]
    ref, margin = s_colsum(A64, ss1, *leaves[:4], inp["X"].double(), leaves[4])
    (0.37 * ref.sum()).backward()
    # a condition on the inputs: no shrink argument of the KM step sits on its threshold
    assert margin > 1e-6, margin

    sums = out[0].cpu()
    err = float(((sums - ref.detach()).abs() / ref.detach()).max())
    gerr = {nm: nrel(g, leaf.grad) for nm, g, leaf in zip("ZELTP", out[1:], leaves)
            if g is not None}
    print(f"{case[0]}: margin {margin:.3g} colsum {err:.3g} cotangents {gerr}")
    assert err <= 1e-5
    assert (K > 1) == (out[5] is not None) and len(gerr) == (5 if K > 1 else 4)
    assert all(float(leaf.grad.abs().max()) > 0 for leaf in leaves[:4])
    for nm, e in gerr.items():
        assert e <= GTOL, (nm, e)
    assert torch.equal(s0, out[0])                     # mode 0 == mode 1
    for a, b in zip(out, again):                       # deterministic
        assert (a is None and b is None) or torch.equal(a, b)


# ---- the whole path -----------------------------------------------------------------------------
WHOLE = [(c, 1e-4, None) for c in CASES] + [(CASES[0], 1.0, "last")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,lam,coef", WHOLE, ids=IDS + ["v4_script_lam1"])
def test_sl2_training_loss_vs_fp64_autograd(dl, case, lam, coef):
    """lam = 1 with coeffs [0, ..., 0, 1]: the term's gradient alone beside the last layer's
    L1L1 one, so a wrong adjoint cannot hide under the bar."""
    K = case[4]
    coeffs = [0.0] * (K - 1) + [1.0] if coef == "last" else [0.6] * (K - 1) + [1.0]
    net, inp, _ = make_net(dl, case)
    net.requires_grad_(True)
    X = inp["X"].cuda()
    total, per = net.training_loss(X, ALPHA, coeffs, kind="sl2", lam=lam)
    total.backward()
    g1 = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    total2, _ = net.training_loss(X, ALPHA, coeffs, kind="sl2", lam=lam)
    (2 * total2).backward()
    with torch.no_grad():
        ev, per_ev = net.training_loss(X, ALPHA, coeffs, kind="sl2", lam=lam)

    tot64, per64, g64 = objective64(case, tuple(coeffs), lam)
    errs = {k: nrel(g1[k], g) for k, g in g64.items() if g is not None and bool(g.any())}
    worst = max(errs, key=errs.get)
    print(f"{case[0]} lam {lam}: total {float(total.detach()):.8g} vs {float(tot64):.8g}; "
          f"worst gradient {worst} {errs[worst]:.3g}")
    assert abs(float(total) - float(tot64)) <= 1e-5 * abs(float(tot64))
    assert nrel(per, per64) <= 1e-5
    assert len(errs) == len(g1) == 7 * K               # every parameter of every layer
    for k, e in errs.items():
        assert e <= GTOL, (k, e)
    for k, p in net.named_parameters():                # the upstream gradient scales exactly
        assert torch.equal(p.grad, 2 * g1[k]), k
    # evaluation (mode 0, the inference forward) gives the training forward's values
    assert abs(float(ev) - float(total)) <= 1e-6 * abs(float(total)) and nrel(per_ev, per) <= 1e-6


@pytest.mark.gpu
def test_sl2_column_shards_sum_to_the_batch(dl):
    """cols= / batch= as for l1l1: two shards' totals and gradients add up to the whole batch's."""
    case = CASES[4]
    net, inp, _ = make_net(dl, case)
    net.requires_grad_(True)
    X = inp["X"].cuda()
    B = X.shape[1]
    net.training_loss(X, ALPHA, kind="sl2", lam=1.0)[0].backward()
    whole = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    for c0, c1 in ((0, 3), (3, B)):
        net.training_loss(X[:, c0:c1].contiguous(), ALPHA, kind="sl2", lam=1.0, cols=(c0, c1),
                          batch=B)[0].backward()
    for k, p in net.named_parameters():
        assert nrel(p.grad, whole[k]) <= GTOL, k
