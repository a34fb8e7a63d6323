"""numpy restatement of the newS test class's forward (test_syn_l1l1_newS.py:75-272, its _Acols
form and the tied / ptied _Acols scripts), in fp64 by default: the checker of the newS LSKM tests
where no fixture reaches (K = 1,000 depth, many columns).  Pinned to the fixtures the reference
class itself produced (tests/test_news_lskm_cpu.py).  Test code: not product code, not an oracle
module.

`forward(...)` returns a dict: Z, E, L (lists, without the _Acols scripts' prepended initial
triple), sg_count, keep [layers][B] (bool), snorm [layers + 1][B] (entry 0 = mu_0) and margin
[layers][B] = |Snorm - (1 - delta) mu| / ((1 - delta) mu) of every decision.
"""
from __future__ import annotations

import numpy as np


def shrink(x, th):
    return np.maximum(x - th, 0.0) - np.maximum(-x - th, 0.0)


class Updater:
    """mu_updater.py:18-116 (EMA / GS / RT / None)."""

    def __init__(self, method, mu, param):
        self.method, self.mu, self.param = method, mu, param

    def step(self, s, keep):
        if self.method == "None":
            self.mu = np.full_like(s, 1e10)
            return self.mu
        upd = {"EMA": self.param * s + (1 - self.param) * self.mu,
               "GS": (1 - self.param) * self.mu, "RT": s}[self.method]
        self.mu = np.where(keep, upd, self.mu)
        return self.mu


def forward(X, A, Z0, E0, L0, sd, layers, use_learned, use_safeguard, continued, K, alpha,
            delta=-99.0, mu_method="None", mu_param=0.0, fc="per_layer", interval=1,
            dtype=np.float64):
    c = lambda a: np.asarray(a, dtype)  # noqa: E731
    X, A, Z0, E0, L0 = c(X), c(A), c(Z0), c(E0), c(L0)
    A32 = np.asarray(A, np.float32)
    Lip = dtype(np.float32(np.linalg.norm(A32.T @ A32, ord=2)))   # self.L is stored in fp32
    beta = dtype(1.0)
    ss1 = dtype(0.999) / Lip
    ss2 = dtype(1.0) / beta
    p = lambda nm, k: dtype(np.asarray(sd[f"{nm}.{k}"]).reshape(()))  # noqa: E731

    def W(k):
        if fc == "tied":
            return p("ss1", k) * c(sd["fc.weight"])
        if fc == "ptied":
            return p("ss1", k) * c(sd[f"fc.{k // interval}.weight"])
        return c(sd[f"fc.{k}.weight"])

    def km_elz(Ek, Lk, Zn):
        En = shrink(X - A @ Zn - ss2 * Lk, ss2)
        Tn = A @ Zn + En - X
        Ln = Lk + beta * Tn
        Znn = shrink(Zn - ss1 * (A.T @ (Ln + beta * Tn)), ss1 * dtype(alpha))
        return En, Ln, Znn

    def snorm(Ek, Lk, Zn):
        En, _Ln, Znn = km_elz(Ek, Lk, Zn)
        r1 = ((A @ Znn + En - X) ** 2).sum(0)
        d = Znn - Zn
        Ad = A @ d
        return np.sqrt(r1 + (d * d).sum(0) / (beta * ss1) - (Ad * Ad).sum(0))

    Z, E, L = [], [], []
    sg = use_learned and use_safeguard
    out = dict(sg_count=np.zeros(layers), keep=[], snorm=[], margin=[])
    if sg:
        mu = snorm(E0, L0, Z0)
        out["snorm"].append(mu)
        upd = Updater(mu_method, mu, dtype(mu_param))
    for k in range(K):
        if continued and k == layers:
            use_learned = use_safeguard = False
        if k == 0:
            T0 = A @ Z0 + E0 - X
            Ek, Lk = E0, L0
            Zk = shrink(Z0 - ss1 * (A.T @ (L0 + beta * T0)), ss1 * dtype(alpha))
            if use_learned:
                El, Ll = E0, L0
                Zl = shrink(Z0 - W(0) @ (L0 + p("beta1", 0) * T0), p("active_para", 0))
        else:
            Ek, Lk, Zk = km_elz(E[-1], L[-1], Z[-1])
            if use_learned:
                P = A @ Z[-1]
                VVar = L[-1] + p("beta2", k - 1) * (P + E[-1] - X)
                El = shrink(E[-1] - p("ss2", k - 1) * VVar, p("active_para1", k - 1))
                Tl = P + El - X
                Ll = L[-1] + p("beta3", k - 1) * Tl
                Zl = shrink(Z[-1] - W(k) @ (Ll + p("beta1", k) * Tl), p("active_para", k))
        if use_safeguard:
            s = snorm(El, Ll, Zl)
            thr = (dtype(1.0) - dtype(delta)) * mu
            keep = s < thr
            out["snorm"].append(s)
            out["margin"].append(np.abs(s - thr) / thr)
            out["keep"].append(keep)
            mu = upd.step(s, keep)
            E.append(np.where(keep, El, Ek))
            L.append(np.where(keep, Ll, Lk))
            Z.append(np.where(keep, Zl, Zk))
            out["sg_count"][k] = float((~keep).sum())
        elif use_learned:
            E.append(El); L.append(Ll); Z.append(Zl)  # noqa: E702
        else:
            E.append(Ek); L.append(Lk); Z.append(Zk)  # noqa: E702
    out.update(Z=Z, E=E, L=L)
    return out
