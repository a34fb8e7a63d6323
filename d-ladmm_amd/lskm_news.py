"""The newS scripts' classic KM iteration and learned + safeguarded KM (LSKM): the test-script
model of test_syn_l1l1_newS.py:75-272, its `_Acols` form and the tied / partially tied `_Acols`
scripts (test_syn_scalar_tied_newS_Acols.py, test_syn_scalar_ptied_newS_Acols.py) as drop-ins.

Same constructor and `state_dict` as the reference classes (a `DLADMMNetNewS` checkpoint loads
unchanged), plus the settings the scripts read from module globals (alpha, delta, mu_k_method,
mu_k_param, num_iter) as keyword arguments.  `forward(x, use_learned, use_safeguard, continued,
K)` returns (Z, E, L) or, with learned + safeguard, (Z, E, L, sg_count) like the reference.

Differences from `lskm.DLADMMNetLSKM` (test_syn_l1l1_scalar.py), all in the reference:
  * the classic step is the V1 E-form with scalar constants and a step, E = S(X - A Z - ss2 L,
    ss2) with ss2 = 1 / beta (:131-164): kernel variant V7 (`_lib.V7_SCALAR_V1E`);
  * the loop carries the triple (E, L, Z) and each step runs E, L, then Z (:219-234): the
    `DLADMM_F_ELZ` entry of the fused kernels;
  * the safeguard norm is Snorm_ELZ (:167-185), formed without the n x n matrix P2 from the two
    products A Zn, A Znn a `DLADMM_F_ELZ_TAIL` step saves (`dladmm_safeguard_news_f32`).

Execution: pure KM of any K (the K = 1,000 ground truth) is ONE V7 launch, re-indexed as
`DLADMMNetNewS.forward` does; pure learned is the newS forward; `continued` runs its K - layers
KM steps as one ELZ launch from the last triple; a safeguarded layer is the KM candidate, the
L2O candidate, the KM step from the L2O candidate (with its tail product) and the select.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .model import (DLADMMNetNewS, DLADMMNetPTiedNewS, DLADMMNetTiedNewS, _scalar_table)
from .ops import ForwardResult, _PLAN_FLAGS, dladmm_forward

_UPDATERS = {"None": _lib.MU_NONE, "EMA": _lib.MU_EMA, "GS": _lib.MU_GS, "RT": _lib.MU_RT}
# slots of a table row that belong to the E / L half of a step (the rest: its Z half)
_E_SLOTS = [_lib.P_BETA2, _lib.P_BETA3, _lib.P_SS2, _lib.P_SS2B, _lib.P_THETA_E]


class _NewSLSKM:
    """The newS test class over any of the newS training models (mixin: first base)."""
    WSCALE = 1.0      # test_syn_l1l1_newS.py:118: m.weight = A.t() + 1e-3 * randn (no 0.4)
    THZ0 = 0.2        # :107-108
    THE0 = 0.8
    PREPEND_INIT = False

    @staticmethod
    def _check_updater(mu_k_method):
        if mu_k_method == "RM":
            raise NotImplementedError(
                "mu_k_method 'RM': the reference RMUpdater.step returns torch's (values, indices) "
                "pair (mu_updater.py:94), which test_syn_l1l1_newS.py:241 cannot multiply")
        if mu_k_method not in _UPDATERS:
            raise ValueError(f"unknown mu_k_method {mu_k_method!r}")

    def _init_lskm(self, alpha, delta, mu_k_method, mu_k_param, num_iter, prepend_init):
        # the reference's module globals (test_syn_l1l1_newS.py:39-46)
        self.alpha, self.delta = float(alpha), float(delta)
        self.mu_k_method, self.mu_k_param = mu_k_method, float(mu_k_param)
        self.num_iter = int(num_iter)
        self.prepend_init = self.PREPEND_INIT if prepend_init is None else bool(prepend_init)
        self.sg_mask = None

    # --- tables ----------------------------------------------------------------------------
    def _km_table(self, K: int) -> torch.Tensor:
        """KM_ZEL / KM_ELZ constants (:132-134): beta = 1, ss1 = 0.999 / L, ss2 = 1 / beta."""
        dev = self.A.device
        ss1 = (0.999 / self.L.to(dev)).reshape(())
        return _scalar_table(K, dev, b1=1.0, b2=1.0, b3=1.0, the=1.0, thz=ss1 * self.alpha,
                             s1=ss1)

    def _inv_bs(self) -> torch.Tensor:
        """1 / (beta ss1) as Snorm_ELZ forms it (:179: eye / beta / ss1), a device scalar."""
        dev = self.A.device
        return (torch.ones((), device=dev) / 1.0 / (0.999 / self.L.to(dev)).reshape(())) \
            .reshape(1).contiguous()

    def _elz_table(self, ptab: torch.Tensor) -> torch.Tensor:
        """Row k of an ELZ call = step k of :224-234: E / L slots of layer k - 1, Z slots of
        layer k (row 0 is never used: layer 0 is a Z-step only)."""
        t = ptab.clone()
        t[1:, _E_SLOTS] = ptab[:-1, _E_SLOTS]
        return t

    def _At(self) -> torch.Tensor:
        if getattr(self, "_At_c", None) is None or self._At_c.device != self.A.device:
            self._At_c = self.A.t().contiguous()
        return self._At_c

    # --- launches --------------------------------------------------------------------------
    def _zel(self, variant, x, Z, E, L, W, table, want_T=False):
        return dladmm_forward(variant, x, self.A, W, Z, E, L, keep_all=True, want_T=want_T,
                              scalar_params=table)

    def _elz(self, variant, x, Z, E, L, W, table, tail=False, want_T=False):
        """len(W) steps E, L, Z from the triple (DLADMM_F_ELZ); tail: also P[0 .. steps]."""
        m, B = x.shape
        steps, dev = len(W), x.device
        out = ForwardResult(torch.empty((steps, self.d, B), device=dev),
                            torch.empty((steps, m, B), device=dev),
                            torch.empty((steps, m, B), device=dev),
                            torch.empty((steps + 1, m, B), device=dev) if want_T else None, None)
        flags = _PLAN_FLAGS.get() | _lib.F_ELZ
        if tail:
            out.P = torch.empty((steps + 1, m, B), device=dev)
            flags |= _lib.F_ELZ_TAIL
        return dladmm_forward(variant, x, self.A, W, Z, E, L, keep_all=True, want_T=want_T,
                              scalar_params=table, out=out, flags=flags)

    def _km_steps(self, x, Z, E, L, K: int, table=None, **kw):
        return self._elz(_lib.V7_SCALAR_V1E, x, Z, E, L, [self._At()] * K,
                         self._km_table(K) if table is None else table, **kw)

    def _select(self, x, mu, inv_bs, cand_l, cand_k, res, out, k, count, mask, norm_out=None):
        """dladmm_safeguard_news_f32: Snorm_ELZ of the L2O candidate (from the KM step `res`
        taken from it), mu update, per-column select of (E, L, Z).  out None: mu = Snorm."""
        m, B = x.shape
        d = _lib.SafeguardNewsDesc()
        d.abi_version = _lib.ABI_VERSION
        d.m, d.n, d.batch, d.ld = m, self.d, B, B
        d.X = x.data_ptr()
        d.Zl = cand_l[0].data_ptr()
        d.En, d.Znn = res.E[0].data_ptr(), res.Z[0].data_ptr()
        d.Pn, d.Pnn = res.P[0].data_ptr(), res.P[1].data_ptr()
        d.mu, d.inv_bs = mu.data_ptr(), inv_bs.data_ptr()
        d.norm_out = norm_out.data_ptr() if norm_out is not None else None
        if out is not None:
            d.El, d.Ll = cand_l[1].data_ptr(), cand_l[2].data_ptr()
            d.Zk, d.Ek, d.Lk = (t.data_ptr() for t in cand_k)
            Zo, Eo, Lo = out
            d.Zo, d.Eo, d.Lo = Zo[k].data_ptr(), Eo[k].data_ptr(), Lo[k].data_ptr()
            d.count = count[k:k + 1].data_ptr()
            d.mask = mask[k].data_ptr()
        d.delta = self.delta
        d.updater, d.mu_param = _UPDATERS[self.mu_k_method], self.mu_k_param
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().dladmm_safeguard_news_f32(ctypes.byref(d), ctypes.c_void_p(stream)))

    # --- reference methods -----------------------------------------------------------------
    @staticmethod
    def two_norm(z, dim=0):
        return (z ** 2).sum(dim=dim).sqrt()

    def KM_ZEL(self, Zk, Ek, Lk, Tk, X, **kwargs):
        """One classic step in Z, E, L order (:131-146) with the default constants; returns
        (Varn, Zn, En, Tn, Ln).  Tk must be A Zk + Ek - X."""
        if kwargs:
            raise NotImplementedError("dladmm: KM_ZEL runs with the reference defaults only")
        with torch.no_grad():
            r = self._zel(_lib.V7_SCALAR_V1E, X, Zk, Ek, Lk, [self._At()], self._km_table(1),
                          want_T=True)
            Varn = Lk + 1.0 * Tk
        return Varn, r.Z[0], r.E[0], r.T[1], r.L[0]

    def KM_ELZ(self, Ek, Lk, Zn, X, **kwargs):
        """One classic step in E, L, Z order (:149-164); returns (En, Tn, Ln, Varnn, Znn)."""
        if kwargs:
            raise NotImplementedError("dladmm: KM_ELZ runs with the reference defaults only")
        with torch.no_grad():
            r = self._km_steps(X, Zn, Ek, Lk, 1, want_T=True)
            Varnn = r.L[0] + 1.0 * r.T[0]
        return r.E[0], r.T[0], r.L[0], Varnn, r.Z[0]

    def Snorm_ELZ(self, Ek, Lk, Zn, X, **kwargs):
        """The safeguard norm (:167-185), per column."""
        if kwargs:
            raise NotImplementedError("dladmm: Snorm_ELZ runs with the reference defaults only")
        with torch.no_grad():
            nrm = torch.empty(X.shape[1], device=X.device)
            mu = torch.empty_like(nrm)
            res = self._km_steps(X, Zn, Ek, Lk, 1, tail=True)
            self._select(X, mu, self._inv_bs(), (Zn, Ek, Lk), None, res, None, 0, None, None,
                         norm_out=nrm)
        return nrm

    # --- forward ---------------------------------------------------------------------------
    def _l2o_weights(self):
        return [w.detach() for w in self._weights()]

    def forward(self, x, use_learned=False, use_safeguard=False, continued=False,
                K: Optional[int] = None):
        """test_syn_l1l1_newS.py:188-268.  K defaults to the reference's
        `layers if (not continued and (use_learned or use_safeguard)) else num_iter` (:54)."""
        if K is None:
            K = self.layers if (not continued and (use_learned or use_safeguard)) else \
                self.num_iter
        K = int(K)
        if use_safeguard and not use_learned:
            raise AssertionError("safeguarding needs the learned model (:238 assert use_learned)")
        if use_learned and not continued and K > self.layers:
            raise IndexError(f"K={K} learned steps but the model has {self.layers} layers")
        if K < 1:
            raise ValueError("K must be at least 1")
        nl = min(K, self.layers) if use_learned else 0
        dev = x.device
        with torch.no_grad():
            if not use_learned:
                # K steps of KM_ZEL-then-KM_ELZ = the ZEL run of K layers, E / L one layer behind
                r = self._zel(_lib.V7_SCALAR_V1E, x, self.Z0, self.E0, self.L0,
                              [self._At()] * K, self._km_table(K))
                Z = [r.Z[k] for k in range(K)]
                E = [self.E0] + [r.E[k] for k in range(K - 1)]
                L = [self.L0] + [r.L[k] for k in range(K - 1)]
                return self._ret(Z, E, L, None)
            count = None
            if use_safeguard:
                Z, E, L, count = self._safeguarded(x, nl)
            else:
                Z, E, L = DLADMMNetNewS.forward(self, x, nl)
                Z, E, L = list(Z), list(E), list(L)
            if continued and K > nl:   # :201-203: KM from the learned model's last triple
                r2 = self._km_steps(x, Z[-1], E[-1], L[-1], K - nl)
                Z += list(r2.Z)
                E += list(r2.E)
                L += list(r2.L)
            return self._ret(Z, E, L, count)

    def _ret(self, Z, E, L, count):
        if self.prepend_init:   # the _Acols scripts: Z0 / E0 / L0 in front of the lists
            Z, E, L = [self.Z0] + Z, [self.E0] + E, [self.L0] + L
        if count is not None:
            return Z, E, L, count.cpu().numpy().astype(np.float64)
        return Z, E, L

    def _safeguarded(self, x, nl: int):
        m, B = x.shape
        dev = x.device
        Zo = torch.empty((nl, self.d, B), device=dev)
        Eo = torch.empty((nl, m, B), device=dev)
        Lo = torch.empty((nl, m, B), device=dev)
        count = torch.zeros(self.layers, dtype=torch.int32, device=dev)
        mask = torch.zeros((self.layers, B), dtype=torch.uint8, device=dev)
        mu = torch.empty(B, device=dev)
        # this call's tables and weights, assembled once (not per layer)
        km1 = self._km_table(1)
        inv_bs = self._inv_bs()
        ptab = self._tables(dev)["scalar_params"]
        etab = self._elz_table(ptab)
        W = self._l2o_weights()
        At = [self._At()]
        V7 = _lib.V7_SCALAR_V1E
        # mu_0 = Snorm_ELZ(E0, L0, Z0, X) (:196)
        res = self._elz(V7, x, self.Z0, self.E0, self.L0, At, km1, tail=True)
        self._select(x, mu, inv_bs, (self.Z0, self.E0, self.L0), None, res, None, 0, None, None)
        for k in range(nl):
            if k == 0:
                # :205-217: a Z-step only (T0 = A Z0 + E0 - X), E0 / L0 passed through
                zk = self._zel(V7, x, self.Z0, self.E0, self.L0, At, km1).Z[0]
                zl = self._zel(self.VARIANT, x, self.Z0, self.E0, self.L0, W[:1], ptab[:1]).Z[0]
                ck, cl = (zk, self.E0, self.L0), (zl, self.E0, self.L0)
            else:
                Zc, Ec, Lc = Zo[k - 1], Eo[k - 1], Lo[k - 1]
                rk = self._elz(V7, x, Zc, Ec, Lc, At, km1)                        # :222
                rl = self._elz(self.VARIANT, x, Zc, Ec, Lc, W[k:k + 1], etab[k:k + 1])  # :226-234
                ck, cl = (rk.Z[0], rk.E[0], rk.L[0]), (rl.Z[0], rl.E[0], rl.L[0])
            res = self._elz(V7, x, cl[0], cl[1], cl[2], At, km1, tail=True)       # :239
            self._select(x, mu, inv_bs, cl, ck, res, (Zo, Eo, Lo), k, count, mask)
        self.sg_mask = mask
        return list(Zo), list(Eo), list(Lo), count


class DLADMMNetNewSLSKM(_NewSLSKM, DLADMMNetNewS):
    """test_syn_l1l1_newS.py:75-272; `prepend_init=True` gives test_syn_l1l1_newS_Acols.py's
    return lists (Z0 / E0 / L0 inserted in front)."""
    NAME = "DLADMMNet"

    def __init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, *, alpha: float = 0.01,
                 delta: float = -99.0, mu_k_method: str = "None", mu_k_param: float = 0.0,
                 num_iter: int = 200, prepend_init: Optional[bool] = None):
        self._check_updater(mu_k_method)
        DLADMMNetNewS.__init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers)
        self._init_lskm(alpha, delta, mu_k_method, mu_k_param, num_iter, prepend_init)


class DLADMMNetTiedNewSLSKM(_NewSLSKM, DLADMMNetTiedNewS):
    """test_syn_scalar_tied_newS_Acols.py: one shared fc scaled by ss1[k] in the L2O Z-step."""
    NAME = "DLADMMNet"
    PREPEND_INIT = True

    def __init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, *, alpha: float = 0.01,
                 delta: float = -99.0, mu_k_method: str = "None", mu_k_param: float = 0.0,
                 num_iter: int = 200, prepend_init: Optional[bool] = None):
        self._check_updater(mu_k_method)
        DLADMMNetTiedNewS.__init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers)
        self._init_lskm(alpha, delta, mu_k_method, mu_k_param, num_iter, prepend_init)


class DLADMMNetPTiedNewSLSKM(_NewSLSKM, DLADMMNetPTiedNewS):
    """test_syn_scalar_ptied_newS_Acols.py: layer k uses ss1[k] * fc[k // interval]."""
    PREPEND_INIT = True

    def __init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, interval, *,
                 alpha: float = 0.01, delta: float = -99.0, mu_k_method: str = "None",
                 mu_k_param: float = 0.0, num_iter: int = 200,
                 prepend_init: Optional[bool] = None):
        self._check_updater(mu_k_method)
        DLADMMNetPTiedNewS.__init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, interval)
        self._init_lskm(alpha, delta, mu_k_method, mu_k_param, num_iter, prepend_init)
