"""Classic KM iteration and learned + safeguarded KM (LSKM) for the per-row models: the test-script
classes of test_syn_l1l1_ltheta.py:65-248 (V2), test_syn_gt_ltheta.py:43-212 (V2, other classic
constants) and test_syn_l1l1_full.py:68-296 (V3) as drop-ins.

Each class has its parent's constructor, ParameterLists and `state_dict` (V2: per-row beta1, beta2,
active_para, active_para1; V3: also beta3 and ss2), the scripts' weight init A.t() + 1e-3 randn,
and the settings the scripts read from module globals (alpha, delta, mu_k_method, mu_k_param,
num_iter) as keyword arguments.  `forward(x, use_learned, use_safeguard, K)` returns (Z, E, L, T)
or, with learned + safeguard, (Z, E, L, T, sg_count) like the scripts.

The classes differ in the constants of the classic step KM() and of the residual S() =
[beta Tn ; c (En - 2 Ek + Ep)], each formed in fp32 exactly as its script forms it:

    class        beta       ss1        ss2 = theta_e   c
    ltheta       1          0.999 / L  0.999           sqrt(0.999 / (1 - 0.999))
    gt_ltheta    1/sqrt(L)  1/sqrt(L)  0.5             sqrt(c1 / (1 - c1)), c1 = beta 0.5
    full         1          0.5 / L    0.3             sqrt(0.3 / 0.7)

with L = ||A^T A||_2 and theta_z = ss1 alpha.  Every step runs on the HIP kernels:
  * a pure KM run of K iterations is ONE fused V5 launch on the shared A^T;
  * the learned forward is the parent's (V2 / V3, per-row table);
  * learned + safeguard at the 256 x 512 register shape can run as ONE kernel launch,
    `dladmm_lskm_rowp_f32` (csrc/dladmm_lskm_rowp_fused.hip; `fused_safeguard`); elsewhere, or
    with fused_safeguard=False, each layer runs a one-layer V2 / V3 forward, two one-step KM
    launches and `dladmm_safeguard_f32` with the class's beta and c.
"""
from __future__ import annotations

import ctypes
from math import sqrt
from typing import Optional

import numpy as np
import torch

from . import _lib
from .lskm import _UPDATERS
from .model import DLADMMNetFull, DLADMMNetLTheta, _dev, _scalar_table
from .ops import _f32_dev, _workspace, dladmm_forward


class _RowpLSKM:
    """The three scripts' shared body; the classes below supply the parent model and _consts()."""
    WSCALE = 1.0   # m.weight = A.t() + 1e-3 * randn (test_syn_l1l1_ltheta.py:104), no 0.4
    NAME = "DLADMMNet"
    # fused_safeguard=None takes the one-launch kernel where it exists: it beat the multi-launch
    # path by more than that path's spread at both batches for V2 and V3
    FUSED_DEFAULT = True

    def __init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, *, alpha: float = 0.01,
                 delta: float = -99.0, mu_k_method: str = "None", mu_k_param: float = 0.0,
                 num_iter: int = 200, fused_safeguard: Optional[bool] = None):
        super().__init__(m, n, d, batch_size, A, Z0, E0, L0, layers)
        self.At = self.A.t()
        self.A_np = A.detach().cpu().numpy()
        self.L = _dev((np.linalg.norm(np.matmul(self.A_np.transpose(), self.A_np), ord=2)
                       * torch.ones(1, 1)).float())
        # the learned + safeguarded loop as one launch (dladmm_lskm_rowp_f32): True requires it,
        # False keeps the per-layer launches, None follows FUSED_DEFAULT
        self.fused_safeguard = fused_safeguard
        if mu_k_method == "RM":
            raise NotImplementedError(
                "mu_k_method 'RM': the reference RMUpdater.step returns torch's (values, indices) "
                "pair (mu_updater.py:94), which test_syn_l1l1_ltheta.py:212 cannot multiply")
        if mu_k_method not in _UPDATERS:
            raise ValueError(f"unknown mu_k_method {mu_k_method!r}")
        self.alpha, self.delta = float(alpha), float(delta)
        self.mu_k_method, self.mu_k_param = mu_k_method, float(mu_k_param)
        self.num_iter = int(num_iter)

    def _consts(self, dev):
        """(beta, ss1, ss2, c): beta / ss1 fp32 0-dim tensors or floats, ss2 and c floats."""
        raise NotImplementedError  # pragma: no cover - per class

    def _km_table(self, K: int) -> torch.Tensor:
        dev = self.A.device
        beta, ss1, ss2, _ = self._consts(dev)
        thz = ss1 * self.alpha                                      # fp32 ss1 * alpha
        return _scalar_table(K, dev, b1=beta, b2=beta, b3=beta, ss2=ss2, the=ss2, thz=thz, s1=ss1)

    def _beta_c(self):
        beta, _, _, c = self._consts(self.A.device)
        return (float(beta), float(c))

    def _At(self) -> torch.Tensor:
        if getattr(self, "_At_c", None) is None or self._At_c.device != self.A.device:
            self._At_c = self.A.t().contiguous()
        return self._At_c

    def _km(self, x, Z, E, L, K: int, table: Optional[torch.Tensor] = None):
        """K classic iterations from (Z, E, L) as one fused launch; T_0 = A Z + E - X."""
        return dladmm_forward(_lib.V5_TIED, x, self.A, [self._At()] * K, Z, E, L, keep_all=True,
                              want_T=True,
                              scalar_params=self._km_table(K) if table is None else table)

    def _l2o(self, x, Z, E, L, k: int, nl: int, rtab: torch.Tensor):
        """Learned layers k .. k+nl-1 (the parent's V2 / V3 body) from (Z, E, L)."""
        return dladmm_forward(self.VARIANT, x, self.A,
                              [self.fc[j].weight.detach() for j in range(k, k + nl)], Z, E, L,
                              keep_all=True, want_T=True,
                              row_params=rtab[k:k + nl].contiguous())

    # --- reference methods -----------------------------------------------------------------
    def KM(self, Zk, Ek, Lk, Tk, X, **kwargs):
        """One classic step with the script's constants; returns (Varn, Zn, En, Tn, Ln).  Tk must
        be A Zk + Ek - X (as everywhere in the scripts)."""
        if kwargs:
            raise NotImplementedError("dladmm: KM runs with the script's constants only")
        with torch.no_grad():
            r = self._km(X, Zk, Ek, Lk, 1)
            Varn = Lk + self._consts(self.A.device)[0] * Tk
        return Varn, r.Z[0], r.E[0], r.T[1], r.L[0]

    def S(self, Zk, Ek, Lk, Tk, X, Ep, **kwargs):
        """Fixed-point residual [beta Tn ; c (En - 2 Ek + Ep)] of a classic step."""
        _, Zn, En, Tn, Ln = self.KM(Zk, Ek, Lk, Tk, X, **kwargs)
        beta, _, _, c = self._consts(self.A.device)
        return torch.cat([beta * Tn, c * (En - 2 * Ek + Ep)])

    @staticmethod
    def two_norm(z, dim=0):
        return (z ** 2).sum(dim=dim).sqrt()

    def _safeguard(self, x, mu, cand_l, cand_k, s_step, Ep, out, k_out, count, bc):
        """dladmm_safeguard_f32: |S| of the L2O candidate, mu update, per-column select."""
        m, B = x.shape
        d = _lib.SafeguardDesc()
        d.abi_version = _lib.ABI_VERSION
        d.m, d.n, d.batch, d.ld = m, self.d, B, B
        d.Es, d.Ts, d.Ep, d.mu = s_step.E[0].data_ptr(), s_step.T[1].data_ptr(), Ep.data_ptr(), \
            mu.data_ptr()
        if out is None:   # mu_0 = |S(Z0, E0, L0, T0, X, E0)|
            d.El = Ep.data_ptr()
        else:
            d.Zl, d.El, d.Ll, d.Tl = (cand_l.Z[0].data_ptr(), cand_l.E[0].data_ptr(),
                                      cand_l.L[0].data_ptr(), cand_l.T[1].data_ptr())
            d.Zk, d.Ek, d.Lk, d.Tk = (cand_k.Z[0].data_ptr(), cand_k.E[0].data_ptr(),
                                      cand_k.L[0].data_ptr(), cand_k.T[1].data_ptr())
            Zo, Eo, Lo, To = out
            d.Zo, d.Eo, d.Lo = Zo[k_out].data_ptr(), Eo[k_out].data_ptr(), Lo[k_out].data_ptr()
            d.To = To[k_out + 1].data_ptr()
            d.count = count.data_ptr()
        d.beta, d.c = bc
        d.delta = self.delta
        d.updater, d.mu_param = _UPDATERS[self.mu_k_method], self.mu_k_param
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().dladmm_safeguard_f32(ctypes.byref(d), ctypes.c_void_p(stream)))

    def _fused_shape(self) -> bool:
        """The 256 x 512 register shape dladmm_lskm_rowp_f32 is built for (smaller problems run
        in it through zero padding)."""
        m, n = self.A.shape
        return m <= 256 and n <= 512

    def _lskm_fused(self, x, nl: int, rtab, km, bc, Zo, Eo, Lo, To, count):
        """dladmm_lskm_rowp_f32: layers 0 .. nl-1 of the safeguarded loop, one kernel launch."""
        Lb = _lib.lib()
        dev = x.device
        X, A = _f32_dev(x, "X"), _f32_dev(self.A, "A")
        Z0, E0, L0 = _f32_dev(self.Z0, "Z0"), _f32_dev(self.E0, "E0"), _f32_dev(self.L0, "L0")
        m, B = X.shape
        n = A.shape[1]
        Ws = [_f32_dev(self.fc[k].weight.detach().contiguous(), f"W[{k}]") for k in range(nl)]
        rtab = rtab[:nl].contiguous()
        warr = _lib.ptr_array([w.data_ptr() for w in Ws])
        d = _lib.LskmRowpDesc()
        d.abi_version = _lib.ABI_VERSION
        d.m, d.n, d.batch, d.layers, d.emode = m, n, B, nl, self.VARIANT
        d.X, d.ld_x = X.data_ptr(), X.stride(0)
        d.A, d.ld_a = A.data_ptr(), A.stride(0)
        d.Z0, d.ld_z0 = Z0.data_ptr(), Z0.stride(0)
        d.E0, d.ld_e0 = E0.data_ptr(), E0.stride(0)
        d.L0, d.ld_l0 = L0.data_ptr(), L0.stride(0)
        d.W, d.ld_w = ctypes.cast(warr, ctypes.POINTER(ctypes.c_void_p)), m
        d.row_params, d.row_stride = rtab.data_ptr(), rtab.shape[2]
        d.km_params = km.data_ptr()
        d.beta, d.c = bc
        d.delta = self.delta
        d.updater, d.mu_param = _UPDATERS[self.mu_k_method], self.mu_k_param
        d.Z, d.E, d.L, d.T, d.ld_out = Zo.data_ptr(), Eo.data_ptr(), Lo.data_ptr(), \
            To.data_ptr(), B
        d.count = count.data_ptr()
        wsb = Lb.dladmm_lskm_rowp_workspace_bytes(ctypes.byref(d))
        ws = _workspace(dev, max(wsb, 1))
        d.workspace, d.workspace_bytes = ws.data_ptr(), wsb
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(Lb.dladmm_lskm_rowp_f32(ctypes.byref(d), ctypes.c_void_p(stream)))

    def forward(self, x, use_learned=True, use_safeguard=True, K: Optional[int] = None,
                fused_safeguard: Optional[bool] = None):
        """The scripts' forward (test_syn_l1l1_ltheta.py:160-244), under no_grad.  K defaults to
        their `layers if use_learned or use_safeguard else num_iter`.  fused_safeguard overrides
        the constructor's setting for this call."""
        fused = self.fused_safeguard if fused_safeguard is None else fused_safeguard
        if fused and not self._fused_shape():
            raise ValueError(
                f"dladmm: fused_safeguard=True needs the 256 x 512 register shape (m <= 256, "
                f"n <= 512), got m={self.A.shape[0]}, n={self.A.shape[1]}")
        if K is None:
            K = self.layers if (use_learned or use_safeguard) else self.num_iter
        if use_safeguard and not use_learned:
            raise AssertionError("safeguarding needs the learned model (assert use_learned)")
        if use_learned and K > self.layers:
            raise IndexError(f"K={K} learned steps but the model has {self.layers} layers")
        _f32_dev(x, "X")
        if x.dim() != 2 or x.shape[0] != self.A.shape[0] or x.shape[1] != self.Z0.shape[1]:
            raise ValueError(f"dladmm: X of shape {tuple(x.shape)} does not match A "
                             f"{tuple(self.A.shape)} and Z0 {tuple(self.Z0.shape)}")
        with torch.no_grad():
            if not use_learned:
                r = self._km(x, self.Z0, self.E0, self.L0, K)
                return list(r.Z), list(r.E), list(r.L), list(r.T)
            m, B = x.shape
            dev = x.device
            rtab = self._tables(dev)["row_params"]     # assembled once per call
            if not use_safeguard:
                r = self._l2o(x, self.Z0, self.E0, self.L0, 0, K, rtab)
                return list(r.Z), list(r.E), list(r.L), list(r.T)
            Zo = torch.empty((K, self.d, B), device=dev)
            Eo = torch.empty((K, m, B), device=dev)
            Lo = torch.empty((K, m, B), device=dev)
            To = torch.empty((K + 1, m, B), device=dev)
            count = torch.zeros(self.layers, dtype=torch.int32, device=dev)
            if fused is None:
                fused = self.FUSED_DEFAULT and self._fused_shape()
            # the classic step's table and the norm's (beta, c): once per call
            km1, bc = self._km_table(1), self._beta_c()
            if fused and K > 0 and B > 0:
                self._lskm_fused(x, K, rtab, km1, bc, Zo, Eo, Lo, To, count)
            else:
                mu = torch.empty(B, device=dev)
                # mu_0 = |S(Z0, E0, L0, T0, X, E0)|; T0 = A Z0 + E0 - X
                s0 = self._km(x, self.Z0, self.E0, self.L0, 1, km1)
                To[0].copy_(s0.T[0])
                self._safeguard(x, mu, None, None, s0, self.E0, None, 0, None, bc)
                Zc, Ec, Lc = self.Z0, self.E0, self.L0
                for k in range(K):
                    cl = self._l2o(x, Zc, Ec, Lc, k, 1, rtab)              # the L2O candidate
                    ck = self._km(x, Zc, Ec, Lc, 1, km1)                   # the classic one
                    cs = self._km(x, cl.Z[0], cl.E[0], cl.L[0], 1, km1)    # S(L2O, Ep)
                    self._safeguard(x, mu, cl, ck, cs, Ec, (Zo, Eo, Lo, To), k, count[k:k + 1],
                                    bc)
                    Zc, Ec, Lc = Zo[k], Eo[k], Lo[k]
            return (list(Zo), list(Eo), list(Lo), list(To),
                    count.cpu().numpy().astype(np.float64))


class DLADMMNetLThetaLSKM(_RowpLSKM, DLADMMNetLTheta):
    """test_syn_l1l1_ltheta.py:65-248: beta = 1, ss1 = 0.999 / L, ss2 = 0.999 (:146-149)."""

    def _consts(self, dev):
        return 1.0, (0.999 / self.L.to(dev)).reshape(()), 0.999, sqrt(0.999 / (1 - 0.999))


class DLADMMNetGtLThetaLSKM(DLADMMNetLThetaLSKM):
    """test_syn_gt_ltheta.py:43-212: beta = ss1 = 1 / sqrt(L), ss2 = 0.5, and c an fp32 tensor
    expression (:113-121)."""

    def _consts(self, dev):
        beta = (1.0 / self.L.to(dev).sqrt()).reshape(())
        c1 = beta * 0.5
        return beta, beta, 0.5, float((c1 / (1 - c1)).sqrt())


class DLADMMNetFullLSKM(_RowpLSKM, DLADMMNetFull):
    """test_syn_l1l1_full.py:68-296: beta = 1, ss1 = 0.5 / L, ss2 = 0.3 (:153-156).  The script's
    switch to ss2 = 0.9 at k == 15 (:157-159) is not implemented: its forward never passes `k` to
    S(), so the switch never fires."""

    def _consts(self, dev):
        return 1.0, (0.5 / self.L.to(dev)).reshape(()), 0.3, sqrt(0.3 / (1 - 0.3))
