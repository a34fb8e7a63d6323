"""Classic KM iteration and learned + safeguarded KM (LSKM) for the lena model (V1): the
test-script class of test_lena_lskm.py:41-192 as a drop-in.

Same constructor, parameters and `state_dict` as the V1 model (per-sample beta1 / beta2 of shape
(m, batch_size), fixed thresholds 0.025 / 0.06), plus the settings the script reads from module
globals (alpha, delta, mu_k_method, mu_k_parameter, num_iter) as keyword arguments with the
script's values.  `forward(x, use_learned, use_safeguard, K)` returns (Z, E, L) or, with learned +
safeguard, (Z, E, L, sg_count) like the script: no T.

This class differs from lskm.DLADMMNetLSKM in the classic step (beta = ss1 = 1 / sqrt(L),
ss2 = 0.5), in the safeguard norm (|T_new| of the classic step alone: no E term, no beta factor)
and in the learned step (EM_V1 with per-sample betas).  Every step runs on the HIP kernels:
  * the classic step S() (:91-106) is the fused kernel's V5 path with the shared weight A^T; a
    pure KM run of K iterations is ONE launch;
  * the learned forward is the V1 model's;
  * learned + safeguard at the 256 x 512 register shape is ONE kernel launch,
    `dladmm_lskm_lena_f32` (csrc/dladmm_lskm_lena_fused.hip; `fused_safeguard`); elsewhere, or with
    fused_safeguard=False, each layer runs a one-layer V1 forward, two one-step KM launches and
    `dladmm_safeguard_f32` with beta = 1, c = 0.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .lskm import _UPDATERS
from .model import DLADMMNet, _dev, _scalar_table
from .ops import _f32_dev, _workspace, dladmm_forward


class DLADMMNetLenaLSKM(DLADMMNet):
    """test_lena_lskm.py:41-192.  m.weight = A.t() + 1e-3 * randn (:77), name() "DLADMMNet"."""

    def __init__(self, m, n, d, batch_size, A, Z0, E0, L0, layers, *, alpha: float = 0.45,
                 delta: float = 0.01, mu_k_method: str = "EMA", mu_k_param: float = 0.3,
                 num_iter: int = 200, fused_safeguard: Optional[bool] = None):
        super().__init__(m, n, d, batch_size, A, Z0, E0, L0, layers)
        # :55-56
        self.At = self.A.t()
        self.A_np = A.detach().cpu().numpy()
        self.L = _dev((np.linalg.norm(np.matmul(self.A_np.transpose(), self.A_np), ord=2)
                       * torch.ones(1, 1)).float())
        # the learned + safeguarded loop as one launch (dladmm_lskm_lena_f32): True requires it,
        # False keeps the per-layer launches, None takes it wherever the kernel exists
        self.fused_safeguard = fused_safeguard
        if mu_k_method == "RM":
            raise NotImplementedError(
                "mu_k_method 'RM': the reference RMUpdater.step returns torch's (values, indices) "
                "pair (mu_updater.py:94), which test_lena_lskm.py:156 cannot multiply")
        if mu_k_method not in _UPDATERS:
            raise ValueError(f"unknown mu_k_method {mu_k_method!r}")
        # the script's module globals (:14-24)
        self.alpha, self.delta = float(alpha), float(delta)
        self.mu_k_method, self.mu_k_param = mu_k_method, float(mu_k_param)
        self.num_iter = int(num_iter)

    # --- the classic step's constants (:92-94): beta = ss1 = 1 / sqrt(L), ss2 = 0.5 -----------
    def _km_table(self, K: int) -> torch.Tensor:
        dev = self.A.device
        ss1 = (1.0 / self.L.to(dev).sqrt()).reshape(())             # fp32, as 1.0 / self.L.sqrt()
        thz = ss1 * self.alpha                                      # fp32 ss1 * alpha
        return _scalar_table(K, dev, b1=ss1, b2=ss1, b3=ss1, ss2=0.5, the=0.5, thz=thz, s1=ss1)

    def _At(self) -> torch.Tensor:
        if getattr(self, "_At_c", None) is None or self._At_c.device != self.A.device:
            self._At_c = self.A.t().contiguous()
        return self._At_c

    def _km(self, x, Z, E, L, K: int, table: Optional[torch.Tensor] = None):
        """K classic iterations from (Z, E, L) as one fused launch; T_0 = A Z + E - X."""
        return dladmm_forward(_lib.V5_TIED, x, self.A, [self._At()] * K, Z, E, L, keep_all=True,
                              want_T=True,
                              scalar_params=self._km_table(K) if table is None else table)

    def _l2o(self, x, Z, E, L, k: int, tables: dict):
        """Learned layer k (:131-135 / :142-146) from (Z, E, L)."""
        return dladmm_forward(_lib.V1_LENA, x, self.A, [self.fc[k].weight.detach()], Z, E, L,
                              keep_all=True, want_T=True,
                              scalar_params=tables["scalar_params"][k:k + 1].contiguous(),
                              beta1_elem=tables["beta1_elem"][k:k + 1],
                              beta2_elem=tables["beta2_elem"][k:k + 1])

    def S(self, Zk, Ek, Lk, Tk, X, **kwargs):
        """One classic step (:91-106); returns (Varnew, Znew, Enew, Tnew, Lnew).  Tk must be
        A Zk + Ek - X (as everywhere in the script)."""
        if kwargs:
            raise NotImplementedError("dladmm: S runs with the script's constants only")
        with torch.no_grad():
            r = self._km(X, Zk, Ek, Lk, 1)
            Varn = Lk + (1.0 / self.L.sqrt()) * Tk
        return Varn, r.Z[0], r.E[0], r.T[1], r.L[0]

    @staticmethod
    def two_norm(z):
        return (z ** 2).sum(dim=0).sqrt()

    def _safeguard(self, x, mu, cand_l, cand_k, s_step, Ep, out, k_out, count):
        """dladmm_safeguard_f32 with beta = 1, c = 0: |T_new| of the step from the L2O candidate,
        mu update, per-column select.  out None: mu_0 = |T_new| of the step `s_step` (:120)."""
        d = _lib.SafeguardDesc()
        d.abi_version = _lib.ABI_VERSION
        m, B = x.shape
        d.m, d.n, d.batch, d.ld = m, self.d, B, B
        d.Es, d.Ts, d.Ep, d.mu = s_step.E[0].data_ptr(), s_step.T[1].data_ptr(), Ep.data_ptr(), \
            mu.data_ptr()
        if out is None:
            d.El = Ep.data_ptr()
        else:
            d.Zl, d.El, d.Ll, d.Tl = (cand_l.Z[0].data_ptr(), cand_l.E[0].data_ptr(),
                                      cand_l.L[0].data_ptr(), cand_l.T[1].data_ptr())
            d.Zk, d.Ek, d.Lk, d.Tk = (cand_k.Z[0].data_ptr(), cand_k.E[0].data_ptr(),
                                      cand_k.L[0].data_ptr(), cand_k.T[1].data_ptr())
            Zo, Eo, Lo, To = out
            d.Zo, d.Eo, d.Lo = Zo[k_out].data_ptr(), Eo[k_out].data_ptr(), Lo[k_out].data_ptr()
            d.To = To.data_ptr()
            d.count = count.data_ptr()
        d.beta, d.c, d.delta = 1.0, 0.0, self.delta
        d.updater, d.mu_param = _UPDATERS[self.mu_k_method], self.mu_k_param
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().dladmm_safeguard_f32(ctypes.byref(d), ctypes.c_void_p(stream)))

    def _fused_shape(self) -> bool:
        """The 256 x 512 register shape dladmm_lskm_lena_f32 is built for (smaller problems run
        in it through zero padding)."""
        m, n = self.A.shape
        return m <= 256 and n <= 512

    def _lskm_fused(self, x, nl: int, tables: dict, Zo, Eo, Lo, count):
        """dladmm_lskm_lena_f32: layers 0 .. nl-1 of the safeguarded loop, one kernel launch."""
        Lb = _lib.lib()
        dev = x.device
        X, A = _f32_dev(x, "X"), _f32_dev(self.A, "A")
        Z0, E0, L0 = _f32_dev(self.Z0, "Z0"), _f32_dev(self.E0, "E0"), _f32_dev(self.L0, "L0")
        m, B = X.shape
        n = A.shape[1]
        if A.shape[0] != m or tuple(Z0.shape) != (n, B) or tuple(E0.shape) != (m, B) or \
                tuple(L0.shape) != (m, B):
            raise RuntimeError("dladmm: Z0/E0/L0 shapes do not broadcast with X")
        Ws = [_f32_dev(self.fc[k].weight.detach().contiguous(), f"W[{k}]") for k in range(nl)]
        b1 = [_f32_dev(b, f"beta1[{k}]") for k, b in enumerate(tables["beta1_elem"][:nl])]
        b2 = [_f32_dev(b, f"beta2[{k}]") for k, b in enumerate(tables["beta2_elem"][:nl])]
        ldb = b1[0].stride(0)
        for b in b1 + b2:
            if tuple(b.shape) != (m, B) or b.stride(0) != ldb:
                raise RuntimeError(f"dladmm: per-sample beta of shape {tuple(b.shape)} does not "
                                   f"broadcast with X {tuple(X.shape)}")
        ptab = tables["scalar_params"][:nl].contiguous()
        km = self._km_table(1)
        warr = _lib.ptr_array([w.data_ptr() for w in Ws])
        a1 = _lib.ptr_array([b.data_ptr() for b in b1])
        a2 = _lib.ptr_array([b.data_ptr() for b in b2])
        d = _lib.LskmLenaDesc()
        d.abi_version = _lib.ABI_VERSION
        d.m, d.n, d.batch, d.layers = m, n, B, nl
        d.X, d.ld_x = X.data_ptr(), X.stride(0)
        d.A, d.ld_a = A.data_ptr(), A.stride(0)
        d.Z0, d.ld_z0 = Z0.data_ptr(), Z0.stride(0)
        d.E0, d.ld_e0 = E0.data_ptr(), E0.stride(0)
        d.L0, d.ld_l0 = L0.data_ptr(), L0.stride(0)
        d.W, d.ld_w = ctypes.cast(warr, ctypes.POINTER(ctypes.c_void_p)), m
        d.beta1_elem = ctypes.cast(a1, ctypes.POINTER(ctypes.c_void_p))
        d.beta2_elem = ctypes.cast(a2, ctypes.POINTER(ctypes.c_void_p))
        d.ld_beta = ldb
        d.scalar_params, d.km_params = ptab.data_ptr(), km.data_ptr()
        d.delta = self.delta
        d.updater, d.mu_param = _UPDATERS[self.mu_k_method], self.mu_k_param
        d.Z, d.E, d.L, d.ld_out = Zo.data_ptr(), Eo.data_ptr(), Lo.data_ptr(), B
        d.count = count.data_ptr()
        wsb = Lb.dladmm_lskm_lena_workspace_bytes(ctypes.byref(d))
        ws = _workspace(dev, max(wsb, 1))
        d.workspace, d.workspace_bytes = ws.data_ptr(), wsb
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(Lb.dladmm_lskm_lena_f32(ctypes.byref(d), ctypes.c_void_p(stream)))

    def forward(self, x, use_learned=True, use_safeguard=True, K: Optional[int] = None,
                fused_safeguard: Optional[bool] = None):
        """test_lena_lskm.py:108-188, under no_grad.  K defaults to the script's
        `layers if use_learned or use_safeguard else num_iter` (:38).  fused_safeguard overrides
        the constructor's setting for this call."""
        fused = self.fused_safeguard if fused_safeguard is None else fused_safeguard
        if fused and not self._fused_shape():
            raise ValueError(
                f"dladmm: fused_safeguard=True needs the 256 x 512 register shape (m <= 256, "
                f"n <= 512), got m={self.A.shape[0]}, n={self.A.shape[1]}")
        if K is None:
            K = self.layers if (use_learned or use_safeguard) else self.num_iter
        if use_safeguard and not use_learned:
            raise AssertionError("safeguarding needs the learned model (:150 assert use_learned)")
        if use_learned and K > self.layers:
            raise IndexError(f"K={K} learned steps but the model has {self.layers} layers")
        _f32_dev(x, "X")
        if x.shape[1] != self._pcols:
            raise ValueError(
                f"dladmm: X has {x.shape[1]} columns but the per-sample betas are "
                f"(m, {self._pcols}): the lena model runs batches of batch_size columns only")
        with torch.no_grad():
            if not use_learned:
                r = self._km(x, self.Z0, self.E0, self.L0, K)
                return list(r.Z), list(r.E), list(r.L)
            m, B = x.shape
            dev = x.device
            tables = self._tables(dev)
            if not use_safeguard:
                r = dladmm_forward(_lib.V1_LENA, x, self.A,
                                   [self.fc[k].weight.detach() for k in range(K)],
                                   self.Z0, self.E0, self.L0, keep_all=True, want_T=False,
                                   scalar_params=tables["scalar_params"][:K].contiguous(),
                                   beta1_elem=tables["beta1_elem"][:K],
                                   beta2_elem=tables["beta2_elem"][:K])
                return list(r.Z), list(r.E), list(r.L)
            Zo = torch.empty((K, self.d, B), device=dev)
            Eo = torch.empty((K, m, B), device=dev)
            Lo = torch.empty((K, m, B), device=dev)
            count = torch.zeros(self.layers, dtype=torch.int32, device=dev)
            if fused is None:
                fused = self._fused_shape()
            if fused and K > 0 and B > 0:
                self._lskm_fused(x, K, tables, Zo, Eo, Lo, count)
            else:
                mu = torch.empty(B, device=dev)
                To = torch.empty((m, B), device=dev)   # the selected T: not an output
                km1 = self._km_table(1)
                # mu_0 = |S(Z0, E0, L0, T0, X)[-2]| (:120)
                s0 = self._km(x, self.Z0, self.E0, self.L0, 1, km1)
                self._safeguard(x, mu, None, None, s0, self.E0, None, 0, None)
                Zc, Ec, Lc = self.Z0, self.E0, self.L0
                for k in range(K):
                    cl = self._l2o(x, Zc, Ec, Lc, k, tables)               # :129-146
                    ck = self._km(x, Zc, Ec, Lc, 1, km1)                   # :127 / :139
                    cs = self._km(x, cl.Z[0], cl.E[0], cl.L[0], 1, km1)    # :151
                    self._safeguard(x, mu, cl, ck, cs, Ec, (Zo, Eo, Lo, To), k, count[k:k + 1])
                    Zc, Ec, Lc = Zo[k], Eo[k], Lo[k]
            return list(Zo), list(Eo), list(Lo), count.cpu().numpy().astype(np.float64)
