"""DLADMM_F_BF16_FUSED: the flag's value and names, and the host-only plan it selects (forward
path 7) -- no device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(dl, **kw):
    d = dl._lib.FwdDesc()
    d.abi_version = dl._lib.ABI_VERSION
    d.variant = dl._lib.V4_SCALAR
    d.m, d.n, d.batch, d.layers = 256, 512, 1000, 15
    d.keep_all, d.loss_kind = 1, 1
    d.precision = dl._lib.PREC_BF16
    fake = 1 << 40  # never dereferenced: only validation / sizing is exercised here
    for f in ("X", "A", "Z0", "E0", "L0", "scalar_params", "row_params", "Z", "E", "L", "T",
              "loss_sums"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = 1000
    d.ld_a, d.ld_w, d.row_stride = 512, 256, 512
    w = dl._lib.ptr_array([fake + 4096 * k for k in range(15)])
    d.W = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    for k, v in kw.items():
        setattr(d, k, v)
    return d, w


def test_flag_value_and_names(dl):
    ops = __import__("importlib").import_module("d-ladmm_amd.ops")
    assert dl._lib.F_BF16_FUSED == 8192 and dl._lib.ABI_VERSION == 6
    with ops.plan_flags(bf16_fused=True) as f:
        assert f == 8192
    hdr = open(os.path.join(ROOT, "include", "dladmm.h")).read()
    assert re.search(r"DLADMM_F_BF16_FUSED\s*=\s*8192\b", hdr)
    assert re.search(r"#define\s+DLADMM_ABI_VERSION\s+6\b", hdr)


@pytest.mark.parametrize("kw,fl,path", [
    ({}, "F_BF16_FUSED", 7),
    ({}, None, 3),
    ({}, "F_BF16_FUSED|F_PER_LAYER", 3),
    ({"variant": "V2_LTHETA"}, "F_BF16_FUSED", 3),
    ({"m": 512, "ld_w": 512}, "F_BF16_FUSED", 3),
    ({"batch": 998}, "F_BF16_FUSED", 3),   # rows not in 16-byte pieces
])
def test_plan_takes_path_7_only_where_the_kernel_fits(kw, fl, path, dl):
    L = dl._lib.lib()
    kw = {k: getattr(dl._lib, v) if isinstance(v, str) else v for k, v in kw.items()}
    d, _keep = _desc(dl, **kw)
    for name in (fl or "").split("|"):
        d.flags |= getattr(dl._lib, name) if name else 0
    assert L.dladmm_fwd_path(ctypes.byref(d)) == path


def test_flag_changes_nothing_in_fp32(dl):
    L = dl._lib.lib()
    for extra, path in ((0, 6), (dl._lib.F_NO_XSPLIT, 5), (dl._lib.F_NO_ROWSPLIT, 1)):
        d, _keep = _desc(dl, precision=dl._lib.PREC_F32, flags=extra)
        ws = L.dladmm_fwd_workspace_bytes(ctypes.byref(d))
        d.flags |= dl._lib.F_BF16_FUSED
        assert L.dladmm_fwd_path(ctypes.byref(d)) == path
        assert L.dladmm_fwd_workspace_bytes(ctypes.byref(d)) == ws


def test_workspace_packs_a_shared_weight_once(dl):
    L = dl._lib.lib()
    d, _keep = _desc(dl, flags=dl._lib.F_BF16_FUSED)
    ws = L.dladmm_fwd_workspace_bytes(ctypes.byref(d))
    assert ws >= 16 * 256 * 512 * 2 and ws % 256 == 0
    w1 = dl._lib.ptr_array([1 << 40] * 15)
    d.W = ctypes.cast(w1, ctypes.POINTER(ctypes.c_void_p))
    assert L.dladmm_fwd_workspace_bytes(ctypes.byref(d)) == ws - 14 * 256 * 512 * 2
