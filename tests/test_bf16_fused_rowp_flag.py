"""DLADMM_F_BF16_FUSED_ROWP: the flag's value and names, and the host-only plan it selects for the
per-row variants V2 / V3 (forward path 7 only together with DLADMM_F_BF16_FUSED) -- no device
work.  The descriptor is tests/test_bf16_fused_flag.py's (256 x 512, batch 1000, bf16)."""
import ctypes
import os
import re

import pytest

from test_bf16_fused_flag import ROOT, _desc

BOTH = "F_BF16_FUSED|F_BF16_FUSED_ROWP"


def _plan(dl, fl, variant="V3_FULL", **kw):
    d, keep = _desc(dl, variant=getattr(dl._lib, variant), **kw)
    for name in fl.split("|"):
        d.flags |= getattr(dl._lib, name) if name else 0
    L = dl._lib.lib()
    return L.dladmm_fwd_path(ctypes.byref(d)), L.dladmm_fwd_workspace_bytes(ctypes.byref(d)), keep


def test_flag_value_and_names(dl):
    ops = __import__("importlib").import_module("d-ladmm_amd.ops")
    assert dl._lib.F_BF16_FUSED_ROWP == 16384 and dl._lib.ABI_VERSION == 6
    with ops.plan_flags(bf16_fused=True, bf16_fused_rows=True) as f:
        assert f == 8192 | 16384
    hdr = open(os.path.join(ROOT, "include", "dladmm.h")).read()
    assert re.search(r"DLADMM_F_BF16_FUSED_ROWP\s*=\s*16384\b", hdr)


@pytest.mark.parametrize("kw,fl,path", [
    ({}, BOTH, 7),
    ({"variant": "V2_LTHETA"}, BOTH, 7),
    ({"m": 250, "n": 500, "ld_a": 500, "ld_w": 250, "row_stride": 500}, BOTH, 7),
    ({"row_stride": 514}, BOTH, 7),   # any row stride: the table is read dword by dword
    ({}, "F_BF16_FUSED_ROWP", 3),
    ({"variant": "V2_LTHETA"}, "F_BF16_FUSED_ROWP", 3),
    ({}, BOTH + "|F_PER_LAYER", 3),
    ({"m": 512, "ld_w": 512}, BOTH, 3),
    ({"batch": 998}, BOTH, 3),        # rows not in 16-byte pieces
    ({"variant": "V4_SCALAR"}, "F_BF16_FUSED_ROWP", 3),   # no effect on another variant
])
def test_plan_takes_path_7_for_rows_only_with_both_flags(kw, fl, path, dl):
    assert _plan(dl, fl, **kw)[0] == path


def test_flag_changes_nothing_in_fp32(dl):
    for prec in (dl._lib.PREC_F32, dl._lib.PREC_F32_SPLIT):
        assert _plan(dl, "", precision=prec)[:2] == _plan(dl, BOTH, precision=prec)[:2]
        assert _plan(dl, BOTH, precision=prec)[0] == 1


def test_workspace_is_the_scalar_variants_path_7_size(dl):
    p4, ws4, _k4 = _plan(dl, "F_BF16_FUSED", variant="V4_SCALAR")
    p3, ws3, _k3 = _plan(dl, BOTH)
    assert p4 == p3 == 7 and ws3 == ws4 > 0
