"""The plan flags of the prologue-product reuse (include/dladmm.h DLADMM_F_P0_SAVE /
DLADMM_F_P0_REUSE): their values in the header and the binding, their effect on the plan (none on
the path, the P0 region on the workspace where they act), and the key logic of ops.PrologueCache
on plain CPU tensors.  No device needed; the calls themselves are covered by
tests/test_gpu_p0_reuse.py."""
import copy
import ctypes
import os
import pickle
import re
from importlib import import_module

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_values_match_the_header_and_the_abi_stays():
    lib = import_module("d-ladmm_amd._lib")
    with open(os.path.join(ROOT, "include", "dladmm.h")) as f:
        hdr = f.read()
    for name, value in (("P0_SAVE", 512), ("P0_REUSE", 1024)):
        m = re.search(r"DLADMM_F_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == value == getattr(lib, "F_" + name)
    flags = [getattr(lib, n) for n in dir(lib) if n.startswith("F_")]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)
    # new flag bits and a library-private workspace region: no layout change
    assert re.search(r"#define\s+DLADMM_ABI_VERSION\s+6\b", hdr) and lib.ABI_VERSION == 6


def _desc(lib, B=65536, **kw):
    d = lib.FwdDesc()
    d.abi_version = lib.ABI_VERSION
    d.variant = lib.V4_SCALAR
    d.m, d.n, d.batch, d.layers = 256, 512, B, 15
    d.keep_all, d.loss_kind = 1, 1
    fake = 1 << 40  # never dereferenced: only validation / sizing is exercised here
    for f in ("X", "A", "Z0", "E0", "L0", "scalar_params", "Z", "E", "L", "T", "loss_sums"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z0 = d.ld_e0 = d.ld_l0 = d.ld_out = B
    d.ld_a, d.ld_w = 512, 256
    w = lib.ptr_array([fake + 4096 * k for k in range(15)])
    d.W = ctypes.cast(w, ctypes.POINTER(ctypes.c_void_p))
    for k, v in kw.items():
        setattr(d, k, v)
    return d, w


def test_plan_path_unchanged_and_workspace_grows_where_the_flags_act():
    lib = import_module("d-ladmm_amd._lib")
    L = lib.lib()
    m, B = 256, 65536
    d, _keep = _desc(lib, B)
    path = L.dladmm_fwd_path(ctypes.byref(d))
    ws = L.dladmm_fwd_workspace_bytes(ctypes.byref(d))
    assert path == 1 and ws > 0
    for f in (lib.F_P0_SAVE, lib.F_P0_REUSE, lib.F_P0_SAVE | lib.F_P0_REUSE):
        d.flags = f
        assert L.dladmm_fwd_path(ctypes.byref(d)) == path
        assert L.dladmm_fwd_workspace_bytes(ctypes.byref(d)) >= ws + m * B * 4
    # split-f16 (path 4) and the row-split paths ignore the flags
    for kw in (dict(precision=lib.PREC_F32_SPLIT), dict(precision=lib.PREC_BF16)):
        s, _k = _desc(lib, B, **kw)
        p0, w0 = L.dladmm_fwd_path(ctypes.byref(s)), L.dladmm_fwd_workspace_bytes(ctypes.byref(s))
        s.flags = lib.F_P0_SAVE
        assert L.dladmm_fwd_path(ctypes.byref(s)) == p0 != 1
        assert L.dladmm_fwd_workspace_bytes(ctypes.byref(s)) == w0
    r, _k = _desc(lib, 1000)
    p0, w0 = L.dladmm_fwd_path(ctypes.byref(r)), L.dladmm_fwd_workspace_bytes(ctypes.byref(r))
    r.flags = lib.F_P0_REUSE
    assert L.dladmm_fwd_path(ctypes.byref(r)) == p0 == 6
    assert L.dladmm_fwd_workspace_bytes(ctypes.byref(r)) == w0
    r.flags |= lib.F_NO_ROWSPLIT    # path 1: they act
    assert L.dladmm_fwd_path(ctypes.byref(r)) == 1
    r.flags = lib.F_NO_ROWSPLIT
    w1 = L.dladmm_fwd_workspace_bytes(ctypes.byref(r))
    r.flags |= lib.F_P0_SAVE
    assert L.dladmm_fwd_workspace_bytes(ctypes.byref(r)) >= w1 + m * 1000 * 4


def test_cache_key_logic_on_cpu_tensors():
    ops = import_module("d-ladmm_amd.ops")
    dev = torch.device("cpu")
    A, Z0 = torch.randn(4, 8), torch.randn(8, 6)

    def key(A, Z0, B=6):
        return (4, 4, 8, B, 3, "f32", ops._tensor_sig(A), ops._tensor_sig(Z0), 1024)

    c = ops.PrologueCache()
    s0, s1 = ("cpu", None, 0), ("cpu", None, 1)
    ws, hit = c.lookup(s0, key(A, Z0), 1024, dev)
    assert not hit and ws.numel() >= 1024
    # a miss is not a fill until the call was enqueued
    assert not c.lookup(s0, key(A, Z0), 1024, dev)[1]
    c.commit(s0, key(A, Z0), (A, Z0))
    ws2, hit = c.lookup(s0, key(A, Z0), 1024, dev)
    assert hit and ws2.data_ptr() == ws.data_ptr()
    # another stream never shares the workspace
    ws3, hit = c.lookup(s1, key(A, Z0), 1024, dev)
    assert not hit and ws3.data_ptr() != ws.data_ptr()
    # in-place ops, a view with other strides, a new tensor, another batch: all miss
    Z0.mul_(2)
    assert not c.lookup(s0, key(A, Z0), 1024, dev)[1]
    c.commit(s0, key(A, Z0), (A, Z0))
    assert c.lookup(s0, key(A, Z0), 1024, dev)[1]
    A.add_(1)
    assert not c.lookup(s0, key(A, Z0), 1024, dev)[1]
    c.commit(s0, key(A, Z0), (A, Z0))
    assert not c.lookup(s0, key(A, Z0[:, :3], 3), 1024, dev)[1]
    c.commit(s0, key(A, Z0), (A, Z0))
    assert not c.lookup(s0, key(A, Z0.clone()), 1024, dev)[1]
    # a column shard passed as a view keys on its own offset and strides, stably
    c.commit(s0, key(A, Z0[:, 2:5], 3), (A, Z0[:, 2:5]))
    assert c.lookup(s0, key(A, Z0[:, 2:5], 3), 1024, dev)[1]
    assert not c.lookup(s0, key(A, Z0[:, 1:4], 3), 1024, dev)[1]
    # a larger workspace for the same key refills
    c.commit(s0, key(A, Z0), (A, Z0))
    assert not c.lookup(s0, key(A, Z0), 4096, dev)[1]
    # least recently used streams fall out; invalidate drops everything
    for i in range(2, 2 + ops.PrologueCache.MAX_STREAMS):
        c.lookup(("cpu", None, i), key(A, Z0), 1024, dev)
    assert len(c._slots) == ops.PrologueCache.MAX_STREAMS and s0 not in c._slots
    c.invalidate()
    assert not c._slots
    # copies of a model start with an empty cache of their own
    c.lookup(s0, key(A, Z0), 1024, dev)
    c.commit(s0, key(A, Z0), (A, Z0))
    assert not copy.deepcopy(c)._slots and not pickle.loads(pickle.dumps(c))._slots


def test_forward_result_reports_reuse_and_models_default_on():
    ops = import_module("d-ladmm_amd.ops")
    model = import_module("d-ladmm_amd.model")
    assert ops.ForwardResult(None, None, None, None, None).p0_reused is False
    assert model._DLADMMBase.reuse_prologue is True
    assert callable(model._DLADMMBase.invalidate_cache)
