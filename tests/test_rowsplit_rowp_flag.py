"""The plan flag that opts the per-row-parameter variants V2 / V3 into the small-batch row-split
forms (include/dladmm.h DLADMM_F_ROWSPLIT_ROWP): its value in the binding and its name in
ops.plan_flags.  No device needed."""
import os
import re
from importlib import import_module


def test_rowsplit_rows_flag_value_and_name():
    lib = import_module("d-ladmm_amd._lib")
    ops = import_module("d-ladmm_amd.ops")
    assert lib.F_ROWSPLIT_ROWP == 256
    with ops.plan_flags(rowsplit_rows=True) as f:
        assert f & lib.F_ROWSPLIT_ROWP
        with ops.plan_flags(rowsplit_rows=False) as g:
            assert not g & lib.F_ROWSPLIT_ROWP
    # a bit of its own
    others = [getattr(lib, n) for n in dir(lib) if n.startswith("F_") and n != "F_ROWSPLIT_ROWP"]
    assert all(not (o & lib.F_ROWSPLIT_ROWP) for o in others)


def test_rowsplit_rows_flag_matches_the_header():
    lib = import_module("d-ladmm_amd._lib")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dladmm.h")) as f:
        hdr = f.read()
    m = re.search(r"DLADMM_F_ROWSPLIT_ROWP\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == lib.F_ROWSPLIT_ROWP
    # a new flag bit, no layout change: the ABI version stays
    assert re.search(r"#define\s+DLADMM_ABI_VERSION\s+6\b", hdr) and lib.ABI_VERSION == 6
