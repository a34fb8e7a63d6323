"""The counted vmcnt windows of the fused kernel's weight ring, replayed on the host (no GPU).

tests/ring_windows_replay.cc includes d-ladmm_amd/csrc/dladmm_ring_windows.h -- the header the
kernel takes its piece schedule and its windows from -- and lists, per instantiation and wave,
every vector-memory operation in issue order.  It fails if a barrier's window counts more
operations than were issued after the awaited chunk's last LDS-DMA piece (a data race), if a piece
is issued after the barrier that awaits it, or into a slot before the barrier that frees it.

One build per knob set: the library's defaults and every ring form the knobs offer.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ring_windows_replay.cc")
INC = os.path.join(ROOT, "d-ladmm_amd", "csrc")

OLD = ["-DDLADMM_RING2=0"]   # every instantiation on the knobs as given
KNOBS = {
    "default": [],
    "default_stagger2": ["-DDLADMM_DMA_STAGGER=2"],
    "before": OLD,
    "nocnt": OLD + ["-DDLADMM_CNT=0"],
    "late": OLD + ["-DDLADMM_DMA_LATE=1"],
    "spread": OLD + ["-DDLADMM_DMA_SPREAD=1"],
    "spread_stagger1": OLD + ["-DDLADMM_DMA_SPREAD=1", "-DDLADMM_DMA_STAGGER=1"],
    "spread_stagger2": OLD + ["-DDLADMM_DMA_SPREAD=1", "-DDLADMM_DMA_STAGGER=2"],
    "own3": OLD + ["-DDLADMM_SLOTS=3", "-DDLADMM_RING_OWN=1"],
    "own3_spread": OLD + ["-DDLADMM_SLOTS=3", "-DDLADMM_RING_OWN=1", "-DDLADMM_DMA_SPREAD=1"],
    "chunk32x2": OLD + ["-DDLADMM_CHUNK=32", "-DDLADMM_SLOTS=2", "-DDLADMM_RING_OWN=1"],
    "chunk32x2_spread": OLD + ["-DDLADMM_CHUNK=32", "-DDLADMM_SLOTS=2", "-DDLADMM_RING_OWN=1",
                         "-DDLADMM_DMA_SPREAD=1"],
    "chunk32x2_spread_stagger2": OLD + ["-DDLADMM_CHUNK=32", "-DDLADMM_SLOTS=2", "-DDLADMM_RING_OWN=1",
                                  "-DDLADMM_DMA_SPREAD=1", "-DDLADMM_DMA_STAGGER=2"],
    "chunk32x3_spread": OLD + ["-DDLADMM_CHUNK=32", "-DDLADMM_SLOTS=3", "-DDLADMM_RING_OWN=1",
                         "-DDLADMM_DMA_SPREAD=1"],
}


def _cxx():
    for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


@pytest.mark.parametrize("name", sorted(KNOBS))
def test_ring_windows_replay(name, tmp_path):
    exe = str(tmp_path / "replay")
    subprocess.run([_cxx(), "-std=c++17", "-O0", "-I", INC] + KNOBS[name] + [SRC, "-o", exe],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)  # the slack of every instantiation
    assert p.returncode == 0, p.stdout[-2000:]
    assert p.stdout.rstrip().endswith("ok")
    # every instantiation was replayed: 3 shapes x 4 parameter kinds x 4 forms, each with and
    # without the kernel's permission for the two-slot ring
    assert sum(1 for ln in p.stdout.splitlines() if ln.startswith("MB ")) == 96


def test_replay_sees_a_window_one_too_large(tmp_path):
    """The replay is a witness only if it fails on a wrong count: the spread form's windows
    started one step early (at the latest wave's last piece instead of after it)."""
    hdr = open(os.path.join(INC, "dladmm_ring_windows.h")).read()
    good = "R::SPREAD ? R::OLAST + 1 : 0"
    assert hdr.count(good) == 1
    (tmp_path / "dladmm_ring_windows.h").write_text(hdr.replace(good, "R::SPREAD ? R::OLAST : 0"))
    exe = str(tmp_path / "replay")
    subprocess.run([_cxx(), "-std=c++17", "-O0", "-I", str(tmp_path), "-DDLADMM_DMA_SPREAD=1",
                    "-DDLADMM_DMA_STAGGER=2", "-DDLADMM_RING2=0", SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1 and "FAIL" in p.stdout


def test_build_checks_the_scratch_census():
    """build.py compiles the fused fp32 units with the compiler's resource remarks and fails when
    a fused kernel's scratch exceeds the recorded census (the list of instantiations that keep the
    four-slot ring rests on it)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "dladmm_build_census", os.path.join(ROOT, "d-ladmm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    for u in b.CENSUS_UNITS:
        assert u in b.UNITS and os.path.exists(os.path.join(b.CSRC, u))
    head = "k.h:9:1: remark: Function Name: _ZN6dladmm12fused_kernelI%sEEvNS_9FusedArgsE [-R]\n"
    size = "k.h:9:1: remark:     ScratchSize [bytes/lane]: %d [-R]\n"
    elz_v4, v4_load = "Li256ELi512ELi1ELi0ELb1ELb0ELb1", "Li256ELi512ELi1ELi0ELb0ELb1ELb0"
    b.check_scratch("u", head % v4_load + size % 0 + head % elz_v4 + size % 416)
    with pytest.raises(RuntimeError):
        b.check_scratch("u", head % v4_load + size % 4)
    with pytest.raises(RuntimeError):
        b.check_scratch("u", head % elz_v4 + size % 420)
