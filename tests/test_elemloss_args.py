"""dladmm_elemloss_f32's descriptor validation and training_loss(kind="gt" | "rw")'s argument
errors -- CPU only: every case returns before any device work."""
import ctypes

import pytest
import torch


def _desc(dl, **kw):
    d = dl._lib.ElemLossDesc()
    d.abi_version = dl._lib.ABI_VERSION
    d.m, d.n, d.batch, d.layers, d.power, d.mode = 250, 500, 20, 3, 2, 1
    fake = 1 << 40  # never dereferenced: only validation / sizing is exercised here
    for f in ("Z", "E", "Zref", "Eref", "w", "colsum", "total", "gZ", "gE", "workspace"):
        setattr(d, f, fake)
    d.ld_z = d.ld_e = d.ld_zref = d.ld_eref = d.ld_g = 20
    d.z_layer_stride = d.gz_layer_stride = 500 * 20
    d.e_layer_stride = d.ge_layer_stride = 250 * 20
    d.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("fields,code", [
    (dict(abi_version=99), -1), (dict(Z=None, E=None), -5), (dict(ld_z=-20), -3),
    (dict(ld_eref=-1), -3), (dict(ld_g=19), -3), (dict(workspace_bytes=0), -6),
    (dict(workspace=None), -6), (dict(colsum=None), -5), (dict(w=None), -5),
    (dict(gE=None), -5), (dict(power=3), -7), (dict(mode=2), -7), (dict(layers=0), -4),
    (dict(batch=0), -3), (dict(ld_z=1 << 20), -7),
    (dict(n=3000000), -7), (dict(layers=40000), -7),   # slabs / 2 K past a grid dimension
])
def test_validation_codes(dl, fields, code):
    L = dl._lib.lib()
    assert L.dladmm_elemloss_f32(ctypes.byref(_desc(dl, **fields)), None) == code


def test_workspace_bytes_follow_the_tile_and_the_operands(dl):
    wsb = dl._lib.lib().dladmm_elemloss_workspace_bytes
    slab = lambda rows, sr: -(-rows // sr)  # noqa: E731
    # narrow tile: slabs of 32 rows of [Z rows to a multiple of 4; E rows]; fp64 [slabs][K][2][B]
    assert wsb(ctypes.byref(_desc(dl))) == slab(750, 32) * 3 * 2 * 20 * 8
    assert wsb(ctypes.byref(_desc(dl, Z=None))) == slab(250, 32) * 3 * 2 * 20 * 8
    assert wsb(ctypes.byref(_desc(dl, n=30, m=16))) == -(-slab(48, 32) * 3 * 2 * 20 * 8 // 256) * 256
    # wide tile from batch 2048: slabs of 64 rows
    assert wsb(ctypes.byref(_desc(dl, batch=2047))) == slab(750, 32) * 3 * 2 * 2047 * 8 + 128
    assert wsb(ctypes.byref(_desc(dl, batch=2048))) == slab(750, 64) * 3 * 2 * 2048 * 8
    assert wsb(ctypes.byref(_desc(dl, Z=None, E=None))) == 0
    # the sums-only form needs no w / gZ / gE; NULL references pass: next check is the workspace
    L = dl._lib.lib()
    assert L.dladmm_elemloss_f32(ctypes.byref(_desc(dl, mode=0, w=None, gZ=None, gE=None, Zref=None,
                                                    Eref=None, workspace_bytes=0)), None) == -6


def _net(dl, cls, m=16, n=32, B=4, K=2):
    g = torch.Generator().manual_seed(5)
    return getattr(dl, cls)(m=m, n=0, d=n, batch_size=B, A=torch.randn(m, n, generator=g),
                            Z0=torch.zeros(n, B), E0=torch.zeros(m, B), L0=torch.zeros(m, B),
                            layers=K)


@pytest.mark.parametrize("cls", ["DLADMMNet", "DLADMMNetLTheta", "DLADMMNetScalar"])
def test_training_loss_argument_errors(dl, cls):
    net = _net(dl, cls)
    x, zl, el = torch.zeros(16, 4), torch.zeros(32, 4), torch.zeros(16, 4)
    with pytest.raises(ValueError, match="needs z_label and e_label"):
        net.training_loss(x, 0.001, kind="gt")
    with pytest.raises(ValueError, match="needs z_label and e_label"):
        net.training_loss(x, 0.001, kind="gt", z_label=zl)
    for bad_z, bad_e in ((el, el), (zl, torch.zeros(16, 3)), (torch.zeros(32), el)):
        with pytest.raises(ValueError, match="needs z_label"):
            net.training_loss(x, 0.001, kind="gt", z_label=bad_z, e_label=bad_e)
    for kind in ("rw", "l1l1"):
        with pytest.raises(ValueError, match="belong to kind='gt'"):
            net.training_loss(x, 0.001, kind=kind, z_label=zl, e_label=el)
    with pytest.raises(ValueError, match="reduction"):
        net.training_loss(x, 0.001, kind="gt", z_label=zl, e_label=el, reduction="max")
    with pytest.raises(ValueError, match="coeffs"):
        net.training_loss(x, 0.001, coeffs=[1.0], kind="rw")
