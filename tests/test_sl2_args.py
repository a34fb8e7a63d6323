"""dladmm_sl2_f32's descriptor validation and training_loss(kind="sl2")'s argument errors -- CPU
only: every case returns before any device work."""
import ctypes

import pytest
import torch


def _desc(dl, **kw):
    d = dl._lib.Sl2Desc()
    d.abi_version = dl._lib.ABI_VERSION
    d.m, d.n, d.batch, d.mode = 250, 500, 20, 1
    d.beta, d.ss1, d.ss2, d.thz, d.c = 1.0, 0.08, 0.3, 8e-5, 0.65
    fake = 1 << 40  # never dereferenced: only validation / sizing is exercised here
    for f in ("X", "A", "Z", "E", "L", "T", "Ep", "coef", "colsum", "gZ", "gE", "gL", "gT",
              "gEp", "workspace"):
        setattr(d, f, fake)
    d.ld_x = d.ld_z = d.ld_e = d.ld_l = d.ld_t = d.ld_ep = d.ld_g = 20
    d.ld_a = 500
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("field,value,code", [
    ("abi_version", 99, -1), ("X", None, -5), ("colsum", None, -5), ("gZ", None, -5),
    ("gT", None, -5), ("coef", None, -5), ("m", 257, -7), ("n", 513, -7), ("thz", 0.0, -7),
    ("thz", -1e-4, -7), ("ss2", 0.0, -7), ("mode", 2, -7), ("batch", 0, -3), ("ld_t", 19, -3),
])
def test_validation_codes(dl, field, value, code):
    L = dl._lib.lib()
    assert L.dladmm_sl2_f32(ctypes.byref(_desc(dl, **{field: value})), None) == code


def test_workspace_bytes_and_optional_fields(dl):
    L = dl._lib.lib()
    assert L.dladmm_sl2_workspace_bytes(ctypes.byref(_desc(dl))) == 2 * 256 * 512 * 4
    assert L.dladmm_sl2_workspace_bytes(ctypes.byref(_desc(dl, m=257))) == 0
    # a NULL gEp and, in mode 0, NULL cotangents pass validation: the next check is the workspace
    assert L.dladmm_sl2_f32(ctypes.byref(_desc(dl, gEp=None, workspace_bytes=0)), None) == -6
    assert L.dladmm_sl2_f32(ctypes.byref(_desc(dl, mode=0, gZ=None, coef=None,
                                               workspace_bytes=0)), None) == -6


def _net(dl, cls, m, n, B=4, K=2):
    g = torch.Generator().manual_seed(5)
    return getattr(dl, cls)(m=m, n=0, d=n, batch_size=B, A=torch.randn(m, n, generator=g),
                            Z0=torch.zeros(n, B), E0=torch.zeros(m, B), L0=torch.zeros(m, B),
                            layers=K)


@pytest.mark.parametrize("cls", ["DLADMMNetScalarSl2", "DLADMMNetFull"])
def test_training_loss_argument_errors(dl, cls):
    net = _net(dl, cls, 16, 32)
    x = torch.zeros(16, 4)
    with pytest.raises(ValueError, match="unknown loss kind"):
        net.training_loss(x, 0.001, kind="sl3")
    with pytest.raises(ValueError, match="needs x"):      # wrong column count
        net.training_loss(torch.zeros(16, 3), 0.001, kind="sl2")
    with pytest.raises(ValueError, match="coeffs"):
        net.training_loss(x, 0.001, coeffs=[1.0], kind="sl2")
    for m, n in ((257, 32), (16, 513)):
        with pytest.raises(ValueError, match="m <= 256, n <= 512"):
            _net(dl, cls, m, n).training_loss(torch.zeros(m, 4), 0.001, kind="sl2")
