"""The per-row LSKM classes (lskm_rowp.py) without a GPU: constructor defaults, state_dict keys
equal to the parents', the unsupported updater, and the device check of forward."""
import numpy as np
import pytest
import torch

import problems as P

CLASSES = [("DLADMMNetLThetaLSKM", "DLADMMNetLTheta"), ("DLADMMNetGtLThetaLSKM", "DLADMMNetLTheta"),
           ("DLADMMNetFullLSKM", "DLADMMNetFull")]


def build(dl, name, **kw):
    inp = P.make_inputs(16, 32, 4, 77)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return getattr(dl, name)(m=16, n=0, d=32, batch_size=4, A=t(inp["A"]), Z0=t(inp["Z0"]),
                             E0=t(inp["E0"]), L0=t(inp["L0"]), layers=3, **kw), t(inp["X"])


@pytest.mark.parametrize("name,parent", CLASSES)
def test_defaults_and_state_dict(name, parent, dl):
    net, _ = build(dl, name)
    assert (net.alpha, net.delta, net.mu_k_method, net.mu_k_param, net.num_iter,
            net.fused_safeguard) == (0.01, -99.0, "None", 0.0, 200, None)
    par, _ = build(dl, parent)
    assert isinstance(net, getattr(dl, parent))
    assert list(net.state_dict()) == list(par.state_dict())
    net.load_state_dict(par.state_dict(), strict=True)
    assert net.name() == "DLADMMNet"


@pytest.mark.parametrize("name,parent", CLASSES)
def test_rm_and_unknown_updater(name, parent, dl):
    with pytest.raises(NotImplementedError):
        build(dl, name, mu_k_method="RM")
    with pytest.raises(ValueError):
        build(dl, name, mu_k_method="nope")


@pytest.mark.parametrize("name,parent", CLASSES)
def test_cpu_tensor_raises(name, parent, dl):
    net, X = build(dl, name)
    with pytest.raises(RuntimeError):   # a CPU tensor: no fallback, as everywhere else
        net(X)
