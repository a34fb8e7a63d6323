"""DLADMMNetLenaLSKM without a device: construction, the reference checkpoint layout, errors."""
import numpy as np
import pytest
import torch


def test_lena_lskm_module(dl):
    m, n, B, K = 16, 32, 4, 15
    g = torch.Generator().manual_seed(5)
    A = torch.randn(m, n, generator=g) / 4
    args = (m, 0, n, B, A, torch.rand(n, B, generator=g) / n, torch.zeros(m, B), torch.zeros(m, B), K)
    net = dl.DLADMMNetLenaLSKM(*args)
    assert (net.alpha, net.delta, net.mu_k_method, net.mu_k_param, net.num_iter,
            net.fused_safeguard) == (0.45, 0.01, "EMA", 0.3, 200, None)
    assert net.name() == "DLADMMNet"
    want = np.float32(np.linalg.norm(A.numpy().T @ A.numpy(), ord=2))
    assert net.L.shape == (1, 1) and float(net.L) == float(want)
    # the reference V1 class's state_dict: beta1.k, beta2.k (m, batch_size), fc.k.weight
    sd = {}
    for k in range(K):
        sd[f"beta1.{k}"] = torch.full((m, B), 0.5 + k)
        sd[f"beta2.{k}"] = torch.full((m, B), 1.5 + k)
        sd[f"fc.{k}.weight"] = torch.randn(n, m, generator=g)
    assert len(sd) == 45
    net.load_state_dict(sd, strict=True)
    assert float(net.beta2[14].detach()[3, 1]) == 15.5
    with pytest.raises(NotImplementedError):
        dl.DLADMMNetLenaLSKM(*args, mu_k_method="RM")
    with pytest.raises(RuntimeError):   # a CPU tensor: no fallback, as everywhere else
        net(torch.zeros(m, B))
