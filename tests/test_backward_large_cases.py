"""The condition the seeds of tests/bwd_large_cases.py were chosen for, pinned on the CPU: for
every case whose oracle reference tests/test_gpu_backward_large.py applies its bar to, the fp32
oracle stays within GTOL / 3 of the fp64 oracle on every key -- so max(GTOL, 3 x gap) is GTOL and
no near-threshold shrink-mask flip of the reference itself widens it --, no input of a kink of
the fp64 forward or loss (a shrink against its threshold, the l1 residual against 0) lies within
MARGIN_SIGMAS x the fp32 rounding error of those inputs of the kink (another summation order
would take the other branch there), and no gradient the loss can reach is identically
zero (a vanishing reference checks nothing)."""
import numpy as np
import pytest

import bwd_large_cases as C


def test_case_table_is_the_issued_one():
    """The shapes and variants of every GPU test, and that each has a seed."""
    assert len(C.ORACLE_CASES) == 3 * 4 + 9 + 2 * 4
    assert len(set(C.REFERENCE_CASES)) == len(C.REFERENCE_CASES)
    for shape, variant in (C.ORACLE_CASES + C.FUSED_CASES + C.SHARD_CASES +
                           C.SPLIT_WGRAD_CASES + C.DETERMINISM_CASES):
        m, n, B, K = C.SHAPES[shape]
        assert m > 256 or n > 512, shape    # past the register-resident shapes
        assert C.SEEDS[shape][variant] > 0
    # the split-f16 weight gradient takes whole 32-column sub-chunks (wgrad_x3_fits): the
    # chunk arithmetic of make_bwd_plan at the 5 x 3 tiling of 300 x 530
    def chunks(B, tiles=15):
        bpad = (B + 15) // 16 * 16
        steps = bpad // 16
        nch = max(1, min(-(-512 // tiles), steps))
        chunk = -(-steps // nch) * 16
        return bpad, chunk, -(-bpad // chunk)
    assert chunks(1000) == (1008, 32, 32)          # 31 chunks of 32 columns and one of 16
    assert chunks(333) == (336, 16, 21)
    assert chunks(561) == (576, 32, 18)
    fits = [B for B in range(1, 562) if chunks(B)[0] % 32 == 0 and chunks(B)[1] % 32 == 0]
    assert fits[0] == 561                          # the smallest batch the split kernel takes


@pytest.mark.parametrize("shape,variant,loss", C.REFERENCE_CASES)
def test_oracle_gap_and_nonzero_reference(shape, variant, loss):
    ref, gap = C.reference(shape, variant, loss)
    none = C.unreachable(variant, C.SHAPES[shape][3], loss)
    assert none <= set(ref)
    for key, g in ref.items():
        assert np.all(np.isfinite(g)), key
        if key in none:
            assert not np.any(g), key   # outside the loss's graph: the oracle's VJP is 0
            continue
        assert gap[key] <= C.GAP_MAX, (key, gap[key])
        assert np.any(g), key
    margin, sigma = C.kink_margin(shape, variant)
    assert margin >= C.MARGIN_SIGMAS * sigma, (margin, sigma)
