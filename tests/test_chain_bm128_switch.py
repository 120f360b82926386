"""The switches of the chain kernel's 128-row tile, without a GPU:
DEFER_CHAIN_BM128 follows the convention of the other A/B switches, and
ops.conv1x1_chain checks bm on every device."""

import pytest
import torch

import defer_amd.ops as ops


def test_bad_env_mode_error_text(monkeypatch):
    monkeypatch.setenv("DEFER_CHAIN_BM128", "1")
    with pytest.raises(ValueError) as e:
        ops._env_chain_bm()
    assert str(e.value) == ("DEFER_CHAIN_BM128='1': expected unset, '0' or "
                            "'force'")


@pytest.mark.parametrize("value, bm", [(None, 0), ("0", 64), ("force", 128)])
def test_env_mode_maps_to_tile_rows(monkeypatch, value, bm):
    if value is None:
        monkeypatch.delenv("DEFER_CHAIN_BM128", raising=False)
    else:
        monkeypatch.setenv("DEFER_CHAIN_BM128", value)
    assert ops._env_chain_bm() == bm


def test_bm_is_checked_on_cpu_and_ignored_by_the_reference():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, 3, 64, generator=g).bfloat16()
    res = torch.randn(1, 3, 3, 64, generator=g).bfloat16()
    w3 = (torch.randn(64, 1, 1, 64, generator=g) * 0.1).bfloat16()
    w1 = (torch.randn(64, 1, 1, 64, generator=g) * 0.1).bfloat16()
    args = (x, w3, None, None, res, "relu", w1, None, None, "relu")
    for bad in (1, 32, 96, 256, "128"):
        with pytest.raises(ValueError):
            ops.conv1x1_chain(*args, bm=bad)
    y0, a0 = ops.conv1x1_chain(*args)
    for bm in (0, 64, 128):
        y, a = ops.conv1x1_chain(*args, bm=bm)
        assert torch.equal(y, y0) and torch.equal(a, a0)
