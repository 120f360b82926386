"""CPU: the Swin graphs, ref.window_attention against float64, the refusals
of ops.window_attention (the same messages as on the GPU) and the bf16
kernel's work split."""

import pytest
import torch

from defer_amd import ops
from defer_amd.models import MODELS, swin_b, swin_s, swin_t
from defer_amd.models.layers import WindowAttention
from defer_amd.ops import reference as ref
from defer_amd.parallel.partitioner import auto_partition, node_times
from test_window_attention_gpu import _random_case, _winatt64


@pytest.mark.parametrize("make,params,blocks", [(swin_t, 28_288_354, 12),
                                                (swin_s, 49_606_258, 24),
                                                (swin_b, 87_768_224, 24)])
def test_swin_graphs(make, params, blocks):
    model, name = make(), make.__name__
    assert sum(p.numel() for p in model.parameters()) == params
    assert MODELS[name] is make
    names = [n.name for n in model.graph.nodes]
    block = ("ln1", "qkv", "attn", "proj", "add_1", "ln2", "mlp_1", "mlp_2",
             "add_2")
    assert names[:11] == [f"{name}_patch_embed", f"{name}_patch_layernorm"] + [
        f"{name}_stage_0_block_0_{s}" for s in block]
    assert names[20:23] == [f"{name}_merge_1_{s}"
                            for s in ("gather", "ln", "reduce")]
    adds = [n for n in names if "_add_" in n]
    assert len(adds) == 2 * blocks
    assert set(model.graph.valid_cut_points()).issuperset(adds)
    # odd blocks shift by half a window, except where the map is the window
    for n in model.graph.nodes:
        if isinstance(n.layer, WindowAttention):
            s, b = (int(v) for v in n.name.split("_")[3:6:2])
            assert n.layer.shift == (3 if b % 2 and s < 3 else 0), n.name


def test_swin_cost_model_and_partition():
    model = swin_t()
    chosen, stages = auto_partition(model, 4)
    assert len(set(chosen)) == 3 and len(stages) == 4
    flops, out_bytes, _ = node_times(model.graph)
    assert flops["swin_t_stage_0_block_1_attn"] == 4 * 49 * 49 * 32 * 3 * 64
    assert out_bytes["swin_t_merge_1_gather"] == 28 * 28 * 384 * 2


@pytest.mark.parametrize("case", [(6, 6, 3, 1, 1, 3), (14, 21, 7, 3, 2, 3)],
                         ids=str)
def test_reference_window_attention_against_float64(case):
    h, w, s = case[5], case[2], case[3]
    qkv, table = _random_case(*case, 0)
    want, _ = _winatt64(qkv, table, h, w, s)
    got = ops.window_attention(qkv, table, h, w, s)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert (got.double() - want).abs().max() < 1e-5
    assert torch.equal(got, ref.window_attention(qkv, table, h, w, s))


def test_window_attention_and_patch_merge_refusals_on_the_cpu():
    x, t = torch.zeros(2, 6, 6, 3 * 2 * 32), torch.zeros(25, 2)
    for qkv, tab, heads, w, s, rule in (
            (x.half(), t.half(), 2, 3, 0, "bf16 or fp32"),
            (x.transpose(1, 2), t, 2, 3, 0, "contiguous"),
            (x[0], t, 2, 3, 0, "4-D"),
            (x, t, 4, 3, 0, "3 * heads * 32"),
            (x, t, 2, 1, 0, "window^2 <= 64"),
            (x, t, 2, 9, 0, "window^2 <= 64"),
            (x, t, 2, 4, 0, "divide H and W"),
            (x, t, 2, 3, 3, "0 <= shift < window"),
            (x, t[:9], 2, 3, 0, "bias_table must be"),
            (x, t.bfloat16(), 2, 3, 0, "bias_table must be")):
        with pytest.raises(RuntimeError) as e:
            ops.window_attention(qkv, tab, heads, w, s)
        assert rule in str(e.value), rule
    assert ops.window_attention(x[:0], t, 2, 3, 1).shape == (0, 6, 6, 64)
    with pytest.raises(RuntimeError, match="must be even"):
        ops.patch_merge(torch.zeros(1, 2, 3, 8))
    assert ops.patch_merge(torch.zeros(1, 2, 4, 8)).shape == (1, 1, 2, 32)


def test_window_attention_plan():
    one = ops.window_attention_plan(1, 7, 7, 3, 7)
    assert (one["tokens"], one["groups"], one["windows"]) == (49, 4, 1)
    assert (one["pairs"], one["blocks"], one["idle_waves"]) == (3, 1, 1)
    six = ops.window_attention_plan(2, 14, 21, 3, 7)
    assert (six["windows"], six["pairs"], six["blocks"]) == (6, 36, 9)
    assert six["idle_waves"] == 0 and six["lds_bytes"] == 26624
