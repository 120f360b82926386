"""CPU: the ViT graphs, the Attention branch of the cost model, ref.attention
and the refusals of ops.attention (the same messages as on the GPU)."""

import pytest
import torch

from defer_amd import ops
from defer_amd.models import MODELS, vit_b16, vit_s16
from defer_amd.ops import reference as ref
from defer_amd.parallel.partitioner import auto_partition, node_times


def test_vit_graphs():
    b16 = vit_b16()
    assert sum(p.numel() for p in b16.parameters()) == 86_567_656
    assert sum(p.numel() for p in vit_s16().parameters()) == 22_050_664
    assert MODELS["vit_b16"] is vit_b16 and MODELS["vit_s16"] is vit_s16
    names = [n.name for n in b16.graph.nodes]
    assert names[:11] == ["vit_b16_patch_embed", "vit_b16_embed"] + [
        f"vit_b16_block_0_{s}" for s in ("ln1", "qkv", "attn", "proj", "add_1",
                                         "ln2", "mlp_1", "mlp_2", "add_2")]
    cuts = set(b16.graph.valid_cut_points())
    adds = [n for n in names if "_add_" in n]
    assert len(adds) == 24 and cuts.issuperset(adds)
    chosen, stages = auto_partition(b16, 4)
    assert len(set(chosen)) == 3 and len(stages) == 4
    flops, _, _ = node_times(b16.graph)
    assert flops["vit_b16_block_0_attn"] == 4 * 197 * 197 * 64 * 12


def test_reference_attention_against_float64():
    n, t, h, d = 2, 17, 3, 64
    qkv = torch.randn(n, t, 3 * h * d, generator=torch.Generator().manual_seed(3))
    q, k, v = qkv.double().reshape(n, t, 3, h, d).unbind(2)
    p = torch.softmax(torch.einsum("nthd,nshd->nhts", q, k) * d ** -0.5, -1)
    want = torch.einsum("nhts,nshd->nthd", p, v).reshape(n, t, h * d)
    got = ops.attention(qkv, h)
    assert got.dtype == torch.float32 and got.shape == (n, t, h * d)
    assert (got.double() - want).abs().max() < 1e-5
    assert torch.equal(got, ref.attention(qkv, h))
    assert torch.equal(ops.attention(qkv.unsqueeze(1), h)[:, 0], got)


def test_attention_refusals_on_the_cpu():
    x = torch.zeros(2, 5, 3 * 2 * 64)
    for qkv, heads, rule in ((x, 4, "D == 64"), (x.half(), 2, "bf16 or fp32"),
                             (x.transpose(0, 1), 2, "contiguous"),
                             (x[0], 2, "rank >= 3"),
                             (x, 5, "3 * heads * D"),
                             (x[:, :0], 2, "T >= 1")):
        with pytest.raises(RuntimeError) as e:
            ops.attention(qkv, heads)
        assert rule in str(e.value)
    assert ops.attention(x[:0], 2).shape == (0, 5, 128)
