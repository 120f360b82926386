"""The --dtype flag of the command-line entry points, and the CPU branch
of the two fused 1x1 ops, which the fp32 GPU routing must leave alone."""

import os
import subprocess
import sys

import pytest
import torch

import defer_amd.ops as ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = [sys.executable, "-m", "defer_amd.node"]
STREAM = [sys.executable, os.path.join(ROOT, "examples", "stream_infer.py")]


def _run(cmd, **env):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                          cwd=ROOT, env=dict(os.environ, **env))


@pytest.mark.parametrize("cmd", [NODE, STREAM], ids=["node", "stream_infer"])
def test_help_shows_dtype(cmd):
    out = _run(cmd + ["--help"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--dtype" in out.stdout
    assert "bf16" in out.stdout and "fp32" in out.stdout


def test_node_cpu_fp32_runs_one_item():
    out = _run(NODE + ["--device", "cpu", "--dtype", "fp32", "--items", "1",
                       "--batch", "1", "--report", "1"],
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29791", WORLD_SIZE="1",
               RANK="0", LOCAL_RANK="0")
    assert out.returncode == 0, out.stderr[-2000:]
    assert "images/sec" in out.stdout


def test_stream_infer_cpu_fp32_runs_one_item():
    out = _run(STREAM + ["--device", "cpu", "--dtype", "fp32", "--items",
                         "1", "--batch", "1"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "images/sec" in out.stdout


def test_cpu_rejects_bf16():
    out = _run(STREAM + ["--device", "cpu", "--dtype", "bf16", "--items",
                         "1"])
    assert out.returncode != 0
    assert "fp32 only" in out.stderr


def test_fused_1x1_ops_on_cpu_fp32_are_the_two_call_composition():
    x = torch.randn(2, 5, 7, 32)
    w3 = torch.randn(64, 1, 1, 32) * 0.2
    w1 = torch.randn(16, 1, 1, 64) * 0.2
    s3, b3 = torch.rand(64) + 0.5, torch.randn(64) * 0.1
    s1, b1 = torch.rand(16) + 0.5, torch.randn(16) * 0.1
    res = torch.randn(2, 5, 7, 64)

    y, a2 = ops.conv1x1_chain(x, w3, s3, b3, res, "relu", w1, s1, b1,
                              "relu")
    y_ref = ops.conv2d_bn_act(x, w3, s3, b3, 1, 0, "relu", res)
    a2_ref = ops.conv2d_bn_act(y_ref, w1, s1, b1, 1, 0, "relu", None)
    assert y.dtype == torch.float32
    assert torch.equal(y, y_ref) and torch.equal(a2, a2_ref)

    ps, pb = torch.rand(32) + 0.5, torch.randn(32) * 0.1
    for os_, ob in ((None, None), (s3, b3)):
        got = ops.conv1x1_prebn(x, w3, ps, pb, os_, ob)
        z = ops.batchnorm_apply(x, ps, pb, "relu")
        want = ops.conv2d_bn_act(z, w3, None, None, 1, 0, "none", None)
        if os_ is not None:
            want = ops.batchnorm_apply(want, os_, ob, "relu")
        assert torch.equal(got, want)
