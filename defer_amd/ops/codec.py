"""Activation codec ops: fixed-rate ZFP, LZ4 and the lossless pack wire
(GPU kernels; numpy references on CPU). The ZFP wire is fixed-size per
tensor shape+rate, so pipeline recv buffers are preallocated rings
(comm.py); LZ4 and pack outputs are data-dependent and ride the
variable-size ring."""

import numpy as np
import torch

from defer_amd.ops import zfp_ref


def zfp_wire_bytes(shape, rate: int) -> int:
    return zfp_ref.wire_bytes(tuple(shape), rate)


def zfp_encode(x: torch.Tensor, rate: int, out=None) -> torch.Tensor:
    if x.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for zfp_encode")
        return m.zfp_encode(x.contiguous(), rate, out)
    w = zfp_ref.encode(x.float().numpy(), rate)
    t = torch.from_numpy(np.ascontiguousarray(w).copy())
    if out is not None:
        out.copy_(t)
        return out
    return t


def lz4_compress(x: torch.Tensor) -> torch.Tensor:
    """x: uint8 tensor -> uint8 stream (variable length). GPU tensors use
    the gfx950 HIP kernels (csrc/lz4.hip); CPU uses the bit-exact
    reference (ops/lz4_ref.py)."""
    if x.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for lz4_compress")
        return m.lz4_compress(x.contiguous().view(-1))
    from defer_amd.ops import lz4_ref

    return torch.from_numpy(
        lz4_ref.compress(x.contiguous().view(-1).numpy()).copy())


def lz4_decompress(comp: torch.Tensor, raw_len: int) -> torch.Tensor:
    if comp.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for lz4_decompress")
        return m.lz4_decompress(comp.contiguous().view(-1), raw_len)
    from defer_amd.ops import lz4_ref

    out = lz4_ref.decompress(comp.contiguous().view(-1).numpy())
    assert out.size == raw_len, (out.size, raw_len)
    return torch.from_numpy(out.copy())


def zfp_decode(wire: torch.Tensor, shape, rate: int,
               dtype=torch.float32) -> torch.Tensor:
    if wire.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for zfp_decode")
        return m.zfp_decode(wire, list(shape), rate,
                            dtype == torch.bfloat16)
    a = zfp_ref.decode(wire.numpy(), tuple(shape), rate)
    return torch.from_numpy(a).to(dtype)


# ---- lossless wire (csrc/pack.hip on GPU, ops/pack_ref.py on CPU) --------

def _pack_bits(dtype) -> int:
    if dtype == torch.bfloat16:
        return 16
    if dtype == torch.float32:
        return 32
    raise TypeError(
        f"the lossless wire packs bf16 or fp32 tensors, got {dtype}")


def pack_wire_bytes_max(shape, dtype) -> int:
    """Worst-case lossless wire size for a tensor of this shape/dtype."""
    from defer_amd.ops import pack_ref

    numel = 1
    for d in tuple(shape):
        numel *= int(d)
    return pack_ref.wire_bytes_max(numel, _pack_bits(dtype))


def pack_encode(x: torch.Tensor) -> torch.Tensor:
    """x: bf16 or fp32 tensor -> exact-size uint8 wire from which
    pack_decode rebuilds every bit pattern."""
    bits = _pack_bits(x.dtype)
    if x.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for pack_encode")
        return m.pack_encode(x.contiguous())
    from defer_amd.ops import pack_ref

    xc = x.detach().contiguous()
    if bits == 16:
        a = xc.view(torch.int16).numpy().view(np.uint16)
    else:
        a = xc.view(torch.int32).numpy().view(np.uint32)
    return torch.from_numpy(pack_ref.encode(a))


def pack_decode(wire: torch.Tensor, shape,
                dtype=torch.bfloat16) -> torch.Tensor:
    bits = _pack_bits(dtype)
    if wire.is_cuda:
        from defer_amd import ops as _ops

        m = _ops._load_hip()
        if m is None:
            raise RuntimeError("HIP extension missing for pack_decode")
        return m.pack_decode(wire.contiguous(), list(shape), bits == 16)
    from defer_amd.ops import pack_ref

    w = wire.contiguous().view(-1).numpy()
    if bits == 16:
        a = pack_ref.decode(w, tuple(shape), np.uint16)
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    a = pack_ref.decode(w, tuple(shape), np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).view(torch.float32)
