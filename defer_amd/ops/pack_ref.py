"""Lossless activation wire: zero-mask + exponent-offset packing. This
numpy file is the bit-exact spec; the gfx950 kernels in csrc/pack.hip
match it byte for byte.

Why this shape: boundary activations are post-ReLU bf16 (or fp32) —
their mantissas are noise, but about half the values are exact zeros and
the exponents of the rest cluster within a few binades. So per group of
64 values the wire keeps a non-zero bitmask and, for the non-zeros only,
the 7 bf16 mantissa bits plus the exponent as a `w`-bit offset from the
group's smallest exponent. Every field has a fixed width inside its
group: there is no serial bit stream, encode and decode are one wave
lane per value.

Input. The tensor is flattened and viewed as bit patterns of E = 16
(bf16) or 32 (fp32) bits. Patterns are never interpreted as floats: NaN,
Inf, denormals and -0.0 are ordinary patterns and round-trip exactly.

Group. 64 consecutive elements; the last group is padded with pattern 0.

Group record (u32 words; a group whose patterns are all 0 has NO record,
its length is 0). For bf16, with exp = bits 7-14, mantissa7 = bits 0-6
and sign = bit 15 of the pattern:

  word 0      header: emin  (bits 0-7)   smallest exp among the non-zeros
                      w     (bits 8-11)  bit length of emax - emin, 0..8
                      smode (bits 12-13) 0 = every non-zero has sign 0,
                                         1 = every one has sign 1,
                                         2 = a sign bit per value
                      haslo (bit 14)     fp32 only, below
  words 1-2   u64 mask, bit L set iff element L's pattern != 0
  then        ceil(cnt * F / 32) words: the k-th non-zero element
              (k = popcount of the mask below lane L) owns the F bits at
              bit offset k * F, LSB first, F = 7 + w + (smode == 2):
                  mantissa7 | (exp - emin) << 7 | sign << (7 + w)

fp32. The mask tests the full 32-bit pattern; the high 16 bits go through
exactly the bf16 field above. If any non-zero element of the group has a
non-zero low half, haslo = 1 and every field carries the 16 raw low bits
on top (F <= 32); otherwise the low halves cost nothing, so an fp32
tensor of bf16-representable values costs what its bf16 form costs.

There is no raw mode: the largest record is 3 + 2 * E words (35 for
bf16, 67 for fp32), so the worst-case expansion stays below 1.11x and a
record length in words fits a u8.

Wire (little endian):
  16-byte header: u32 MAGIC | u32 E | u64 numel
  u32 chunk_off[nchunks + 1]   word offset of each chunk's first record
                               in the payload; a chunk is 256 groups
  u8  len[ngroups]             record lengths in words, zero-padded to a
                               multiple of 4 bytes
  payload words, records in group order
A decoder workgroup needs its chunk's offset and a scan of its own 256
lengths — no global scan.
"""

import numpy as np

MAGIC = 0x314B5044          # "DPK1"
GROUP = 64
CHUNK_GROUPS = 256
HEADER_BYTES = 16

_BITLEN = np.array([int(v).bit_length() for v in range(256)], dtype=np.int64)


def _geometry(numel: int):
    ngroups = (numel + GROUP - 1) // GROUP
    nchunks = (ngroups + CHUNK_GROUPS - 1) // CHUNK_GROUPS
    return ngroups, nchunks


def max_record_words(E: int) -> int:
    return 3 + 2 * E


def table_bytes(numel: int) -> int:
    """Bytes in front of the payload: header, chunk_off[], padded len[]."""
    ngroups, nchunks = _geometry(numel)
    return HEADER_BYTES + 4 * (nchunks + 1) + (ngroups + 3) // 4 * 4


def wire_bytes_max(numel: int, E: int) -> int:
    """Worst-case wire size (every group a full-width record)."""
    assert E in (16, 32), E
    ngroups, _ = _geometry(numel)
    return table_bytes(numel) + 4 * ngroups * max_record_words(E)


def _patterns(arr):
    a = np.ascontiguousarray(arr).reshape(-1)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    if a.dtype == np.uint16:
        return a, 16
    if a.dtype == np.uint32:
        return a, 32
    raise TypeError(
        f"pack_ref: expected uint16 (bf16 patterns), uint32 or float32, "
        f"got {a.dtype}")


def _group_params(pat, E):
    """Per-group header fields and record lengths for flat patterns."""
    numel = pat.size
    ngroups, _ = _geometry(numel)
    p = np.zeros(ngroups * GROUP, dtype=np.uint32)
    p[:numel] = pat
    p = p.reshape(ngroups, GROUP)
    nz = p != 0
    hi = (p >> 16) if E == 32 else p
    exp = ((hi >> 7) & 0xFF).astype(np.int64)
    sign = (hi >> 15) & 1
    emin = np.where(nz, exp, 255).min(axis=1)
    emax = np.where(nz, exp, 0).max(axis=1)
    cnt = nz.sum(axis=1)
    any_nz = cnt > 0
    w = _BITLEN[np.where(any_nz, emax - emin, 0)]
    npos = (nz & (sign == 0)).sum(axis=1)
    smode = np.where(npos == cnt, 0, np.where(npos == 0, 1, 2))
    smode = np.where(any_nz, smode, 0)
    if E == 32:
        haslo = (nz & ((p & 0xFFFF) != 0)).any(axis=1).astype(np.int64)
    else:
        haslo = np.zeros(ngroups, dtype=np.int64)
    F = 7 + w + (smode == 2) + 16 * haslo
    lens = np.where(any_nz, 3 + (cnt * F + 31) // 32, 0)
    return p, nz, emin, w, smode, haslo, F, lens


def group_lengths(arr) -> np.ndarray:
    """Record length in words of every group (vectorised)."""
    pat, E = _patterns(arr)
    return _group_params(pat, E)[7]


def encoded_bytes(arr) -> int:
    """Exact wire size of `arr` without building the wire."""
    pat, E = _patterns(arr)
    return table_bytes(pat.size) + 4 * int(_group_params(pat, E)[7].sum())


def encode(arr) -> np.ndarray:
    """arr: uint16 (bf16 bit patterns), uint32 or float32, any shape.
    Returns the exact-size uint8 wire."""
    pat, E = _patterns(arr)
    numel = pat.size
    ngroups, nchunks = _geometry(numel)
    p, nz, emin, w, smode, haslo, F, lens = _group_params(pat, E)

    off = np.zeros(ngroups + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    assert total < 2 ** 32, "payload exceeds the u32 chunk offsets"
    payload = np.zeros(total + 1, dtype=np.uint32)  # +1: spill guard word

    has = lens > 0
    roff = off[:-1][has]
    payload[roff] = (emin[has] | (w[has] << 8) | (smode[has] << 12)
                     | (haslo[has] << 14)).astype(np.uint32)
    lane = np.arange(GROUP, dtype=np.uint64)
    mask = (nz.astype(np.uint64) << lane).sum(axis=1, dtype=np.uint64)
    payload[roff + 1] = (mask[has] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    payload[roff + 2] = (mask[has] >> np.uint64(32)).astype(np.uint32)

    # fields of the non-zero elements, in group-major (= wire) order
    gi, li = np.nonzero(nz)
    v = p[gi, li].astype(np.uint64)
    hi = (v >> np.uint64(16)) if E == 32 else v
    wg = w[gi].astype(np.uint64)
    field = (hi & np.uint64(0x7F)) | (
        (((hi >> np.uint64(7)) & np.uint64(0xFF))
         - emin[gi].astype(np.uint64)) << np.uint64(7))
    top = np.uint64(7) + wg
    per_sign = (smode[gi] == 2)
    field |= np.where(per_sign, (hi >> np.uint64(15)) & np.uint64(1),
                      np.uint64(0)) << top
    top = top + per_sign.astype(np.uint64)
    field |= np.where(haslo[gi] == 1, v & np.uint64(0xFFFF),
                      np.uint64(0)) << top
    k = (np.cumsum(nz, axis=1) - 1)[gi, li]
    bit = (off[:-1][gi] + 3) * 32 + k * F[gi]
    word = bit >> 5
    sh = (bit & 31).astype(np.uint64)
    wide = field << sh                       # F + 31 <= 63 bits
    np.bitwise_or.at(payload, word,
                     (wide & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    np.bitwise_or.at(payload, word + 1,
                     (wide >> np.uint64(32)).astype(np.uint32))
    assert payload[total] == 0

    chunk_off = off[np.minimum(np.arange(nchunks + 1) * CHUNK_GROUPS,
                               ngroups)].astype(np.uint32)
    tb = table_bytes(numel)
    wire = np.zeros(tb + 4 * total, dtype=np.uint8)
    wire[0:4] = np.array([MAGIC], dtype="<u4").view(np.uint8)
    wire[4:8] = np.array([E], dtype="<u4").view(np.uint8)
    wire[8:16] = np.array([numel], dtype="<u8").view(np.uint8)
    p0 = HEADER_BYTES
    wire[p0:p0 + 4 * (nchunks + 1)] = chunk_off.astype("<u4").view(np.uint8)
    p0 += 4 * (nchunks + 1)
    wire[p0:p0 + ngroups] = lens.astype(np.uint8)
    wire[tb:] = payload[:total].astype("<u4").view(np.uint8)
    return wire


def decode(wire, shape, dtype) -> np.ndarray:
    """wire: uint8 array from encode() (or the GPU kernels); dtype:
    np.uint16 (bf16 patterns), np.uint32 or np.float32."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint16), np.dtype(np.uint32),
                     np.dtype(np.float32)):
        raise TypeError(f"pack_ref: cannot decode to {dtype}")
    E = 16 if dtype == np.dtype(np.uint16) else 32
    wire = np.ascontiguousarray(wire, dtype=np.uint8)
    numel = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    if wire.size < HEADER_BYTES:
        raise ValueError("pack_ref: wire shorter than its header")
    magic, wire_E = (int(v) for v in wire[0:8].view("<u4"))
    wire_numel = int(wire[8:16].view("<u8")[0])
    if magic != MAGIC:
        raise ValueError(f"pack_ref: bad magic {magic:#x}")
    if wire_E != E or wire_numel != numel:
        raise ValueError(
            f"pack_ref: wire holds {wire_numel} x {wire_E}-bit patterns, "
            f"asked for {numel} x {E}-bit")
    ngroups, nchunks = _geometry(numel)
    tb = table_bytes(numel)
    p0 = HEADER_BYTES
    chunk_off = wire[p0:p0 + 4 * (nchunks + 1)].view("<u4").astype(np.int64)
    p0 += 4 * (nchunks + 1)
    lens = wire[p0:p0 + ngroups].astype(np.int64)
    off = np.zeros(ngroups + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    if wire.size != tb + 4 * total:
        raise ValueError(
            f"pack_ref: wire is {wire.size} bytes, tables say "
            f"{tb + 4 * total}")
    want_off = off[np.minimum(np.arange(nchunks + 1) * CHUNK_GROUPS,
                              ngroups)]
    if not np.array_equal(chunk_off, want_off):
        raise ValueError("pack_ref: chunk offsets disagree with lengths")
    payload = np.zeros(total + 1, dtype=np.uint32)
    payload[:total] = wire[tb:].view("<u4")

    out = np.zeros((ngroups, GROUP), dtype=np.uint32)
    has = lens > 0
    roff = off[:-1][has]
    hdr = payload[roff].astype(np.int64)
    emin = np.zeros(ngroups, dtype=np.int64)
    w = np.zeros(ngroups, dtype=np.int64)
    smode = np.zeros(ngroups, dtype=np.int64)
    haslo = np.zeros(ngroups, dtype=np.int64)
    emin[has] = hdr & 0xFF
    w[has] = (hdr >> 8) & 0xF
    smode[has] = (hdr >> 12) & 3
    haslo[has] = (hdr >> 14) & 1
    F = 7 + w + (smode == 2) + 16 * haslo
    mask = np.zeros(ngroups, dtype=np.uint64)
    mask[has] = payload[roff + 1].astype(np.uint64) | (
        payload[roff + 2].astype(np.uint64) << np.uint64(32))
    lane = np.arange(GROUP, dtype=np.uint64)
    nz = ((mask[:, None] >> lane[None, :]) & np.uint64(1)).astype(bool)

    gi, li = np.nonzero(nz)
    k = (np.cumsum(nz, axis=1) - 1)[gi, li]
    Fg = F[gi]
    bit = (off[:-1][gi] + 3) * 32 + k * Fg
    word = bit >> 5
    sh = (bit & 31).astype(np.uint64)
    wide = payload[word].astype(np.uint64) | (
        payload[word + 1].astype(np.uint64) << np.uint64(32))
    field = (wide >> sh) & ((np.uint64(1) << Fg.astype(np.uint64))
                            - np.uint64(1))
    wg = w[gi].astype(np.uint64)
    mant = field & np.uint64(0x7F)
    eoff = (field >> np.uint64(7)) & ((np.uint64(1) << wg) - np.uint64(1))
    exp = eoff + emin[gi].astype(np.uint64)
    top = np.uint64(7) + wg
    per_sign = smode[gi] == 2
    sign = np.where(per_sign, (field >> top) & np.uint64(1),
                    (smode[gi] == 1).astype(np.uint64))
    top = top + per_sign.astype(np.uint64)
    hi = mant | (exp << np.uint64(7)) | (sign << np.uint64(15))
    if E == 32:
        lo = np.where(haslo[gi] == 1, (field >> top) & np.uint64(0xFFFF),
                      np.uint64(0))
        val = (hi << np.uint64(16)) | lo
    else:
        val = hi
    out[gi, li] = val.astype(np.uint32)
    flat = out.reshape(-1)[:numel]
    if E == 16:
        return flat.astype(np.uint16).reshape(shape)
    return flat.view(dtype).reshape(shape) if dtype == np.float32 \
        else flat.reshape(shape)
