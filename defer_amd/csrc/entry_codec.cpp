// Torch entry points of the wire codecs: fixed-rate zfp (codec.hip), the fp8
// wire (codec.hip), lz4 (lz4.hip) and the lossless pack wire (pack.hip).
#include <cstring>

#include "entry_util.h"

namespace {

using namespace defer_bind;

std::tuple<int64_t, int64_t, int64_t> field_shape(const Tensor& t) {
    auto sz = t.sizes();
    int nd = sz.size();
    if (nd == 1) return {1, 1, sz[0]};
    if (nd == 2) return {1, sz[0], sz[1]};
    int64_t d0 = 1;
    for (int i = 0; i + 2 < nd; ++i) d0 *= sz[i];
    return {d0, sz[nd - 2], sz[nd - 1]};
}

Tensor zfp_encode(Tensor x, int64_t rate, c10::optional<Tensor> out,
                  int64_t phases = 3) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    bool bf16 = x.scalar_type() == at::kBFloat16;
    TORCH_CHECK(bf16 || x.scalar_type() == at::kFloat, "bf16/f32 only");
    auto [d0, d1, d2] = field_shape(x);
    long nb = ((d0 + 3) / 4) * ((d1 + 3) / 4) * ((d2 + 3) / 4);
    long bytes = nb * rate * 8;
    Tensor o;
    if (out) {
        TORCH_CHECK(out->numel() == bytes && out->is_contiguous()
                    && out->scalar_type() == at::kByte, "bad out buffer");
        o = *out;
    } else {
        o = at::empty({bytes},
                      x.options().dtype(at::kByte));
    }
    defer_hip::launch_zfp_encode(bptr(x), bptr_mut(o), bf16, (int)d0,
                                 (int)d1, (int)d2, (int)rate,
                                 cur_stream(), (int)phases);
    return o;
}

Tensor zfp_decode(Tensor wire, std::vector<int64_t> shape, int64_t rate,
                  bool bf16_out) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte, "bad wire");
    auto o = at::empty(shape, wire.options().dtype(
                                  bf16_out ? at::kBFloat16 : at::kFloat));
    auto [d0, d1, d2] = field_shape(o);
    defer_hip::launch_zfp_decode(bptr(wire), bptr_mut(o), bf16_out,
                                 (int)d0, (int)d1, (int)d2, (int)rate,
                                 cur_stream());
    return o;
}

// fp8 e4m3fn wire: one fused HIP path (init + atomic amax + cast, the
// scale never visits the host) replacing the torch fallback's ~5
// dispatches. Wire layout matches comm.Codec exactly.
void fp8_encode(Tensor x, Tensor out) {
    check_bf16(x, "x");
    long n = x.numel();
    TORCH_CHECK(out.is_cuda() && out.is_contiguous()
                && out.scalar_type() == at::kByte
                && out.numel() == n + 4, "bad fp8 wire buffer");
    defer_hip::launch_fp8_encode(bptr(x), n, bptr_mut(out),
                                 cur_stream());
}

Tensor fp8_decode(Tensor wire, std::vector<int64_t> shape) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte, "bad wire");
    auto y = at::empty(shape, wire.options().dtype(at::kBFloat16));
    TORCH_CHECK(y.numel() + 4 == wire.numel(), "wire/shape mismatch");
    defer_hip::launch_fp8_decode(bptr(wire), y.numel(), bptr_mut(y),
                                 cur_stream());
    return y;
}

Tensor lz4_compress(Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous()
                && x.scalar_type() == at::kByte, "x must be GPU u8 contig");
    long n = x.numel();
    TORCH_CHECK(n > 0, "empty input");
    auto scratch = at::empty({defer_hip::lz4_scratch_bytes(n)},
                             x.options());
    auto o = at::empty({defer_hip::lz4_max_compressed(n)}, x.options());
    defer_hip::launch_lz4_compress(bptr(x), n, bptr_mut(scratch),
                                   bptr_mut(o), cur_stream());
    // total compressed size = header word [2 + nblocks] (syncs the stream;
    // the hop needs the byte count on the host to post the send anyway)
    long nb = (n + 4095) / 4096;
    auto hdr_cpu = o.narrow(0, 4 * (2 + nb), 4).to(at::kCPU);
    uint32_t total;
    std::memcpy(&total, hdr_cpu.data_ptr(), 4);
    return o.narrow(0, 0, 4 * (2 + nb + 1) + (long)total);
}

// Fully async zfp+lz4 hop encode: compress `x` (u8, the ZFP wire) into
// the caller's preallocated worst-case `out` ring slot and write the
// total wire byte count into `len_out` (device int64) — no host sync.
// The hop sends `len_out` as the size message straight from the device
// and reads the host copy one item later (comm.VarP2PRing), keeping the
// sender's host loop ahead of the device (the round-1 version's
// per-item .to(kCPU) sync serialized the pipeline).
void lz4_compress_into(Tensor x, Tensor scratch, Tensor out,
                       Tensor len_out) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous()
                && x.scalar_type() == at::kByte, "x must be GPU u8 contig");
    long n = x.numel();
    TORCH_CHECK(n > 0, "empty input");
    TORCH_CHECK(scratch.numel() >= defer_hip::lz4_scratch_bytes(n)
                && scratch.is_cuda(), "scratch too small");
    TORCH_CHECK(out.numel() >= defer_hip::lz4_max_compressed(n)
                && out.is_cuda() && out.scalar_type() == at::kByte,
                "out too small");
    TORCH_CHECK(len_out.is_cuda() && len_out.numel() == 1
                && len_out.scalar_type() == at::kLong, "bad len_out");
    hipStream_t s = cur_stream();
    defer_hip::launch_lz4_compress(bptr(x), n, bptr_mut(scratch),
                                   bptr_mut(out), s);
    defer_hip::launch_lz4_wire_len(bptr(out), n, bptr_mut(len_out), s);
}

Tensor lz4_decompress(Tensor comp, int64_t raw_len) {
    TORCH_CHECK(comp.is_cuda() && comp.is_contiguous()
                && comp.scalar_type() == at::kByte, "bad comp buffer");
    TORCH_CHECK(raw_len > 0, "raw_len must be positive");
    auto o = at::empty({raw_len}, comp.options());
    defer_hip::launch_lz4_decompress(bptr(comp), bptr_mut(o), raw_len,
                                     cur_stream());
    return o;
}

// ---- lossless wire (csrc/pack.hip, spec in ops/pack_ref.py) ----
int pack_elem_bits(const Tensor& x) {
    TORCH_CHECK(x.scalar_type() == at::kBFloat16
                || x.scalar_type() == at::kFloat,
                "lossless wire packs bf16 or fp32, got ", x.scalar_type());
    return x.scalar_type() == at::kBFloat16 ? 16 : 32;
}

void pack_check_numel(long n, int bits) {
    TORCH_CHECK(n > 0, "empty input");
    // chunk_off[] holds u32 word offsets into the payload
    TORCH_CHECK(defer_hip::pack_wire_bytes_max(n, bits) / 4 < (1ll << 32),
                "tensor too large for the lossless wire's u32 offsets");
}

// Fully async lossless hop encode: pack `x` into the caller's worst-case
// `out` ring slot and write the exact wire byte count into `len_out`
// (device int64) — the same contract as lz4_compress_into. Bytes of
// `out` past the wire are left untouched.
void pack_encode_into(Tensor x, Tensor scratch, Tensor out,
                      Tensor len_out) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    int bits = pack_elem_bits(x);
    long n = x.numel();
    pack_check_numel(n, bits);
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous()
                && scratch.scalar_type() == at::kByte
                && scratch.numel() >= defer_hip::pack_scratch_bytes(n, bits)
                && (uintptr_t)scratch.data_ptr() % 4 == 0,
                "scratch too small or misaligned");
    TORCH_CHECK(out.is_cuda() && out.is_contiguous()
                && out.scalar_type() == at::kByte
                && out.numel() >= defer_hip::pack_wire_bytes_max(n, bits)
                && (uintptr_t)out.data_ptr() % 4 == 0,
                "out too small or misaligned");
    TORCH_CHECK(len_out.is_cuda() && len_out.numel() == 1
                && len_out.scalar_type() == at::kLong, "bad len_out");
    defer_hip::launch_pack_encode(bptr(x), n, bits == 16,
                                  bptr_mut(scratch), bptr_mut(out),
                                  bptr_mut(len_out), cur_stream());
}

// convenience form: exact-size wire (syncs the stream to read the size)
Tensor pack_encode(Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be GPU contig");
    int bits = pack_elem_bits(x);
    long n = x.numel();
    pack_check_numel(n, bits);
    auto bopt = x.options().dtype(at::kByte);
    auto scratch = at::empty({defer_hip::pack_scratch_bytes(n, bits)}, bopt);
    auto o = at::empty({defer_hip::pack_wire_bytes_max(n, bits)}, bopt);
    auto len = at::empty({1}, x.options().dtype(at::kLong));
    defer_hip::launch_pack_encode(bptr(x), n, bits == 16,
                                  bptr_mut(scratch), bptr_mut(o),
                                  bptr_mut(len), cur_stream());
    long total = len.item<int64_t>();
    return o.narrow(0, 0, total);
}

Tensor pack_decode(Tensor wire, std::vector<int64_t> shape, bool bf16_out) {
    TORCH_CHECK(wire.is_cuda() && wire.is_contiguous()
                && wire.scalar_type() == at::kByte
                && (uintptr_t)wire.data_ptr() % 4 == 0, "bad wire");
    auto y = at::empty(shape, wire.options().dtype(
                                  bf16_out ? at::kBFloat16 : at::kFloat));
    long n = y.numel();
    pack_check_numel(n, bf16_out ? 16 : 32);
    TORCH_CHECK(wire.numel() >= defer_hip::pack_table_bytes(n),
                "wire shorter than its tables for this shape");
    defer_hip::launch_pack_decode(bptr(wire), wire.numel(), bptr_mut(y), n,
                                  bf16_out, cur_stream());
    return y;
}

}  // namespace

void bind_codec(py::module_& m) {
    m.def("zfp_encode", &zfp_encode, py::arg("x"), py::arg("rate"),
          py::arg("out") = py::none(), py::arg("phases") = 3);
    m.def("zfp_decode", &zfp_decode);
    m.def("fp8_encode", &fp8_encode);
    m.def("fp8_decode", &fp8_decode);
    m.def("lz4_compress", &lz4_compress);
    m.def("lz4_compress_into", &lz4_compress_into);
    m.def("lz4_scratch_bytes",
          [](int64_t n) { return defer_hip::lz4_scratch_bytes(n); });
    m.def("lz4_decompress", &lz4_decompress);
    m.def("pack_scratch_bytes", [](int64_t n, int64_t bits) {
        return defer_hip::pack_scratch_bytes(n, (int)bits);
    });
    m.def("pack_wire_bytes_max", [](int64_t n, int64_t bits) {
        return defer_hip::pack_wire_bytes_max(n, (int)bits);
    });
    m.def("pack_encode_into", &pack_encode_into);
    m.def("pack_encode", &pack_encode);
    m.def("pack_decode", &pack_decode);
}
