// Host-visible launcher API for the defer_amd gfx950 kernel library.
// Implemented in the .hip TUs; called from the torch bindings. The bf16
// conv launchers and their kernel selection are in conv_plan.h.
#pragma once

#include <hip/hip_runtime.h>

namespace defer_hip {

// bf16 pointers are passed as void* across the host boundary.
struct ConvParams {
    const void* x;      // [NB, H, W, Cin] bf16 (or [M][K] in gemm mode)
    const void* w;      // [Cout][K] bf16 (OHWI flattened)
    const float* scale; // [Cout] or null
    const float* bias;  // [Cout] or null
    const void* res;    // [M][Cout] bf16 or null
    void* out;          // [M][Cout] bf16
    const void* zbuf;   // >=16 B zeros
    int M, K, Cout;
    int NB, H, W, Cin;
    int OH, OW, R, S, stride, pad;
    // magic-multiply reciprocals (filled by launch_conv_igemm):
    // floor(n/d) = umulhi(n, ceil(2^32/d)) for n*d < 2^32.
    // The window kernels do not divide; they reuse `smul` as a
    // full-sync debug flag (ConvPlan::full_sync, DEFER_CONV_VARIANT=W,
    // forces vmcnt(0) drains every phase).
    unsigned int owmul, ohmul, cmul, smul;
    // upper bound of the ReLU epilogues (the relu kernels clamp to
    // [0, act_hi]): +inf for ReLU, which leaves every bit as it was, 6 for
    // ReLU6. Unused when the kernel has no activation.
    float act_hi;
};

void launch_pad_channels(const void* x, void* y, long rows, int C, int C8,
                         hipStream_t s);
// STEM path helpers: spatial zero-pad + weight repack to (r, run) K-order
void launch_pad2d(const void* x, void* y, int NB, int H, int W, int C,
                  int PH, int PW, int ph0, int pw0, hipStream_t s);
void launch_swin_repack_w(const void* w, void* wp, int Cout, int R,
                          int C, int Kpad, hipStream_t s);
void launch_stem_repack_w(const void* w, void* wp, int Cout, int R, int S,
                          int C, int TR, hipStream_t s);

// fused pre-activation 1x1 conv: out = relu(x*ps+pb) @ w^T
// (DenseNet BNActConv; bit-identical to bn_act -> conv GEMM mode)
void launch_gemm_prebn(const void* x, const void* w, const float* ps,
                       const float* pb, const float* os, const float* ob,
                       const void* zbuf, void* out, int M, int K,
                       int Cout, hipStream_t s);

// chained 1x1 expand + residual + act -> next 1x1 reduce (chain.hip):
//   y  = act3((x[M,K1] @ w3[N1,K1]^T) * s3 + b3 + res[M,N1])
//   a2 = act1((y @ w1[N2,N1]^T) * s1 + b1)
// both bit-identical to two GEMM-mode launch_conv_igemm calls. Returns
// the grid and the tile height it launched, blocks == 0 (nothing launched)
// when the shape has no instantiation or, with force == false, is not in
// the measured-win policy table. max_blocks caps the grid (0 = policy) so
// small M can exercise several m-tiles per block. bm picks the rows of a
// tile: 0 = the measured policy, 64, or 128 (served for K1 = N2 = 256;
// every other class runs 64 rows whatever bm says).
struct ChainLaunch { int blocks, bm; };
ChainLaunch launch_conv1x1_chain(const void* x, const void* w3,
                                 const float* s3, const float* b3,
                                 const void* res, void* y, bool relu3,
                                 const void* w1, const float* s1,
                                 const float* b1, void* a2, bool relu1,
                                 int M, int K1, int N1, int N2, bool force,
                                 int max_blocks, int bm, hipStream_t s);
// the same pair with a projected residual made inside the kernel:
//   res = bf16((xp[M,KP] @ wp[N1,KP]^T) * sp + bp)
// in place of a res tensor; bit-identical to a GEMM-mode launch_conv_igemm
// for res followed by launch_conv1x1_chain. Serves K1 = KP = N2 = 64 (the
// ResNet layer1 shortcut); without force only the measured class, N1 =
// 256. Returns the grid it launched, 0 when it launched nothing.
int launch_conv1x1_chain_proj(const void* x, const void* w3, const float* s3,
                              const float* b3, const void* xp,
                              const void* wp, const float* sp,
                              const float* bp, void* y, bool relu3,
                              const void* w1, const float* s1,
                              const float* b1, void* a2, bool relu1, int M,
                              int K1, int KP, int N1, int N2, bool force,
                              int max_blocks, hipStream_t s);

// fused stem (stem_pool.hip): 7x7/s2/p3 Cin=3 Cout=64 conv + folded BN +
// ReLU + 3x3/s2/p1 max-pool, writing only the pooled tensor; bit-identical
// to launch_pad2d + the STEM launch_conv_igemm + launch_maxpool. x is the
// raw input (the zero padding is folded into the kernel's staging) and wp
// the launch_stem_repack_w weights (TR = 24).
struct StemPoolParams {
    const void* x;      // [NB, H, W, 3] bf16
    const void* wp;     // [64][168] bf16
    const float* scale; // [64]
    const float* bias;  // [64]
    void* out;          // [NB, POH, POW, 64] bf16
    int NB, H, W;       // input dims
    int OH, OW;         // conv output dims
    int POH, POW;       // pooled output dims
    int bands, rpb;     // filled by the launcher: bands/image, rows/band
};
// true when the fused kernel covers this conv + pool class and width
bool stem_pool_supported(int Cin, int Cout, int R, int S, int stride,
                         int pad, bool relu, int pk, int ps, int pp,
                         int OH, int OW);
// max_blocks caps the grid (0 = policy) so a few blocks walk many bands.
// Returns the parameters it launched with (bands and rpb filled in).
StemPoolParams launch_stem_pool(const StemPoolParams& p, int max_blocks,
                                hipStream_t s);

void launch_bn_act(const void* x, const float* scale, const float* bias,
                   void* y, long total8, int c8, bool relu, hipStream_t s);
void launch_add_act(const void* a, const void* b, void* y, long total8,
                    bool relu, hipStream_t s);
void launch_relu(const void* x, void* y, long total8, hipStream_t s);
void launch_relu6(const void* x, void* y, long total8, hipStream_t s);
void launch_hardswish(const void* x, void* y, long total8, hipStream_t s);
// two-input NHWC channel concat (c1, c2 % 8 == 0)
void launch_cat2(const void* a, const void* b, void* y, long rows,
                 int c1, int c2, hipStream_t s);
void launch_softmax(const void* x, void* y, int rows, int cols,
                    hipStream_t s);
void launch_maxpool(const void* x, void* y, int NB, int H, int W, int C,
                    int OH, int OW, int k, int stride, int pad,
                    hipStream_t s);
void launch_avgpool(const void* x, void* y, int NB, int H, int W, int C,
                    int OH, int OW, int k, int stride, int pad,
                    hipStream_t s);
void launch_gap(const void* x, void* y, int NB, int HW, int C,
                hipStream_t s);

// ---- fp32 execution path (conv_f32.hip, ops_f32.hip) ----
// Exact-f32 implicit-GEMM conv on the f32-input MFMA:
// out = act(conv(x, w) * scale[c] + bias[c] + res). Cin % 4 == 0 and
// Cout % 4 == 0 (the bindings channel-pad odd-Cin stems); scale, bias
// and res may each be null (1, 0, none).
struct ConvF32Params {
    const float* x;     // [NB, H, W, Cin] (or [M][K] in gemm mode)
    const float* w;     // [Cout][K] (OHWI flattened)
    const float* scale; // [Cout] or null
    const float* bias;  // [Cout] or null
    const float* res;   // [M][Cout] or null
    float* out;         // [M][Cout]
    int M, K, Cout;
    int H, W, Cin;
    int OH, OW, S, stride, pad;
    int relu;           // an ACT_* of common.h, ACT_HARDSWISH included
};
// tile: 0 = heuristic, 1 = 128x128, 2 = 128x64 (A/B measurement switch)
void launch_conv_f32(const ConvF32Params& p, bool gemm_mode, int tile,
                     hipStream_t s);
void launch_pad_channels_f32(const float* x, float* y, long rows, int C,
                             int C4, hipStream_t s);

// fp32 elementwise / concat / pooling / softmax: 4 floats per lane where
// the bf16 kernels take 8 (total4 = numel / 4, c4 = C / 4)
void launch_bn_act_f32(const float* x, const float* scale, const float* bias,
                       float* y, long total4, int c4, bool relu,
                       hipStream_t s);
void launch_add_act_f32(const float* a, const float* b, float* y,
                        long total4, bool relu, hipStream_t s);
void launch_relu_f32(const float* x, float* y, long total4, hipStream_t s);
void launch_relu6_f32(const float* x, float* y, long total4, hipStream_t s);
void launch_hardswish_f32(const float* x, float* y, long total4,
                          hipStream_t s);
void launch_cat2_f32(const float* a, const float* b, float* y, long rows,
                     int c1, int c2, hipStream_t s);
void launch_softmax_f32(const float* x, float* y, int rows, int cols,
                        hipStream_t s);
void launch_maxpool_f32(const float* x, float* y, int NB, int H, int W,
                        int C, int OH, int OW, int k, int stride, int pad,
                        hipStream_t s);
void launch_avgpool_f32(const float* x, float* y, int NB, int H, int W,
                        int C, int OH, int OW, int k, int stride, int pad,
                        hipStream_t s);
void launch_gap_f32(const float* x, float* y, int NB, int HW, int C,
                    hipStream_t s);

// depthwise conv + folded BN + activation (dwconv.hip), NHWC x and [R][S][C]
// w with R == S in {3, 5}, stride in {1, 2}, 0 <= pad <= R / 2; C % 8 == 0
// (bf16) or C % 4 == 0 (fp32); scale and bias non-null fp32[C]; act is
// ACT_NONE, ACT_RELU, ACT_RELU6 or ACT_HARDSWISH. Element offsets are 64-bit.
void launch_dwconv(const void* x, const void* w, const float* scale,
                   const float* bias, void* y, int NB, int H, int W, int C,
                   int OH, int OW, int R, int stride, int pad, int act,
                   hipStream_t s);
void launch_dwconv_f32(const float* x, const float* w, const float* scale,
                       const float* bias, float* y, int NB, int H, int W,
                       int C, int OH, int OW, int R, int stride, int pad,
                       int act, hipStream_t s);

// squeeze-excite (se.hip). launch_se_gate: g[n][c] = hardsigmoid(w2 @
// act(w1 @ mean_hw(x[n]) + b1) + b2), fp32 [NB][C]; x is [NB][HW][C], w1
// [Cr][C] and w2 [C][Cr] in the compute dtype (f32 ? float : bf16), b1 and
// b2 fp32 or null; C % 8 == 0 (bf16) or C % 4 == 0 (fp32), Cr >= 1, HW >= 1,
// C + Cr <= SE_MAX_LDS_FLOATS; act is ACT_NONE or ACT_RELU.
// launch_channel_scale: y = x * g[n][c], 64-bit element offsets.
constexpr int SE_MAX_LDS_FLOATS = 8192;
void launch_se_gate(const void* x, const void* w1, const float* b1,
                    const void* w2, const float* b2, float* g, int NB,
                    int HW, int C, int Cr, int act, bool f32,
                    hipStream_t s);
void launch_channel_scale(const void* x, const float* g, void* y, long NB,
                          long HW, int C, bool f32, hipStream_t s);

// NCHW <-> NHWC conversion with an optional fp32 <-> bf16 conversion in the
// same pass (layout.hip). x is [N, C, HW] when to_nhwc, [N, HW, C]
// otherwise, and y the other one; both contiguous. fp32 -> bf16 rounds to
// nearest even. Offsets are 64-bit; N*C*HW < 2^31 is the bindings' rule.
void launch_layout(const void* x, void* y, long N, int C, long HW,
                   bool to_nhwc, bool bf16_in, bool bf16_out, hipStream_t s);

// fixed-rate ZFP-style codec (see csrc/codec.hip / ops/zfp_ref.py)
// phases: 3 = full encode; 1/2 run only the transform / serialize phase
// (perf-bisection harness for tools/codecbench.py --phases)
void launch_zfp_encode(const void* x, void* out, bool bf16_in, int d0,
                       int d1, int d2, int rate, hipStream_t s,
                       int phases = 3);
void launch_zfp_decode(const void* wire, void* y, bool bf16_out, int d0,
                       int d1, int d2, int rate, hipStream_t s);

// fp8 e4m3fn wire codec: [4-byte fp32 amax][n bytes e4m3 of x*448/amax]
// (bit-compatible with the torch fallback in parallel/comm.py)
void launch_fp8_encode(const void* x, long n, void* out, hipStream_t s);
void launch_fp8_decode(const void* wire, long n, void* y, hipStream_t s);

// LZ4-style block compressor (see csrc/lz4.hip / ops/lz4_ref.py)
long lz4_max_compressed(long n);
long lz4_scratch_bytes(long n);
void launch_lz4_compress(const void* in, long n, void* scratch, void* out,
                         hipStream_t s);
// writes the total wire length (header + payload bytes) of a stream
// produced by launch_lz4_compress into *len_out (device int64), async
void launch_lz4_wire_len(const void* out_stream, long n, void* len_out,
                         hipStream_t s);
void launch_lz4_decompress(const void* comp, void* out, long raw_len,
                           hipStream_t s);

// lossless zero-mask + exponent-offset wire (see csrc/pack.hip /
// ops/pack_ref.py); elem_bits = 16 (bf16) or 32 (fp32)
long pack_table_bytes(long numel);   // header + chunk_off[] + len[]
long pack_wire_bytes_max(long numel, int elem_bits);
long pack_scratch_bytes(long numel, int elem_bits);
// encodes numel values of x into `out` (>= pack_wire_bytes_max bytes,
// 4-byte aligned) and writes the exact wire byte count into *size_out
// (device int64, may be null); async, no host sync
void launch_pack_encode(const void* x, long numel, bool bf16_in,
                        void* scratch, void* out, void* size_out,
                        hipStream_t s);
// wire_bytes bounds the reads: records past it decode to zeros
void launch_pack_decode(const void* wire, long wire_bytes, void* y,
                        long numel, bool bf16_out, hipStream_t s);

}  // namespace defer_hip
