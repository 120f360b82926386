// Lossless activation wire for gfx950: zero-mask + exponent-offset packing
// of bf16 / fp32 bit patterns, bit-exact to the Python spec in
// defer_amd/ops/pack_ref.py (format, field layout and size formulas are
// documented there).
//
// Shape of the work: a group is 64 values = one wave, one lane per value;
// a chunk is 256 groups = one workgroup of 4 waves (64 groups per wave).
// Every field has a fixed width inside its group, so there is no serial
// bit parse in either direction.
//
// Encode is three launches, the compress / offsets / gather shape of
// lz4.hip — workgroups never wait on each other:
//   1. pack_encode_kernel  one workgroup per chunk builds the chunk's
//      records in LDS (fields OR-ed into a zeroed record with LDS atomics:
//      OR commutes, so the bytes do not depend on lane timing), scans its
//      256 lengths and writes the chunk compactly into its scratch slot
//      (worst-case stride), its len[] bytes and its total.
//   2. pack_offsets_kernel one workgroup scans the chunk totals into
//      chunk_off[] and writes the wire header.
//   3. pack_gather_kernel  moves the chunks behind the tables and writes
//      the wire size into a device int64 (the hop's size message never
//      visits the host).
// Decode is one launch: a workgroup reads its chunk_off entry, scans its
// own 256 len bytes and decodes wave-per-group.
#include "common.h"
#include "kernels.h"

#define PK_MAGIC 0x314B5044u    // "DPK1"
#define PK_CHUNK 256            // groups per chunk = threads per workgroup
#define PK_HDR 16               // header bytes
#define PK_RW(E) (3 + 2 * (E))  // largest record, words
#define PK_BATCH 8              // groups a wave has in flight (divides 64)

namespace {

struct PackGeom {
    long ngroups, nchunks;
    long len_off;       // byte offset of len[]
    long payload_off;   // byte offset of the payload words
};

__host__ __device__ inline PackGeom pack_geom(long numel) {
    PackGeom g;
    g.ngroups = (numel + WAVE - 1) / WAVE;
    g.nchunks = (g.ngroups + PK_CHUNK - 1) / PK_CHUNK;
    g.len_off = PK_HDR + 4 * (g.nchunks + 1);
    g.payload_off = g.len_off + (g.ngroups + 3) / 4 * 4;
    return g;
}

}  // namespace

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// wave-wide minimum of both 16-bit halves of v at once (v_pk_min_u16):
// one shuffle chain serves the group's emin and, complemented, its emax
__device__ __forceinline__ u32 wave_pk_min_u16(u32 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)v, d);
        v = __builtin_bit_cast(
            u32, __builtin_elementwise_min(__builtin_bit_cast(u16x2, v),
                                           __builtin_bit_cast(u16x2, o)));
    }
    return v;
}

// lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int rank_below(u64 mask) {
    return (int)__builtin_amdgcn_mbcnt_hi(
        (u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

// Inclusive scan of one value per thread over the 256-thread workgroup.
// `buf` is 256 words of LDS; returns this thread's inclusive sum, and
// buf[255] holds the total after the call.
__device__ __forceinline__ u32 block_scan256(u32 v, u32* buf) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < PK_CHUNK; d <<= 1) {
        u32 add = (t >= d) ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    return buf[t];
}

// One group (the wave's 64 patterns, `pat` per lane) -> its record at `r`,
// a zeroed LDS record; returns the record length in words (0 = no record).
// The whole wave must call it together.
template <int E>
__device__ __forceinline__ u32 encode_group(u32 pat, u32* r, int lane) {
    const bool nz = pat != 0;
    const u64 mask = __ballot(nz);
    if (mask == 0) return 0;                        // wave-uniform
    const u32 hi = (E == 16) ? pat : (pat >> 16);
    const int ex = (int)((hi >> 7) & 0xFF);
    const u32 sgn = (hi >> 15) & 1;
    // low half: ex, high half: 255 - ex; zeros are neutral (255)
    const u32 mm = wave_pk_min_u16(
        nz ? ((u32)ex | ((u32)(255 - ex) << 16)) : 0x00FF00FFu);
    const int emin = (int)(mm & 0xFFFF);
    const int emax = 255 - (int)(mm >> 16);
    const int w = 32 - __clz(emax - emin);          // bit length, 0..8
    const u64 smask = __ballot(nz && sgn);
    const int smode = smask == 0 ? 0 : (smask == mask ? 1 : 2);
    const int haslo = (E == 32) && (__ballot(nz && (pat & 0xFFFF)) != 0);
    const int cnt = __popcll(mask);
    const int F = 7 + w + (smode == 2) + 16 * haslo;    // <= E
    if (lane == 0)
        r[0] = (u32)emin | ((u32)w << 8) | ((u32)smode << 12) |
               ((u32)haslo << 14);
    if (lane == 1) r[1] = (u32)mask;
    if (lane == 2) r[2] = (u32)(mask >> 32);
    if (nz) {
        u32 field = (hi & 0x7F) | ((u32)(ex - emin) << 7);
        int top = 7 + w;
        if (smode == 2) field |= sgn << top++;
        if (haslo) field |= (pat & 0xFFFF) << top;
        const int bit = rank_below(mask) * F;
        const u64 wide = (u64)field << (bit & 31);
        u32* p = r + 3 + (bit >> 5);
        atomicOr(p, (u32)wide);
        // a non-zero spill lies inside ceil(cnt*F/32) words
        if ((u32)(wide >> 32)) atomicOr(p + 1, (u32)(wide >> 32));
    }
    return 3 + (u32)((cnt * F + 31) >> 5);
}

// ---- encode: one workgroup per chunk -------------------------------------
template <int E>
__global__ void __launch_bounds__(PK_CHUNK)
pack_encode_kernel(const void* __restrict__ xin, long numel, long ngroups,
                   u32* __restrict__ scratch, u32* __restrict__ totals,
                   u8* __restrict__ len_out) {
    constexpr int RW = PK_RW(E);
    __shared__ u32 rec[PK_CHUNK * RW];      // 35 KB (bf16) / 67 KB (fp32)
    __shared__ u32 lens[PK_CHUNK];
    __shared__ u32 scan[PK_CHUNK];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = tid >> 6;
    const long chunk = blockIdx.x;

    for (int i = tid; i < PK_CHUNK * RW; i += PK_CHUNK) rec[i] = 0;
    __syncthreads();

    // a wave's 64 groups in batches of PK_BATCH: the loads of a batch are
    // issued together, so one memory latency covers PK_BATCH groups
    for (int it0 = 0; it0 < WAVE; it0 += PK_BATCH) {
        u32 pats[PK_BATCH];
#pragma unroll
        for (int j = 0; j < PK_BATCH; ++j) {
            const long idx =
                (chunk * PK_CHUNK + wave * WAVE + it0 + j) * WAVE + lane;
            pats[j] = 0;
            if (idx < numel)
                pats[j] = (E == 16)
                              ? (u32)((const unsigned short*)xin)[idx]
                              : ((const u32*)xin)[idx];
        }
#pragma unroll
        for (int j = 0; j < PK_BATCH; ++j) {
            const int gl = wave * WAVE + it0 + j;   // group within chunk
            const u32 len = encode_group<E>(pats[j], rec + gl * RW, lane);
            if (lane == 0) lens[gl] = len;
        }
    }
    __syncthreads();

    // offsets of the chunk's records, its len[] bytes and its total
    const u32 mylen = lens[tid];
    const u32 incl = block_scan256(mylen, scan);
    const long gt = chunk * PK_CHUNK + tid;
    if (gt < (ngroups + 3) / 4 * 4)         // padding bytes are zero
        len_out[gt] = (gt < ngroups) ? (u8)mylen : (u8)0;
    if (tid == PK_CHUNK - 1) totals[chunk] = incl;
    lens[tid] = incl - mylen;               // own slot: no reader yet
    __syncthreads();

    // compact copy-out: a wave writes its records back to back
    u32* dst = scratch + chunk * (long)(PK_CHUNK * RW);
    for (int it = 0; it < WAVE; ++it) {
        const int gl = wave * WAVE + it;
        const u32 off = lens[gl];
        const u32 end = (gl == PK_CHUNK - 1) ? scan[PK_CHUNK - 1]
                                             : lens[gl + 1];
        const u32* r = rec + gl * RW;
        for (u32 j = lane; j < end - off; j += WAVE) dst[off + j] = r[j];
    }
}

// ---- offsets: one workgroup scans the chunk totals, writes the header ----
__global__ void __launch_bounds__(PK_CHUNK)
pack_offsets_kernel(const u32* __restrict__ totals, u8* __restrict__ out,
                    long nchunks, long numel, u32 ebits) {
    __shared__ u32 scan[PK_CHUNK];
    __shared__ u32 carry;
    u32* hdr = (u32*)out;
    u32* chunk_off = (u32*)(out + PK_HDR);
    const int t = threadIdx.x;
    if (t == 0) {
        hdr[0] = PK_MAGIC;
        hdr[1] = ebits;
        hdr[2] = (u32)((u64)numel & 0xFFFFFFFFu);
        hdr[3] = (u32)((u64)numel >> 32);
        chunk_off[0] = 0;
        carry = 0;
    }
    __syncthreads();
    for (long c0 = 0; c0 < nchunks; c0 += PK_CHUNK) {
        const long c = c0 + t;
        const u32 v = (c < nchunks) ? totals[c] : 0;
        const u32 incl = block_scan256(v, scan);
        if (c < nchunks) chunk_off[c + 1] = carry + incl;
        __syncthreads();
        if (t == 0) carry += scan[PK_CHUNK - 1];
        __syncthreads();
    }
}

// ---- gather: compact the chunks behind the tables, publish the size ------
__global__ void __launch_bounds__(PK_CHUNK)
pack_gather_kernel(const u32* __restrict__ scratch, u8* __restrict__ out,
                   long nchunks, long payload_off, int rec_words,
                   long long* __restrict__ size_out) {
    const u32* chunk_off = (const u32*)(out + PK_HDR);
    u32* payload = (u32*)(out + payload_off);
    if (blockIdx.x == 0 && threadIdx.x == 0 && size_out)
        *size_out = (long long)payload_off +
                    4ll * (long long)chunk_off[nchunks];
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const u32 off = chunk_off[c], end = chunk_off[c + 1];
        const u32* src = scratch + c * (long)(PK_CHUNK * rec_words);
        u32* dst = payload + off;
        for (u32 i = threadIdx.x; i < end - off; i += PK_CHUNK)
            dst[i] = src[i];
    }
}

// ---- decode: one workgroup per chunk -------------------------------------
// payload_words bounds every record read, so a truncated or foreign wire
// decodes to zeros instead of reading past the buffer.
template <int E>
__global__ void __launch_bounds__(PK_CHUNK)
pack_decode_kernel(const u8* __restrict__ wire, void* __restrict__ yout,
                   long numel, long ngroups, long nchunks,
                   long payload_words) {
    __shared__ u32 scan[PK_CHUNK];
    __shared__ u32 offs[PK_CHUNK];
    __shared__ u32 lens[PK_CHUNK];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = tid >> 6;
    const long chunk = blockIdx.x;
    const PackGeom geo = pack_geom(numel);
    const u32* chunk_off = (const u32*)(wire + PK_HDR);
    const u8* lenp = wire + geo.len_off;
    const u32* payload = (const u32*)(wire + geo.payload_off);

    const long gt = chunk * PK_CHUNK + tid;
    const u32 mylen = (gt < ngroups) ? (u32)lenp[gt] : 0;
    const u32 incl = block_scan256(mylen, scan);
    offs[tid] = incl - mylen;
    lens[tid] = mylen;
    __syncthreads();
    const long base = (long)chunk_off[chunk];

    // a wave's 64 groups in batches of PK_BATCH, in three phases, so that
    // the two dependent loads of a group (header, then field words) each
    // cost one memory latency per batch. Groups past ngroups have length
    // 0 here and store nothing (idx >= numel).
    for (int it0 = 0; it0 < WAVE; it0 += PK_BATCH) {
        const u32* recs[PK_BATCH];
        u32 rlen[PK_BATCH], hdrs[PK_BATCH];
        u64 masks[PK_BATCH];
#pragma unroll
        for (int j = 0; j < PK_BATCH; ++j) {
            const int gl = wave * WAVE + it0 + j;
            const u32 len = lens[gl];
            const long roff = base + (long)offs[gl];
            const bool ok = len >= 3 && roff + (long)len <= payload_words;
            recs[j] = payload + (ok ? roff : 0);
            rlen[j] = ok ? len : 0;
            hdrs[j] = 0;
            masks[j] = 0;
            if (ok) {
                hdrs[j] = recs[j][0];
                masks[j] = (u64)recs[j][1] | ((u64)recs[j][2] << 32);
            }
        }
        u64 wides[PK_BATCH];
#pragma unroll
        for (int j = 0; j < PK_BATCH; ++j) {
            const u32 hdr = hdrs[j];
            const int F = 7 + (int)((hdr >> 8) & 0xF) +
                          (((hdr >> 12) & 3) == 2) +
                          ((E == 32) ? 16 * (int)((hdr >> 14) & 1) : 0);
            const int bit = rank_below(masks[j]) * F;
            const u32 wi = 3 + (u32)(bit >> 5);
            wides[j] = 0;
            if (((masks[j] >> lane) & 1) && F <= 32 && wi < rlen[j]) {
                u64 wide = recs[j][wi];
                if ((bit & 31) + F > 32 && wi + 1 < rlen[j])
                    wide |= (u64)recs[j][wi + 1] << 32;
                wides[j] = wide >> (bit & 31);
            }
        }
#pragma unroll
        for (int j = 0; j < PK_BATCH; ++j) {
            const u32 hdr = hdrs[j];
            const int emin = (int)(hdr & 0xFF);
            const int w = (int)((hdr >> 8) & 0xF);
            const int smode = (int)((hdr >> 12) & 3);
            const int haslo = (E == 32) ? (int)((hdr >> 14) & 1) : 0;
            const int F = 7 + w + (smode == 2) + 16 * haslo;
            u32 pat = 0;
            if (((masks[j] >> lane) & 1) && F <= 32) {
                const u32 field = (u32)wides[j] & (u32)((1ull << F) - 1);
                const u32 ex = ((field >> 7) & ((1u << w) - 1)) + (u32)emin;
                int top = 7 + w;
                u32 sgn = (smode == 1);
                if (smode == 2) sgn = (field >> top++) & 1;
                const u32 hi = (field & 0x7F) | ((ex & 0xFF) << 7) |
                               (sgn << 15);
                if (E == 16)
                    pat = hi;
                else
                    pat = (hi << 16) |
                          (haslo ? ((field >> top) & 0xFFFF) : 0u);
            }
            const long idx =
                (chunk * PK_CHUNK + wave * WAVE + it0 + j) * WAVE + lane;
            if (idx < numel) {
                if (E == 16)
                    ((unsigned short*)yout)[idx] = (unsigned short)pat;
                else
                    ((u32*)yout)[idx] = pat;
            }
        }
    }
}

// ---------------------------------------------------------------------------
namespace defer_hip {

long pack_table_bytes(long numel) { return pack_geom(numel).payload_off; }

long pack_wire_bytes_max(long numel, int elem_bits) {
    PackGeom g = pack_geom(numel);
    return g.payload_off + 4 * g.ngroups * (long)PK_RW(elem_bits);
}

long pack_scratch_bytes(long numel, int elem_bits) {
    PackGeom g = pack_geom(numel);
    // per-chunk slots at worst-case stride, then the chunk totals
    return g.nchunks * (long)PK_CHUNK * PK_RW(elem_bits) * 4 +
           g.nchunks * 4;
}

void launch_pack_encode(const void* x, long numel, bool bf16_in,
                        void* scratch, void* out, void* size_out,
                        hipStream_t s) {
    PackGeom g = pack_geom(numel);
    if (g.nchunks <= 0) return;
    const int E = bf16_in ? 16 : 32;
    u32* scr = (u32*)scratch;
    u32* totals = scr + g.nchunks * (long)PK_CHUNK * PK_RW(E);
    u8* o = (u8*)out;
    if (bf16_in)
        hipLaunchKernelGGL(pack_encode_kernel<16>, dim3(g.nchunks),
                           dim3(PK_CHUNK), 0, s, x, numel, g.ngroups, scr,
                           totals, o + g.len_off);
    else
        hipLaunchKernelGGL(pack_encode_kernel<32>, dim3(g.nchunks),
                           dim3(PK_CHUNK), 0, s, x, numel, g.ngroups, scr,
                           totals, o + g.len_off);
    hipLaunchKernelGGL(pack_offsets_kernel, dim3(1), dim3(PK_CHUNK), 0, s,
                       totals, o, g.nchunks, numel, (u32)E);
    int gather_grid = g.nchunks < 4096 ? (int)g.nchunks : 4096;
    hipLaunchKernelGGL(pack_gather_kernel, dim3(gather_grid),
                       dim3(PK_CHUNK), 0, s, scr, o, g.nchunks,
                       g.payload_off, PK_RW(E), (long long*)size_out);
}

void launch_pack_decode(const void* wire, long wire_bytes, void* y,
                        long numel, bool bf16_out, hipStream_t s) {
    PackGeom g = pack_geom(numel);
    if (g.nchunks <= 0) return;
    const long payload_words = (wire_bytes - g.payload_off) / 4;
    if (bf16_out)
        hipLaunchKernelGGL(pack_decode_kernel<16>, dim3(g.nchunks),
                           dim3(PK_CHUNK), 0, s, (const u8*)wire, y, numel,
                           g.ngroups, g.nchunks, payload_words);
    else
        hipLaunchKernelGGL(pack_decode_kernel<32>, dim3(g.nchunks),
                           dim3(PK_CHUNK), 0, s, (const u8*)wire, y, numel,
                           g.ngroups, g.nchunks, payload_words);
}

}  // namespace defer_hip
