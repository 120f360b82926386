// Kernel selection for the bf16 convolutions: which kernel family, tile
// config and grid a geometry runs. Host-only and pure (a function of the
// ConvParams geometry, the path flags and one variant letter), so the
// policy can be observed (ops.conv_plan) and tested without a GPU. The
// launchers take a plan, look the kernel up in a table and launch it.
#pragma once

#include <array>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels.h"

enum { AMODE_GEMM = 0, AMODE_CONV = 1, AMODE_RSC = 2, AMODE_STEM = 3 };

namespace defer_hip {

constexpr int CONV_BK = 64;    // K-tile of conv_igemm_kernel (BK)
constexpr int WIN_TW = 16;     // window tile width of the window kernels
// policy threshold in output tiles (docs/OPTIMIZATION_LOG.md, round 6)
constexpr int WS_POLICY_MIN_TILES = 512;

struct ConvPlan {
    enum Family { IGEMM, WIN, WS, SWIN } family = IGEMM;
    // IGEMM: conv_igemm_kernel<ACT, RES, amode, bp, BM, BN, DA, DB, WPS>
    int amode = 0, bp = 0, BM = 0, BN = 0, DA = 0, DB = 0, WPS = 0;
    // WIN: conv_win_kernel<ACT, RES, 64, TH, 256, 2>; full_sync (debug)
    // travels to the kernel in ConvParams::smul
    int TH = 0;
    bool full_sync = false;
    // SWIN: conv_swin_kernel<ACT, R, stride>; grid_x 0 = does not qualify
    int R = 0, stride = 0;
    int grid_x = 0, grid_y = 1;
    // WS: grid size and the 8x16 output tiles the busiest block walks
    int blocks = 0, tiles_per_block = 0;
};

// the kernel's template arguments after ACT, HAS_RES: the dispatch key
inline std::array<int, 7> plan_key(const ConvPlan& pl) {
    if (pl.family == ConvPlan::WIN) return {64, pl.TH, 256, 2};
    if (pl.family == ConvPlan::SWIN) return {pl.R, pl.stride};
    return {pl.amode, pl.bp, pl.BM, pl.BN, pl.DA, pl.DB, pl.WPS};
}

inline std::string to_string(const ConvPlan& pl) {
    std::string o = "family " + std::to_string(pl.family) + ", args";
    for (int k : plan_key(pl)) o += " " + std::to_string(k);
    return o + ", grid " + std::to_string(pl.grid_x) + " x " +
           std::to_string(pl.grid_y);
}

// an invariant of the policy that the dispatch table relies on: the
// combinations it excludes have no instantiation
#define CONV_PLAN_INVARIANT(pl, cond)                                     \
    if (!(cond))                                                          \
    throw std::logic_error("conv plan breaks '" #cond "': " + to_string(pl))

// DEFER_CONV_VARIANT, latched at first use; only its first letter counts.
// variants: default = measured policy; "legacy" = symmetric-depth
// policy pre-v2; "small" = force the high-occupancy small-tile
// config everywhere it is legal (experiment harness); 'w' = force the
// window kernels wherever they cover the shape; 'W' = force win AND
// full vmcnt(0) drains (debug)
inline char conv_variant() {
    static const char variant = [] {
        const char* e = getenv("DEFER_CONV_VARIANT");
        return e ? e[0] : '\0';
    }();
    return variant;
}

// TH x 16 output tiles of one image, and the window paths' padding rule:
// partial tiles are handled but waste compute; <= ~18% overhead
inline long win_tiles(const ConvParams& p, int TH) {
    return (long)((p.OH + TH - 1) / TH) * ((p.OW + WIN_TW - 1) / WIN_TW);
}
inline bool win_padding_ok(const ConvParams& p, int TH) {
    return win_tiles(p, TH) * TH * WIN_TW * 100 <= (long)p.OH * p.OW * 118;
}

// small-Cin window path: Cin padded to 8, Cout 64, R in {3,7},
// stride in {1,2}, 8x16 output tiles with <=18% padding waste;
// grid_x stays 0 when the shape does not qualify (the caller falls back)
inline ConvPlan plan_swin(const ConvParams& p, char variant) {
    ConvPlan pl;
    pl.family = ConvPlan::SWIN;
    pl.R = p.R;
    pl.stride = p.stride;
    // R==7 was implemented and dropped: the run-packed spatial-prepad
    // stem path (K=168) beats the zero-padded window K=448 at Cin=3
    if (p.Cout != 64 || p.R != 3 || !(p.stride == 1 || p.stride == 2) ||
        !win_padding_ok(p, 8))
        return pl;
    long mt2 = (long)p.NB * win_tiles(p, 8);
    const bool forced = variant == 'w' || variant == 'W';
    if (forced || mt2 >= 512) pl.grid_x = mt2 > 768 ? 768 : (int)mt2;
    return pl;
}

// conv_ws_kernel covers this geometry
inline bool conv_ws_supported(const ConvParams& p) {
    // element offsets inside one image are 32-bit in the kernel
    return p.R == 3 && p.S == 3 && p.stride == 1 && p.pad == 1 &&
           p.Cin == 64 && p.Cout == 64 && p.K == 9 * 64 && p.NB >= 1 &&
           p.H >= 1 && p.W >= 1 && p.OH == p.H && p.OW == p.W &&
           (long)p.H * p.W < (1L << 24) &&
           (long)p.NB * p.OH * p.OW < (1LL << 31);
}

// mode selects between the weight-stationary kernel (conv_ws.hip) and the
// older paths for the class it covers: 0 = the measured policy (never when
// a variant forces one of the older kernels), 1 = wherever it covers the
// shape, 2 = never. max_blocks caps that kernel's grid (0 = the 512
// resident blocks) so a few blocks walk many tiles.
inline ConvPlan plan_conv(const ConvParams& p, bool gemm_mode,
                          bool stem_mode, int ws_mode, int max_blocks,
                          char variant) {
    ConvPlan pl;
    if (ws_mode != 2 && p.M > 0 && conv_ws_supported(p)) {
        const long tiles = (long)p.NB * win_tiles(p, 8);
        // a forced DEFER_CONV_VARIANT is there to exercise the older kernels
        if (ws_mode == 1 ||
            (variant == '\0' && tiles >= WS_POLICY_MIN_TILES)) {
            // 2 blocks fit a CU, 512 on the chip; spread the rounds evenly
            // over the blocks (7168 tiles: 512 blocks x 14)
            long gx = max_blocks > 0 ? max_blocks : 512;
            if (gx > tiles) gx = tiles;
            const long rounds = (tiles + gx - 1) / gx;
            gx = (tiles + rounds - 1) / rounds;
            pl.family = ConvPlan::WS;
            pl.grid_x = pl.blocks = (int)gx;
            pl.tiles_per_block = (int)rounds;
            return pl;
        }
    }
    const int nk = (p.K + CONV_BK - 1) / CONV_BK;
    const bool bp = (nk == 1) && !stem_mode;
    const bool rsc = !gemm_mode && !stem_mode && !bp &&
                     (p.Cin % 64 == 0) && (p.R * p.S <= 32);
    const int amode = stem_mode ? AMODE_STEM
                                : gemm_mode ? AMODE_GEMM
                                            : (rsc ? AMODE_RSC
                                                   : AMODE_CONV);
    // tile selection. BN128 halves A re-staging and doubles MFMA per
    // staged byte; memory-bound small-K shapes keep the 3-deep BN64
    // pipeline. BM=64 for small-M shapes (more blocks on the 256 CUs).
    // DEFER_CONV_VARIANT=legacy reverts to the symmetric-depth policy
    // (A/B comparison harness).
    const bool legacy = variant == 'l';
    const bool force_small = variant == 's';
    const bool force_win = variant == 'w' || variant == 'W';

    // window-reuse path: 3x3/s1/p1 with TH x 16 output tiles (TH 8 or
    // 4); stages each input window once per 64-channel block instead of
    // once per (r,s) k-tile (9x less A traffic into LDS). Partial tiles
    // are handled (zero-filled windows, guarded stores) but waste
    // compute; require <= ~18% padding overhead. Cout>128 shapes
    // (56x56x256-class) stay on the BN128 RSC config: the BN64 window
    // kernel pays 2-4x the B re-staging (measured loss) and a BN128
    // window instantiation spills ~250 B/lane at this register budget.
    // Cout <= 128 only. Wider variants were all built and measured
    // slower than the BN128 RSC config they would replace: BN128 x 4
    // waves spills ~250 B/lane; BN128 x 512 threads at 4 waves/SIMD
    // spills ~200 B/lane; at 2 waves/SIMD it runs ONE 8-wave block per
    // CU and loses the cross-block epilogue overlap (b3 179 -> 211 us,
    // same failure mode as the BM256 implicit-GEMM tile).
    const bool win_ok =
        (!legacy && !force_small) && !gemm_mode && !stem_mode &&
        p.R == 3 && p.S == 3 && p.stride == 1 && p.pad == 1 &&
        (p.Cin % 64 == 0) && (p.Cout % 64 == 0) && p.Cout <= 128;
    auto win_fit = [&](int TH) {
        if (!win_padding_ok(p, TH)) return false;
        return force_win ||
               (long)p.NB * win_tiles(p, TH) * ((p.Cout + 127) / 128) >= 512;
    };
    // TH=4 measured slower than the BN128 RSC config on the 28-px
    // shapes it would serve (2x B re-staging + 14% tile waste), so the
    // default policy uses TH=8 only; TH=4 stays exercised by the forced
    // numerics harness (tools/wincheck.py)
    const int THsel = !win_ok          ? 0
                      : win_fit(8)     ? 8
                      : (force_win && win_fit(4)) ? 4
                                       : 0;
    if (THsel) {
        const int BNw = 64;
        const int mt2 = (int)((long)p.NB * win_tiles(p, THsel));
        const int nyw = p.Cout / BNw;
        int gxw = mt2;
        if ((long)mt2 * nyw > 768) {
            gxw = 768 / nyw > 0 ? 768 / nyw : 1;
            if (gxw > mt2) gxw = mt2;
        }
        pl.family = ConvPlan::WIN;
        pl.TH = THsel;
        pl.full_sync = variant == 'W';   // full-sync debug flag
        pl.grid_x = gxw;
        pl.grid_y = nyw;
        return pl;
    }
    const int mt128 = (p.M + 127) / 128;
    int BMsel, BNsel;
    const bool deepK = p.K >= 1024;
    // 1x1 convs (any stride — stride-2 projections gather via AMODE_RSC
    // but share the GEMM arithmetic shape) follow the GEMM policy.
    const bool one1 = gemm_mode || (p.R == 1 && p.S == 1 && p.pad == 0);
    // 1x1 shapes with K>=512: wide n-tile (halves A re-staging; measured
    // −10…14% on the L3/L4 1x1s; K=128/256 shapes regress with BN128 —
    // epilogue-frequency-bound — and keep BN64)
    const bool wide = (deepK || (!legacy && one1 && !bp &&
                                 p.K >= 512)) &&
                      p.Cout >= 128;
    // pure-bandwidth 1x1s (K<=256): small tiles + 3-4 blocks/CU — these
    // shapes are HBM/L3-streaming-bound (MFMA <10% busy), so occupancy
    // and independent load streams beat tile efficiency
    // measured small-tile winners besides the 1x1s: the stem paths and
    // shallow-K 3x3s at moderate M (deep-K 3x3s and the giant-M VGG
    // b1.c2 regress -2..-20% at BM64 — B-tile re-staging doubles)
    const bool small_conv =
        stem_mode || (!one1 && (p.K <= 128 ||
                                (p.K <= 576 && p.M <= 450000)));
    const bool smallgemm =
        (force_small || (!legacy && ((one1 && !wide) || small_conv))) &&
        (long)((p.M + 63) / 64) * ((p.Cout + 63) / 64) >= 768;
    // NOTE: a BM=256 x BN=128 512-thread 1-block/CU config was measured
    // for the big-M deep-K 3x3s (to halve B re-staging: the BM128 D2
    // config demands ~117 B/cyc/CU of L2 tile traffic vs ~56 available)
    // and lost 10-24% — one resident block loses the cross-block
    // epilogue/prologue overlap that two independent blocks provide.
    if (smallgemm) {
        BNsel = 64;
        BMsel = 64;
    } else if (wide) {
        BNsel = 128;
        BMsel = (mt128 * (p.Cout / 128) >= 384) ? 128 : 64;
    } else {
        BNsel = 64;
        BMsel = (mt128 * ((p.Cout + 63) / 64) >= 384) ? 128 : 64;
    }
    // underfill guard: 256 CUs want >=256 workgroups; narrow the n-tile
    // before leaving CUs idle (small-M deep-K shapes, e.g. 7x7x512)
    if (BNsel == 128 &&
        (long)((p.M + BMsel - 1) / BMsel) * ((p.Cout + 127) / 128) < 256) {
        BNsel = 64;
        BMsel = 64;
    }
    const int mtiles = (p.M + BMsel - 1) / BMsel;
    const int ny = (p.Cout + BNsel - 1) / BNsel;
    int gx = mtiles;
    const int target = smallgemm ? (bp ? 1536 : 1152) : 768;
    if ((long)mtiles * ny > target) {
        gx = target / ny > 0 ? target / ny : 1;
        if (gx > mtiles) gx = mtiles;
    }
    pl.family = ConvPlan::IGEMM;
    pl.amode = amode;
    pl.bp = bp;
    pl.BM = BMsel;
    pl.BN = BNsel;
    pl.grid_x = gx;
    pl.grid_y = ny;

    // depths (A-ring, B-ring). Measured on MI355X: symmetric depths win
    // (boundary activations are L3/L2-resident, so one to two compute
    // phases already cover the load latency and extra LDS per block
    // costs more than deeper cover buys); the asymmetric deep-A variants
    // (DEFER_CONV_VARIANT unset ... kept instantiated) lost 6-22% and
    // remain only for the B_PERSIST single-K-tile shapes where a 4-deep
    // A ring measured neutral-to-slightly-better.
    pl.WPS = 2;
    if (BMsel == 128 && BNsel == 128) {
        pl.DA = pl.DB = 2;
    } else if (BMsel == 64 && BNsel == 128) {
        pl.DA = pl.DB = 3;
    } else if (smallgemm) {
        if (bp) { pl.DA = 4; pl.DB = 2; pl.WPS = 4; }  // 40 KB LDS, 4 blk/CU
        else { pl.DA = pl.DB = 3; pl.WPS = 3; }        // 48 KB LDS, 3 blk/CU
    } else if (bp && !legacy) {                        // BN 64, BM 128 or 64
        pl.DA = 4;
        pl.DB = 2;
    } else {
        pl.DA = pl.DB = 3;
    }
    // What the dispatch table leaves out. bp: K fits one tile and it is
    // not the STEM gather; rsc asks for !bp, so bp runs GEMM or CONV only.
    CONV_PLAN_INVARIANT(pl, !pl.bp || pl.amode == AMODE_GEMM ||
                                pl.amode == AMODE_CONV);
    // BN 128 comes from `wide` alone: K >= 1024 (16 k-tiles) or !bp
    CONV_PLAN_INVARIANT(pl, pl.BN != 128 || !pl.bp);
    // the asymmetric 4,2 depths are taken only with bp, and 2,2 only by
    // the 128x128 tile
    CONV_PLAN_INVARIANT(pl, !(pl.DA == 4 && pl.DB == 2) || pl.bp);
    CONV_PLAN_INVARIANT(pl, (pl.DA == 2) == (pl.BM == 128 && pl.BN == 128));
    // the small-tile occupancy configs: 4 blocks/CU with bp, 3 without
    CONV_PLAN_INVARIANT(pl, pl.WPS == 2 || (pl.BM == 64 && pl.BN == 64 &&
                                            pl.WPS == (pl.bp ? 4 : 3)));
    return pl;
}

// Launchers: take a plan, look the kernel up, launch; a plan with no
// table row throws. launch_conv_igemm serves IGEMM, WIN and SWIN (the small-Cin
// window stem path: Cin pre-padded to 8, weights pre-repacked j-major
// zero-padded) and fills the magic-multiply reciprocals. act picks the
// instantiation: 0 = none, 1 = the ReLU clamped to ConvParams::act_hi, 2 =
// hardswish (a bool gives none / relu).
void launch_conv_igemm(const ConvParams& p, const ConvPlan& plan, int act,
                       bool has_res, hipStream_t s);
// weight-stationary window kernel (conv_ws.hip): 3x3/s1/p1 convs with
// Cin = Cout = 64 keep the whole weight tensor in registers and stage only
// input windows to LDS; bit-identical to launch_conv_igemm on the same
// ConvParams (act as in launch_conv_igemm, with or without residual).
struct ConvWsLaunch {
    int blocks;            // grid size
    int tiles_per_block;   // 8x16 output tiles the busiest block walks
};
ConvWsLaunch launch_conv_ws(const ConvParams& p, int act, bool has_res,
                            int max_blocks, hipStream_t s);

// The dispatch table, for ops.conv_plan and the tests: the template
// arguments after ACT of the kernel a plan launches (throws when the table
// has no row for it), and every row as "family: arguments".
std::string conv_kernel_args(const ConvPlan& plan, bool has_res);
std::vector<std::string> conv_table_rows();

}  // namespace defer_hip
