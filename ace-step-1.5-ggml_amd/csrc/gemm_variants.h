// The GEMM tile variants: the one description of what a variant id means, which shapes it handles, and which id
// launch_gemm picks for a shape.  Plain C++17, no HIP: read by the launchers (kernels/gemm.hip, kernels/gemm_q.hip take
// their template arguments from the rows), by the C-ABI's argument checks and by the CPU tests
// (tests/test_gemm_variants_cpu.py).
//
// A variant is a base id (a row below) + 100 * S for split-K over S = 2..4 blocks per tile (splitk_join).  The ids
// are ABI (ace_mi_gemm_variant, ACE_MI_GEMM_OVERRIDE, the tests' lists, tools/, the committed profiles): a new tile
// gets a new id, a retired one leaves a hole (17, 19), none is ever renumbered.
#pragma once
#include <cstdint>

namespace acemi {

enum class GemmFamily : int {
    None = 0,
    Tile = 1,       // gemm_kernel<BM, BN, WM, WN, .., PIPE>: depth = PIPE (0 / 1 double-buffered, 3 / 4 k-tiles in a ring)
    PingPong = 2,   // gemm8_kernel<BM>: 8 waves in two groups on a BM x 256 tile
    WarpSpec = 3,   // gemm_ws_kernel<BM, BN, .., NS>: 4 MFMA + 4 loader waves, depth = NS ring slots
    QTile = 4,      // gemm_q_kernel<BM, BN, WM, WN>: round 1's ds_write dequant
    QRing = 5,      // gemm_qr_kernel<BM, NW>: LDS-staged dequant, wn = NW waves side by side (BN = 32 NW)
    QWarpSpec = 6,  // gemm_wsq_kernel<BM, BN, .., NS>: the expansion on loader waves, depth = NS ring slots
};

struct GemmKernelSel {
    GemmFamily family;
    int bm, bn, wm, wn, depth;  // (fields a family does not have are 0)
    constexpr bool needs_n256() const { return bn == 256; }
    // the fused attention prep (EPI_QKV_PREP): one head per 128-column tile; the ping-pong and LDS-staged dequant
    // kernels also do two heads on 256 columns
    constexpr bool has_prep() const {
        return bn == 128 || ((family == GemmFamily::PingPong || family == GemmFamily::QRing) && bn == 256);
    }
};
constexpr GemmKernelSel gk_none() { return {GemmFamily::None, 0, 0, 0, 0, 0}; }
constexpr GemmKernelSel gk_tile(int bm, int bn, int wm, int wn, int pipe) { return {GemmFamily::Tile, bm, bn, wm, wn, pipe}; }
constexpr GemmKernelSel gk_pingpong(int bm) { return {GemmFamily::PingPong, bm, 256, 0, 0, 0}; }
constexpr GemmKernelSel gk_ws(int bm, int bn, int ns) { return {GemmFamily::WarpSpec, bm, bn, 0, 0, ns}; }
constexpr GemmKernelSel gk_qtile(int bm, int bn, int wm, int wn) { return {GemmFamily::QTile, bm, bn, wm, wn, 0}; }
constexpr GemmKernelSel gk_qring(int bm, int nw) { return {GemmFamily::QRing, bm, 32 * nw, 0, nw, 0}; }
constexpr GemmKernelSel gk_wsq(int bm, int bn, int ns) { return {GemmFamily::QWarpSpec, bm, bn, 0, 0, ns}; }

enum GemmVariantId : int {
    GV_128x128_P0 = 0,
    GV_128x128 = 1,
    GV_256x256 = 2,
    GV_256x128 = 3,
    GV_192x128 = 4,
    GV_192x256 = 5,
    GV_192x64 = 6,
    GV_96x128 = 7,
    GV_64x128 = 8,
    GV_64x64 = 9,
    GV_PP_256x256 = 10,
    GV_PP_192x256 = 11,
    GV_64x64_RING4 = 12,
    GV_64x128_RING3 = 13,
    GV_96x128_RING3 = 14,
    GV_128x128_RING3 = 15,
    GV_192x128_W8 = 16,
    GV_WS_192x128 = 18,
    GV_QR_192x128 = 20,
    GV_QR_192x256 = 21,
    GV_QR_128x128 = 22,
    GV_QR_64x128 = 23,
    GV_QR_256x128 = 24,
    GV_WSQ_192x128 = 25,
};
constexpr int GEMM_VARIANT_ID_MAX = 25, GEMM_SPLIT_MAX = 4;  // (split-K joins gather at most 4 parts: SplitKMax)
constexpr int gemm_split(int id, int S) { return id + 100 * S; }

struct GemmVariantRow {
    int id;
    const char* name;
    GemmKernelSel dense;  // 16-bit weights (None: the id is for quantized weights only)
    GemmKernelSel quant;  // Q8_0 / Q4_K / Q6_K weights (None: dense only)
    int dense_split;      // largest split-K factor the picker admits, dense weights (1 = none)
    int quant_split;      // ... quantized weights
    int prep_sibling;     // the 128-column sibling that runs the fused attention prep in its place (itself if it can)
};

constexpr GemmVariantRow GEMM_VARIANTS[] = {
    {GV_128x128_P0, "128x128, 4 waves, unpipelined (quantized: the same tile as 1)",  //
     gk_tile(128, 128, 2, 2, 0), gk_qtile(128, 128, 2, 2), 1, 1, GV_128x128_P0},
    {GV_128x128, "128x128, 4 waves, double-buffered",  //
     gk_tile(128, 128, 2, 2, 1), gk_qtile(128, 128, 2, 2), 2, 1, GV_128x128},
    {GV_256x256, "256x256, 8 waves (2x4), double-buffered",  //
     gk_tile(256, 256, 2, 4, 1), gk_qtile(256, 256, 2, 4), 1, 1, GV_256x128},
    {GV_256x128, "256x128, 4 waves, double-buffered",  //
     gk_tile(256, 128, 2, 2, 1), gk_qtile(256, 128, 2, 2), 2, 1, GV_256x128},
    {GV_192x128, "192x128, 4 waves, double-buffered",  //
     gk_tile(192, 128, 2, 2, 1), gk_qtile(192, 128, 2, 2), 2, 1, GV_192x128},
    {GV_192x256, "192x256, 8 waves (2x4), double-buffered",  //
     gk_tile(192, 256, 2, 4, 1), gk_qtile(192, 256, 2, 4), 1, 1, GV_192x128},
    {GV_192x64, "192x64, 4 waves, double-buffered (dense only)",  //
     gk_tile(192, 64, 2, 2, 1), gk_none(), 4, 1, GV_128x128},
    {GV_96x128, "96x128, 4 waves, double-buffered",  //
     gk_tile(96, 128, 2, 2, 1), gk_qtile(96, 128, 2, 2), 4, 1, GV_96x128},
    {GV_64x128, "64x128, 4 waves, double-buffered (dense only: short sequences)",  //
     gk_tile(64, 128, 2, 2, 1), gk_none(), 4, 1, GV_64x128},
    {GV_64x64, "64x64, 4 waves, double-buffered (dense only: short sequences, narrow outputs)",  //
     gk_tile(64, 64, 2, 2, 1), gk_none(), 4, 1, GV_64x128},
    {GV_PP_256x256, "256x256, 8-wave ping-pong (dense only)",  //
     gk_pingpong(256), gk_none(), 2, 1, GV_PP_256x256},
    {GV_PP_192x256, "192x256, 8-wave ping-pong (dense only)",  //
     gk_pingpong(192), gk_none(), 2, 1, GV_PP_192x256},
    {GV_64x64_RING4, "64x64, 4 waves, 4 k-tiles in the ring (dense only: cold weights at short sequences)",  //
     gk_tile(64, 64, 2, 2, 4), gk_none(), 4, 1, GV_64x128_RING3},
    {GV_64x128_RING3, "64x128, 4 waves, 3 k-tiles in the ring (dense only)",  //
     gk_tile(64, 128, 2, 2, 3), gk_none(), 4, 1, GV_64x128_RING3},
    {GV_96x128_RING3, "96x128, 4 waves, 3 k-tiles in the ring (dense only)",  //
     gk_tile(96, 128, 2, 2, 3), gk_none(), 4, 1, GV_96x128_RING3},
    // (the picker admits S <= 4 here as for the other rings; the 128x128 join gathers two parts only, SplitKMax, so
    //  315 / 415 fail at launch)
    {GV_128x128_RING3, "128x128, 4 waves, 3 k-tiles in the ring (dense only)",  //
     gk_tile(128, 128, 2, 2, 3), gk_none(), 4, 1, GV_128x128_RING3},
    // 8 waves (4 x 2) on a 192x128 tile: one tile per CU at M = 3000, N = 2048 (256 tiles), two waves per SIMD
    {GV_192x128_W8, "192x128, 8 waves (4x2), double-buffered (dense only)",  //
     gk_tile(192, 128, 4, 2, 1), gk_none(), 1, 1, GV_192x128_W8},
    // warp-specialized (4 MFMA + 4 loader waves) 192x128, three k-tiles in the ring (forced only: +18 % isolated at
    // the K = 6144 down projection, neutral in the sampling loop; a 3-stage single-role 192x128 tile (0.7x) and a
    // 4-slot ring (equal or slower) measured in round 4 are not built)
    {GV_WS_192x128, "192x128, warp-specialized, 3 k-tiles in the ring (dense only, forced only)",  //
     gk_ws(192, 128, 3), gk_none(), 1, 1, GV_WS_192x128},
    {GV_QR_192x128, "192x128, 4 waves, LDS-staged dequant (quantized only)",  //
     gk_none(), gk_qring(192, 4), 1, 1, GV_QR_192x128},
    {GV_QR_192x256, "192x256, 8 waves, LDS-staged dequant (quantized only)",  //
     gk_none(), gk_qring(192, 8), 1, 1, GV_QR_192x256},
    {GV_QR_128x128, "128x128, 4 waves, LDS-staged dequant (quantized only, forced only)",  //
     gk_none(), gk_qring(128, 4), 1, 4, GV_QR_128x128},
    {GV_QR_64x128, "64x128, 4 waves, LDS-staged dequant (quantized only, forced only)",  //
     gk_none(), gk_qring(64, 4), 1, 4, GV_QR_64x128},
    {GV_QR_256x128, "256x128, 4 waves, LDS-staged dequant (quantized only)",  //
     gk_none(), gk_qring(256, 4), 1, 1, GV_QR_256x128},
    {GV_WSQ_192x128, "192x128, warp-specialized dequant, 3 k-tiles in the ring (quantized only)",  //
     gk_none(), gk_wsq(192, 128, 3), 1, 1, GV_WSQ_192x128},
};
constexpr int GEMM_VARIANT_ROWS = sizeof(GEMM_VARIANTS) / sizeof(GEMM_VARIANTS[0]);

// the row of a base id, or nullptr (17, 19 and everything outside 0..25)
constexpr const GemmVariantRow* gemm_variant_row(int id) {
    for (int i = 0; i < GEMM_VARIANT_ROWS; ++i)
        if (GEMM_VARIANTS[i].id == id) return &GEMM_VARIANTS[i];
    return nullptr;
}

namespace gemm_variants_detail {
constexpr bool table_ok() {
    for (int i = 0; i < GEMM_VARIANT_ROWS; ++i) {
        const GemmVariantRow& r = GEMM_VARIANTS[i];
        const GemmVariantRow* sib = gemm_variant_row(r.prep_sibling);
        if (r.id < 0 || r.id > GEMM_VARIANT_ID_MAX || (i > 0 && r.id <= GEMM_VARIANTS[i - 1].id)) return false;
        if (r.dense_split < 1 || r.dense_split > GEMM_SPLIT_MAX || r.quant_split < 1 || r.quant_split > GEMM_SPLIT_MAX) return false;
        // a sibling is its own sibling and serves the weight kinds the row serves, with a kernel that has the prep
        if (!sib || sib->prep_sibling != sib->id) return false;
        if (r.dense.family != GemmFamily::None && !sib->dense.has_prep()) return false;
        if (r.quant.family != GemmFamily::None && !sib->quant.has_prep()) return false;
    }
    return true;
}
static_assert(table_ok(), "GEMM_VARIANTS: ids ascending within 0..25, split factors 1..4, prep siblings that have the prep");
}  // namespace gemm_variants_detail

// The C-ABI's check of a forced variant: -1 (automatic) or base id 0..25 + 100 * S, S <= 4.  With allow_unchecked, also
// the same + 0x10000 (self-test diagnostics: launched without gemm_variant_supports).  Holes pass here and fail at
// launch ("gemm: bad variant").
constexpr bool gemm_variant_arg_ok(int v, bool allow_unchecked = false) {
    if (v < -1 || (allow_unchecked ? v > 0x1ffff : v >= 0x10000)) return false;
    const int vb = v >= 0 ? (v & 0xffff) : v;
    return vb % 100 <= GEMM_VARIANT_ID_MAX && vb <= 424;  // (425 has always been refused: 25 has no split-K)
}

// The tile / split-K factor handles this shape and weight kind.  (An id without a row counts as the id ranges always
// counted it -- 17 and 19 as dense ids without split-K -- so that forcing one fails at launch with "bad variant" instead
// of quietly running the automatic pick.)
constexpr bool gemm_variant_supports(int v, int N, int K, bool quant) {
    const int f = v % 100, S = v / 100;
    const GemmVariantRow* r = gemm_variant_row(f);
    if (!r) return S <= 1 && !(quant && f < 20);
    const GemmKernelSel& k = quant ? r->quant : r->dense;
    if (k.family == GemmFamily::None) return false;
    if (k.needs_n256() && N % 256 != 0) return false;
    return S <= 1 || (S <= (quant ? r->quant_split : r->dense_split) && K / 64 >= 2 * S);
}

// The fused attention prep (EPI_QKV_PREP) works on whole heads (128 columns): a tile that cannot is replaced by its
// 128-column sibling.  An automatically picked split-K id drops its 100 * S first (the narrow-output split-K pick is not for
// the prep); a forced one keeps it.
constexpr int gemm_prep_sibling(int v, bool forced) {
    if (v >= 100 && !forced) v %= 100;
    const GemmVariantRow* r = gemm_variant_row(v);  // (a split-K id has no row: kept as it is)
    return r ? r->prep_sibling : v;
}

// Tile choice: measured kernel ceiling (random bf16 operands, MI355X: v1 ~950, v2 ~1120 TFLOP/s at
// large shapes) times the wave-quantization efficiency of the grid over 256 CUs (v1: 2 blocks/CU,
// 64 KiB LDS each; v2: 1 block/CU, 128 KiB) and the M-edge utilisation.
// Tile choice from the measured table (tools/gemm_bench.py on MI355X, profiles/r01_gemm_bench.log): at
// M = 3000 the 192-row tiles make 16 exact M blocks, so 192x128 fills the chip in whole rounds where
// 128x128 leaves a half round (qkv: 512 vs 768 tiles, 1036 vs 854 TFLOP/s; gate|up 1536 tiles, 900 vs
// 827); with only N = 2048 (256 tiles) the 128x128 tile's two blocks per CU win (down 779 vs 684).
// Dequant-fused: 192x256 (one block per CU, the dequant VALU spread over 8 waves) leads where it
// gives at least one tile per CU (gate|up 655 vs 525, qkv 709 vs 502), else 192x128 (down 506 vs 437).
// Dense N = 2048 at M = 3000: 96x128 makes 512 tiles, exactly two blocks per CU (down 857 vs 775,
// o / cross 662 vs 569).
inline double gemm_m_edge(int M, int bm) { return (double)M / (double)(((M + bm - 1) / bm) * bm); }

// Quantized weights: the LDS-staged dequant kernel (gemm_qr_kernel, variants 20-24 [+ 100 S]); the round-1
// ds_write dequant kernel (gemm_q_kernel, 0-7) only when forced.  Long sequences: 192-row tiles (8 waves where
// N % 256 == 0 leaves a full round of 256-column tiles); short ones: 128 / 64-row tiles, split over K until
// the grid covers the 256 CUs.
inline int gemm_pick_auto_q(int M, int N, int K, int fmt) {
    const int64_t mb192 = (M + 191) / 192;
    (void)fmt;
    if (M > 1024) {
        // M = 3000 (tools/wsq_bench.py, profiles/r05/wsq/): gate|up / qkv on the 8-wave register-dequant tile (21),
        // the N = 2048 projections on the warp-specialized tile (25: the expansion on loader waves; down 662 vs 539,
        // o 560 vs 451 TFLOP/s for the 4-wave register-dequant tile)
        if (N > 2048 && N % 256 == 0 && mb192 * (N / 256) >= 256) return GV_QR_192x256;
        return GV_WSQ_192x128;
    }
    // Short sequences: round 1's LDS-dequant kernel (96 x 128).  Whole forwards through the 64 / 128-row
    // register-dequant tiles (22, 23, split or not) were not run-to-run identical (tools/diag_det.py, round 3;
    // every kernel-level test of them passes, the attention-prep epilogue is the one path those tests do not
    // reach) -- forced only.
    (void)K;
    return GV_96x128;
}

// The automatic pick for a shape (before the prep sibling step).  The rules are the record of the in-loop A/B
// measurements named beside them; their order matters.
inline int gemm_pick_auto(int M, int N, int K, bool quant, int fmt) {
    const int64_t mb192 = (M + 191) / 192;
    const bool edge_ok = gemm_m_edge(M, 192) >= gemm_m_edge(M, 128) - 0.02;
    if (quant) return gemm_pick_auto_q(M, N, K, fmt);
    // (a skinny weight-stream kernel for M <= 128 ran the 10 s block linears 2x slower than the tiles below --
    // every 16-column workgroup re-read all of A with 16-byte row-scattered loads -- and was removed in round 4)
    // 8-wave ping-pong tiles for batched sequences (tools/gemm_msweep.py on MI355X, TFLOP/s): M = 12000 gate|up
    // 1011 (256x256) vs 941 (v2), qkv 933 vs 902, down 922 (192x256) vs 818, o 814 vs 786; M = 24000 gate|up
    // 1089 vs 1016, qkv 941 vs 897, down 955 vs 915, o 767 (v2) vs 724; M = 6000 down 921 (192x256) vs 853.
    // At M = 3000 the 4-wave tiles stay ahead (their second block per CU hides prologue and epilogue).
    // narrow outputs (proj_out: N = 128 at M = 3000 -- 16 tiles of 192 rows on a 256-CU chip, 28 TFLOP/s):
    // 64x64 tiles (94 workgroups).  Not split over K: the summation order then stays the one every other tile
    // (and the dequant-fused kernels) uses, which the staged == fused test relies on
    if (N <= 128 && M >= 512) return GV_64x64;
    // 600 s single sequences (M = 7500) and similar, 6800 <= M < 8192: the 256x256 ping-pong tiles (one round of
    // 240 tiles for the N = 2048 projections) and the 8-wave 192x128 tiles for qkv.  Measured in the sampling loop
    // (bench.py --seconds 600, same-box A/B against the previous picks, profiles/r03_pick_ab_600s/): 29.75 -> 33.25
    // steps/s.  The isolated-GEMM sweep (profiles/r03_msweep_v16_*.jsonl) also favoured the 192x128 8-wave tiles at
    // M = 4500..12000, but inside the loop (cold weights, fresh activations) they were neutral at M = 6000 and 2 %
    // slower at M = 12000 (profiles/r03_bs_ab/), so the picks below 6800 and from 8192 stay as they were.
    if (M >= 6800 && M < 8192) {
        if (N <= 2048 && N % 256 == 0) return GV_PP_256x256;
        // qkv (N = 4096) on the 192x256 ping-pong tile with the fused prep: 26.94 steps/s at 600 s against 26.43-26.59
        // for the 8-wave 192x128 tile (profiles/r05/pick_inloop_600s/); o / down / gate|up stay (192x256: 25.2 / 25.3 / 26.2)
        if (N == 4096 && N % 256 == 0) return GV_PP_192x256;
        if (N <= 4096) return GV_192x128_W8;
        if (N % 256 == 0) return GV_PP_256x256;
    }
    if (N % 256 == 0 && M >= 8192) {
        if (N >= 4096) return GV_PP_256x256;
        // (M = 24000, eight 240 s items: o / cross q / cross o on the ping-pong 256x256 tile 83.7 item-steps/s against
        //  80.9-81.0 for the 4-wave-family 256x256 and 82.9 for 192x256, profiles/r05/pick_inloop_bs8/)
        if (M >= 20000) return GV_PP_256x256;
        return GV_PP_192x256;
    }
    // two 240 s items (M = 6000): the ping-pong tiles, measured as whole bs = 2 lines through ACE_MI_GEMM_OVERRIDE
    // (profiles/r05/pick_inloop_bs2/, item-steps/s): gate|up on 256x256 (1152 tiles, 4.5 rounds) 76.1 against 72.2-72.5
    // for the 192x128 4-wave pick (192x256 75.3, 256x256 4-wave-family 73.8); then, with that pick, o / cross q / cross o
    // (N = K = 2048, 256 tiles: one round) on 192x256 78.8 against 76.0-76.5 (256x256 76.9, 256x128 72.1) and qkv on
    // 192x256 77.5 (256x256 75.9); the K = 6144 down projection stays on 192x256 (256x256 71.8, 8-wave 192x128 72.3)
    if (N % 256 == 0 && M >= 5000 && M < 6800) return N >= 8192 ? GV_PP_256x256 : GV_PP_192x256;
    if (N % 256 == 0 && M >= 4500 && N <= 2048 && K >= 4096) return GV_PP_192x256;
    if (edge_ok && mb192 * (N / 128) >= 384) return GV_192x128;
    // short sequences (60 s: M = 750): too few 96-row tiles to cover the CUs -> 64-row tiles, and
    // 64x64 when even those leave CUs idle (M = 750: N = 2048 projections 273-337 -> 364-453 TFLOP/s,
    // qkv 519 -> 567, tools/gemm_small_m.py)
    // split-K (tools/gemm_msweep.py, MI355X): only the K = 6144 down projection between the short and the
    // full-length tiles gains (M = 1500: 96x128 over 2 parts 722 vs 637 TFLOP/s for 64x128); elsewhere the
    // join's device-coherent partial round trip (~3-4 us after the main loop) costs more than the fuller grid
    // (and at 60 s, M = 750: 163.4 steps/s against 158.5-159.4 for the 64x128 3-stage split-K pick,
    //  profiles/r05/pick_inloop_60s/)
    if (N <= 2048 && K >= 4096 && M >= 600 && M < 2000) return gemm_split(GV_96x128, 2);
    const int64_t mb96 = (M + 95) / 96, mb64 = (M + 63) / 64;
    // Short sequences read every weight cold (each layer's weights were last touched one step earlier), so the
    // picks below follow the cold-weight sweep (ACE_MI_BENCH_COLD=24, profiles/r03_msweep_cold_ns.jsonl), where
    // the multi-stage rings keep more weight tiles in flight:
    //  10 s (M = 125): gate|up 64x128 3-stage (296 vs 267 TFLOP/s for 64x64), qkv / o 64x64 4-stage (146 vs 114,
    //  76 vs 74), the K = 6144 down 64x64 4-stage over 2 K parts (126 vs 69);
    //  60 s (M = 750): qkv 96x128 (495 vs 433 for 64x128), down 64x128 3-stage over 2 K parts (387 vs 349)
    if (M <= 256) {
        if (K >= 4096) return gemm_split(GV_64x64_RING4, 2);
        return N >= 8192 ? GV_64x128_RING3 : GV_64x64_RING4;
    }
    if (K >= 4096 && mb96 * (N / 128) <= 256 && mb64 * (N / 128) < 256) return gemm_split(GV_64x128_RING3, 2);
    if (mb96 * (N / 128) <= 256) {
        if (mb96 * (N / 128) == 256) return GV_96x128;  // one full round of 96-row tiles (60 s qkv)
        return mb64 * (N / 128) >= 256 ? GV_64x128 : GV_64x64;
    }
    if (gemm_m_edge(M, 96) >= gemm_m_edge(M, 128) - 0.02) return GV_96x128;  // N = 2048: 512 tiles, two per CU
    return GV_128x128;
}

// What pick_variant answers: a forced variant (tests / micro-benchmarks; >= 0x10000: diagnostics, no support check)
// or a per-shape override (dense weights only) if it handles the shape, else the automatic pick.  A forced or
// overriding variant that does not handle the shape is ignored, not an error.
inline int gemm_resolve_variant(int forced, int override_v, int M, int N, int K, bool quant, int fmt) {
    if (forced >= 0x10000) return forced & 0xffff;
    if (forced >= 0 && gemm_variant_supports(forced, N, K, quant)) return forced;
    if (!quant && override_v >= 0 && gemm_variant_supports(override_v, N, K, quant)) return override_v;
    return gemm_pick_auto(M, N, K, quant, fmt);
}

}  // namespace acemi
