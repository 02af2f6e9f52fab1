// The attention launch plan: the one description of how launch_attention lays a shape's blocks over the grid -- the
// key-split policy, the launch-index -> (block, key-range part) map and the key-tile range of a part.  Plain C++17, no
// HIP calls: read by the launcher and by both kernels (kernels/attention.hip: attn2_kernel, attn_kh_kernel take their
// block from attn_block_of), by the host emulation (tests/host/kernel_emul.cpp) and, through the self-test entries, by
// the CPU tests (tests/test_attn_plan_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)  // (__forceinline__ spelled out: this header does not need hip_runtime.h before it)
#define ACEMI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ACEMI_HD inline
#endif

namespace acemi {

constexpr int ATTN_D = 128;  // head dimension
constexpr int ATTN_KT = 64;  // keys per tile

// What the environment sets (kernels/attention.hip reads it once per process), plus the CU count.
struct AttnPolicy {
    int ksplit_mode;  // ACE_MI_ATTN_KSPLIT: 0 auto, 1 never, 2 always (where a workspace exists), 3 auto without the
                      // short-range split, 4 the short-range split whatever the grid
    int tail;         // ACE_MI_ATTN_TAIL_SPLIT: 1 = tail split (default), 0 = every block split
    int tail_min;     // ACE_MI_ATTN_TAIL_MIN: see attn_plan (default 16 = never)
    int xcd_order;    // ACE_MI_ATTN_XCD_ORDER: 1 = XCD-aware block order (default), 0 = plain order (A/B measurements)
    int kh;           // ACE_MI_ATTN_KH: -1 the rule of attn_plan, 0 attn2 always, 1 attn_kh_kernel always
    int n_cu;
};
constexpr AttnPolicy attn_policy_default(int n_cu) { return {0, 1, 16, 1, -1, n_cu}; }
constexpr AttnPolicy ATTN_POLICY_UNSET = {-1, -1, -1, -1, -1, -1};
// `base` with every field of `over` that is not -1 in its place (the tests' override of a process's policy)
constexpr AttnPolicy attn_policy_with(const AttnPolicy& base, const AttnPolicy& over) {
    return {over.ksplit_mode >= 0 ? over.ksplit_mode : base.ksplit_mode,
            over.tail >= 0 ? over.tail : base.tail,
            over.tail_min >= 0 ? over.tail_min : base.tail_min,
            over.xcd_order >= 0 ? over.xcd_order : base.xcd_order,
            over.kh >= 0 ? over.kh : base.kh,
            over.n_cu >= 0 ? over.n_cu : base.n_cu};
}

// What the rules read from AttnArgs.
struct AttnShape {
    int B, Hq, Hkv, nq, nk, window;
    bool causal;
    bool has_part;  // a key-split workspace exists (AttnArgs::part)
    bool split, pv_split, f8;
    bool out_f32;
};

enum class AttnKernel : int { Attn2 = 0, AttnKh = 1 };
enum class AttnMerge : int { None = 0, Uniform2 = 1, Uniform4 = 2, Tail = 3 };

struct AttnPlan {
    int ksplit, split_from, xcd_order;  // -> AttnArgs
    int n_blk;                          // logical blocks (item, kv head, query tile)
    unsigned grid;                      // workgroups of the main launch
    AttnKernel kernel;
    AttnMerge merge;
    unsigned merge_grid;  // workgroups of attn_merge_kernel (8 rows each); 0 without a merge
};

ACEMI_HD int attn_min(int a, int b) { return a < b ? a : b; }
ACEMI_HD int attn_max(int a, int b) { return a > b ? a : b; }

// f32 words of the key-split workspace (AttnArgs::part) for `rows` = B * nq * Hq output rows: up to four key-split
// parts, unnormalised O rows + (running max, sum) per row
inline size_t attn_part_floats(size_t rows) { return 4 * rows * (ATTN_D + 2); }

inline AttnPlan attn_plan(const AttnShape& a, const AttnPolicy& p) {
    const int rep = a.Hq / a.Hkv;
    const int qpb = 128 / rep;
    const int n_qt = (a.nq + qpb - 1) / qpb;
    AttnPlan b{};
    b.ksplit = 1;
    b.split_from = 0;
    b.xcd_order = p.xcd_order;
    const int64_t blocks = (int64_t)a.B * a.Hkv * n_qt;
    const int span = a.window > 0 ? attn_min(a.nk, qpb + 2 * a.window) : a.nk;
    const int ntiles = (span + ATTN_KT - 1) / ATTN_KT;
    {
        // a grid of fewer than ~1.6 rounds over the CUs idles a third of the chip in its last
        // round: split each block's key range in two (B = 1 at 240 s: 376 blocks -> 752)
        // (measured: full 240 s 317 -> 262 us incl. the merge; at 8 key tiles or fewer -- cross attention,
        // sliding windows -- the extra prologue and merge cost more than the round saves)
        // ACE_MI_ATTN_KSPLIT=1 never / 2 always (where a workspace exists) / 3 auto without the short-range split /
        // 4 see below / auto
        const int mode = p.ksplit_mode;
        // blocks resident per CU: one in every mode (launch_attention)
        const int per_cu = 1;
        const int64_t slots = (int64_t)p.n_cu * per_cu;
        int S = 1;
        // tail split (default; ACE_MI_ATTN_TAIL_SPLIT=0: every block split): when the whole blocks overfill one
        // round by at most half a round, run one round of whole blocks and split only the rest -- the same
        // 1 + 1/2 rounds of key tiles per CU as splitting every block, one block prologue fewer per CU, a third of
        // the rows through the merge (240 s, B = 1: 256 whole blocks + 2 x 120 halves).  ACE_MI_ATTN_TAIL_MIN: the
        // fewest key tiles per block for which it is used where every-block splitting is not (default 16 = never)
        const int64_t F = slots & ~int64_t(7);
        const bool tail_fits =
            p.tail && (mode == 0 || mode == 3) && F > 0 && blocks > F && 2 * (blocks - F) <= slots;
        if (ntiles >= 16) {
            if (blocks * 10 < slots * 16) S = 2;
        } else if (mode == 4 || (mode == 0 && blocks * 2 <= slots)) {
            // short key ranges (cross attention, sliding windows, short sequences) split too when the grid fills at
            // most half a round (ACE_MI_ATTN_KSPLIT=4: whatever the grid), while it stays within one round and every
            // part keeps >= 2 key tiles.  Round 3 (the first kernel, profiles/r03_trace_60s_*.txt) lost: 698 us +
            // 48 merges 275 us per forward against ~950 us unsplit.  With attn2 it pays: 60 s (96 blocks on 256 CUs)
            // 165.1 against 163.1-163.4 steps/s (profiles/r05/attn_ksplit_short.txt)
            while (S < 4 && blocks * 2 * S <= slots && ntiles >= 4 * S) S *= 2;
        } else if (tail_fits && ntiles >= p.tail_min) {
            S = 2;
        }
        if (a.has_part && mode == 2) b.ksplit = 2;
        else if (a.has_part && (mode == 0 || mode == 3 || mode == 4)) b.ksplit = S;
        if (tail_fits && b.ksplit == 2) b.split_from = (int)F;
        // (round 5 also built an in-kernel merge -- the last part of a group merging through an sc1 partial round
        // trip and a ticket, no merge launch: neutral at 60 s, 4 % slower lines at 240 s, profiles/r05/attn_fused_merge.txt;
        // removed from the product library in round 6)
    }
    // (f32 output, AttnShape::out_f32: the same split policy -- whole blocks write f32 rows themselves, the merges
    // write f32 rows; until round 6 every block ran in two key-range parts with a full merge, 0.84 ms per 240 s
    // step of the quantized-activation mode)
    b.n_blk = (int)blocks;
    // XCD-aware order (attn_block_of): whole multiples of 8 launch indices per range
    b.grid = b.split_from > 0 ? (unsigned)(b.split_from + 8 * ((2 * (blocks - b.split_from) + 7) / 8))
                              : (unsigned)(8 * ((blocks * b.ksplit + 7) / 8));
    // f8c kernel: attn_kh_kernel (two waves per SIMD) where a block streams >= 16 key tiles (full self-attention
    // layers; measured 240 s: full 173.3 vs 175.2 us, bs 8 1.340 vs 1.355 ms), attn2 on short ranges (cross 50.8 vs
    // 48.1 us, sliding 42.4 vs 41.4: the 8-wave prologue and the pair merge outweigh the gain), profiles/r06/attn_kh/
    const bool kh = p.kh == 1 || (p.kh < 0 && ntiles >= 16);
    b.kernel = a.split && a.pv_split && a.f8 && kh ? AttnKernel::AttnKh : AttnKernel::Attn2;
    b.merge = AttnMerge::None;
    b.merge_grid = 0;
    if (b.split_from > 0) {
        b.merge = AttnMerge::Tail;
        b.merge_grid = (unsigned)((blocks - b.split_from) * 16);  // 128 rows per split block, 8 per workgroup
    } else if (b.ksplit > 1) {
        const int64_t rows = (int64_t)a.B * a.nq * a.Hq;
        b.merge = b.ksplit == 2 ? AttnMerge::Uniform2 : AttnMerge::Uniform4;
        b.merge_grid = (unsigned)((rows + 7) / 8);
    }
    return b;
}

// The workgroup's logical block (item, kv head, query tile) and key-range part.  Uniform layout: every block in
// ksplit parts, XCD-aware order over all of them (the hardware deals launch index j to XCD j % 8; logical
// index (j % 8) * per + j / 8 gives each XCD one contiguous run, i.e. the blocks of one (item, kv head), whose
// K / V^T tiles they all stream, share one XCD's L2).  Tail split (split_from = F > 0, a multiple of 8): launch
// indices [0, F) are whole blocks 0..F-1 (one full round), the rest the two key-range halves of blocks F..n-1
// (the last, partial round split so it fills the chip), XCD-aware within each range.  valid is false for the up
// to 7 empty trailing workgroups of a range.
struct AttnBlock {
    int blk, part, parts;
    bool valid;
};
ACEMI_HD AttnBlock attn_block_of(int ksplit, int split_from, int xcd_order, int n_blk, int x) {
    auto xcd = [&](int i, int n) { return xcd_order ? (i & 7) * ((n + 7) >> 3) + (i >> 3) : i; };
    if (split_from > 0) {
        const int F = split_from;
        if (x < F) {
            const int blk = xcd(x, F);
            return {blk, 0, 1, blk < F};
        }
        const int n2 = 2 * (n_blk - F);
        const int y = xcd(x - F, n2);
        return {F + (y >> 1), y & 1, 2, y < n2};
    }
    const int n = n_blk * ksplit;
    const int y = xcd(x, n);
    return {y / ksplit, y % ksplit, ksplit, y < n};
}

// The key tiles [kt_begin, kt_begin + n) that part `part` of `parts` streams for the block of queries [q0, q0 + qpb):
// the block's tiles (those a window or the causal mask leaves visible to any of its queries) in `parts` equal runs,
// the last ones shorter or empty (n = 0).  The kernels keep these lines in their own bodies (calling
// this changed their scalar prologue and measured outside the previous build's spread); a change is made there too.
struct AttnKeyTiles {
    int kt_begin, n;
};
ACEMI_HD AttnKeyTiles attn_key_tiles(int nk, int window, bool causal, int q0, int qpb, int part, int parts) {
    int klo = 0, khi = nk;
    if (window > 0) {
        klo = attn_max(0, q0 - window);
        khi = attn_min(nk, q0 + qpb - 1 + window + 1);
    }
    if (causal) khi = attn_min(khi, q0 + qpb);
    const int n_all = attn_max(0, (khi + ATTN_KT - 1) / ATTN_KT - klo / ATTN_KT);
    const int chunk = (n_all + parts - 1) / parts;
    return {klo / ATTN_KT + part * chunk, attn_max(0, attn_min(chunk, n_all - part * chunk))};
}

}  // namespace acemi
