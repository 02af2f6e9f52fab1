// Fan the KV cache of a prefilled prompt out to several sequences (runtime/lm.cpp, ace_mi_lm_fanout): the G = 1 or 2
// sequences of the source cache each become S sequences of the destination cache, destination sequence g * S + s a bit
// copy of source sequence g.  With G = 2 that puts the conditional rows at 0 .. S-1 and the unconditional rows at
// S .. 2S-1, the pairing of launch_lm_select (row s with row s + S).
//
//   source       K and V [layer][G][hkv][cap_src][128] fp16, key mask [G][cap_src] int32
//   destination  K and V [layer][G * S][hkv][cap_dst][128] fp16, key mask [G * S][cap_dst] int32
//
// Positions [0, n) are copied as 16-byte words, no arithmetic (NaN and Inf patterns survive); positions [n, cap_dst) of
// the destination are not written.  The two caches are different allocations: the sequence count sits inside the layer
// stride, so a re-layout in place would read rows another workgroup has already overwritten.
//
// One workgroup per (block of 16 positions, destination sequence, layer x kv head): 16 lanes cover the 256 bytes of one
// position's row, coalesced, for K and for V; the workgroups of layer 0, kv head 0 also copy the key mask words of their
// positions.  Runs once per request, so the grid is the plain one and nothing is tuned.
#include <hip/hip_runtime.h>

#include "../kernels.h"

namespace acemi {

namespace {

constexpr int LM_D = 128;
constexpr int FANOUT_POS = 16;  // positions per workgroup: 16 positions x 16 words = 256 threads

__global__ void __launch_bounds__(256) lm_cache_fanout_kernel(LmFanoutArgs a) {
    const int p = blockIdx.x * FANOUT_POS + (threadIdx.x >> 4), w = threadIdx.x & 15;
    if (p >= a.n) return;
    const int d = blockIdx.y, g = d / a.S;
    const int li = blockIdx.z / a.hkv, h = blockIdx.z % a.hkv;
    const int64_t src = ((((int64_t)li * a.G + g) * a.hkv + h) * a.cap_src + p) * LM_D + w * 8;
    const int64_t dst = ((((int64_t)li * a.G * a.S + d) * a.hkv + h) * a.cap_dst + p) * LM_D + w * 8;
    const uint4 k = *(const uint4*)(a.k_src + src);
    const uint4 v = *(const uint4*)(a.v_src + src);
    *(uint4*)(a.k_dst + dst) = k;
    *(uint4*)(a.v_dst + dst) = v;
    if (blockIdx.z == 0 && w == 0) a.mask_dst[(int64_t)d * a.cap_dst + p] = a.mask_src[(int64_t)g * a.cap_src + p];
}

}  // namespace

void launch_lm_cache_fanout(const LmFanoutArgs& a, hipStream_t s) {
    lm_fanout_check(a);
    const dim3 grid((unsigned)ceil_div(a.n, FANOUT_POS), (unsigned)(a.G * a.S), (unsigned)(a.layers * a.hkv));
    hipLaunchKernelGGL(lm_cache_fanout_kernel, grid, dim3(256), 0, s, a);
    ACEMI_HIP(hipGetLastError());
}

}  // namespace acemi
