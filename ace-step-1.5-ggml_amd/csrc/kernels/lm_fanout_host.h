// Plain C++ restatement of kernels/lm_fanout.hip's launcher (launch_lm_cache_fanout of kernels.h) for a build of the
// runtime without a device compiler, as lm_sample_host.h is for token selection: included by runtime/lm.cpp alone,
// empty under hipcc.  The same index arithmetic over the same two layouts; positions [0, n) are copied row by row as
// bytes, positions [n, cap_dst) of the destination are not touched.
#pragma once

#ifndef __HIP__
#include <cstring>

#include "../kernels.h"

namespace acemi {

void launch_lm_cache_fanout(const LmFanoutArgs& a, hipStream_t) {
    lm_fanout_check(a);
    constexpr int64_t D = 128;
    for (int li = 0; li < a.layers; ++li)
        for (int d = 0; d < a.G * a.S; ++d) {
            const int g = d / a.S;
            for (int h = 0; h < a.hkv; ++h) {
                const int64_t src = (((int64_t)li * a.G + g) * a.hkv + h) * a.cap_src * D;
                const int64_t dst = (((int64_t)li * a.G * a.S + d) * a.hkv + h) * a.cap_dst * D;
                std::memcpy(a.k_dst + dst, a.k_src + src, (size_t)a.n * D * 2);
                std::memcpy(a.v_dst + dst, a.v_src + src, (size_t)a.n * D * 2);
            }
        }
    for (int d = 0; d < a.G * a.S; ++d)
        std::memcpy(a.mask_dst + (int64_t)d * a.cap_dst, a.mask_src + (int64_t)(d / a.S) * a.cap_src, (size_t)a.n * 4);
}

}  // namespace acemi
#endif  // !__HIP__
