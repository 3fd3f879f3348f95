// vr_half.h -- f16 record volumes: a record of B IEEE binary16 bins kept packed,
// two halves per 32-bit register, and widened to float only where it is decoded.
// Used by the f16 march (vr_half.hip) and the statistics bake (vr_stats.hip).
#pragma once

#include "vr_device.h"

namespace vr {

// B halves in (B + 1) / 2 registers (B = 1: the low 16 bits of one)
template <int B>
struct RecH {
    uint32_t w[(B + 1) / 2];
};

// One record in the widest loads its size allows: 2 B one ushort, 4 B one dword,
// 8 B one dwordx2, 16 B one dwordx4, 32 / 64 B two / four dwordx4.  Records are
// aligned to min(16, 2 B) bytes (hipMalloc, or checked for an adopted buffer).
template <int B>
__device__ __forceinline__ void load_rec_h(const _Float16 *__restrict__ vol, uint64_t vidx,
                                           RecH<B> &r) {
    static_assert(B == 1 || B == 2 || B == 4 || B == 8 || B == 16 || B == 32,
                  "f16 records: 1, 2, 4, 8, 16 or 32 bins");
    const _Float16 *src = vol + vidx * (uint64_t)B;
    if constexpr (B == 1) {
        r.w[0] = *reinterpret_cast<const uint16_t *>(src);
    } else if constexpr (B == 2) {
        r.w[0] = *reinterpret_cast<const uint32_t *>(src);
    } else if constexpr (B == 4) {
        const uint2 q = *reinterpret_cast<const uint2 *>(src);
        r.w[0] = q.x; r.w[1] = q.y;
    } else {
#pragma unroll
        for (int i = 0; i < B / 8; i++) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[i];
            r.w[4 * i + 0] = q.x; r.w[4 * i + 1] = q.y; r.w[4 * i + 2] = q.z; r.w[4 * i + 3] = q.w;
        }
    }
}

__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);  // exact, subnormals kept
}

template <int B>
__device__ __forceinline__ void widen_rec(const RecH<B> &r, float (&p)[B]) {
    if constexpr (B == 1) {
        p[0] = half_bits_to_float(r.w[0]);
    } else {
#pragma unroll
        for (int i = 0; i < B / 2; i++) {
            p[2 * i] = half_bits_to_float(r.w[i] & 0xFFFFu);
            p[2 * i + 1] = half_bits_to_float(r.w[i] >> 16);
        }
    }
}

}  // namespace vr
