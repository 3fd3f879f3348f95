// vr_quantile.hip -- the quantile query, method 11: a
// frame of Q(q), the value where a voxel's CDF reaches q (median, percentile),
// or of the spread Q(q_hi) - Q(q_lo) (interquartile range).
//
//  k_march_quant<T,B,SPREAD>  the per-ray pipelined march of vr_query.h over float
//                             or _Float16 records in x rows, with quant_stat
//                             (vr_device.h) per corner: the prefix sums of the
//                             bins, a chain of selects for the bin the CDF
//                             crosses q in, one IEEE division.  q_lo and q_hi
//                             arrive as a kernel argument of their own
//                             (QuantArgs after Params).
//  k_bake_quant<T,B,SPREAD>   the same quant_stat of every voxel, once, into one
//                             float plane in the 16 x 2 x 1 bricks of
//                             vr_bake_stats; a frame from the plane is
//                             bit-identical.
#include "vr_query.h"

namespace vr {

template <bool SPREAD>
struct QuantStat {
    float q_lo, q_hi;
    template <typename T, int B>
    __device__ __forceinline__ float operator()(const LinRec<T, B> &r) const {
        if constexpr (std::is_same<T, float>::value) {
            return quant_stat<B, SPREAD>(r.p, q_lo, q_hi);
        } else {
            float p[B];
            widen_rec<B>(r.h, p);
            return quant_stat<B, SPREAD>(p, q_lo, q_hi);
        }
    }
};

// Corners gathered per batch: lin_batch, halved for 32 bins, where the prefix sums
// (B floats, with the widened record live across the two scans of the spread)
// would otherwise take the instance past 256 registers.
template <typename T, int B>
constexpr int quant_batch() {
    return B >= 32 ? lin_batch<T, B>() / 2 : lin_batch<T, B>();
}

// Waves per SIMD the register allocation may assume: VR_LIN_MAXWAVES' caps.  At
// B = 8 a cap of 2, 3 or 4 gives the same code objects.
#ifndef VR_QUANT_MAXWAVES
#define VR_QUANT_MAXWAVES(B) ((B) >= 16 ? 2 : (B) >= 8 ? 3 : 8)
#endif
template <typename T, int B, bool SPREAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, VR_QUANT_MAXWAVES(B)))) void k_march_quant(const T *__restrict__ vol, Params P, QuantArgs Q) {
    march_lin_kernel<T, B, quant_batch<T, B>()>(vol, P, QuantStat<SPREAD>{Q.q_lo, Q.q_hi});
}

template <typename T, int B, bool SPREAD>
__global__ __launch_bounds__(256) void k_bake_quant(const T *__restrict__ vol, Params P,
                                                    QuantArgs Q, float *__restrict__ out,
                                                    uint64_t psy, uint64_t psz) {
    bake_lin_kernel<T, B>(vol, P, QuantStat<SPREAD>{Q.q_lo, Q.q_hi}, out, psy, psz);
}

hipError_t launch_march_quant(const void *vol, bool half, const Params &P, const QuantArgs &Q,
                              bool spread, uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU; the kernel itself uses no LDS
    if (!with_value<0, 1>(spread, [&](auto SP) {
            return with_records(vol, half, P.nb, [&](auto v, auto B) {
                using T = ElemOf<decltype(v)>;
                hipLaunchKernelGGL((k_march_quant<T, decltype(B)::value, decltype(SP)::value != 0>),
                                   grid, block, lds, s, v, P, Q);
            });
        }))
        return hipErrorInvalidValue;  // no runtime-B instance
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_quant", P.nb, 11);
    return e;
}

hipError_t launch_bake_quant(const void *vol, bool half, const Params &P, const QuantArgs &Q,
                             bool spread, float *out, uint64_t psy, uint64_t psz, hipStream_t s) {
    dim3 grid;
    const dim3 block(256);
    if (!bake_lin_grid(P, grid)) return hipErrorInvalidValue;
    if (!with_value<0, 1>(spread, [&](auto SP) {
            return with_records(vol, half, P.nb, [&](auto v, auto B) {
                using T = ElemOf<decltype(v)>;
                hipLaunchKernelGGL((k_bake_quant<T, decltype(B)::value, decltype(SP)::value != 0>),
                                   grid, block, 0, s, v, P, Q, out, psy, psz);
            });
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vr
