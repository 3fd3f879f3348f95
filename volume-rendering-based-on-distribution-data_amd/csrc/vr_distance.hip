// vr_distance.hip -- the distribution-distance query, method 12 (DESIGN.md section
// 20): a frame of D(p, h), how far every voxel's record p is from one target
// record h under the L1, earth mover's or Kolmogorov-Smirnov distance (or of the
// similarity 1 - D).
//
//  k_march_dist<T,B,METRIC>  the per-ray pipelined march of vr_query.h over float
//                            or _Float16 records in x rows, with dist_stat
//                            (vr_device.h) per corner: a subtract and an add of
//                            the magnitude per bin (L1), or a subtract, a running
//                            sum and an add / max of its magnitude (EMD / KS).
//                            The target and the similarity flag arrive as a
//                            kernel argument of their own (DistTarget after
//                            Params: wave-uniform, read with scalar loads, h_i an
//                            SGPR operand of the subtraction).
//  k_bake_dist<T,B,METRIC>   the same dist_stat of every voxel, once, into one
//                            float plane in the 16 x 2 x 1 bricks of
//                            vr_bake_stats; a frame from the plane is
//                            bit-identical.
#include "vr_query.h"

namespace vr {

// the statistic of the shared loops (vr_query.h): dist_stat against the launch's target
template <int METRIC>
struct DistStat {
    const DistTarget &H;
    template <typename T, int B>
    __device__ __forceinline__ float operator()(const LinRec<T, B> &r) const {
        if constexpr (std::is_same<T, float>::value) {
            return dist_stat<B, METRIC>(r.p, H.h, H.similarity != 0);
        } else {
            float p[B];
            widen_rec<B>(r.h, p);
            return dist_stat<B, METRIC>(p, H.h, H.similarity != 0);
        }
    }
};

// Waves per SIMD the register allocation may assume: VR_LIN_MAXWAVES' caps
// (DESIGN.md section 20.2 compares the register counts across caps).
#ifndef VR_DIST_MAXWAVES
#define VR_DIST_MAXWAVES(B) ((B) >= 16 ? 2 : (B) >= 8 ? 3 : 8)
#endif
template <typename T, int B, int METRIC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, VR_DIST_MAXWAVES(B)))) void k_march_dist(const T *__restrict__ vol, Params P, DistTarget H) {
    march_lin_kernel<T, B, lin_batch<T, B>()>(vol, P, DistStat<METRIC>{H});
}

template <typename T, int B, int METRIC>
__global__ __launch_bounds__(256) void k_bake_dist(const T *__restrict__ vol, Params P,
                                                   DistTarget H, float *__restrict__ out,
                                                   uint64_t psy, uint64_t psz) {
    bake_lin_kernel<T, B>(vol, P, DistStat<METRIC>{H}, out, psy, psz);
}

template <typename T, int METRIC>
static hipError_t march_dist_t(const T *vol, const Params &P, const DistTarget &H,
                               uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU; the kernel itself uses no LDS
    switch (P.nb) {
    case 1: hipLaunchKernelGGL((k_march_dist<T, 1, METRIC>), grid, block, lds, s, vol, P, H); break;
    case 2: hipLaunchKernelGGL((k_march_dist<T, 2, METRIC>), grid, block, lds, s, vol, P, H); break;
    case 4: hipLaunchKernelGGL((k_march_dist<T, 4, METRIC>), grid, block, lds, s, vol, P, H); break;
    case 8: hipLaunchKernelGGL((k_march_dist<T, 8, METRIC>), grid, block, lds, s, vol, P, H); break;
    case 16: hipLaunchKernelGGL((k_march_dist<T, 16, METRIC>), grid, block, lds, s, vol, P, H); break;
    case 32: hipLaunchKernelGGL((k_march_dist<T, 32, METRIC>), grid, block, lds, s, vol, P, H); break;
    default: return hipErrorInvalidValue;  // no runtime-B instance
    }
    return hipGetLastError();
}

template <typename T>
static hipError_t march_dist_m(const T *vol, const Params &P, const DistTarget &H, int metric,
                               uint32_t nslots, hipStream_t s) {
    switch (metric) {
    case 0: return march_dist_t<T, 0>(vol, P, H, nslots, s);
    case 1: return march_dist_t<T, 1>(vol, P, H, nslots, s);
    case 2: return march_dist_t<T, 2>(vol, P, H, nslots, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_march_dist(const void *vol, bool half, const Params &P, const DistTarget &H,
                             int metric, uint32_t nslots, hipStream_t s) {
    const hipError_t e =
        half ? march_dist_m(static_cast<const _Float16 *>(vol), P, H, metric, nslots, s)
             : march_dist_m(static_cast<const float *>(vol), P, H, metric, nslots, s);
    if (e == hipSuccess) note_kernel("k_march_dist", P.nb, 12);
    return e;
}

template <typename T, int METRIC>
static hipError_t bake_dist_t(const T *vol, const Params &P, const DistTarget &H, float *out,
                              uint64_t psy, uint64_t psz, hipStream_t s) {
    dim3 grid;
    const dim3 block(256);
    if (!bake_lin_grid(P, grid)) return hipErrorInvalidValue;
    switch (P.nb) {
    case 1: hipLaunchKernelGGL((k_bake_dist<T, 1, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    case 2: hipLaunchKernelGGL((k_bake_dist<T, 2, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    case 4: hipLaunchKernelGGL((k_bake_dist<T, 4, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    case 8: hipLaunchKernelGGL((k_bake_dist<T, 8, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    case 16: hipLaunchKernelGGL((k_bake_dist<T, 16, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    case 32: hipLaunchKernelGGL((k_bake_dist<T, 32, METRIC>), grid, block, 0, s, vol, P, H, out, psy, psz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename T>
static hipError_t bake_dist_m(const T *vol, const Params &P, const DistTarget &H, int metric,
                              float *out, uint64_t psy, uint64_t psz, hipStream_t s) {
    switch (metric) {
    case 0: return bake_dist_t<T, 0>(vol, P, H, out, psy, psz, s);
    case 1: return bake_dist_t<T, 1>(vol, P, H, out, psy, psz, s);
    case 2: return bake_dist_t<T, 2>(vol, P, H, out, psy, psz, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_bake_dist(const void *vol, bool half, const Params &P, const DistTarget &H,
                            int metric, float *out, uint64_t psy, uint64_t psz, hipStream_t s) {
    return half ? bake_dist_m(static_cast<const _Float16 *>(vol), P, H, metric, out, psy, psz, s)
                : bake_dist_m(static_cast<const float *>(vol), P, H, metric, out, psy, psz, s);
}

}  // namespace vr
