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

hipError_t launch_march_dist(const void *vol, bool half, const Params &P, const DistTarget &H,
                             int metric, uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU; the kernel itself uses no LDS
    if (!with_value<0, 1, 2>(metric, [&](auto M) {
            return with_records(vol, half, P.nb, [&](auto v, auto B) {
                using T = ElemOf<decltype(v)>;
                hipLaunchKernelGGL((k_march_dist<T, decltype(B)::value, decltype(M)::value>), grid,
                                   block, lds, s, v, P, H);
            });
        }))
        return hipErrorInvalidValue;  // no such metric, or no runtime-B instance
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_dist", P.nb, 12);
    return e;
}

hipError_t launch_bake_dist(const void *vol, bool half, const Params &P, const DistTarget &H,
                            int metric, float *out, uint64_t psy, uint64_t psz, hipStream_t s) {
    dim3 grid;
    const dim3 block(256);
    if (!bake_lin_grid(P, grid)) return hipErrorInvalidValue;
    if (!with_value<0, 1, 2>(metric, [&](auto M) {
            return with_records(vol, half, P.nb, [&](auto v, auto B) {
                using T = ElemOf<decltype(v)>;
                hipLaunchKernelGGL((k_bake_dist<T, decltype(B)::value, decltype(M)::value>), grid,
                                   block, 0, s, v, P, H, out, psy, psz);
            });
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vr
