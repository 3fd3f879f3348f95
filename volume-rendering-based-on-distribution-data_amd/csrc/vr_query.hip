// vr_query.hip -- the weighted-bin query, method 10: a
// frame of s = sum w_i p_i, a fixed linear functional of every voxel's bins
// (range probability, CDF at an isovalue, tail mass, a custom moment: only the
// weights differ).
//
//  k_march_lin<T,B>  the per-ray pipelined march (march_pipe_tile, vr_march.h;
//                    march_h_tile, vr_half.hip) over float or _Float16 records
//                    in x rows: one lane per ray, the next gathers in flight
//                    while this step decodes.  Only the per-corner statistic is
//                    new: lin_stat (vr_device.h), a float multiply and add per
//                    bin against weights that arrive as a kernel argument of
//                    their own (BinWeights after Params: wave-uniform, read
//                    with scalar loads and used as SGPR operands).
//  k_bake_lin<T,B>   the same lin_stat of every voxel, once, into one float plane
//                    in the 16 x 2 x 1 bricks of vr_bake_stats; a frame from the
//                    plane is bit-identical (the same eight floats enter the
//                    same filter).
#include "vr_query.h"

namespace vr {

// the statistic of the shared loops (vr_query.h): lin_stat against the launch's weights
struct LinStat {
    const BinWeights &W;
    template <typename T, int B>
    __device__ __forceinline__ float operator()(const LinRec<T, B> &r) const {
        if constexpr (std::is_same<T, float>::value) {
            return lin_stat<B>(r.p, W.w);
        } else {
            float p[B];
            widen_rec<B>(r.h, p);
            return lin_stat<B>(p, W.w);
        }
    }
};

// Waves per SIMD the register allocation may assume: the caps of the f16 march
// (VR_PIPEH_MAXWAVES, vr_half.hip) -- 3 at B = 8, 2 for the wide records, none
// for narrow ones.
#ifndef VR_LIN_MAXWAVES
#define VR_LIN_MAXWAVES(B) ((B) >= 16 ? 2 : (B) >= 8 ? 3 : 8)
#endif
template <typename T, int B>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, VR_LIN_MAXWAVES(B)))) void k_march_lin(const T *__restrict__ vol, Params P, BinWeights W) {
    march_lin_kernel<T, B, lin_batch<T, B>()>(vol, P, LinStat{W});
}

template <typename T, int B>
__global__ __launch_bounds__(256) void k_bake_lin(const T *__restrict__ vol, Params P,
                                                  BinWeights W, float *__restrict__ out,
                                                  uint64_t psy, uint64_t psz) {
    bake_lin_kernel<T, B>(vol, P, LinStat{W}, out, psy, psz);
}

hipError_t launch_march_lin(const void *vol, bool half, const Params &P, const BinWeights &W,
                            uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU; the kernel itself uses no LDS
    if (!with_records(vol, half, P.nb, [&](auto v, auto B) {
            using T = ElemOf<decltype(v)>;
            hipLaunchKernelGGL((k_march_lin<T, decltype(B)::value>), grid, block, lds, s, v, P, W);
        }))
        return hipErrorInvalidValue;  // no runtime-B instance
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_lin", P.nb, 10);
    return e;
}

hipError_t launch_bake_lin(const void *vol, bool half, const Params &P, const BinWeights &W,
                           float *out, uint64_t psy, uint64_t psz, hipStream_t s) {
    dim3 grid;
    const dim3 block(256);
    if (!bake_lin_grid(P, grid)) return hipErrorInvalidValue;
    if (!with_records(vol, half, P.nb, [&](auto v, auto B) {
            using T = ElemOf<decltype(v)>;
            hipLaunchKernelGGL((k_bake_lin<T, decltype(B)::value>), grid, block, 0, s, v, P, W, out,
                               psy, psz);
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vr
