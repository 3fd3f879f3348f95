// vr_crossing.hip -- the level-crossing query, method 13:
// a frame of the probability that the isosurface v = theta passes through the
// cell a sample lies in, 1 - prod F_c - prod (1 - F_c) over the cell's 8 corners
// with F_c = P(v_c < theta) and the corners taken as independent.  The first
// query that is a joint function of the 8 corner distributions: nothing is
// blended, the combine below stands where blend8 stands in the other marches.
//
//  k_march_cross<T,B>       the per-ray pipelined march of vr_query.h over float
//                           or _Float16 records in x rows with method 10's
//                           lin_stat per corner (F_c = sum w_i p_i against the
//                           crossing weights, a BinWeights kernel argument after
//                           Params) and CrossCombine instead of the filter.
//  k_march_cross_plane<GM>  the same one-lane pipelined march over a plane of F
//                           (one float per voxel in the 16 x 2 x 1 bricks of
//                           vr_bake_stats: the crossing plane k_bake_lin made, or
//                           a GMM range plane), fetched with gather8<1, GM>'s
//                           four pair loads; GM 1: 32-bit indices (the planes
//                           plane_narrow admits), GM 2: 64-bit indices.
// No bake kernel: the plane of F is k_bake_lin's (vr_query.hip).
#include "vr_query.h"

namespace vr {

// F_c of the shared loops: lin_stat against the launch's crossing weights
struct CrossStat {
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

// (the combine, CrossCombine: vr_query.h, shared with vr_transfer.hip)

// Waves per SIMD the register allocation may assume: VR_LIN_MAXWAVES' caps
#ifndef VR_CROSS_MAXWAVES
#define VR_CROSS_MAXWAVES(B) ((B) >= 16 ? 2 : (B) >= 8 ? 3 : 8)
#endif
template <typename T, int B>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, VR_CROSS_MAXWAVES(B)))) void k_march_cross(const T *__restrict__ vol, Params P, BinWeights W) {
    march_lin_kernel<T, B, lin_batch<T, B>()>(vol, P, CrossStat{W}, CrossCombine{});
}

// march_pipe_tile (vr_march.h) over a plane of F with the combine for the filter:
// two sets of 8 floats, the next step's four pair loads issued unconditionally
// (clamped indices: always inside the plane) before this step's combine
template <int GM>
__device__ __forceinline__ int march_cross_plane_tile(const float *__restrict__ plane,
                                                      const Params &P, uint32_t slot,
                                                      uint32_t tile, uint32_t tid) {
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
    const CrossCombine comb;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    float t = r.tnear;
    float px = r.ox + r.dx * r.tnear, py = r.oy + r.dy * r.tnear, pz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int n = 0;
    bool alive = true;
    Foot fa = footprint(P, px, py, pz), fb;
    float ra[8][1], rb[8][1];
    gather8<1, GM>(plane, P, fa, ra);
    auto step = [&](int i, const Foot &fc, const float (&rc)[8][1], Foot &fn, float (&rn)[8][1]) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        fn = footprint(P, nx, ny, nz);
        gather8<1, GM>(plane, P, fn, rn);
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = rc[j][0];
        const float sample = comb(s, fc);
        n = i + 1;
        if (composite(P, sample, sx, sy, sz, sw) || !cont) {
            alive = false;
        } else {
            t = tn;
            px = nx;
            py = ny;
            pz = nz;
        }
    };
    for (int i = 0; i < kMaxSteps; i += 2) {
        step(i, fa, ra, fb, rb);
        if (!alive) break;
        step(i + 1, fb, rb, fa, ra);
        if (!alive) break;
    }
    write_pixel(P, q.o, n, sx * P.brightness, sy * P.brightness, sz * P.brightness,
                sw * P.brightness);
    return n;
}

template <int GM>
__global__ __launch_bounds__(256) void k_march_cross_plane(const float *__restrict__ plane, Params P) {
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    const int n = march_cross_plane_tile<GM>(plane, P, slot, tile, threadIdx.x);
    if (P.tile_cost) record_tile_cost(P, tile, n);  // all lanes have reconverged here
}

hipError_t launch_march_cross(const void *vol, bool half, const Params &P, const BinWeights &W,
                              uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU; the kernel itself uses no LDS
    if (!with_records(vol, half, P.nb, [&](auto v, auto B) {
            using T = ElemOf<decltype(v)>;
            hipLaunchKernelGGL((k_march_cross<T, decltype(B)::value>), grid, block, lds, s, v, P, W);
        }))
        return hipErrorInvalidValue;  // no runtime-B instance
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_cross", P.nb, 13);
    return e;
}

hipError_t launch_march_cross_plane(const float *plane, const Params &P, uint32_t nslots,
                                    hipStream_t s) {
    if (P.nb != 1 || P.nx <= 0 || P.ny <= 0 || P.nz <= 0) return hipErrorInvalidValue;
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);
    // gather8 MODE 1 forms the index with 24-bit multiplies in 32 bits
    const bool narrow = P.sy < (1u << 24) && P.sz < (1u << 24) && (uint64_t)P.nz < (1u << 24) &&
                        P.sz * (uint64_t)P.nz < (1ull << 32);
    if (narrow) hipLaunchKernelGGL((k_march_cross_plane<1>), grid, block, lds, s, plane, P);
    else hipLaunchKernelGGL((k_march_cross_plane<2>), grid, block, lds, s, plane, P);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_cross_plane", 1, 13);
    return e;
}

}  // namespace vr
