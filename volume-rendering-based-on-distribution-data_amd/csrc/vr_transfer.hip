// vr_transfer.hip -- frames of a baked plane classified through a user-defined
// transfer function: a table of n RGBA float entries,
// 1 <= n <= 256, sampled exactly as the built-in nine are (lin_axis with n for 9,
// lerpq per channel; nothing in the table clamped), then composite's arithmetic
// unchanged.  A table holding the reference's nine entries gives the built-in
// frames bit for bit.
//
//  k_march_plane_tf<GM, CROSS>  k_march_cross_plane's one-lane pipelined march
//                               (vr_crossing.hip) over a plane of one float per
//                               voxel in the 16 x 2 x 1 bricks of vr_bake_stats,
//                               fetched with gather8<1, GM>'s four pair loads
//                               (GM 1: 32-bit indices, GM 2: 64-bit ones).
//                               CROSS false: the sample is the trilinear blend of
//                               the 8 corners (the statistics, weighted, quantile,
//                               distance and GMM planes); true: CrossCombine
//                               (planes of F, method 13).  The table is staged
//                               from the library's device copy into 4 KiB of LDS.
#include <cstdlib>

#include "vr_query.h"

namespace vr {

// The table in LDS, one float4 per entry at 16 i: a sample reads entries i0 and
// i1 as two 16-byte reads.  ds_read_b128 conflicts are counted per 16-lane group
// on (address / 4) % 64, so two lanes of a group collide only on distinct entries
// a multiple of 16 apart; the lanes of a wave are neighbouring rays, whose samples
// -- and so entries -- are mostly equal (a broadcast) or adjacent (other banks).
// A channel-major layout would take four 4-byte reads per entry instead.
struct TfTable {
    const float4 *tab;  // LDS
    int n;
};

// composite (vr_march.h) with the table for tf_entry and n for 9
__device__ __forceinline__ bool composite_tf(const Params &P, const TfTable &tf, float sample,
                                             float &sx, float &sy, float &sz, float &sw) {
    int i0, i1;
    float a;
    lin_axis((sample - P.toff) * P.tscale, tf.n, i0, i1, a);  // indices clamped to [0, n - 1]
    const float4 t0 = tf.tab[i0], t1 = tf.tab[i1];
    float4 col = make_float4(lerpq(t0.x, t1.x, a), lerpq(t0.y, t1.y, a), lerpq(t0.z, t1.z, a),
                             lerpq(t0.w, t1.w, a));
    col.w = col.w * P.density;
    col.x = col.x * col.w;
    col.y = col.y * col.w;
    col.z = col.z * col.w;
    const float om = 1.0f - sw;
    sx = sx + col.x * om;
    sy = sy + col.y * om;
    sz = sz + col.z * om;
    sw = sw + col.w * om;
    return sw > kOpacityThreshold;
}

// march_cross_plane_tile (vr_crossing.hip) with the sample functor BL and
// composite_tf: two sets of 8 floats, the next step's four pair loads issued
// unconditionally (clamped indices: always inside the plane) before this step's work
template <int GM, typename BL>
__device__ __forceinline__ int march_plane_tf_tile(const float *__restrict__ plane,
                                                   const Params &P, const TfTable &tf,
                                                   uint32_t slot, uint32_t tile, uint32_t tid) {
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
    const BL bl;
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
        const float sample = bl(s, fc);
        n = i + 1;
        if (composite_tf(P, tf, sample, sx, sy, sz, sw) || !cont) {
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

// table: kTfMax float4 in device memory, the first n set.  Thread t < n stages
// entry t (one 16-byte load, one 16-byte LDS write); the barrier comes before the
// padding slots of a tile list leave (phi_stage's rule, vr_gmm.hip).
template <int GM, bool CROSS>
__global__ __launch_bounds__(256) void k_march_plane_tf(const float *__restrict__ plane, Params P,
                                                        const float4 *__restrict__ table, int n) {
    __shared__ float4 s_tab[kTfMax];
    if (threadIdx.x < (uint32_t)n) s_tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    const TfTable tf = {s_tab, n};
    using BL = std::conditional_t<CROSS, CrossCombine, Blend8>;
    const int ns = march_plane_tf_tile<GM, BL>(plane, P, tf, slot, tile, threadIdx.x);
    if (P.tile_cost) record_tile_cost(P, tile, ns);  // all lanes have reconverged here
}

hipError_t launch_march_plane_tf(const float *plane, const Params &P, const float4 *table, int n,
                                 bool cross, uint32_t nslots, hipStream_t s) {
    if (P.nb != 1 || P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || !table || n < 1 || n > kTfMax)
        return hipErrorInvalidValue;
    const dim3 grid(nslots), block(256);
    // VR_WG_PER_CU: the request that caps workgroups per CU counts the table's
    // static LDS in, so a cap still yields the stated number
    constexpr size_t kStatic = sizeof(float4) * kTfMax;
    const size_t cap = occupancy_lds(P);
    const size_t lds = cap > kStatic ? cap - kStatic : 0;
    // launch_march_cross_plane's rule (gather8 MODE 1: 24-bit multiplies in 32 bits);
    // VR_TF_WIDE=1 forces the 64-bit instance (tests: small planes run both)
    bool narrow = P.sy < (1u << 24) && P.sz < (1u << 24) && (uint64_t)P.nz < (1u << 24) &&
                  P.sz * (uint64_t)P.nz < (1ull << 32);
    if (const char *e = tuning("VR_TF_WIDE")) narrow = narrow && std::atoi(e) == 0;
    if (narrow) {
        if (cross) hipLaunchKernelGGL((k_march_plane_tf<1, true>), grid, block, lds, s, plane, P, table, n);
        else hipLaunchKernelGGL((k_march_plane_tf<1, false>), grid, block, lds, s, plane, P, table, n);
    } else {
        if (cross) hipLaunchKernelGGL((k_march_plane_tf<2, true>), grid, block, lds, s, plane, P, table, n);
        else hipLaunchKernelGGL((k_march_plane_tf<2, false>), grid, block, lds, s, plane, P, table, n);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_plane_tf", 1, cross ? 13 : 0);
    return e;
}

}  // namespace vr
