// vr_project.hip -- ray projections of a baked plane: the
// maximum, the minimum or the mean of the samples along a ray, classified once per
// ray through the transfer-function table.  No opacity test is made in the march:
// whether a ray takes another step depends on t alone, so its length is known
// before any load returns.
//
//  k_march_proj<GM, CROSS, MODE>  one lane per ray over a plane of one float per
//                                 voxel in the 16 x 2 x 1 bricks of vr_bake_stats,
//                                 fetched with gather8<1, GM>'s four pair loads
//                                 (GM 1: 32-bit indices, GM 2: 64-bit ones), kProjDepth
//                                 steps in flight.  CROSS false: the sample is the
//                                 trilinear blend of the 8 corners; true: CrossCombine
//                                 (planes of F, method 13).  MODE: kProjMax / MIN /
//                                 MEAN.  The table is read from the library's device
//                                 copy after the loop, two 16-byte loads per ray: no
//                                 LDS, no barrier.
#include <cstdlib>

#include "vr_query.h"

namespace vr {

// steps of a ray in flight: sets of four pair loads issued ahead of the step that
// reduces them
#ifndef VR_PROJ_DEPTH
#define VR_PROJ_DEPTH 4  // (3: an out-of-tree tuning build, EXTRA=-DVR_PROJ_DEPTH=3)
#endif
constexpr int kProjDepth = VR_PROJ_DEPTH;
static_assert(kProjDepth == 3 || kProjDepth == 4, "march_proj_tile names its sets");

// one step in flight: the 8 floats of gather8's four pair loads before the x select,
// and what the sample needs of the footprint
struct ProjSet {
    float v[8][1];
    float ax, ay, az;
    bool ox;  // the footprint's x pair is two voxels (gather8's select)
};

// The four pair loads of step (px, py, pz) into set.  gather8 selects each pair's
// second float by f.x1 != f.x0 as soon as it is loaded, which would wait for the
// loads here; it is handed a footprint whose x pair is always two voxels, so its
// selects fold away and the loads stay in flight, and the select is made by
// proj_sample when the step is reduced (the same loads, the same floats).
template <int GM>
__device__ __forceinline__ void proj_issue(const float *__restrict__ plane, const Params &P,
                                           float px, float py, float pz, ProjSet &set) {
    Foot f = footprint(P, px, py, pz);
    set.ax = f.ax;
    set.ay = f.ay;
    set.az = f.az;
    set.ox = f.x1 != f.x0;
    f.x1 = f.x0 + 1;  // (read by gather8's comparison only)
    gather8<1, GM>(plane, P, f, set.v);
}

template <typename BL>
__device__ __forceinline__ float proj_sample(const ProjSet &set) {
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const float lo = set.v[j][0], hi = set.v[j + 1][0];  // (values: no select of addresses)
        s[j] = lo;
        s[j + 1] = set.ox ? hi : lo;
    }
    Foot f;
    f.ax = set.ax;
    f.ay = set.ay;
    f.az = set.az;
    return BL{}(s, f);
}

// the reduction of one sample into acc: a compare and a select (a NaN sample is
// skipped, -0 does not replace +0), or the running sum in step order
template <int MODE>
__device__ __forceinline__ float proj_reduce(float acc, float s) {
    if constexpr (MODE == kProjMax) return (s > acc) ? s : acc;
    else if constexpr (MODE == kProjMin) return (s < acc) ? s : acc;
    else return acc + s;
}

// march_plane_tf_tile's ray (vr_transfer.hip) without the opacity test.  The t / pos
// chain of the reference runs kProjDepth steps ahead of the reduction: a step is
// issued only if the ray takes it (`more`), so ng, the steps issued, is the ray's
// length once the chain ends, and step i is reduced iff i < ng -- decided before
// step i's loads are waited for.
template <int GM, typename BL, int MODE>
__device__ __forceinline__ int march_proj_tile(const float *__restrict__ plane, const Params &P,
                                               const float4 *__restrict__ table, int ntab,
                                               uint32_t slot, uint32_t tile, uint32_t tid) {
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
    float gt = r.tnear;
    float gx = r.ox + r.dx * r.tnear, gy = r.oy + r.dy * r.tnear, gz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int ng = 0;
    bool more = true;
    ProjSet set[kProjDepth];
    // the next step (it exists: `more`) into a set; the t / pos chain moves on
    auto issue_now = [&](ProjSet &sk) {
        proj_issue<GM>(plane, P, gx, gy, gz, sk);
        ng = ng + 1;
        gt = gt + kTStep;                           // K:701
        more = !(gt > r.tfar) && (ng < kMaxSteps);  // K:703, K:381
        gx = gx + stx;                              // K:706
        gy = gy + sty;
        gz = gz + stz;
    };
    // the ray takes all of the next kProjDepth steps to issue, ng .. ng + kProjDepth - 1
    // (the t chain alone, the same additions issue_now makes)
    auto full_round = [&]() {
        bool m = more;
        float t = gt;
#pragma unroll
        for (int k = 1; k < kProjDepth; k++) {
            t = t + kTStep;
            m = m && !(t > r.tfar) && (ng + k < kMaxSteps);
        }
        return m;
    };
    float acc = MODE == kProjMax ? -__builtin_huge_valf()
                : MODE == kProjMin ? __builtin_huge_valf() : 0.0f;
    int n = 0;
    // Whole rounds.  A branch around an issue that the wave may skip makes the count
    // of loads issued after a set unknown when the set is waited for, and the wait
    // becomes one for every load in flight.  So while every marching ray of the wave
    // has a whole round to issue, the round is straight-line code -- kProjDepth x
    // (reduce a set, refill it), no lane predicate anywhere -- and each set is waited
    // for with the younger ones still in flight.  (The sets by name: no indexed
    // access, so they stay in registers.)
    if (__all(full_round())) {
        issue_now(set[0]);
        issue_now(set[1]);
        issue_now(set[2]);
        if constexpr (kProjDepth == 4) issue_now(set[3]);
        auto round_step = [&](ProjSet &sk) {
            acc = proj_reduce<MODE>(acc, proj_sample<BL>(sk));
            n = n + 1;
            issue_now(sk);
        };
        while (__all(full_round())) {
            round_step(set[0]);
            round_step(set[1]);
            round_step(set[2]);
            if constexpr (kProjDepth == 4) round_step(set[3]);
        }
    } else {
        auto issue = [&](ProjSet &sk) {
            if (more) issue_now(sk);
        };
        issue(set[0]);
        issue(set[1]);
        issue(set[2]);
        if constexpr (kProjDepth == 4) issue(set[3]);
    }
    // The rest -- the last steps of the wave's rays, and waves whose rays differ in
    // length by more than the whole rounds cover: a step is issued by the lanes that
    // take it, and a ray that has ended inside a round keeps its acc and n.
    auto step = [&](ProjSet &sk) {
        if (n < ng) {
            acc = proj_reduce<MODE>(acc, proj_sample<BL>(sk));
            n = n + 1;
            if (more) issue_now(sk);
        }
    };
    do {
        step(set[0]);
        step(set[1]);
        step(set[2]);
        if constexpr (kProjDepth == 4) step(set[3]);
    } while (n < ng);
    if constexpr (MODE == kProjMean) acc = acc / (float)n;
    // composite_tf's classification, once: two entries of the device table
    int i0, i1;
    float a;
    lin_axis((acc - P.toff) * P.tscale, ntab, i0, i1, a);  // indices clamped to [0, ntab - 1]
    const float4 t0 = table[i0], t1 = table[i1];
    const float4 col = make_float4(lerpq(t0.x, t1.x, a), lerpq(t0.y, t1.y, a),
                                   lerpq(t0.z, t1.z, a), lerpq(t0.w, t1.w, a));
    write_pixel(P, q.o, n, col.x * col.w * P.brightness, col.y * col.w * P.brightness,
                col.z * col.w * P.brightness, col.w * P.brightness);
    return n;
}

// the kernarg segment of k_march_plane_tf: plane, Params, table, n
template <int GM, bool CROSS, int MODE>
__global__ __launch_bounds__(256) void k_march_proj(const float *__restrict__ plane, Params P,
                                                    const float4 *__restrict__ table, int n) {
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    using BL = std::conditional_t<CROSS, CrossCombine, Blend8>;
    const int ns = march_proj_tile<GM, BL, MODE>(plane, P, table, n, slot, tile, threadIdx.x);
    if (P.tile_cost) record_tile_cost(P, tile, ns);  // all lanes have reconverged here
}

template <int GM, bool CROSS>
static void launch_proj_mode(int mode, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                             const float *plane, const Params &P, const float4 *table, int n) {
    if (mode == kProjMax)
        hipLaunchKernelGGL((k_march_proj<GM, CROSS, kProjMax>), grid, block, lds, s, plane, P, table, n);
    else if (mode == kProjMin)
        hipLaunchKernelGGL((k_march_proj<GM, CROSS, kProjMin>), grid, block, lds, s, plane, P, table, n);
    else
        hipLaunchKernelGGL((k_march_proj<GM, CROSS, kProjMean>), grid, block, lds, s, plane, P, table, n);
}

hipError_t launch_march_proj(const float *plane, const Params &P, const float4 *table, int n,
                             bool cross, int mode, uint32_t nslots, hipStream_t s) {
    if (P.nb != 1 || P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || !table || n < 1 || n > kTfMax ||
        mode < kProjMax || mode > kProjMean)
        return hipErrorInvalidValue;
    const dim3 grid(nslots), block(256);
    const size_t lds = occupancy_lds(P);  // VR_WG_PER_CU (the kernel has no LDS of its own)
    // launch_march_plane_tf's rule (gather8 MODE 1: 24-bit multiplies in 32 bits);
    // VR_TF_WIDE=1 forces the 64-bit instance (tests: small planes run both)
    bool narrow = P.sy < (1u << 24) && P.sz < (1u << 24) && (uint64_t)P.nz < (1u << 24) &&
                  P.sz * (uint64_t)P.nz < (1ull << 32);
    if (const char *e = tuning("VR_TF_WIDE")) narrow = narrow && std::atoi(e) == 0;
    if (narrow) {
        if (cross) launch_proj_mode<1, true>(mode, grid, block, lds, s, plane, P, table, n);
        else launch_proj_mode<1, false>(mode, grid, block, lds, s, plane, P, table, n);
    } else {
        if (cross) launch_proj_mode<2, true>(mode, grid, block, lds, s, plane, P, table, n);
        else launch_proj_mode<2, false>(mode, grid, block, lds, s, plane, P, table, n);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        note_kernel(mode == kProjMax   ? "k_march_proj_max"
                    : mode == kProjMin ? "k_march_proj_min"
                                          : "k_march_proj_mean",
                    1, cross ? 13 : 0);
    return e;
}

}  // namespace vr
