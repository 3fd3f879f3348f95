// vr_shade.hip -- headlight gradient shading of frames from a baked plane (DESIGN.md
// section 25): k_march_plane_tf's march (vr_transfer.hip) with every classified
// sample's colour lit by the gradient of the trilinear interpolant inside its cell,
// the light at the eye.  The gradient is a blend of differences of the 8 corner
// values the step already holds, two of its three components from blend8's own
// intermediates, so a lit frame issues exactly the loads of the unlit one.  Opacity
// is not lit: rays end where they end without the light.
//
//  k_march_lit<GM, CROSS>  one lane per ray over a plane of one float per voxel in
//                          the 16 x 2 x 1 bricks of vr_bake_stats, fetched with
//                          gather8<1, GM>'s four pair loads (GM 1: 32-bit indices,
//                          GM 2: 64-bit ones).  CROSS false: the sample is the
//                          trilinear blend of the 8 corners; true: CrossCombine
//                          (planes of F, method 13), the gradient that of F.  The
//                          table is staged from the library's device copy into
//                          4 KiB of LDS; the light is a 16-byte kernel argument.
#include <cstdlib>

#include "vr_query.h"

namespace vr {

// the table in LDS, one float4 per entry (TfTable of vr_transfer.hip)
struct LitTable {
    const float4 *tab;  // LDS
    int n;
};

// The sample of a step and the cosine between the gradient of the interpolant and
// the ray (section 25.1).  Every operation separate, in the order written; sqrtf and
// the division are the correctly rounded ones (no fast-math flag in this build).
// c00 .. c11, c0, c1 are blend8's intermediates: lerpq(c0, c1, az) is blend8's float.
template <bool CROSS>
__device__ __forceinline__ float lit_sample(const Params &P, const Ray &r, const float (&s)[8],
                                            const Foot &f, float &c) {
    const float c00 = lerpq(s[0], s[1], f.ax);
    const float c10 = lerpq(s[2], s[3], f.ax);
    const float c01 = lerpq(s[4], s[5], f.ax);
    const float c11 = lerpq(s[6], s[7], f.ax);
    const float c0 = lerpq(c00, c10, f.ay);
    const float c1 = lerpq(c01, c11, f.ay);
    const float gx = lerpq(lerpq(s[1] - s[0], s[3] - s[2], f.ay),
                           lerpq(s[5] - s[4], s[7] - s[6], f.ay), f.az);
    const float gy = lerpq(c10 - c00, c11 - c01, f.az);
    const float gz = c1 - c0;
    // per voxel -> per unit of the volume's [-1, 1] box, up to the common factor 1/2
    const float Gx = gx * (float)P.nx, Gy = gy * (float)P.ny, Gz = gz * (float)P.nz;
    const float g2 = (Gx * Gx + Gy * Gy) + Gz * Gz;
    const float gd = (Gx * r.dx + Gy * r.dy) + Gz * r.dz;
    c = (g2 > 0.0f) ? fabsf(gd) / sqrtf(g2) : 1.0f;  // no gradient: lit as if facing the eye
    c = (c < 1.0f) ? c : 1.0f;                       // (a NaN becomes 1)
    if constexpr (CROSS) return CrossCombine{}(s, f);
    else return lerpq(c0, c1, f.az);
}

// composite_tf (vr_transfer.hip) with the colour lit before it is weighted by its
// opacity: col = col * shade + spec per colour channel, alpha untouched
__device__ __forceinline__ bool composite_lit(const Params &P, const LitTable &tf, const Light &L,
                                              float sample, float c, float &sx, float &sy,
                                              float &sz, float &sw) {
    int i0, i1;
    float a;
    lin_axis((sample - P.toff) * P.tscale, tf.n, i0, i1, a);  // indices clamped to [0, n - 1]
    const float4 t0 = tf.tab[i0], t1 = tf.tab[i1];
    float4 col = make_float4(lerpq(t0.x, t1.x, a), lerpq(t0.y, t1.y, a), lerpq(t0.z, t1.z, a),
                             lerpq(t0.w, t1.w, a));
    const float shade = L.ka + L.kd * c;
    // c ^ (2 ^ k) by k squarings.  The light is uniform over the launch, so the loop
    // and the branch are scalar: k multiplications, none for a light without a
    // highlight, whose spec is ks itself (0 <= p <= 1, never a NaN, so ks * p of a zero
    // ks is that zero, sign and all)
    float spec = L.ks;
    if (L.ks > 0.0f) {
        float p = c;
#pragma unroll 1
        for (int j = 0; j < L.k; j++) p = p * p;
        spec = L.ks * p;
    }
    col.x = col.x * shade + spec;
    col.y = col.y * shade + spec;
    col.z = col.z * shade + spec;
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

// march_plane_tf_tile (vr_transfer.hip) with lit_sample and composite_lit: two sets of
// 8 floats, the next step's four pair loads issued unconditionally (clamped indices:
// always inside the plane) before this step's work
template <int GM, bool CROSS>
__device__ __forceinline__ int march_lit_tile(const float *__restrict__ plane, const Params &P,
                                              const LitTable &tf, const Light &L, uint32_t slot,
                                              uint32_t tile, uint32_t tid) {
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
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
        float c;
        const float sample = lit_sample<CROSS>(P, r, s, fc, c);
        n = i + 1;
        if (composite_lit(P, tf, L, sample, c, sx, sy, sz, sw) || !cont) {
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

// k_march_plane_tf's arguments and the light.  Thread t < n stages entry t; the
// barrier comes before the padding slots of a tile list leave.
template <int GM, bool CROSS>
__global__ __launch_bounds__(256) void k_march_lit(const float *__restrict__ plane, Params P,
                                                   const float4 *__restrict__ table, int n,
                                                   Light L) {
    __shared__ float4 s_tab[kTfMax];
    if (threadIdx.x < (uint32_t)n) s_tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    const LitTable tf = {s_tab, n};
    const int ns = march_lit_tile<GM, CROSS>(plane, P, tf, L, slot, tile, threadIdx.x);
    if (P.tile_cost) record_tile_cost(P, tile, ns);  // all lanes have reconverged here
}

hipError_t launch_march_lit(const float *plane, const Params &P, const float4 *table, int n,
                            const Light &L, bool cross, uint32_t nslots, hipStream_t s) {
    if (P.nb != 1 || P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || !table || n < 1 || n > kTfMax ||
        L.k < 0 || L.k > kLightMaxLog2)
        return hipErrorInvalidValue;
    const dim3 grid(nslots), block(256);
    // VR_WG_PER_CU: the request counts the table's static LDS in (launch_march_plane_tf)
    constexpr size_t kStatic = sizeof(float4) * kTfMax;
    const size_t cap = occupancy_lds(P);
    const size_t lds = cap > kStatic ? cap - kStatic : 0;
    // launch_march_plane_tf's rule (gather8 MODE 1: 24-bit multiplies in 32 bits);
    // VR_TF_WIDE=1 forces the 64-bit instance (tests: small planes run both)
    bool narrow = P.sy < (1u << 24) && P.sz < (1u << 24) && (uint64_t)P.nz < (1u << 24) &&
                  P.sz * (uint64_t)P.nz < (1ull << 32);
    if (const char *e = tuning("VR_TF_WIDE")) narrow = narrow && std::atoi(e) == 0;
    if (narrow) {
        if (cross) hipLaunchKernelGGL((k_march_lit<1, true>), grid, block, lds, s, plane, P, table, n, L);
        else hipLaunchKernelGGL((k_march_lit<1, false>), grid, block, lds, s, plane, P, table, n, L);
    } else {
        if (cross) hipLaunchKernelGGL((k_march_lit<2, true>), grid, block, lds, s, plane, P, table, n, L);
        else hipLaunchKernelGGL((k_march_lit<2, false>), grid, block, lds, s, plane, P, table, n, L);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_lit", 1, cross ? 13 : 0);
    return e;
}

}  // namespace vr
