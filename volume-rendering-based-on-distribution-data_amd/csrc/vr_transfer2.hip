// vr_transfer2.hip -- frames of two baked planes of one volume classified through
// a user-defined 2-D transfer function: a table of nu x nv
// RGBA float entries, entry (i, j) at 4 * (j * nu + i), 1 <= nu, nv <= 256 and
// nu * nv <= 1024.  At every sample the march forms su from plane u and sv from
// plane v out of one footprint, looks the table up bilinearly (lin_axis on each
// axis, lerpq along u in rows j0 and j1, lerpq of the two along v; nothing in the
// table clamped), then composite's arithmetic unchanged.
//
//  k_march_tf2<GM, CU, CV>  k_march_plane_tf's one-lane pipelined march
//                           (vr_transfer.hip) over two planes of one float per
//                           voxel in the 16 x 2 x 1 bricks of vr_bake_stats, of
//                           the same pitches: the four pair indices of a step
//                           are formed once (gather8 MODE 1 / 2's, GM 1: 32-bit,
//                           GM 2: 64-bit) and loaded from both bases.  CU / CV
//                           false: that axis' sample is the trilinear blend of
//                           its 8 corners; true: CrossCombine (a plane of F,
//                           method 13).  The table is staged from the library's
//                           device copy into 16 KiB of LDS.
#include <cstdlib>

#include "vr_query.h"

namespace vr {

// The table in LDS, one float4 per entry at 16 (j nu + i): a sample reads the
// entries (i0, j0), (i1, j0), (i0, j1), (i1, j1) as four 16-byte reads.
// ds_read_b128 conflicts are counted per 16-lane group on (address / 4) % 64, so
// two lanes of a group collide only on distinct entries a multiple of 16 apart
// (in a row: 16 u-steps; across rows: where nu * (j - j') is one).  The lanes of
// a wave are neighbouring rays, whose samples -- and so entries -- are mostly
// equal (a broadcast) or adjacent in u (other banks); u fastest keeps the pair
// (i0, i1) of a row in neighbouring bank quads.  A channel-major layout would
// take sixteen 4-byte reads per sample instead of four 16-byte ones.
struct Tf2Table {
    const float4 *tab;  // LDS
    int nu, nv;
    float voff, vscale;
};

// composite (vr_march.h) with the bilinear lookup for transfer.  The four reads
// are issued before the first use, so the waits count lgkmcnt down from 3 and the
// planes' prefetch stays on vmcnt.
__device__ __forceinline__ bool composite_tf2(const Params &P, const Tf2Table &tf, float su,
                                              float sv, float &sx, float &sy, float &sz,
                                              float &sw) {
    int i0, i1, j0, j1;
    float a, b;
    lin_axis((su - P.toff) * P.tscale, tf.nu, i0, i1, a);  // indices clamped to [0, nu - 1]
    lin_axis((sv - tf.voff) * tf.vscale, tf.nv, j0, j1, b);
    const int r0 = j0 * tf.nu, r1 = j1 * tf.nu;
    const float4 t00 = tf.tab[r0 + i0], t01 = tf.tab[r0 + i1];
    const float4 t10 = tf.tab[r1 + i0], t11 = tf.tab[r1 + i1];
    float4 col = make_float4(lerpq(lerpq(t00.x, t01.x, a), lerpq(t10.x, t11.x, a), b),
                             lerpq(lerpq(t00.y, t01.y, a), lerpq(t10.y, t11.y, a), b),
                             lerpq(lerpq(t00.z, t01.z, a), lerpq(t10.z, t11.z, a), b),
                             lerpq(lerpq(t00.w, t01.w, a), lerpq(t10.w, t11.w, a), b));
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

// gather8<1, GM> (vr_march.h MODE 1 / 2) for two planes of the same pitches: the
// four pair indices once, one 8-byte load per pair and plane.  The pairs are kept
// as loaded -- (y0, z0), (y1, z0), (y0, z1), (y1, z1) -- and the clamped footprint's
// choice between a pair's halves is left to corners8, at the step that consumes
// them: nothing here reads a loaded value, so no wait follows the loads.
template <int GM>
__device__ __forceinline__ void gather_pairs2(const float *__restrict__ pu,
                                              const float *__restrict__ pv, const Params &P,
                                              const Foot &f, vr_f2a4 (&ru)[4], vr_f2a4 (&rv)[4]) {
    static_assert(GM == 1 || GM == 2, "baked planes in x-row bricks");
    const uint32_t bx = plane_bx((uint32_t)f.x0);
    uint64_t i00, i10, i01, i11;
    if constexpr (GM == 1) {
        const uint32_t sy = (uint32_t)P.sy, sz = (uint32_t)P.sz;
        const uint32_t z0 = __umul24((uint32_t)f.z0, sz), z1 = __umul24((uint32_t)f.z1, sz);
        const uint32_t y0 = __umul24((uint32_t)f.y0 >> 1, sy) + ((uint32_t)f.y0 & 1u) * 16u + bx;
        const uint32_t y1 = __umul24((uint32_t)f.y1 >> 1, sy) + ((uint32_t)f.y1 & 1u) * 16u + bx;
        i00 = z0 + y0; i10 = z0 + y1; i01 = z1 + y0; i11 = z1 + y1;
    } else {
        const uint32_t sy = (uint32_t)P.sy;  // a slice is < 2^32 floats
        const uint32_t y0 = ((uint32_t)f.y0 >> 1) * sy + ((uint32_t)f.y0 & 1u) * 16u + bx;
        const uint32_t y1 = ((uint32_t)f.y1 >> 1) * sy + ((uint32_t)f.y1 & 1u) * 16u + bx;
        i00 = (uint64_t)f.z0 * P.sz + y0; i10 = (uint64_t)f.z0 * P.sz + y1;
        i01 = (uint64_t)f.z1 * P.sz + y0; i11 = (uint64_t)f.z1 * P.sz + y1;
    }
    ru[0] = load_pair64(pu, i00); ru[1] = load_pair64(pu, i10);
    ru[2] = load_pair64(pu, i01); ru[3] = load_pair64(pu, i11);
    rv[0] = load_pair64(pv, i00); rv[1] = load_pair64(pv, i10);
    rv[2] = load_pair64(pv, i01); rv[3] = load_pair64(pv, i11);
}

// the 8 corners of the footprint f in gather order (x = c & 1, y = c & 2, z = c & 4)
// out of its four pairs: where the volume's edge clamps x1 to x0 both x corners are
// the pair's first half (gather8's rule)
__device__ __forceinline__ void corners8(const vr_f2a4 (&r)[4], const Foot &f, float (&s)[8]) {
    const bool ox = f.x1 != f.x0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        s[2 * k] = r[k].x;
        s[2 * k + 1] = ox ? r[k].y : r[k].x;
    }
}

// march_plane_tf_tile (vr_transfer.hip) over two planes: two sets of 2 x 4 pairs
// (2 x 8 floats), the next step's eight pair loads issued unconditionally (clamped
// indices: always inside the planes) before this step's work
template <int GM, typename BU, typename BV>
__device__ __forceinline__ int march_tf2_tile(const float *__restrict__ pu,
                                              const float *__restrict__ pv, const Params &P,
                                              const Tf2Table &tf, uint32_t slot, uint32_t tile,
                                              uint32_t tid) {
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
    const BU bu;
    const BV bv;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    float t = r.tnear;
    float px = r.ox + r.dx * r.tnear, py = r.oy + r.dy * r.tnear, pz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int n = 0;
    bool alive = true;
    Foot fa = footprint(P, px, py, pz), fb;
    vr_f2a4 ua[4], va[4], ub[4], vb[4];
    gather_pairs2<GM>(pu, pv, P, fa, ua, va);
    auto step = [&](int i, const Foot &fc, const vr_f2a4 (&uc)[4], const vr_f2a4 (&vc)[4], Foot &fn,
                    vr_f2a4 (&un)[4], vr_f2a4 (&vn)[4]) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        fn = footprint(P, nx, ny, nz);
        gather_pairs2<GM>(pu, pv, P, fn, un, vn);
        float cu[8], cv[8];
        corners8(uc, fc, cu);
        corners8(vc, fc, cv);
        const float su = bu(cu, fc), sv = bv(cv, fc);
        n = i + 1;
        if (composite_tf2(P, tf, su, sv, sx, sy, sz, sw) || !cont) {
            alive = false;
        } else {
            t = tn;
            px = nx;
            py = ny;
            pz = nz;
        }
    };
    for (int i = 0; i < kMaxSteps; i += 2) {
        step(i, fa, ua, va, fb, ub, vb);
        if (!alive) break;
        step(i + 1, fb, ub, vb, fa, ua, va);
        if (!alive) break;
    }
    write_pixel(P, q.o, n, sx * P.brightness, sy * P.brightness, sz * P.brightness,
                sw * P.brightness);
    return n;
}

// table: kTf2Max float4 in device memory, the first nu * nv set.  Thread t stages
// entries t, t + 256, ... below nu * nv (a 16-byte load and a 16-byte LDS write
// each); the barrier comes before the padding slots of a tile list leave
// (phi_stage's rule, vr_gmm.hip).
template <int GM, bool CU, bool CV>
__global__ __launch_bounds__(256) void k_march_tf2(const float *__restrict__ pu,
                                                   const float *__restrict__ pv, Params P,
                                                   const float4 *__restrict__ table, int nu,
                                                   int nv, float voff, float vscale) {
    __shared__ float4 s_tab[kTf2Max];
    const int n = min(nu * nv, kTf2Max);
    for (int e = (int)threadIdx.x; e < n; e += 256) s_tab[e] = table[e];
    __syncthreads();
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    const Tf2Table tf = {s_tab, nu, nv, voff, vscale};
    using BU = std::conditional_t<CU, CrossCombine, Blend8>;
    using BV = std::conditional_t<CV, CrossCombine, Blend8>;
    const int ns = march_tf2_tile<GM, BU, BV>(pu, pv, P, tf, slot, tile, threadIdx.x);
    if (P.tile_cost) record_tile_cost(P, tile, ns);  // all lanes have reconverged here
}

template <int GM>
static void launch_tf2(dim3 grid, dim3 block, size_t lds, hipStream_t s, const float *pu,
                       const float *pv, const Params &P, const float4 *table, int nu, int nv,
                       float voff, float vscale, bool cu, bool cv) {
    switch ((cu ? 1 : 0) + (cv ? 2 : 0)) {
    case 0: hipLaunchKernelGGL((k_march_tf2<GM, false, false>), grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale); break;
    case 1: hipLaunchKernelGGL((k_march_tf2<GM, true, false>), grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale); break;
    case 2: hipLaunchKernelGGL((k_march_tf2<GM, false, true>), grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale); break;
    default: hipLaunchKernelGGL((k_march_tf2<GM, true, true>), grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale); break;
    }
}

hipError_t launch_march_tf2(const float *pu, const float *pv, const Params &P, const float4 *table,
                            int nu, int nv, float voff, float vscale, bool cu, bool cv,
                            uint32_t nslots, hipStream_t s) {
    if (P.nb != 1 || P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || !pu || !pv || !table || nu < 1 ||
        nv < 1 || nu > 256 || nv > 256 || nu * nv > kTf2Max)
        return hipErrorInvalidValue;
    const dim3 grid(nslots), block(256);
    // VR_WG_PER_CU: the request that caps workgroups per CU counts the table's
    // static LDS in, so a cap still yields the stated number
    constexpr size_t kStatic = sizeof(float4) * kTf2Max;
    const size_t cap = occupancy_lds(P);
    const size_t lds = cap > kStatic ? cap - kStatic : 0;
    // launch_march_plane_tf's rule (24-bit multiplies in 32 bits); VR_TF_WIDE=1
    // forces the 64-bit instance (tests: small planes run both)
    bool narrow = P.sy < (1u << 24) && P.sz < (1u << 24) && (uint64_t)P.nz < (1u << 24) &&
                  P.sz * (uint64_t)P.nz < (1ull << 32);
    if (const char *e = tuning("VR_TF_WIDE")) narrow = narrow && std::atoi(e) == 0;
    if (narrow) launch_tf2<1>(grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale, cu, cv);
    else launch_tf2<2>(grid, block, lds, s, pu, pv, P, table, nu, nv, voff, vscale, cu, cv);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_march_tf2", 2, (cu ? 1 : 0) + (cv ? 2 : 0));
    return e;
}

}  // namespace vr
