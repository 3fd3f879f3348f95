// vr_gmm.hip -- Gaussian-mixture (GMM) distribution volumes: BASELINE config 5
// (2048^3 x 16-component GMM, 3840x2160, 8 GPUs), DESIGN.md section 11.
//
// The reference stores histograms only (K:722-773); a GMM record is this
// build's extension, marched with the reference's own
// ray/step/transfer/composite semantics (K:282-717: the same make_ray,
// footprint, quantised trilinear blend, composite and early exit as methods
// 1/2), decoding the record statistic at every step:
//   mean     m = sum_k w_k mu_k                       (method 1, sample = m)
//   variance v = sum_k w_k (sigma_k^2 + mu_k^2) - m^2  (method 2, sample = 16 v)
// HBM layout: two planes, (w, mu) pairs [voxel][K][2] (8K bytes: 128 B = one
// cache line per voxel at K = 16) and sigma [voxel][K] (4K bytes), so the mean
// reads only the first plane.
//
// Decode across the wavefront: L = K/4 consecutive lanes share one ray (K = 16:
// 4 lanes, 16 rays per wave).  Lane s of the group loads 4 components of each
// corner record (32 bytes of (w, mu), 16 of sigma; the group reads the whole
// record), forms a partial sum, and log2(L) DPP steps complete it on every
// lane of the group.  Four components per lane balances the two costs of a
// ray-step: the record registers (8 corners x 8 floats) and the per-ray work
// every lane of a group repeats (footprint, corner addresses, blend, transfer
// function, composite), which made an 8-lane group VALU-issue-bound.  The
// canonical arithmetic the oracle restates (oracle/vr_oracle.c orc_gmm_*):
//   lane s partials over components k = 4s .. 4s + 3:
//     pm = w_k0 mu_k0;  pm = fma(w_k, mu_k, pm)
//     pq = w_k0 fma(s_k0, s_k0, mu_k0 mu_k0);  pq = fma(w_k, fma(s_k, s_k, mu_k mu_k), pq)
//   T(p) = p0 + p1                                           (L = 2, K = 8)
//        = (p0 + p1) + (p2 + p3)                             (L = 4, K = 16)
//        = ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) (L = 8, K = 32)
//   m = T(pm), v = T(pq) - m m.
//
// Active-ray refill: a wave owns 64 rays (a 64-pixel tile row, or 64 entries
// of an alive list) and marches 64/L at a time; when a group's ray ends (early
// exit, tfar, 500 steps, or leaving the slab) the wave ballots the free
// groups and hands them the next rays by prefix rank (mbcnt), so no lanes idle
// behind a long ray while work remains.
//
// Slabs (out-of-core / multi-GPU sort-last): only the slices
// [z_base, z_base + nzs) are resident; a launch takes the samples whose
// footprint z0 lies in [z_lo, z_hi) and hands every ray that leaves that range
// alive to the next slab as an exact state (sums, t, pos, samples taken), so a
// chain of slab launches in march order reproduces the whole-volume march bit
// for bit.
//
// f16 records: the same two planes with IEEE binary16
// elements -- 4K bytes of (w, mu) and 2K of sigma per voxel.  k_march_gmm_h is
// the march above instantiated on the stored type: the corner chunks stay
// packed, two halves per register, and are widened (exactly) only where the
// partial sums are formed, so a frame is bit-identical to the fp32 march of
// the widened records.  Lanes per ray as above, L = K/4: a lane's chunk of a
// corner is one 16-byte load of (w, mu) and one 8-byte load of sigma.  (L = K/8,
// two partials per lane added in-lane, measured slower at 1024^3 x 16 in every
// scene: DESIGN.md 14.3.)
//
// Range probability (query method 10): the march and the
// bake are templates over the per-corner statistic; GmmMoment<M> is the mean /
// variance above, GmmRangeStat the mixture's mass in [lo, hi),
//   sum_k w_k (Phi((hi - mu_k) / sigma_k) - Phi((lo - mu_k) / sigma_k)),
// with Phi - 1/2 from the cubic table of vr_phitab.h, staged in LDS.
//
// Quantile (query method 11): GmmQuantStat is the value at
// which the mixture's CDF, built of the same table, reaches q W -- a bisection of
// kGmmQuantSteps steps over the support [a0, b0] -- or the difference of two.
//
// What the statistics share: gmm_march is every march and
// gmm_bake_voxel every bake kernel's body -- a __global__ stages the table if its
// statistic reads it and names the functor; with_gmm_k / with_gmm_records /
// with_gmm_march turn K, the element type and SPREAD into a compiled instance
// for all six launchers, and bake_gmm_grid is the grid of the three bakes.
#include "vr_half.h"
#include "vr_internal.h"
#include "vr_march.h"
#include "vr_phitab.h"

namespace vr {

// alive-list entry: 36 bytes, 9 words -- the colour sums, t, the position and
// the pixel (23 bits: W*H <= 2^23, 3840x2160 fits) with the samples taken
// (9 bits: <= 500, K:381) in one word.  Every ray handed between ranks crosses
// xGMI as one entry, so its size is the chain's hand-off cost.
constexpr int kGmmRayWords = 9;
constexpr uint32_t kGmmPixBits = 23;
static_assert((uint32_t)kMaxSteps < (1u << (32 - kGmmPixBits)), "samples taken fit beside the pixel");
struct GmmRay {
    float sx, sy, sz, sw;
    float t, px, py, pz;
    uint32_t pix_n;               // pix | n << 23
};
static_assert(sizeof(GmmRay) == 4 * kGmmRayWords, "GmmRay is 9 words");

// ---- cross-lane sum over an L-lane group, T(p) above ----
template <int CTRL>
__device__ __forceinline__ float dppc(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int L>
__device__ __forceinline__ float group_sum(float p) {
    float s = p + dppc<0xB1>(p);                 // quad_perm [1,0,3,2]: lane ^ 1
    if constexpr (L >= 4) s = s + dppc<0x4E>(s);  // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (L >= 8) s = s + dppc<0x141>(s); // row_half_mirror: the other quad's sum
    return s;
}

// this lane's 4 components of one corner record, in the stored type T; part4()
// hands them to the statistic as floats
template <typename T, int M>
struct GmmPart;
template <int M>
struct GmmPart<float, M> {
    float4 wm[2];                 // (w, mu) of components 4s .. 4s + 3
    float4 sg[1];                 // sigma of the same components (method 2 only)
    __device__ __forceinline__ void part4(float (&w)[4], float (&mu)[4], float (&sd)[4]) const {
        const float4 a = wm[0], b = wm[1];
        w[0] = a.x; mu[0] = a.y; w[1] = a.z; mu[1] = a.w;
        w[2] = b.x; mu[2] = b.y; w[3] = b.z; mu[3] = b.w;
        if constexpr (M == 2) {
            const float4 c = sg[0];
            sd[0] = c.x; sd[1] = c.y; sd[2] = c.z; sd[3] = c.w;
        }
    }
};
// binary16: a (w, mu) pair is one register (w the low half), two sigmas another;
// widened only here, at decode
template <int M>
struct GmmPart<_Float16, M> {
    uint4 wm;                     // (w, mu) of components 4s .. 4s + 3
    uint2 sg;                     // sigma of the same components (method 2 only)
    __device__ __forceinline__ void part4(float (&w)[4], float (&mu)[4], float (&sd)[4]) const {
        const uint32_t p[4] = {wm.x, wm.y, wm.z, wm.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            w[i] = half_bits_to_float(p[i] & 0xFFFFu);
            mu[i] = half_bits_to_float(p[i] >> 16);
        }
        if constexpr (M == 2) {
            sd[0] = half_bits_to_float(sg.x & 0xFFFFu);
            sd[1] = half_bits_to_float(sg.x >> 16);
            sd[2] = half_bits_to_float(sg.y & 0xFFFFu);
            sd[3] = half_bits_to_float(sg.y >> 16);
        }
    }
};

// the canonical 4-component partials
__device__ __forceinline__ float gmm_pm(const float (&w)[4], const float (&mu)[4]) {
    float pm = w[0] * mu[0];
    pm = __builtin_fmaf(w[1], mu[1], pm);
    pm = __builtin_fmaf(w[2], mu[2], pm);
    pm = __builtin_fmaf(w[3], mu[3], pm);
    return pm;
}
__device__ __forceinline__ float gmm_pq(const float (&w)[4], const float (&mu)[4],
                                        const float (&sd)[4]) {
    float pq = w[0] * __builtin_fmaf(sd[0], sd[0], mu[0] * mu[0]);
    pq = __builtin_fmaf(w[1], __builtin_fmaf(sd[1], sd[1], mu[1] * mu[1]), pq);
    pq = __builtin_fmaf(w[2], __builtin_fmaf(sd[2], sd[2], mu[2] * mu[2]), pq);
    pq = __builtin_fmaf(w[3], __builtin_fmaf(sd[3], sd[3], mu[3] * mu[3]), pq);
    return pq;
}

// statistic of one corner (whole group participates)
template <int L, int M, typename T>
__device__ __forceinline__ float gmm_stat(const GmmPart<T, M> &r) {
    float w[4], mu[4], sd[4];
    r.part4(w, mu, sd);
    const float m = group_sum<L>(gmm_pm(w, mu));
    if constexpr (M == 1) {
        return m;
    } else {
        const float q = group_sum<L>(gmm_pq(w, mu, sd));
        const float mm = m * m;
        return (q - mm) * 16.0f;
    }
}

// The per-corner statistic of a march or bake: kLoad names the planes it reads
// (1: (w, mu) only, 2: sigma too) and stat<L>() is called by every lane of the group.
template <int M>
struct GmmMoment {
    static constexpr int kLoad = M;
    template <int L, typename T>
    __device__ __forceinline__ float stat(const GmmPart<T, M> &r) const {
        return gmm_stat<L, M>(r);
    }
};

// ---- range probability ----
// The table in device memory (staged into LDS by phi_stage) and on the host
// (vr_gmm_phi_table): the same constants.
__device__ const float kPhiTabDev[4][kPhiRows] = VR_PHI_TABLE;
static const float kPhiTabHost[4][kPhiRows] = VR_PHI_TABLE;

const float *gmm_phi_table_host() { return &kPhiTabHost[0][0]; }

// Fills the workgroup's copy of the table; every thread of the 256 must call it,
// before any wave leaves the kernel (it holds the kernel's only barrier).
__device__ __forceinline__ void phi_stage(float *tab) {
    const float *src = &kPhiTabDev[0][0];
    for (uint32_t i = threadIdx.x; i < 4u * kPhiRows; i += 256u) tab[i] = src[i];
    __syncthreads();
}

// E(z) = Phi(z) - 1/2: odd, a = min(|z|, ZMAX) (a NaN z takes ZMAX), segment
// i = (int)(a / h) <= kPhiSeg, t = a - i h (both exact: h is a power of two), a
// cubic in t with separate multiplies and adds.  The four coefficients sit in
// four arrays, so lanes with scattered i read four dwords, not one 16-byte row.
__device__ __forceinline__ float gmm_phi_e(const float *tab, float z) {
    const float a = __builtin_fminf(__builtin_fabsf(z), kPhiZMax);
    const int i = (int)(a * kPhiInvH);
    const float t = a - (float)i * kPhiH;
    const float e = tab[i] + t * (tab[kPhiRows + i] + t * (tab[2 * kPhiRows + i] + t * tab[3 * kPhiRows + i]));
    return __builtin_copysignf(e, z);
}

struct GmmRangeStat {
    static constexpr int kLoad = 2;
    float lo, hi;
    const float *tab;             // the workgroup's LDS copy of the table
    // one component's mass in [lo, hi); sigma = 0 (or 1 / sigma not finite): a Dirac at mu
    __device__ __forceinline__ float term(float w, float mu, float sd) const {
        const float r = 1.0f / sd;
        const bool ok = sd > 0.0f && __builtin_isfinite(r);
        const float zh = (hi - mu) * r, zl = (lo - mu) * r;
        const float eh = ok ? gmm_phi_e(tab, zh) : (mu < hi ? 0.5f : -0.5f);
        const float el = ok ? gmm_phi_e(tab, zl) : (mu < lo ? 0.5f : -0.5f);
        return w * (eh - el);
    }
    template <int L, typename T>
    __device__ __forceinline__ float stat(const GmmPart<T, 2> &r) const {
        float w[4], mu[4], sd[4];
        r.part4(w, mu, sd);
        float p = term(w[0], mu[0], sd[0]);
        p = p + term(w[1], mu[1], sd[1]);
        p = p + term(w[2], mu[2], sd[2]);
        p = p + term(w[3], mu[3], sd[3]);
        return group_sum<L>(p);
    }
};

// ---- quantile ----
// min / max over an L-lane group: group_sum's DPP pattern (order-independent)
template <int L>
__device__ __forceinline__ float group_min(float p) {
    float s = __builtin_fminf(p, dppc<0xB1>(p));
    if constexpr (L >= 4) s = __builtin_fminf(s, dppc<0x4E>(s));
    if constexpr (L >= 8) s = __builtin_fminf(s, dppc<0x141>(s));
    return s;
}
template <int L>
__device__ __forceinline__ float group_max(float p) {
    float s = __builtin_fmaxf(p, dppc<0xB1>(p));
    if constexpr (L >= 4) s = __builtin_fmaxf(s, dppc<0x4E>(s));
    if constexpr (L >= 8) s = __builtin_fmaxf(s, dppc<0x141>(s));
    return s;
}

// Q(q): where the table CDF C(x) = sum_k w_k (1/2 + E((x - mu_k) / sigma_k)) reaches
// q W, W the sum of the weights, by kGmmQuantSteps bisections of the support
// [a0, b0] = [min (mu - ZMAX sigma), max (mu + ZMAX sigma)] over the components of
// positive weight; SPREAD: Q(q_hi) - Q(q_lo).  A lane keeps its four components'
// w, mu, 1 / sigma and Dirac flags in registers across the search; every lane of a
// group sees the same C(mid) (group_sum is symmetric) and takes the same branch, and
// the step count is fixed, so the wave does not diverge.
template <bool SPREAD>
struct GmmQuantStat {
    static constexpr int kLoad = 2;
    float q_lo, q_hi;
    const float *tab;             // the workgroup's LDS copy of the table
    template <int L>
    __device__ __forceinline__ float search(const float (&w)[4], const float (&mu)[4],
                                            const float (&r)[4], const bool (&ok)[4], float a0,
                                            float b0, float tau) const {
        float lo = a0, hi = b0;
#pragma nounroll
        for (int it = 0; it < kGmmQuantSteps; it++) {
            const float mid = (lo + hi) * 0.5f;
            float p = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                // (the table is read for a Dirac too, then discarded: a select, so the
                // loop body has no branch; gmm_phi_e clamps any z to a row of the table)
                const float et = gmm_phi_e(tab, (mid - mu[i]) * r[i]);
                const float ed = mu[i] < mid ? 0.5f : -0.5f;
                const float e = ok[i] ? et : ed;
                const float c = w[i] * (0.5f + e);
                p = i ? p + c : c;
            }
            const bool below = group_sum<L>(p) < tau;
            lo = below ? mid : lo;
            hi = below ? hi : mid;
        }
        return hi;
    }
    template <int L, typename T>
    __device__ __forceinline__ float stat(const GmmPart<T, 2> &rec) const {
        float w[4], mu[4], sd[4], r[4];
        bool ok[4];
        rec.part4(w, mu, sd);
        float a0 = __builtin_inff(), b0 = -__builtin_inff(), live = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            r[i] = 1.0f / sd[i];
            ok[i] = sd[i] > 0.0f && __builtin_isfinite(r[i]);
            const float reach = kPhiZMax * sd[i];
            if (w[i] > 0.0f) {
                a0 = __builtin_fminf(a0, mu[i] - reach);
                b0 = __builtin_fmaxf(b0, mu[i] + reach);
                live = 1.0f;
            }
        }
        a0 = group_min<L>(a0);
        b0 = group_max<L>(b0);
        live = group_max<L>(live);
        float p = w[0];
        p = p + w[1];
        p = p + w[2];
        p = p + w[3];
        const float W = group_sum<L>(p);
        float q = search<L>(w, mu, r, ok, a0, b0, q_lo * W);
        q = live > 0.0f ? q : 0.0f;
        if constexpr (SPREAD) {
            float qh = search<L>(w, mu, r, ok, a0, b0, q_hi * W);
            qh = live > 0.0f ? qh : 0.0f;
            q = qh - q;
        }
        return q;
    }
};

// ray state of one group (identical on its L lanes)
struct GmmState {
    Ray r;
    float t, px, py, pz, stx, sty, stz;
    float sx, sy, sz, sw;
    uint32_t pix;
    int n;
};

// Sets up the ray of entry e (frame mode: pixel e of the wave's tile row;
// list mode: alive-list entry e).  Returns false if the entry holds no ray
// (outside the image or the list, or a miss -- written as the reference does).
__device__ __forceinline__ bool gmm_begin(const Params &P, uint32_t wave_base, uint32_t e,
                                          uint32_t row_x0, uint32_t row_y, bool write,
                                          GmmState &s) {
    uint32_t x, y;
    const GmmRay *in = nullptr;
    if (P.rays_in) {
        const uint32_t k = wave_base + e;
        if (k >= P.n_rays_in) return false;
        in = reinterpret_cast<const GmmRay *>(P.rays_in) + k;
        s.pix = in->pix_n & ((1u << kGmmPixBits) - 1u);
        x = s.pix % P.W;
        y = s.pix / P.W;
    } else {
        x = row_x0 + e;
        y = row_y;
        if (x >= P.CW || y >= P.CH) return false;
        s.pix = y * P.W + x;
    }
    if (!make_ray(P, x, y, s.r)) {
        if (write) write_miss(P, s.pix);
        return false;
    }
    s.stx = s.r.dx * kTStep;
    s.sty = s.r.dy * kTStep;
    s.stz = s.r.dz * kTStep;
    if (in) {
        s.sx = in->sx; s.sy = in->sy; s.sz = in->sz; s.sw = in->sw;
        s.t = in->t; s.px = in->px; s.py = in->py; s.pz = in->pz;
        s.n = (int)(in->pix_n >> kGmmPixBits);
    } else {
        s.sx = s.sy = s.sz = s.sw = 0.0f;
        s.t = s.r.tnear;
        s.px = s.r.ox + s.r.dx * s.r.tnear;
        s.py = s.r.oy + s.r.dy * s.r.tnear;
        s.pz = s.r.oz + s.r.dz * s.r.tnear;
        s.n = 0;
    }
    return true;
}

// linear voxel index of (x, y, z) in the resident slices
__device__ __forceinline__ uint64_t gmm_vox(const Params &P, int x, int y, int z) {
    return ((uint64_t)(z - P.z_base) * (uint64_t)P.ny + (uint64_t)y) * (uint64_t)P.nx + (uint64_t)x;
}

// the 8 corner records' chunks of lane `sub`: one 64-bit base address, the
// other corners by 32-bit offsets (x pair 0/1 record, y pair 0/1 row, z pair
// 0/1 slice; a slice is < 2^32 bytes for nx*ny <= 2^26 / K).
// z is clamped to the resident slices (a slab's discarded last look-ahead).
// f16: a lane's chunk is one 16-byte load of (w, mu) and one 8-byte load of
// sigma, which is the alignment vr_init_gmm_f16 asks of an adopted plane.
template <typename T, int K, int M>
__device__ __forceinline__ void gmm_gather(const Params &P, const Foot &f, uint32_t sub,
                                           GmmPart<T, M> (&r)[8]) {
    const int zl = P.z_base, zh = P.z_base + P.nzs - 1;
    const int z0 = min(max(f.z0, zl), zh), z1 = min(max(f.z1, zl), zh);
    const uint64_t v = gmm_vox(P, f.x0, f.y0, z0);
    const uint32_t ox = (uint32_t)(f.x1 - f.x0);
    const uint32_t oy = (uint32_t)(f.y1 - f.y0) * (uint32_t)P.nx;
    const uint32_t oz = (uint32_t)(z1 - z0) * (uint32_t)P.nx * (uint32_t)P.ny;
    const uint32_t off[8] = {0u, ox, oy, ox + oy, oz, oz + ox, oz + oy, oz + oy + ox};
    if constexpr (sizeof(T) == 4) {
        const float4 *a = reinterpret_cast<const float4 *>(P.gwm + v * (2u * K)) + sub * 2u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 *q = a + (size_t)off[j] * (K / 2);
            r[j].wm[0] = q[0];
            r[j].wm[1] = q[1];
        }
        if constexpr (M == 2) {
            const float4 *b = reinterpret_cast<const float4 *>(P.gsg + v * K) + sub;
#pragma unroll
            for (int j = 0; j < 8; j++) r[j].sg[0] = b[(size_t)off[j] * (K / 4)];
        }
    } else {
        const _Float16 *hwm = reinterpret_cast<const _Float16 *>(P.gwm);
        const uint4 *a = reinterpret_cast<const uint4 *>(hwm + v * (2u * K)) + sub;
#pragma unroll
        for (int j = 0; j < 8; j++) r[j].wm = a[(size_t)off[j] * (K / 4)];
        if constexpr (M == 2) {
            const _Float16 *hsg = reinterpret_cast<const _Float16 *>(P.gsg);
            const uint2 *b = reinterpret_cast<const uint2 *>(hsg + v * K) + sub;
#pragma unroll
            for (int j = 0; j < 8; j++) r[j].sg = b[(size_t)off[j] * (K / 4)];
        }
    }
}

// appends the group's ray to the alive list (groups of the wave that leave
// together share one atomic)
template <int L>
__device__ __forceinline__ void gmm_emit(const Params &P, const GmmState &s, uint32_t lane,
                                         uint32_t sub) {
    const uint64_t out = __ballot(sub == 0);
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(out))
        base = atomicAdd(P.n_rays_out, (uint32_t)__popcll(out));
    base = __shfl(base, __builtin_ctzll(out), 64);
    const uint32_t k = base + (uint32_t)__popcll(out & ((1ull << (lane & ~(uint32_t)(L - 1))) - 1ull));
    // the list's capacity (include/vr.h): no slab emits more rays than enter
    // it and the library zeroes the counter before the launch, so this is a
    // second guard -- entries past it are dropped, never written past the end
    const uint64_t cap = P.rays_in ? (uint64_t)P.n_rays_in : (uint64_t)P.W * P.H;
    if ((uint64_t)k < cap) {
        // the group's L lanes share the 9 words: lane sub writes words sub,
        // sub + L, ... (K = 8: two lanes, five and four words)
        const uint32_t w[kGmmRayWords] = {
            __float_as_uint(s.sx), __float_as_uint(s.sy), __float_as_uint(s.sz),
            __float_as_uint(s.sw), __float_as_uint(s.t), __float_as_uint(s.px),
            __float_as_uint(s.py), __float_as_uint(s.pz),
            s.pix | ((uint32_t)s.n << kGmmPixBits)};
        uint32_t *dst = P.rays_out + (uint64_t)k * kGmmRayWords;
#pragma unroll
        for (int j = 0; j < kGmmRayWords; j++)
            if ((uint32_t)(j % L) == sub) dst[j] = w[j];
    }
}

// the march of every kernel, T the stored element, S the statistic
template <typename T, int K, typename S, bool COUNT>
__device__ __forceinline__ void gmm_march(const Params &P, const S &st) {
    constexpr int M = S::kLoad;
    constexpr int L = K / 4;              // lanes per ray
    constexpr uint32_t R = 64u / L;       // rays in flight per wave
    static_assert(L == 2 || L == 4 || L == 8, "K = 8, 16 or 32");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g = lane / L, sub = lane % L;
    uint32_t wave_base = 0, row_x0 = 0, row_y = 0;
    if (P.rays_in) {
        wave_base = (blockIdx.x * 4u + wave) * 64u;
        if (wave_base >= P.n_rays_in) return;
    } else {
        const uint32_t slot = launch_slot(P);
        const uint32_t tile = tile_of(P, slot);
        if (tile == kPad) return;
        row_x0 = (tile % P.tiles_x) * kTileW;
        row_y = (tile / P.tiles_x) * kTileH + wave;
    }
    GmmState s;
    uint32_t next = R;          // wave-uniform: entries handed out so far
    bool act = gmm_begin(P, wave_base, g, row_x0, row_y, sub == 0, s);
    const uint64_t below = (1ull << (lane & ~(uint32_t)(L - 1))) - 1ull;  // lanes of earlier groups
    while (true) {
        // refill groups without a ray (ballot over the groups' first lanes,
        // prefix rank among them)
        // P.path == 1 (VR_GMM_LOCKSTEP): a new batch only when the whole wave is
        // idle, so the wave's rays stay adjacent and at the same step
        while (!(P.path == 1 && __ballot(act) != 0)) {
            const uint64_t idle = __ballot(!act && sub == 0);
            if (idle == 0 || next >= 64) break;
            const uint32_t e = next + (uint32_t)__popcll(idle & below);
            if (!act && e < 64) act = gmm_begin(P, wave_base, e, row_x0, row_y, sub == 0, s);
            next += __popcll(idle);
        }
        if (__ballot(act) == 0) break;
        if (act) {
            const Foot f = footprint(P, s.px, s.py, s.pz);
            if (P.rays_out && (f.z0 < P.z_lo || f.z0 >= P.z_hi)) {
                gmm_emit<L>(P, s, lane, sub);  // leaves the slab alive: exact state onwards
                act = false;
            } else {
                if constexpr (COUNT) {
                    if (sub == 0) {
                        mark_voxel(P.mark, gmm_vox(P, f.x0, f.y0, f.z0)); mark_voxel(P.mark, gmm_vox(P, f.x1, f.y0, f.z0));
                        mark_voxel(P.mark, gmm_vox(P, f.x0, f.y1, f.z0)); mark_voxel(P.mark, gmm_vox(P, f.x1, f.y1, f.z0));
                        mark_voxel(P.mark, gmm_vox(P, f.x0, f.y0, f.z1)); mark_voxel(P.mark, gmm_vox(P, f.x1, f.y0, f.z1));
                        mark_voxel(P.mark, gmm_vox(P, f.x0, f.y1, f.z1)); mark_voxel(P.mark, gmm_vox(P, f.x1, f.y1, f.z1));
                    }
                }
                GmmPart<T, M> rc[8];
                gmm_gather<T, K, M>(P, f, sub, rc);
                float sv[8];
#pragma unroll
                for (int j = 0; j < 8; j++) sv[j] = st.template stat<L>(rc[j]);
                s.n = s.n + 1;
                bool end = composite(P, blend8(sv, f), s.sx, s.sy, s.sz, s.sw);  // K:698
                if (!end) {
                    s.t = s.t + kTStep;                                          // K:701
                    end = s.t > s.r.tfar || s.n >= kMaxSteps;                    // K:703, K:381
                    s.px = s.px + s.stx;                                         // K:706
                    s.py = s.py + s.sty;
                    s.pz = s.pz + s.stz;
                }
                if (end) {
                    if (!COUNT && sub == 0)
                        write_pixel(P, s.pix, s.n, s.sx * P.brightness, s.sy * P.brightness,
                                    s.sz * P.brightness, s.sw * P.brightness);
                    act = false;
                }
            }
        }
    }
}

#ifndef VR_GMM_WAVES
#define VR_GMM_WAVES 1
#endif
template <int K, int M, bool COUNT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMM_WAVES, 8))) void k_march_gmm(Params P) {
    gmm_march<float, K, GmmMoment<M>, COUNT>(P, GmmMoment<M>{});
}

// Waves per SIMD the register allocation of the f16 march must reach (1: no
// demand) and may assume (3: a budget of 168 VGPRs; at K = 16 the mean takes 94,
// the variance 141).  DESIGN.md 14.4: the sweep at 1024^3 x 16.
#ifndef VR_GMMH_WAVES
#define VR_GMMH_WAVES 1
#endif
#ifndef VR_GMMH_MAXWAVES
#define VR_GMMH_MAXWAVES 3
#endif
template <int K, int M, bool COUNT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMMH_WAVES, VR_GMMH_MAXWAVES))) void k_march_gmm_h(Params P) {
    gmm_march<_Float16, K, GmmMoment<M>, COUNT>(P, GmmMoment<M>{});
}

// The range-probability marches: the bounds after Params, the table staged before
// gmm_march can return (padding tiles, waves past the alive list).
template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMM_WAVES, 8))) void k_march_gmm_range(Params P, GmmRange Q) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_march<float, K, GmmRangeStat, false>(P, GmmRangeStat{Q.lo, Q.hi, tab});
}
template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMMH_WAVES, VR_GMMH_MAXWAVES))) void k_march_gmm_range_h(Params P, GmmRange Q) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_march<_Float16, K, GmmRangeStat, false>(P, GmmRangeStat{Q.lo, Q.hi, tab});
}

// The quantile marches: the quantiles after Params (q_lo alone unless SPREAD), the
// table staged as above.
template <int K, bool SPREAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMM_WAVES, 8))) void k_march_gmm_quant(Params P, QuantArgs Q) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_march<float, K, GmmQuantStat<SPREAD>, false>(P, GmmQuantStat<SPREAD>{Q.q_lo, Q.q_hi, tab});
}
template <int K, bool SPREAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VR_GMMH_WAVES, VR_GMMH_MAXWAVES))) void k_march_gmm_quant_h(Params P, QuantArgs Q) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_march<_Float16, K, GmmQuantStat<SPREAD>, false>(P, GmmQuantStat<SPREAD>{Q.q_lo, Q.q_hi, tab});
}

// ---- launchers: one dispatch for every statistic ----
// The component counts the kernels are compiled for: f(std::integral_constant<int,
// K>{}) and what it returns (launched); false, nothing called: no instance for K.
// (The order of the lists here and below, and of the launchers in this file, is
// the order of instantiation and so of the kernels in the code object, last named
// first; the kernels that read the table address it relative to where they lie.)
template <typename F>
inline bool with_gmm_k(int K, F &&f) {
    return with_value<32, 16, 8>(K, f);
}

// ... and the planes' element type with them: f(wm, sg, k), the planes as
// const _Float16 * or const float * (ElemOf<decltype(wm)>: that type)
template <typename F>
inline bool with_gmm_records(const void *wm, const void *sg, bool half, int K, F &&f) {
    if (half)
        return with_gmm_k(K, [&](auto k) {
            f(static_cast<const _Float16 *>(wm), static_cast<const _Float16 *>(sg), k);
            return true;
        });
    return with_gmm_k(K, [&](auto k) {
        f(static_cast<const float *>(wm), static_cast<const float *>(sg), k);
        return true;
    });
}

// ... and for a march, whose f16 kernel is a __global__ of its own (its register
// budget differs): f(h, k), h 1 for f16 planes
template <typename F>
inline bool with_gmm_march(bool half, int K, F &&f) {
    return with_value<0, 1>(half, [&](auto h) {
        return with_gmm_k(K, [&](auto k) { return f(h, k); });
    });
}

// the LDS request of a march that stages the table: the VR_WG_PER_CU request leaves
// room for the kernel's static copy
static size_t phi_march_lds(const Params &P) {
    return cap_lds(P, P.wg_per_cu, 0, sizeof(float) * 4 * kPhiRows);
}

hipError_t launch_march_gmm(int K, int method, bool half, const Params &P, uint32_t nblocks,
                            bool count, hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    const dim3 grid(nblocks), block(256);
    const size_t lds = occupancy_lds(P);
    // (a count has instances of its own: the samples, and so the footprints, depend
    // on the statistic)
    if (!with_gmm_march(half, K, [&](auto h, auto k) {
            return with_value<0, 1>(count, [&](auto c) {
                return with_value<2, 1>(method, [&](auto m) {
                    constexpr int KK = decltype(k)::value, M = decltype(m)::value;
                    constexpr bool H = decltype(h)::value != 0, C = decltype(c)::value != 0;
                    if constexpr (!C) note_kernel(H ? "k_march_gmm_h" : "k_march_gmm", KK, M);
                    if constexpr (H)
                        hipLaunchKernelGGL((k_march_gmm_h<KK, M, C>), grid, block, lds, s, P);
                    else
                        hipLaunchKernelGGL((k_march_gmm<KK, M, C>), grid, block, lds, s, P);
                    return true;
                });
            });
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_march_gmm_range(int K, bool half, const Params &P, const GmmRange &Q,
                                  uint32_t nblocks, hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    const dim3 grid(nblocks), block(256);
    const size_t lds = phi_march_lds(P);
    if (!with_gmm_march(half, K, [&](auto h, auto k) {
            constexpr int KK = decltype(k)::value;
            if constexpr (decltype(h)::value != 0)
                hipLaunchKernelGGL((k_march_gmm_range_h<KK>), grid, block, lds, s, P, Q);
            else
                hipLaunchKernelGGL((k_march_gmm_range<KK>), grid, block, lds, s, P, Q);
            return true;
        }))
        return hipErrorInvalidValue;
    note_kernel(half ? "k_march_gmm_range_h" : "k_march_gmm_range", K, 10);
    return hipGetLastError();
}

hipError_t launch_march_gmm_quant(int K, bool half, const Params &P, const QuantArgs &Q,
                                  bool spread, uint32_t nblocks, hipStream_t s) {
    if (nblocks == 0) return hipSuccess;
    const dim3 grid(nblocks), block(256);
    const size_t lds = phi_march_lds(P);
    if (!with_value<0, 1>(half, [&](auto h) {
            return with_value<0, 1>(spread, [&](auto sp) {
                return with_gmm_k(K, [&](auto k) {
                    constexpr int KK = decltype(k)::value;
                    constexpr bool SP = decltype(sp)::value != 0;
                    if constexpr (decltype(h)::value != 0)
                        hipLaunchKernelGGL((k_march_gmm_quant_h<KK, SP>), grid, block, lds, s, P, Q);
                    else
                        hipLaunchKernelGGL((k_march_gmm_quant<KK, SP>), grid, block, lds, s, P, Q);
                    return true;
                });
            });
        }))
        return hipErrorInvalidValue;
    note_kernel(half ? "k_march_gmm_quant_h" : "k_march_gmm_quant", K, 11);
    return hipGetLastError();
}

// ---- baked GMM statistics (vr_bake_gmm_*, DESIGN.md sections 15, 18.3, 19.3) ----
// The mean and the 16 x variance the march decodes at every corner are pure
// functions of one voxel's record, so one pass over the resident records
// decodes them once into two float planes in the 16 x 2 x 1 bricks of the
// histogram volumes' baked planes (plane_index / put_plane, vr_device.h), and a
// frame is then the plane march of vr_kernels.hip / vr_seg.hip on plane
// method - 1.  The planes hold the bits gmm_stat<L, 1> and gmm_stat<L, 2>
// return: the same L = K/4 lanes per voxel, the same partials and DPP sums.
// The range probability and the quantile go into one plane each the same way.
//
// A wave takes 64/L consecutive x voxels of one row, a workgroup 4 waves of
// the same row (grid: x chunks, y rows, resident slices).  Lane s of a group
// loads components 4s .. 4s + 3, so the wave's loads are contiguous: one row
// segment of (w, mu) (fp32: 2 x 16 B per lane, f16: 16 B) and one of sigma (16 /
// 8 B), each record read once for every plane.  The whole group must reach the
// DPP sums: a lane past the row's end decodes the row's last voxel (clamped
// address) and skips the store; only a wave wholly past the end leaves.
// Records are indexed by z - z_base (gmm_vox), the planes by the volume's z.

// The body of a bake kernel: the mapping above and the load of the lane's chunk of
// its voxel's record, both planes; then f(r, put), for every lane of the groups of a
// wave that has voxels (a wave wholly past the row's end has left: wave-uniform).
// put(out, v) stores the voxel's statistic v into the plane at out, by the first
// lane of a group whose voxel lies in the row.
template <typename T, int K, typename F>
__device__ __forceinline__ void gmm_bake_voxel(const T *__restrict__ wm, const T *__restrict__ sg,
                                               uint32_t nx, uint32_t ny, uint32_t z_base,
                                               uint64_t psy, uint64_t psz, F &&f) {
    constexpr int L = K / 4;              // lanes per voxel
    constexpr uint32_t R = 64u / L;       // voxels per wave
    static_assert(L == 2 || L == 4 || L == 8, "K = 8, 16 or 32");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane % L;
    const uint32_t x0 = (blockIdx.x * 4u + wave) * R;
    if (x0 >= nx) return;                 // wave-uniform
    const uint32_t x = x0 + lane / L, y = blockIdx.y, zl = blockIdx.z;
    const bool in = x < nx;
    const uint64_t v = ((uint64_t)zl * ny + y) * nx + (in ? x : nx - 1u);
    GmmPart<T, 2> r;
    if constexpr (sizeof(T) == 4) {
        const float4 *a = reinterpret_cast<const float4 *>(wm + v * (2u * K)) + sub * 2u;
        r.wm[0] = a[0];
        r.wm[1] = a[1];
        r.sg[0] = reinterpret_cast<const float4 *>(sg + v * K)[sub];
    } else {
        r.wm = reinterpret_cast<const uint4 *>(wm + v * (2u * K))[sub];
        r.sg = reinterpret_cast<const uint2 *>(sg + v * K)[sub];
    }
    f(r, [&](float *out, float stat) {
        if (in && sub == 0) put_plane(out, x, y, z_base + zl, psy, psz, stat);
    });
}

// the bake of one plane of statistic st (every lane of a group calls stat<L>)
template <typename T, int K, typename S>
__device__ __forceinline__ void gmm_bake_stat(const T *__restrict__ wm, const T *__restrict__ sg,
                                              uint32_t nx, uint32_t ny, uint32_t z_base,
                                              const S &st, float *__restrict__ out, uint64_t psy,
                                              uint64_t psz) {
    gmm_bake_voxel<T, K>(wm, sg, nx, ny, z_base, psy, psz, [&](const GmmPart<T, 2> &r, auto put) {
        put(out, st.template stat<K / 4>(r));
    });
}

template <typename T, int K>
__global__ __launch_bounds__(256) void k_bake_gmm(const T *__restrict__ wm,
                                                  const T *__restrict__ sg, uint32_t nx,
                                                  uint32_t ny, uint32_t z_base,
                                                  float *__restrict__ out, uint64_t plane,
                                                  uint64_t psy, uint64_t psz) {
    gmm_bake_voxel<T, K>(wm, sg, nx, ny, z_base, psy, psz, [&](const GmmPart<T, 2> &r, auto put) {
        GmmPart<T, 1> rm;                 // the same (w, mu): the mean's operand type
        if constexpr (sizeof(T) == 4) {
            rm.wm[0] = r.wm[0];
            rm.wm[1] = r.wm[1];
        } else {
            rm.wm = r.wm;
        }
        const float m = gmm_stat<K / 4, 1>(rm);
        const float v16 = gmm_stat<K / 4, 2>(r);
        put(out, m);
        put(out + plane, v16);
    });
}

// The range probability of every resident voxel into one plane.  The table is
// staged before a wave past the row's end leaves (phi_stage's barrier).
template <typename T, int K>
__global__ __launch_bounds__(256) void k_bake_gmm_range(const T *__restrict__ wm,
                                                        const T *__restrict__ sg, uint32_t nx,
                                                        uint32_t ny, uint32_t z_base, GmmRange Q,
                                                        float *__restrict__ out, uint64_t psy,
                                                        uint64_t psz) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_bake_stat<T, K>(wm, sg, nx, ny, z_base, GmmRangeStat{Q.lo, Q.hi, tab}, out, psy, psz);
}

// ... and the quantile, the table staged as above
template <typename T, int K, bool SPREAD>
__global__ __launch_bounds__(256) void k_bake_gmm_quant(const T *__restrict__ wm,
                                                        const T *__restrict__ sg, uint32_t nx,
                                                        uint32_t ny, uint32_t z_base, QuantArgs Q,
                                                        float *__restrict__ out, uint64_t psy,
                                                        uint64_t psz) {
    __shared__ float tab[4 * kPhiRows];
    phi_stage(tab);
    gmm_bake_stat<T, K>(wm, sg, nx, ny, z_base, GmmQuantStat<SPREAD>{Q.q_lo, Q.q_hi, tab}, out,
                        psy, psz);
}

// the grid of a bake launch; false: no such K, or more voxels along an axis than a
// grid (y / z: rows and slices) or a plane brick index (plane_bx: x < 2^16) takes
static bool bake_gmm_grid(int K, int nx, int ny, int z_base, int nzs, dim3 &grid) {
    if (K < 4 || nx <= 0 || ny <= 0 || nzs <= 0 || z_base < 0 || nx > 65535 || ny > 65535 ||
        nzs > 65535)
        return false;
    const uint32_t per_wg = 4u * 64u / (uint32_t)(K / 4);  // voxels of a row per workgroup
    grid = dim3(((uint32_t)nx + per_wg - 1) / per_wg, (uint32_t)ny, (uint32_t)nzs);
    return true;
}

hipError_t launch_bake_gmm_range(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                                 int z_base, int nzs, const GmmRange &Q, float *out, uint64_t psy,
                                 uint64_t psz, hipStream_t s) {
    dim3 grid;
    if (!bake_gmm_grid(K, nx, ny, z_base, nzs, grid) ||
        !with_gmm_records(wm, sg, half, K, [&](auto w, auto g, auto k) {
            hipLaunchKernelGGL((k_bake_gmm_range<ElemOf<decltype(w)>, decltype(k)::value>), grid,
                               dim3(256), 0, s, w, g, (uint32_t)nx, (uint32_t)ny,
                               (uint32_t)z_base, Q, out, psy, psz);
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_bake_gmm_quant(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                                 int z_base, int nzs, const QuantArgs &Q, bool spread, float *out,
                                 uint64_t psy, uint64_t psz, hipStream_t s) {
    dim3 grid;
    if (!bake_gmm_grid(K, nx, ny, z_base, nzs, grid) ||
        !with_value<0, 1>(spread, [&](auto sp) {
            return with_gmm_records(wm, sg, half, K, [&](auto w, auto g, auto k) {
                hipLaunchKernelGGL((k_bake_gmm_quant<ElemOf<decltype(w)>, decltype(k)::value,
                                                     decltype(sp)::value != 0>),
                                   grid, dim3(256), 0, s, w, g, (uint32_t)nx, (uint32_t)ny,
                                   (uint32_t)z_base, Q, out, psy, psz);
            });
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_bake_gmm(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                           int z_base, int nzs, float *out, uint64_t plane, uint64_t psy,
                           uint64_t psz, hipStream_t s) {
    dim3 grid;
    if (!bake_gmm_grid(K, nx, ny, z_base, nzs, grid) ||
        !with_gmm_records(wm, sg, half, K, [&](auto w, auto g, auto k) {
            hipLaunchKernelGGL((k_bake_gmm<ElemOf<decltype(w)>, decltype(k)::value>), grid,
                               dim3(256), 0, s, w, g, (uint32_t)nx, (uint32_t)ny,
                               (uint32_t)z_base, out, plane, psy, psz);
        }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- synthetic GMM volume ----
// The section-5 blob field f places the mixture: per component k of voxel v
// (global index x + nx*(y + ny*z)), h = splitmix64(seed ^ 0x6A09E667F3BCC909 ^
// (v*K + k)), a = (h >> 40) 2^-24, r = 0.05 + ((h >> 16) & 0xFFFFFF) 2^-24,
// mu = clamp((0.8 f + 0.1) + 0.2 (a - 0.5), 0, 1),
// sigma = ((h & 0xFFFF) 2^-16) 0.05 + 0.005, w = r / sum_k r (float, in order).
__device__ __forceinline__ uint64_t gmm_hash(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// T: the stored element; (T) of a float rounds to nearest even (_Float16:
// v_cvt_f16_f32, subnormals kept), so the f16 volume is the fp32 one narrowed
template <typename T>
__global__ __launch_bounds__(256) void k_synth_gmm(T *__restrict__ wm, T *__restrict__ sg,
                                                   SynthArgs a, int K, int z_base, int nzs) {
    const uint64_t nvox = (uint64_t)a.nx * a.ny * (uint64_t)nzs;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t lv = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lv < nvox; lv += stride) {
        const uint32_t x = (uint32_t)(lv % (uint64_t)a.nx);
        const uint64_t yz = lv / (uint64_t)a.nx;
        const uint32_t y = (uint32_t)(yz % (uint64_t)a.ny);
        const uint32_t z = (uint32_t)(yz / (uint64_t)a.ny) + (uint32_t)z_base;
        float f = 0.0f;
#pragma unroll
        for (int k = 0; k < kSynthBlobs; k++)
            f = f + ((a.amp[k] * a.gx[k * a.nx + x]) * a.gy[k * a.ny + y]) * a.gz[k * a.nz + z];
        if (f > 1.0f) f = 1.0f;
        const uint64_t v = ((uint64_t)z * a.ny + y) * a.nx + x;
        float sum = 0.0f;
        for (int k = 0; k < K; k++) {
            const uint64_t h = gmm_hash(a.seed ^ 0x6A09E667F3BCC909ull ^ (v * (uint64_t)K + (uint64_t)k));
            const float r = 0.05f + (float)((h >> 16) & 0xFFFFFFull) * 0x1p-24f;
            sum = sum + r;
        }
        for (int k = 0; k < K; k++) {
            const uint64_t h = gmm_hash(a.seed ^ 0x6A09E667F3BCC909ull ^ (v * (uint64_t)K + (uint64_t)k));
            const float u = (float)(h >> 40) * 0x1p-24f;
            const float r = 0.05f + (float)((h >> 16) & 0xFFFFFFull) * 0x1p-24f;
            float mu = (f * 0.8f + 0.1f) + (u - 0.5f) * 0.2f;
            mu = fminf(fmaxf(mu, 0.0f), 1.0f);
            const float sig = ((float)(h & 0xFFFFull) * 0x1p-16f) * 0.05f + 0.005f;
            wm[(lv * K + k) * 2u] = (T)(r / sum);
            wm[(lv * K + k) * 2u + 1u] = (T)mu;
            sg[lv * K + k] = (T)sig;
        }
    }
}

hipError_t launch_synth_gmm(void *wm, void *sg, bool half, const SynthArgs &a, int K, int z_base,
                            int nzs, hipStream_t s) {
    const uint64_t nvox = (uint64_t)a.nx * a.ny * (uint64_t)nzs;
    uint64_t blocks = (nvox + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (blocks == 0) return hipSuccess;
    if (half)
        hipLaunchKernelGGL(k_synth_gmm<_Float16>, dim3((uint32_t)blocks), dim3(256), 0, s,
                           static_cast<_Float16 *>(wm), static_cast<_Float16 *>(sg), a, K, z_base, nzs);
    else
        hipLaunchKernelGGL(k_synth_gmm<float>, dim3((uint32_t)blocks), dim3(256), 0, s,
                           static_cast<float *>(wm), static_cast<float *>(sg), a, K, z_base, nzs);
    return hipGetLastError();
}

}  // namespace vr
