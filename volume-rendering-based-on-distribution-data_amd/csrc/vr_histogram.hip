// vr_histogram.hip -- value ranges and joint histograms of baked planes (DESIGN.md
// section 27).
//
// k_plane_hist<V>: the histogram of one plane (V = 0) or the joint histogram of two
// planes of one grid (V = 1) over a box of voxels, binned into the cells of the
// table a frame will use: for plane value s and window (offset, scale),
//     x = (s - offset) * scale          (two float32 operations, no fma)
//     i = point_axis(x, n)              (clamp01 with NaN -> 0, floor, min(., n - 1))
// and counts[j * nu + i] is the number of voxels with u bin i and v bin j.
// k_plane_range: the minimum and maximum over the box's voxels that are not NaN, by
// the monotone key of the bit pattern (-0 < +0), and the number that are NaN.
//
// Both walk the planes in slot order (16 x 2 x 1 bricks, plane_index): a brick is one
// 128-B line, a lane loads 16 B of it (four slots of one y row), 8 lanes a line, a
// wave 8 consecutive lines.  Only the lines of the bricks, y pairs and slices that
// meet the box are visited; inside a line the apron slot (offset 15 of a row), slots
// beyond the grid and slots outside the box are masked, so each voxel counts once.
// A lane's line is (a, b, c) = (brick, y pair, slice) relative to the box's first;
// the grid's stride in lines is added to it digit by digit (PlaneWalk::da / db / dc),
// so the loop divides nothing.  The loads of the next two lines are in flight while
// a line is counted.
//
// Counting: uint32 counters in LDS, added to without a return value, R = 2^logr
// copies of the histogram interleaved by lane (counter (bin << logr) + (lane & (R -
// 1))), R the largest power of two up to 32 with R * nu * nv * 4 bytes <= 64 KiB:
// with R = 32 the lanes of a group of 32 hit 32 different banks whatever the data.
// Before it counts a line's four slots a wave compares the 4 x 64 bins with its first
// lane's first bin: if all are equal (a homogeneous region; a constant plane always)
// one lane adds the number of counted slots once, instead of 64 lanes adding 1 to one
// address four times.  After a barrier the workgroup sums the copies of each bin and
// adds the non-zero sums to the zeroed uint64 device array with one 64-bit vector
// atomic each.  Integer adds commute: the result does not depend on scheduling.  The
// launcher sizes the grid so that a workgroup visits fewer than 2^32 slots, which
// bounds every uint32 counter.
#include "vr_internal.h"

namespace vr {

namespace {

constexpr uint32_t kHistThreads = 1024;                 // 16 waves: 128 lines a round
constexpr uint32_t kHistLines = kHistThreads / 8u;
constexpr uint32_t kHistLdsBytes = 65536;               // VR_HIST_MAX uint32 counters
constexpr uint32_t kHistMaxRounds = (1u << 20) - 1u;    // x 4096 slots a round < 2^32
static_assert(kHistMax * sizeof(uint32_t) == kHistLdsBytes, "VR_HIST_MAX bins fill the LDS");

// The lines a launch walks and how: the box in bricks, y pairs and slices, the box in
// voxels, and the grid's stride in lines as digits of (bricks, pairs, slices).
struct PlaneWalk {
    uint64_t psy, psz;            // the planes' pitches in floats
    uint32_t kx0, nkx;            // first brick of a row that meets the box, how many
    uint32_t yp0, nyp;            // y pairs
    uint32_t z0, nz;              // slices
    uint32_t x0, xw, y0, yh;      // the box: x0 <= x < x0 + xw, y0 <= y < y0 + yh
    uint32_t da, db, dc;          // stride = (dc * nyp + db) * nkx + da lines
    uint32_t pad;
};

// One lane's walk: its line (a, b, c), the loads of three lines in flight.
template <int V>
struct Walker {
    const PlaneWalk &w;
    const uint4 *pu, *pv;
    uint32_t q;        // the lane's 16 B of a line
    uint32_t a, b, c;  // the line the next load is of

    __device__ __forceinline__ Walker(const PlaneWalk &w_, const float *u, const float *v)
        : w(w_), pu(reinterpret_cast<const uint4 *>(u)), pv(reinterpret_cast<const uint4 *>(v)) {
        const uint64_t line = ((uint64_t)blockIdx.x * kHistThreads + threadIdx.x) >> 3;
        q = threadIdx.x & 7u;
        a = (uint32_t)(line % w.nkx);
        const uint64_t rest = line / w.nkx;
        b = (uint32_t)(rest % w.nyp);
        const uint64_t s = rest / w.nyp;
        c = s < w.nz ? (uint32_t)s : w.nz;
    }
    __device__ __forceinline__ bool live() const { return c < w.nz; }
    // loads the line (a, b, c) if there is one, notes where it was, steps on
    __device__ __forceinline__ void fetch(uint4 &du, uint4 &dv, uint32_t &kx, uint32_t &y,
                                          bool &ok) {
        ok = live();
        kx = w.kx0 + a;
        y = 2u * (w.yp0 + b) + (q >> 2);
        if (ok) {
            const uint64_t at =
                (((uint64_t)(w.z0 + c) * w.psz + (uint64_t)(w.yp0 + b) * w.psy) >> 2) + kx * 8u + q;
            du = pu[at];
            if (V) dv = pv[at];
            a += w.da;
            const uint32_t ca = a >= w.nkx ? 1u : 0u;
            a -= ca ? w.nkx : 0u;
            b += w.db + ca;
            const uint32_t cb = b >= w.nyp ? 1u : 0u;
            b -= cb ? w.nyp : 0u;
            c = min(c + w.dc + cb, w.nz);
        }
    }
    // which of the four slots of the lane's 16 B of line (kx, y) hold a voxel of the box
    __device__ __forceinline__ void mask(uint32_t kx, uint32_t y, bool (&m)[4]) const {
        const uint32_t xo = 4u * (q & 3u), x = kPlaneStride * kx + xo;
        const bool row = y - w.y0 < w.yh;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            m[j] = row && xo + j != kPlaneStride && x + j - w.x0 < w.xw;
    }
};

__device__ __forceinline__ uint32_t bin_of(uint32_t bits, float off, float scale, int n) {
    return (uint32_t)point_axis((__uint_as_float(bits) - off) * scale, n);
}

}  // namespace

template <int V>
__global__ __launch_bounds__(kHistThreads, 8) void k_plane_hist(
    const float *__restrict__ pu, const float *__restrict__ pv, PlaneWalk w, float uoff,
    float uscale, float voff, float vscale, uint32_t nu, uint32_t nv, uint32_t logr,
    unsigned long long *__restrict__ counts) {
    extern __shared__ uint32_t hist[];
    const uint32_t t = threadIdx.x, nbins = nu * nv, rep = t & ((1u << logr) - 1u);
    for (uint32_t i = t; i < (nbins << logr); i += kHistThreads) hist[i] = 0u;
    __syncthreads();
    Walker<V> walk(w, pu, pv);
    uint4 u0, u1, u2, v0, v1, v2;
    u0 = u1 = u2 = v0 = v1 = v2 = make_uint4(0u, 0u, 0u, 0u);
    uint32_t k0, k1, k2, y0, y1, y2;
    bool ok0, ok1, ok2;
    walk.fetch(u0, v0, k0, y0, ok0);
    walk.fetch(u1, v1, k1, y1, ok1);
    while (ok0) {
        walk.fetch(u2, v2, k2, y2, ok2);
        bool m[4];
        walk.mask(k0, y0, m);
        const uint32_t su[4] = {u0.x, u0.y, u0.z, u0.w}, sv[4] = {v0.x, v0.y, v0.z, v0.w};
        uint32_t bin[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bin[j] = bin_of(su[j], uoff, uscale, (int)nu);
            if (V) bin[j] += nu * bin_of(sv[j], voff, vscale, (int)nv);
        }
        // the wave's pre-count of a line of one bin
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin[0]);
        const bool differ = bin[0] != first || bin[1] != first || bin[2] != first || bin[3] != first;
        if (__builtin_amdgcn_ballot_w64(differ) == 0ull) {
            uint32_t n = 0;
            uint64_t any = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint64_t bj = __builtin_amdgcn_ballot_w64(m[j]);
                n += (uint32_t)__popcll(bj);
                any |= bj;
            }
            const uint64_t below = (1ull << (t & 63u)) - 1ull;
            if (((any >> (t & 63u)) & 1ull) && !(any & below))  // the first lane with a voxel
                __hip_atomic_fetch_add(&hist[(first << logr) + rep], n, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j])
                    __hip_atomic_fetch_add(&hist[(bin[j] << logr) + rep], 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        u0 = u1; v0 = v1; k0 = k1; y0 = y1; ok0 = ok1;
        u1 = u2; v1 = v2; k1 = k2; y1 = y2; ok1 = ok2;
    }
    __syncthreads();
    for (uint32_t i = t; i < nbins; i += kHistThreads) {
        uint32_t sum = 0;
        for (uint32_t r = 0; r < (1u << logr); r++) sum += hist[(i << logr) + r];
        if (sum)
            __hip_atomic_fetch_add(&counts[i], (unsigned long long)sum, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kHistThreads, 8) void k_plane_range(const float *__restrict__ p,
                                                                 PlaneWalk w,
                                                                 uint32_t *__restrict__ keys,
                                                                 unsigned long long *__restrict__ n_nan) {
    Walker<0> walk(w, p, p);
    uint4 u0, u1, u2, unused;
    u0 = u1 = u2 = unused = make_uint4(0u, 0u, 0u, 0u);
    uint32_t k0, k1, k2, y0, y1, y2;
    bool ok0, ok1, ok2;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, nan = 0u;
    walk.fetch(u0, unused, k0, y0, ok0);
    walk.fetch(u1, unused, k1, y1, ok1);
    while (ok0) {
        walk.fetch(u2, unused, k2, y2, ok2);
        bool m[4];
        walk.mask(k0, y0, m);
        const uint32_t s[4] = {u0.x, u0.y, u0.z, u0.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool is_nan = (s[j] & 0x7FFFFFFFu) > 0x7F800000u;
            // the monotone key: negative patterns reversed below the non-negative ones
            const uint32_t key = (s[j] & 0x80000000u) ? ~s[j] : s[j] ^ 0x80000000u;
            if (m[j] && !is_nan) {
                lo = min(lo, key);
                hi = max(hi, key);
            }
            nan += m[j] && is_nan ? 1u : 0u;
        }
        u0 = u1; k0 = k1; y0 = y1; ok0 = ok1;
        u1 = u2; k1 = k2; y1 = y2; ok1 = ok2;
    }
    for (int d = 32; d > 0; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d));
        nan += (uint32_t)__shfl_xor((int)nan, d);  // (a workgroup visits < 2^32 slots)
    }
    if ((threadIdx.x & 63u) == 0) {
        if (lo <= hi) {  // the wave saw a number
            atomicMin(&keys[0], lo);
            atomicMax(&keys[1], hi);
        }
        if (nan) atomicAdd(n_nan, (unsigned long long)nan);
    }
}

namespace {

// The walk of box = {x0, x1, y0, y1, z0, z1} (checked by the caller: inside the grid,
// not empty) over planes of grid nx x ny x nz, and the grid that walks it: `cus` x 2
// workgroups (two of 1024 threads fill a CU), no more than there are rounds of lines,
// and as many more as keep a workgroup's slots below 2^32.
hipError_t plan_walk(uint64_t psy, uint64_t psz, int nx, int ny, int nz, const int *box,
                     PlaneWalk &w, uint32_t &grid) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx >= 65536 || ny >= 65536 || nz >= 65536)
        return hipErrorInvalidValue;
    uint64_t sy, sz;
    plane_pitches((uint32_t)nx, (uint32_t)ny, sy, sz);
    if (sy != psy || sz != psz) return hipErrorInvalidValue;
    if (box[0] < 0 || box[0] >= box[1] || box[1] > nx || box[2] < 0 || box[2] >= box[3] ||
        box[3] > ny || box[4] < 0 || box[4] >= box[5] || box[5] > nz)
        return hipErrorInvalidValue;
    w = PlaneWalk();
    w.psy = psy;
    w.psz = psz;
    w.kx0 = (uint32_t)box[0] / kPlaneStride;
    w.nkx = (uint32_t)(box[1] - 1) / kPlaneStride - w.kx0 + 1u;
    w.yp0 = (uint32_t)box[2] / 2u;
    w.nyp = (uint32_t)(box[3] - 1) / 2u - w.yp0 + 1u;
    w.z0 = (uint32_t)box[4];
    w.nz = (uint32_t)(box[5] - box[4]);
    w.x0 = (uint32_t)box[0];
    w.xw = (uint32_t)(box[1] - box[0]);
    w.y0 = (uint32_t)box[2];
    w.yh = (uint32_t)(box[3] - box[2]);
    const uint64_t lines = (uint64_t)w.nkx * w.nyp * w.nz;
    const uint64_t rounds = (lines + kHistLines - 1u) / kHistLines;
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    uint64_t g = std::min<uint64_t>((uint64_t)(cus > 0 ? cus : 256) * 2u, rounds);
    g = std::max<uint64_t>(g, (rounds + kHistMaxRounds - 1u) / kHistMaxRounds);
    if (g == 0 || g > 0x7FFFFFFFull / kHistLines) return hipErrorInvalidValue;
    grid = (uint32_t)g;
    const uint64_t stride = g * kHistLines;
    w.da = (uint32_t)(stride % w.nkx);
    w.db = (uint32_t)((stride / w.nkx) % w.nyp);
    w.dc = (uint32_t)std::min<uint64_t>(stride / w.nkx / w.nyp, w.nz);
    return hipSuccess;
}

}  // namespace

hipError_t launch_plane_hist(const float *pu, const float *pv, uint64_t psy, uint64_t psz, int nx,
                             int ny, int nz, const int *box, float uoff, float uscale, int nu,
                             float voff, float vscale, int nv, unsigned long long *counts,
                             hipStream_t s) {
    if (!pu || !counts || nu < 1 || nv < 1 || (int64_t)nu * nv > (int64_t)kHistMax ||
        (!pv && nv != 1))
        return hipErrorInvalidValue;
    PlaneWalk w;
    uint32_t grid = 0;
    const hipError_t pe = plan_walk(psy, psz, nx, ny, nz, box, w, grid);
    if (pe != hipSuccess) return pe;
    const uint32_t nbins = (uint32_t)(nu * nv);
    uint32_t logr = 0;
    while (logr < 5u && ((uint64_t)nbins << (logr + 1u)) * sizeof(uint32_t) <= kHistLdsBytes) logr++;
    const size_t lds = ((size_t)nbins << logr) * sizeof(uint32_t);
    if (pv)
        hipLaunchKernelGGL(k_plane_hist<1>, dim3(grid), dim3(kHistThreads), lds, s, pu, pv, w, uoff,
                           uscale, voff, vscale, (uint32_t)nu, (uint32_t)nv, logr, counts);
    else
        hipLaunchKernelGGL(k_plane_hist<0>, dim3(grid), dim3(kHistThreads), lds, s, pu, pu, w, uoff,
                           uscale, 0.0f, 1.0f, (uint32_t)nu, 1u, logr, counts);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_plane_hist", 1, pv ? 1 : 0);
    return e;
}

hipError_t launch_plane_range(const float *p, uint64_t psy, uint64_t psz, int nx, int ny, int nz,
                              const int *box, uint32_t *keys, unsigned long long *n_nan,
                              hipStream_t s) {
    if (!p || !keys || !n_nan) return hipErrorInvalidValue;
    PlaneWalk w;
    uint32_t grid = 0;
    const hipError_t pe = plan_walk(psy, psz, nx, ny, nz, box, w, grid);
    if (pe != hipSuccess) return pe;
    hipLaunchKernelGGL(k_plane_range, dim3(grid), dim3(kHistThreads), 0, s, p, w, keys, n_nan);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_plane_range", 1, 0);
    return e;
}

}  // namespace vr
