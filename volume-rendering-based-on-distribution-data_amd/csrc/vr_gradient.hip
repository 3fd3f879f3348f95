// vr_gradient.hip -- gradient-magnitude planes of baked planes.
//
// k_bake_grad: the central-difference gradient magnitude of every voxel of a baked
// plane (one float per voxel in 16 x 2 x 1 bricks, plane_index), into a plane of
// the same layout, and the maximum over the volume.  One float32 operation at a
// time, no fma (the build's -ffp-contract=off), one correctly rounded square root
// per voxel:
//     xm = x > 0 ? x - 1 : 0      xp = x + 1 < nx ? x + 1 : nx - 1       (y, z alike)
//     Gx = (s(xp, y, z) - s(xm, y, z)) * (xp - xm == 2 ? nx * 0.5f : nx)
//     m  = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz)
//
// A 7-point stencil bound by HBM.  Threads map to output slots in brick order, so a
// wave stores two whole 128-B lines; the apron slot of a brick (offset 15: the
// voxel x = 15 (k + 1)) is computed by its own thread like any other.  A workgroup
// of 1024 threads owns a tile of kGradBX bricks by kGradYP y pairs and walks
// kGradZC slices of z: a thread keeps s(z - 1), s(z), s(z + 1) of its own voxel in
// registers (one new load per slice) and finds its x and y neighbours in an LDS
// tile of the current slice with a one-voxel halo, which the first kGradHalo
// threads load, clamped to the volume.  The tile is double-buffered: one barrier
// per slice.  Slice z needs s(z + 1), so the own value is loaded two slices ahead and
// the halo one: while slice z is computed the loads of s(z + 2) and of the halo of
// z + 1 are in flight.
#include "vr_internal.h"

namespace vr {

namespace {

constexpr uint32_t kGradBX = 4;                          // bricks of a tile in x
constexpr uint32_t kGradYP = 8;                          // y pairs of a tile
constexpr uint32_t kGradZC = 64;                         // slices of a z chunk
constexpr uint32_t kGradThreads = 32u * kGradBX * kGradYP;
constexpr uint32_t kGradTW = kPlaneStride * kGradBX + 1; // tile columns, the last apron included
constexpr uint32_t kGradTH = 2u * kGradYP;               // tile rows
constexpr uint32_t kGradLW = kGradTW + 2u;               // with the halo: 63 (odd: no bank conflicts)
constexpr uint32_t kGradLH = kGradTH + 2u;
constexpr uint32_t kGradHalo = 2u * kGradTW + 2u * kGradTH;  // halo voxels of a slice (no corners)
static_assert(kGradThreads == 1024 && kGradHalo <= kGradThreads, "one workgroup, one tile");

// the in-slice part of plane_index (a slice is < 2^32 floats)
__device__ __forceinline__ uint32_t slice_index(uint32_t x, uint32_t y, uint32_t psy) {
    return (y >> 1) * psy + (y & 1u) * 16u + plane_bx(x);
}

}  // namespace

__global__ __launch_bounds__(kGradThreads) void k_bake_grad(const float *__restrict__ src,
                                                            float *__restrict__ out, uint64_t psy,
                                                            uint64_t psz, uint32_t nx, uint32_t ny,
                                                            uint32_t nz,
                                                            uint32_t *__restrict__ max_bits) {
    __shared__ float tile[2][kGradLH * kGradLW];
    const uint32_t t = threadIdx.x;
    // the thread's output slot: brick kx, y pair yp, offset o
    const uint32_t o = t & 31u, b = (t >> 5) % kGradBX, p = t / (32u * kGradBX);
    const uint32_t kx = blockIdx.x * kGradBX + b, yp = blockIdx.y * kGradYP + p;
    const uint32_t nbx = (uint32_t)(psy / 32u), nyp = (ny + 1u) / 2u;
    const uint32_t x0 = blockIdx.x * (kPlaneStride * kGradBX), y0 = blockIdx.y * kGradTH;
    // its voxel, and the voxel's cell in the LDS tile (halo: column 0 and row 0)
    const uint32_t lx = kPlaneStride * b + (o & 15u) + 1u, ly = 2u * p + (o >> 4) + 1u;
    const uint32_t x = x0 + lx - 1u, y = y0 + ly - 1u;
    const bool slot = kx < nbx && yp < nyp;  // the slot exists (vox implies it)
    const bool vox = x < nx && y < ny;       // and holds a voxel: +0 otherwise
    const uint32_t own = vox ? slice_index(x, y, (uint32_t)psy) : 0u;
    const uint32_t dst = yp * (uint32_t)psy + kx * 32u + o;
    const uint32_t cell = ly * kGradLW + lx;
    // the neighbours' cells, clamped at the volume's faces, and the spacings
    const uint32_t cxm = x > 0 ? cell - 1u : cell, cxp = x + 1u < nx ? cell + 1u : cell;
    const uint32_t cym = y > 0 ? cell - kGradLW : cell, cyp = y + 1u < ny ? cell + kGradLW : cell;
    const float hx = cxp - cxm == 2u ? (float)nx * 0.5f : (float)nx;
    const float hy = cyp - cym == 2u * kGradLW ? (float)ny * 0.5f : (float)ny;
    // the thread's halo voxel, if it has one: rows y0 - 1 and y0 + TH over the tile's
    // columns, then columns x0 - 1 and x0 + TW over its rows, clamped to the volume
    const bool hal = t < kGradHalo;
    uint32_t hcell = 0, hoff = 0;
    if (hal) {
        uint32_t hxv, hyv;
        if (t < 2u * kGradTW) {
            const uint32_t r = t / kGradTW, c = t % kGradTW;
            hxv = x0 + c;
            hyv = r ? y0 + kGradTH : (y0 > 0 ? y0 - 1u : 0u);
            hcell = (r ? kGradLH - 1u : 0u) * kGradLW + c + 1u;
        } else {
            const uint32_t r = (t - 2u * kGradTW) / kGradTH, c = (t - 2u * kGradTW) % kGradTH;
            hxv = r ? x0 + kGradTW : (x0 > 0 ? x0 - 1u : 0u);
            hyv = y0 + c;
            hcell = (c + 1u) * kGradLW + (r ? kGradLW - 1u : 0u);
        }
        hoff = slice_index(min(hxv, nx - 1u), min(hyv, ny - 1u), (uint32_t)psy);
    }
    const uint32_t z0 = blockIdx.z * kGradZC, z1 = min(z0 + kGradZC, nz);
    const uint32_t zlast = min(z1, nz - 1u);  // the last slice the chunk reads
    uint32_t mx = 0;
    // One slice: s0 = s(z) goes to the tile with the halo value hc of slice z, sm and
    // sp are s(z - 1) and s(z + 1); sq receives s(z + 2) and hn the halo of z + 1, both
    // loaded before anything is waited for.  Every thread issues both loads (a thread
    // without a voxel or a halo voxel reads float 0 of the slice and drops it), so the
    // number of loads in flight at each wait is fixed and the wait for sp and hc leaves
    // the two new ones in flight.
    auto step = [&](float sm, float s0, float sp, float &sq, float hc, float &hn, uint32_t z) {
        sq = src[(uint64_t)min(z + 2u, zlast) * psz + own];
        hn = src[(uint64_t)min(z + 1u, z1 - 1u) * psz + hoff];
        float *T = tile[z & 1u];
        if (vox) T[cell] = s0;
        if (hal) T[hcell] = hc;
        __syncthreads();
        float m = 0.0f;
        if (vox) {
            const uint32_t zm = z > 0 ? z - 1u : 0u, zp = z + 1u < nz ? z + 1u : nz - 1u;
            const float hz = zp - zm == 2u ? (float)nz * 0.5f : (float)nz;
            const float gx = (T[cxp] - T[cxm]) * hx;
            const float gy = (T[cyp] - T[cym]) * hy;
            const float gz = (sp - sm) * hz;
            m = sqrtf((gx * gx + gy * gy) + gz * gz);
            mx = max(mx, __float_as_uint(m));
        }
        if (slot) out[(uint64_t)z * psz + dst] = m;
    };
    float ra = src[(uint64_t)(z0 > 0 ? z0 - 1u : 0u) * psz + own];
    float rb = src[(uint64_t)z0 * psz + own];
    float rc = src[(uint64_t)min(z0 + 1u, nz - 1u) * psz + own];
    float rd, ha = src[(uint64_t)z0 * psz + hoff], hb;
    // four slices a round: the registers rotate by name, no value is moved
    for (uint32_t z = z0; z < z1; z += 4u) {
        step(ra, rb, rc, rd, ha, hb, z);
        if (z + 1u >= z1) break;
        step(rb, rc, rd, ra, hb, ha, z + 1u);
        if (z + 2u >= z1) break;
        step(rc, rd, ra, rb, ha, hb, z + 2u);
        if (z + 3u >= z1) break;
        step(rd, ra, rb, rc, hb, ha, z + 3u);
    }
    // m >= +0: the maximum of the floats is the unsigned maximum of their bits
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    if ((t & 63u) == 0 && mx) atomicMax(max_bits, mx);
}

hipError_t launch_bake_grad(const float *src, float *out, uint64_t psy, uint64_t psz, int nx,
                            int ny, int nz, uint32_t *max_bits, hipStream_t s) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || nx >= 65536 || ny >= 65536 || nz >= 65536)
        return hipErrorInvalidValue;
    uint64_t sy, sz;
    plane_pitches((uint32_t)nx, (uint32_t)ny, sy, sz);
    if (sy != psy || sz != psz) return hipErrorInvalidValue;
    const uint32_t nbx = (uint32_t)(psy / 32u), nyp = (uint32_t)(ny + 1) / 2u;
    const dim3 grid((nbx + kGradBX - 1u) / kGradBX, (nyp + kGradYP - 1u) / kGradYP,
                    ((uint32_t)nz + kGradZC - 1u) / kGradZC);
    hipLaunchKernelGGL(k_bake_grad, grid, dim3(kGradThreads), 0, s, src, out, psy, psz,
                       (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, max_bits);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) note_kernel("k_bake_grad", 1, 0);
    return e;
}

}  // namespace vr
