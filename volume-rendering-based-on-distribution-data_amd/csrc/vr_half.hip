// vr_half.hip -- f16 record volumes: the per-ray
// pipelined march of methods 1/2/3 over IEEE binary16 records and the kernel
// that narrows a resident fp32 volume to them.
//
//  k_march_pipe_h<B,M,COUNT>  march_pipe_tile (vr_march.h) over _Float16
//                             records: one lane per ray, the next step's 8
//                             corners gathered while this one decodes.  The
//                             prefetched records stay packed, two halves per
//                             VGPR, and a corner is widened to float only when
//                             it is decoded; f16 -> f32 is exact, so from there
//                             on the arithmetic is the fp32 march's
//                             (record_stat / entropy_col per corner, blend8)
//                             and the frame is bit-identical to the fp32 march
//                             of the widened records.  COUNT: the
//                             footprint-marking pass that counts U.
//  k_narrow_f16               fp32 -> f16, round to nearest even, subnormals kept
#include "vr_device.h"
#include "vr_half.h"
#include "vr_internal.h"
#include "vr_march.h"
#include "vr_quad.h"

namespace vr {

__device__ __forceinline__ uint64_t corner_index_h(const Params &P, const Foot &f, int j) {
    const uint64_t z = (j & 4) ? (uint64_t)f.z1 : (uint64_t)f.z0;
    const uint64_t y = (j & 2) ? (uint64_t)f.y1 : (uint64_t)f.y0;
    const uint64_t x = (j & 1) ? (uint64_t)f.x1 : (uint64_t)f.x0;
    return z * P.sz + y * P.sy + x;
}

// corners J0 .. J0 + N - 1 of footprint f (corner j: x = j & 1, y = j & 2, z = j & 4,
// the order of gather8), records in x rows
template <int B, int N>
__device__ __forceinline__ void gather_h(const _Float16 *__restrict__ vol, const Params &P,
                                         const Foot &f, int j0, RecH<B> (&rec)[N]) {
#pragma unroll
    for (int j = 0; j < N; j++) load_rec_h<B>(vol, corner_index_h(P, f, j0 + j), rec[j]);
}

// the statistic of one packed record: widened here, then exactly the fp32
// march's decode (decode8: the entropy through this wave's LDS column)
template <int B, int M>
__device__ __forceinline__ float stat_h(const Params &P, const RecH<B> &r, float *st,
                                        const LogEnt *tab) {
    float p[B];
    widen_rec<B>(r, p);
    if constexpr (M == 3) return entropy_stash<B>(p, st, threadIdx.x & 63u, P.enorm, tab);
    else return record_stat<B, M>(p, P.enorm);
}

// B <= 16: two packed sets of 8 corners (B = 16: 2 x 64 VGPRs), the loop
// unrolled by two so they swap roles without copies -- march_pipe_tile
template <int B, int M, bool COUNT>
__device__ __forceinline__ int march_h_tile(const _Float16 *__restrict__ vol, const Params &P,
                                            uint32_t slot, uint32_t tile, uint32_t tid, float *st,
                                            const LogEnt *tab) {
    uint32_t lx, ly;
    lane_pixel(P, tid, lx, ly);
    const uint32_t x = (tile % P.tiles_x) * kTileW + lx;
    const uint32_t y = (tile / P.tiles_x) * kTileH + ly;
    if (x >= P.CW || y >= P.CH) return -1;  // no cross-lane work in this kernel
    const uint64_t o = P.tile_list ? (uint64_t)slot * 256u + ly * kTileW + lx
                                   : (uint64_t)y * P.W + x;
    Ray r;
    if (!make_ray(P, x, y, r)) {
        write_miss(P, o);
        return -1;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    float t = r.tnear;
    float px = r.ox + r.dx * r.tnear, py = r.oy + r.dy * r.tnear, pz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int n = 0;
    bool alive = true;
    Foot fa = footprint(P, px, py, pz), fb;
    RecH<B> ra[8], rb[8];
    gather_h<B, 8>(vol, P, fa, 0, ra);
    // one step: decode (fc, rc) while the gathers of the next step go to (fn, rn);
    // the next step is gathered unconditionally (clamped indices: always valid)
    auto step = [&](int i, const Foot &fc, const RecH<B> (&rc)[8], Foot &fn, RecH<B> (&rn)[8]) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        fn = footprint(P, nx, ny, nz);
        gather_h<B, 8>(vol, P, fn, 0, rn);
        if constexpr (COUNT) mark_foot(P, fc);
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = stat_h<B, M>(P, rc[j], st, tab);
        const float sample = blend8(s, fc);
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
    write_pixel(P, o, n, sx * P.brightness, sy * P.brightness, sz * P.brightness,
                sw * P.brightness);
    return n;
}

// B = 32: two packed sets of 8 corners would be 256 VGPRs, so the corners go in
// two batches of 4 (64 packed VGPRs each), as march_wide_tile's: while one batch
// decodes, the other -- after a step's second batch, the first batch of the next
// step's footprint, gathered unconditionally -- is in flight.  A 32-bin f16
// record is 64 B, half a line.
template <int M, bool COUNT>
__device__ __forceinline__ int march_h32_tile(const _Float16 *__restrict__ vol, const Params &P,
                                              uint32_t slot, uint32_t tile, uint32_t tid,
                                              float *st, const LogEnt *tab) {
    constexpr int B = 32;
    uint32_t lx, ly;
    lane_pixel(P, tid, lx, ly);
    const uint32_t x = (tile % P.tiles_x) * kTileW + lx;
    const uint32_t y = (tile / P.tiles_x) * kTileH + ly;
    if (x >= P.CW || y >= P.CH) return -1;  // no cross-lane work in this kernel
    const uint64_t o = P.tile_list ? (uint64_t)slot * 256u + ly * kTileW + lx
                                   : (uint64_t)y * P.W + x;
    Ray r;
    if (!make_ray(P, x, y, r)) {
        write_miss(P, o);
        return -1;
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    float t = r.tnear;
    float px = r.ox + r.dx * r.tnear, py = r.oy + r.dy * r.tnear, pz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int n = 0;
    Foot fc = footprint(P, px, py, pz);
    RecH<B> ra[4], rb[4];
    gather_h<B, 4>(vol, P, fc, 0, ra);
    for (int i = 0; i < kMaxSteps; i++) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        const Foot fn = footprint(P, nx, ny, nz);
        if constexpr (COUNT) mark_foot(P, fc);
        float s[8];
        gather_h<B, 4>(vol, P, fc, 4, rb);
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = stat_h<B, M>(P, ra[j], st, tab);
        gather_h<B, 4>(vol, P, fn, 0, ra);
#pragma unroll
        for (int j = 0; j < 4; j++) s[4 + j] = stat_h<B, M>(P, rb[j], st, tab);
        const float sample = blend8(s, fc);
        n = i + 1;
        if (composite(P, sample, sx, sy, sz, sw) || !cont) break;
        t = tn;
        px = nx;
        py = ny;
        pz = nz;
        fc = fn;
    }
    write_pixel(P, o, n, sx * P.brightness, sy * P.brightness, sz * P.brightness,
                sw * P.brightness);
    return n;
}

// Waves per SIMD the register allocation may assume: the caps of
// the fp32 marches this one mirrors -- 3 at B = 8 (k_march_pipe: the budget keeps
// the next step's gathers in flight), 2 for the wide records (k_march_wide), no
// cap for narrow records.
#ifndef VR_PIPEH_MAXWAVES
#define VR_PIPEH_MAXWAVES(B) ((B) >= 16 ? 2 : (B) >= 8 ? 3 : 8)
#endif
template <int B, int M, bool COUNT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, VR_PIPEH_MAXWAVES(B)))) void k_march_pipe_h(const _Float16 *__restrict__ vol, Params P) {
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    float *st = nullptr;
    const LogEnt *tab = nullptr;
    if constexpr (M == 3) {  // entropy: rolled per-bin sums over LDS record columns
        // (in the dynamic LDS, the launch requests sizeof(EntropyLds<B>) at least)
        extern __shared__ __attribute__((aligned(32))) float s_dyn[];
        EntropyLds<B> *el = reinterpret_cast<EntropyLds<B> *>(s_dyn);
        copy_logtab(el->tab);
        __syncthreads();
        st = el->col + (threadIdx.x >> 6) * 64u * B;
        tab = el->tab;
    }
    int n;
    if constexpr (B == 32) n = march_h32_tile<M, COUNT>(vol, P, slot, tile, threadIdx.x, st, tab);
    else n = march_h_tile<B, M, COUNT>(vol, P, slot, tile, threadIdx.x, st, tab);
    if constexpr (!COUNT) {
        if (P.tile_cost) record_tile_cost(P, tile, n);  // all lanes have reconverged here
    }
}

// fp32 -> f16 over the whole pitched buffer (n floats): 16 bytes read and 8
// written per lane, coalesced, for the first n4 groups of four; the floats
// after them one by one (n % 4 of them, or all n when the source is not 16-byte
// aligned: n4 = 0).  (_Float16) of a float is v_cvt_f16_f32: round to nearest
// even, subnormal results kept (the f16 denormal mode of a HIP kernel is IEEE).
__global__ __launch_bounds__(256) void k_narrow_f16(const float *__restrict__ src,
                                                    _Float16 *__restrict__ dst, uint64_t n,
                                                    uint64_t n4) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const uint64_t t0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    for (uint64_t i = t0; i < n4; i += stride) {
        const float4 q = reinterpret_cast<const float4 *>(src)[i];
        const uint32_t a = __builtin_bit_cast(uint16_t, (_Float16)q.x);
        const uint32_t b = __builtin_bit_cast(uint16_t, (_Float16)q.y);
        const uint32_t c = __builtin_bit_cast(uint16_t, (_Float16)q.z);
        const uint32_t d = __builtin_bit_cast(uint16_t, (_Float16)q.w);
        reinterpret_cast<uint2 *>(dst)[i] = make_uint2(a | (b << 16), c | (d << 16));
    }
    for (uint64_t i = (n4 << 2) + t0; i < n; i += stride) dst[i] = (_Float16)src[i];
}

template <int B, bool COUNT>
static hipError_t march_h_b(const MarchPlan &pl, const _Float16 *vol, const Params &P,
                            uint32_t nslots, hipStream_t s) {
    const dim3 grid(nslots), block(256);
    const size_t lds = cap_lds(P, pl.cap);
    switch (pl.method) {
    case 1: hipLaunchKernelGGL((k_march_pipe_h<B, 1, COUNT>), grid, block, lds, s, vol, P); break;
    case 2: hipLaunchKernelGGL((k_march_pipe_h<B, 2, COUNT>), grid, block, lds, s, vol, P); break;
    // (the entropy march's LDS columns and table are part of the request)
    case 3: hipLaunchKernelGGL((k_march_pipe_h<B, 3, COUNT>), grid, block, cap_lds(P, pl.cap, sizeof(EntropyLds<B>)), s, vol, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <bool COUNT>
static hipError_t march_h_dispatch(const MarchPlan &pl, const _Float16 *vol, const Params &P,
                                   uint32_t nslots, hipStream_t s) {
    switch (pl.B) {
    case 1: return march_h_b<1, COUNT>(pl, vol, P, nslots, s);
    case 2: return march_h_b<2, COUNT>(pl, vol, P, nslots, s);
    case 4: return march_h_b<4, COUNT>(pl, vol, P, nslots, s);
    case 8: return march_h_b<8, COUNT>(pl, vol, P, nslots, s);
    case 16: return march_h_b<16, COUNT>(pl, vol, P, nslots, s);
    case 32: return march_h_b<32, COUNT>(pl, vol, P, nslots, s);
    default: return hipErrorInvalidValue;  // no runtime-B path for f16
    }
}

// Kind::PipeH of the plan; pl.count: the footprint-marking pass (P.mark)
hipError_t launch_march_h(const MarchPlan &pl, const void *vol, const Params &P, uint32_t nslots,
                          hipStream_t s) {
    const _Float16 *v = static_cast<const _Float16 *>(vol);
    return pl.count ? march_h_dispatch<true>(pl, v, P, nslots, s)
                    : march_h_dispatch<false>(pl, v, P, nslots, s);
}

hipError_t launch_narrow_f16(const float *src, void *dst, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    // dst is the library's own allocation (256-byte aligned); an adopted source
    // may sit at any float
    const uint64_t n4 = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 ? n >> 2 : 0;
    uint64_t blocks = ((n4 ? n4 : n) + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_narrow_f16, dim3((uint32_t)blocks), dim3(256), 0, s, src,
                       static_cast<_Float16 *>(dst), n, n4);
    return hipGetLastError();
}

}  // namespace vr
