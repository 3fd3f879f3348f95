// vr_query.h -- the per-ray pipelined march and the bake of a per-corner
// statistic of float or _Float16 records in x rows, shared by the weighted-bin
// query (method 10, vr_query.hip), the quantile query (method 11,
// vr_quantile.hip), the distribution-distance query (method 12,
// vr_distance.hip) and the level-crossing query (method 13, vr_crossing.hip).
// The statistic differs: a functor S with
//     template <typename T, int B> float operator()(const LinRec<T, B> &) const
// uniform over the launch (its state comes from a kernel argument after Params).
// What is made of a step's 8 corner statistics is a functor too,
//     float operator()(const float (&s)[8], const Foot &) const
// the trilinear blend (Blend8) unless a query says otherwise (method 13: a joint
// function of the corners, CrossCombine).  The plane march under a user-defined
// transfer function (vr_transfer.hip) takes lin_ray and the two functors from here.
#pragma once
#include "vr_device.h"
#include "vr_half.h"
#include "vr_internal.h"
#include "vr_march.h"

namespace vr {

// a corner's record as it is kept between gather and decode: floats, or the
// halves still packed two per register (widened at decode)
template <typename T, int B>
struct LinRec {
    float p[B];
};
template <int B>
struct LinRec<_Float16, B> {
    RecH<B> h;
};

template <typename T, int B>
__device__ __forceinline__ void load_lin(const T *__restrict__ vol, uint64_t vidx,
                                         LinRec<T, B> &r) {
    if constexpr (std::is_same<T, float>::value) load_rec<B>(vol, vidx, r.p);
    else load_rec_h<B>(vol, vidx, r.h);
}

// corners J0 .. J0 + N - 1 of footprint f (corner j: x = j & 1, y = j & 2,
// z = j & 4, the order of gather8), records in x rows.  The footprint's indices
// are clamped to the volume, so every corner is a valid record.
template <typename T, int B, int N>
__device__ __forceinline__ void gather_lin(const T *__restrict__ vol, const Params &P,
                                           const Foot &f, int j0, LinRec<T, B> (&rec)[N]) {
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int c = j0 + j;
        const uint64_t z = (c & 4) ? (uint64_t)f.z1 : (uint64_t)f.z0;
        const uint64_t y = (c & 2) ? (uint64_t)f.y1 : (uint64_t)f.y0;
        const uint64_t x = (c & 1) ? (uint64_t)f.x1 : (uint64_t)f.x0;
        load_lin<T, B>(vol, z * P.sz + y * P.sy + x, rec[j]);
    }
}

// Corners gathered per batch.  8: two whole sets of 8 corners, the loop unrolled
// by two so they swap roles without copies (march_pipe_tile); it fits while two
// sets stay within 128 registers: fp32 B <= 8, f16 B <= 16.  Wider records go in
// batches of 4 or 2 corners (64 registers a batch, two batches live), as
// march_h32_tile and march_wide_tile do, so no instance needs scratch.
template <typename T, int B>
constexpr int lin_batch() {
    constexpr int regs = std::is_same<T, float>::value ? B : (B + 1) / 2;  // per corner
    return regs <= 8 ? 8 : regs <= 16 ? 4 : 2;
}

// the trilinear filter of the 8 corner statistics (blend8, vr_march.h): the
// default of the loops below
struct Blend8 {
    __device__ __forceinline__ float operator()(const float (&s)[8], const Foot &f) const {
        return blend8(s, f);
    }
};

// The combine of the level-crossing query: all float,
// every operation separate, in corner order (gather8's: x = c & 1, y = c & 2,
// z = c & 4), nothing clamped, subnormal products kept.  The filter weights of the
// footprint are not read: the sample is constant inside a cell.  Corners that the
// clamped footprint makes coincide enter once per fetch.
struct CrossCombine {
    __device__ __forceinline__ float operator()(const float (&s)[8], const Foot &) const {
        float lo = s[0], hi = 1.0f - s[0];
#pragma unroll
        for (int c = 1; c < 8; c++) {
            lo = lo * s[c];
            hi = hi * (1.0f - s[c]);
        }
        return (1.0f - lo) - hi;
    }
};

// the ray of thread tid of a tile; false: outside the rendered rectangle or a
// miss (written), nothing to march
struct LinRay {
    Ray r;
    uint64_t o;
};
__device__ __forceinline__ bool lin_ray(const Params &P, uint32_t slot, uint32_t tile,
                                        uint32_t tid, LinRay &q) {
    uint32_t lx, ly;
    lane_pixel(P, tid, lx, ly);
    const uint32_t x = (tile % P.tiles_x) * kTileW + lx;
    const uint32_t y = (tile / P.tiles_x) * kTileH + ly;
    if (x >= P.CW || y >= P.CH) return false;  // no cross-lane work in this kernel
    q.o = P.tile_list ? (uint64_t)slot * 256u + ly * kTileW + lx : (uint64_t)y * P.W + x;
    if (!make_ray(P, x, y, q.r)) {
        write_miss(P, q.o);
        return false;
    }
    return true;
}

// two sets of 8 corners: march_pipe_tile / march_h_tile with st per corner
template <typename T, int B, typename S, typename BL = Blend8>
__device__ __forceinline__ int march_lin_tile(const T *__restrict__ vol, const Params &P,
                                              const S &st, uint32_t slot, uint32_t tile,
                                              uint32_t tid, const BL &bl = BL{}) {
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
    LinRec<T, B> ra[8], rb[8];
    gather_lin<T, B, 8>(vol, P, fa, 0, ra);
    // one step: decode (fc, rc) while the gathers of the next step go to (fn, rn);
    // the next step is gathered unconditionally (clamped indices: always valid)
    auto step = [&](int i, const Foot &fc, const LinRec<T, B> (&rc)[8], Foot &fn,
                    LinRec<T, B> (&rn)[8]) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        fn = footprint(P, nx, ny, nz);
        gather_lin<T, B, 8>(vol, P, fn, 0, rn);
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = st(rc[j]);
        const float sample = bl(s, fc);
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

// wide records: a step's corners in 8 / N batches of N, two batches live (ra, rb).
// While one batch decodes the next is in flight -- after a step's last batch, the
// first batch of the next step's footprint, gathered unconditionally
// (march_h32_tile's order for N = 4).
template <typename T, int B, int N, typename S, typename BL = Blend8>
__device__ __forceinline__ int march_lin_batched(const T *__restrict__ vol, const Params &P,
                                                 const S &st, uint32_t slot, uint32_t tile,
                                                 uint32_t tid, const BL &bl = BL{}) {
    static_assert(N == 1 || N == 2 || N == 4, "an even number of batches per step");
    LinRay q;
    if (!lin_ray(P, slot, tile, tid, q)) return -1;
    const Ray &r = q.r;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
    float t = r.tnear;
    float px = r.ox + r.dx * r.tnear, py = r.oy + r.dy * r.tnear, pz = r.oz + r.dz * r.tnear;
    const float stx = r.dx * kTStep, sty = r.dy * kTStep, stz = r.dz * kTStep;
    int n = 0;
    Foot fc = footprint(P, px, py, pz);
    LinRec<T, B> ra[N], rb[N];
    gather_lin<T, B, N>(vol, P, fc, 0, ra);
    for (int i = 0; i < kMaxSteps; i++) {
        const float tn = t + kTStep;                               // K:701
        const bool cont = !(tn > r.tfar) && (i + 1 < kMaxSteps);  // K:703, K:381
        const float nx = px + stx, ny = py + sty, nz = pz + stz;   // K:706
        const Foot fn = footprint(P, nx, ny, nz);
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; k += 2 * N) {
            gather_lin<T, B, N>(vol, P, fc, k + N, rb);
#pragma unroll
            for (int j = 0; j < N; j++) s[k + j] = st(ra[j]);
            if (k + 2 * N < 8) gather_lin<T, B, N>(vol, P, fc, k + 2 * N, ra);
            else gather_lin<T, B, N>(vol, P, fn, 0, ra);
#pragma unroll
            for (int j = 0; j < N; j++) s[k + N + j] = st(rb[j]);
        }
        const float sample = bl(s, fc);
        n = i + 1;
        if (composite(P, sample, sx, sy, sz, sw) || !cont) break;
        t = tn;
        px = nx;
        py = ny;
        pz = nz;
        fc = fn;
    }
    write_pixel(P, q.o, n, sx * P.brightness, sy * P.brightness, sz * P.brightness,
                sw * P.brightness);
    return n;
}

// the body of a march kernel: the tile of this workgroup, marched in batches of N
// corners (8: the two-set loop)
template <typename T, int B, int N, typename S, typename BL = Blend8>
__device__ __forceinline__ void march_lin_kernel(const T *__restrict__ vol, const Params &P,
                                                 const S &st, const BL &bl = BL{}) {
    const uint32_t slot = launch_slot(P);
    const uint32_t tile = tile_of(P, slot);
    if (tile == kPad) return;
    int n;
    if constexpr (N == 8) n = march_lin_tile<T, B>(vol, P, st, slot, tile, threadIdx.x, bl);
    else n = march_lin_batched<T, B, N>(vol, P, st, slot, tile, threadIdx.x, bl);
    if (P.tile_cost) record_tile_cost(P, tile, n);  // all lanes have reconverged here
}

// the body of a bake kernel.  One thread per voxel of an x row (grid: x blocks of
// 256, y rows, z slices), as k_bake_raw: each record read once, coalesced, its
// statistic written through put_plane (home position and, for x = 15 k, the
// apron of brick k - 1).
template <typename T, int B, typename S>
__device__ __forceinline__ void bake_lin_kernel(const T *vol, const Params &P, const S &st,
                                                float *out, uint64_t psy, uint64_t psz) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= (uint32_t)P.nx) return;
    const uint64_t off = (uint64_t)blockIdx.z * P.sz + (uint64_t)blockIdx.y * P.sy + x;
    LinRec<T, B> r;
    load_lin<T, B>(vol, off, r);
    put_plane(out, x, blockIdx.y, blockIdx.z, psy, psz, st(r));
}

// Host-side dispatch of the launchers (with_value, vr_internal.h): the bin counts
// the query kernels are compiled for (no runtime-B instance):
// f(std::integral_constant<int, B>{})
template <typename F>
inline bool with_bins(int nb, F &&f) {
    return with_value<1, 2, 4, 8, 16, 32>(nb, [&](auto B) {
        f(B);
        return true;
    });
}

// ... and the records' element type with them: f(v, B), v the volume as
// const float * or const _Float16 * (ElemOf<decltype(v)>, vr_internal.h: that type)
template <typename F>
inline bool with_records(const void *vol, bool half, int nb, F &&f) {
    return with_bins(nb, [&](auto B) {
        if (half) f(static_cast<const _Float16 *>(vol), B);
        else f(static_cast<const float *>(vol), B);
    });
}

// the grid of a bake launch; false: more rows or slices than a grid takes
inline bool bake_lin_grid(const Params &P, dim3 &grid) {
    if (P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || P.ny > 65535 || P.nz > 65535) return false;
    grid = dim3((uint32_t)(P.nx + 255) / 256u, (uint32_t)P.ny, (uint32_t)P.nz);
    return true;
}

}  // namespace vr
