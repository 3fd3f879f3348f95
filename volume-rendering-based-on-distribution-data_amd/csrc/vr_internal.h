// vr_internal.h -- declarations shared by the kernels and their launchers (*.hip)
// and the host-side library state / C-ABI (vr_api.cpp).  The kernel choice of
// the record marches is vr_plan.h's.  Not a public header.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vr_device.h"
#include "vr_plan.h"

namespace vr {

constexpr int kSynthBlobs = 8;   // Gaussian blobs of the scalar field
constexpr int kSynthG = 16;      // spread levels
constexpr int kSynthQ = 4096;    // quantised field levels

struct SynthArgs {
    float amp[kSynthBlobs];
    const float *gx, *gy, *gz;   // [k][n] separable blob factors
    const float *table;          // [g][q][nb] normalised histograms
    int nx, ny, nz, nb;
    uint64_t sy, sz;             // record pitch of a row / slice
    uint64_t seed;
};

// the synthetic volumes' hash: k_synth, k_synth_codec
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Host-side dispatch of the launchers, from a runtime value to the template
// argument of a compiled instance: f(std::integral_constant<int, V>{}) for the V
// among Vs that v equals, and what f returns (launched); false, nothing called:
// no instance for v.
template <int... Vs, typename F>
inline bool with_value(int v, F &&f) {
    return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}

// the element type behind a typed record pointer such a dispatch hands on
template <typename P>
using ElemOf = std::remove_cv_t<std::remove_pointer_t<P>>;

// records an error for vr_last_error() (vr_api.cpp); returns status
int record_error(int status, const char *msg);

// Launches the march a plan names (vr_plan.h: plan_march() is the only place
// that chooses a kernel; the launchers switch on the plan and decide nothing).
// vol: the records or baked plane the plan's kernel reads (halves for
// Kind::PipeH); the layout copies travel in P (bvol, avol).  A plan that names
// an instance that is not compiled returns hipErrorInvalidValue.  A
// non-counting launch records the plan's kernel name for vr_last_kernel().
hipError_t launch_plan(const MarchPlan &plan, const void *vol, const Params &P, uint32_t nslots,
                       hipStream_t s);
// launch_plan's per-file switches: method 7 (vr_m7.hip; -7: over the baked corner
// means), the ray-segmented marches (vr_seg.hip), f16 records (vr_half.hip)
hipError_t launch_march_m7(const MarchPlan &plan, const float *vol, const Params &P,
                           uint32_t nslots, hipStream_t s);
hipError_t launch_march_seg(const MarchPlan &plan, const float *vol, const Params &P,
                            uint32_t nslots, hipStream_t s);
hipError_t launch_march_h(const MarchPlan &plan, const void *vol, const Params &P,
                          uint32_t nslots, hipStream_t s);
// name of the march kernel the last non-counting launch ran (launch_plan: the
// plan's plan_kernel_name; the codec, flexible-block and GMM launchers: note_kernel)
const char *last_march_kernel();
void note_kernel(const char *kind, int B, int method);
// tuning knob `key` set through vr_set_tuning (nullptr if unset); a -DVR_TUNING
// build falls back to the environment.  The default build never reads it.
const char *tuning(const char *key);
hipError_t launch_march_codec(int nb, int method, const Params &P, uint32_t nslots, bool count,
                              hipStream_t s);
hipError_t launch_codec_bytes(const unsigned long long *bits, uint64_t nvox, const int4 *cb,
                              unsigned long long *total, hipStream_t s);
hipError_t launch_codec_check(const int4 *cb, uint64_t n, int ntpl, int nb, int slots,
                              unsigned long long *bad, hipStream_t s);
hipError_t launch_synth_codec(int4 *cb, float2 *err, const SynthArgs &a, int ntpl, int slots,
                              hipStream_t s);
// ---- flexible blocks (methods 8/9/0, vr_flex.hip) ----
// span key: six coordinates of 10 bits, low x/y/z then high x/y/z
__host__ __device__ inline uint64_t span_key(int lx, int ly, int lz, int hx, int hy, int hz) {
    return (uint64_t)lx | (uint64_t)ly << 10 | (uint64_t)lz << 20 | (uint64_t)hx << 30 |
           (uint64_t)hy << 40 | (uint64_t)hz << 50;
}
constexpr int kFlexMaxBins = 64;     // flexNBin (K:97)
constexpr int kFlexMaxDim = 126;     // dyadic split of K:1248-1282 stays within 6 spans per axis
struct FlexTables {                  // device arrays
    int dim, nb;
    const uint64_t *fkeys;           // fractal spans: sorted keys -> chosen entry
    const int32_t *fidx;
    int nfk;
    const int4 *fcode;               // template id, shift, flip, NE
    const float2 *ferr;              // nb (bin, value) pairs per entry
    const uint64_t *skeys;           // simple spans (0-based keys)
    const int32_t *sidx;
    int nsk;
    const int32_t *scount;
    const float2 *shist;             // nb (bin, freq) pairs per entry
    const float *tpl;                // [ntpl][nb]
};
hipError_t launch_flex_corners(const FlexTables &t, int block, int nblk, float *corner_hist,
                               unsigned int *missing, hipStream_t s);
hipError_t launch_flex_blocks(int nb, int nblk, const float *corner_hist, float4 *blocks,
                              hipStream_t s);
hipError_t launch_march_flex(int method, const Params &P, uint32_t nslots, hipStream_t s);
// ---- GMM volumes (config 5, vr_gmm.hip) ----
// half: the planes hold IEEE binary16 (k_march_gmm_h)
hipError_t launch_march_gmm(int K, int method, bool half, const Params &P, uint32_t nblocks,
                            bool count, hipStream_t s);
hipError_t launch_synth_gmm(void *wm, void *sg, bool half, const SynthArgs &a, int K, int z_base,
                            int nzs, hipStream_t s);
// the resident slices [z_base, z_base + nzs) of an nx x ny GMM volume decoded once
// per voxel (k_bake_gmm) into two whole-volume planes of `plane` floats at out
// (mean, then 16 x variance) in 16 x 2 x 1 bricks of pitches psy / psz; nx, ny and
// nzs beyond 65535: hipErrorInvalidValue
hipError_t launch_bake_gmm(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                           int z_base, int nzs, float *out, uint64_t plane, uint64_t psy,
                           uint64_t psz, hipStream_t s);
// ---- range probability of GMM volumes (method 10, vr_gmm.hip) ----
// the bounds of a launch: a kernel argument of their own after Params
struct GmmRange {
    float lo, hi;
};
// k_march_gmm_range / k_march_gmm_range_h: launch_march_gmm's march with the mass of
// the mixture in [lo, hi) per corner; records its name for vr_last_kernel() (M=10)
hipError_t launch_march_gmm_range(int K, bool half, const Params &P, const GmmRange &q,
                                  uint32_t nblocks, hipStream_t s);
// k_bake_gmm_range: the same statistic of the resident slices into one whole-volume
// plane at out (launch_bake_gmm's bricks, pitches and limits)
hipError_t launch_bake_gmm_range(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                                 int z_base, int nzs, const GmmRange &q, float *out, uint64_t psy,
                                 uint64_t psz, hipStream_t s);
// the table of Phi - 1/2 the kernels read: 4 arrays of kPhiRows floats (vr_phitab.h)
const float *gmm_phi_table_host();
// ---- baked statistics (basicDataProcessing, vr_stats.hip): planes of `plane`
// floats each in 16 x 2 x 1 bricks of plane pitches psy / psz (plane_index),
// statistic k+1 (raw) / C = k (codec)
// (half: the records are IEEE binary16, vol addresses halves)
hipError_t launch_bake_raw(const void *vol, bool half, const Params &P, float *out, uint64_t plane,
                           uint64_t psy, uint64_t psz, hipStream_t s);
hipError_t launch_bake_codec(const Params &P, float *out, uint64_t plane, uint64_t psy,
                             uint64_t psz, hipStream_t s);
// 2x2 (x, y) micro-brick copy of an 8-bin volume (oblique views, vr_stats.hip):
// pitches bsy (records per brick row) and bsz (records per slice), brick_index
hipError_t launch_brick8(const float *vol, const Params &P, float *out, uint64_t bsy,
                         uint64_t bsz, hipStream_t s);
// axis-rows copy of a B <= 8 volume (views along y / z, vr_stats.hip) with the
// record strides of axis_copy_strides
hipError_t launch_axis_copy(const float *vol, const Params &P, float *out, uint64_t asx,
                            uint64_t asy, uint64_t asz, hipStream_t s);
// axis copy of one baked plane (views along y / z, vr_stats.hip k_plane_axis):
// axis 1 y rows, 2 z rows, into plane_pitches(fast, pair) = (dsy, dsz) bricks
// 8 x 2 x 2 brick copy of one baked plane (oblique views, vr_stats.hip k_plane8)
// into plane8_pitches(nx, ny) = (dsy, dsz) bricks
hipError_t launch_plane8(const float *src, uint64_t ssy, uint64_t ssz, float *out, uint64_t dsy,
                         uint64_t dsz, int nx, int ny, int nz, hipStream_t s);
hipError_t launch_plane_axis(const float *src, uint64_t ssy, uint64_t ssz, float *out,
                             uint64_t dsy, uint64_t dsz, int nx, int ny, int nz, int axis,
                             hipStream_t s);
// streaming read of bytes (a multiple of 16, 16-B aligned) by nblocks workgroups
// of 256 threads; one xor word per workgroup into out (bench read ceiling)
hipError_t launch_stream_read(const void *buf, uint64_t bytes, uint32_t *out, uint32_t nblocks,
                              hipStream_t s);
// ---- f16 record volumes (vr_half.hip): the per-ray
// pipelined march over binary16 records in x rows (k_march_pipe_h; methods 1/2/3,
// nb in 1, 2, 4, 8, 16, 32), launch_march_h above ----
// n floats at src narrowed to n halves at dst (round to nearest even, subnormals kept)
hipError_t launch_narrow_f16(const float *src, void *dst, uint64_t n, hipStream_t s);
// ---- weighted-bin query (method 10, vr_query.hip) ----
// the bin weights of a launch: a kernel argument of their own after Params
// (wave-uniform kernarg: scalar loads, SGPR operands of the multiplies); the
// first nb entries are used
struct BinWeights {
    float w[32];
};
// k_march_lin: the per-ray pipelined march of sum w_i p_i over the x rows of the
// records (half: binary16), P.nb in 1, 2, 4, 8, 16, 32 (hipErrorInvalidValue
// otherwise); records its name for vr_last_kernel()
hipError_t launch_march_lin(const void *vol, bool half, const Params &P, const BinWeights &w,
                            uint32_t nslots, hipStream_t s);
// k_bake_lin: the same statistic of every voxel into one float plane at out, in
// the 16 x 2 x 1 bricks of pitches psy / psz (launch_bake_raw's layout and limits)
hipError_t launch_bake_lin(const void *vol, bool half, const Params &P, const BinWeights &w,
                           float *out, uint64_t psy, uint64_t psz, hipStream_t s);
// ---- quantile query (method 11, vr_quantile.hip) ----
// the quantiles of a launch: a kernel argument of their own after Params
// (a single quantile: q_lo == q_hi, the kernels of spread = false read q_lo)
struct QuantArgs {
    float q_lo, q_hi;
};
// k_march_quant: the march of launch_march_lin with Q(q_lo), or with
// Q(q_hi) - Q(q_lo) when spread, per corner; same bin counts and errors
hipError_t launch_march_quant(const void *vol, bool half, const Params &P, const QuantArgs &q,
                              bool spread, uint32_t nslots, hipStream_t s);
// k_bake_quant: the same statistic of every voxel into one float plane
// (launch_bake_lin's layout and limits)
hipError_t launch_bake_quant(const void *vol, bool half, const Params &P, const QuantArgs &q,
                             bool spread, float *out, uint64_t psy, uint64_t psz, hipStream_t s);
// ---- quantile of GMM volumes (method 11, vr_gmm.hip) ----
// bisection steps of the search (vr_gmm_quantile_steps)
constexpr int kGmmQuantSteps = 20;
// k_march_gmm_quant / k_march_gmm_quant_h: launch_march_gmm's march with the value at
// which the mixture's CDF reaches q_lo, or Q(q_hi) - Q(q_lo) when spread, per corner;
// records its name for vr_last_kernel() (M=11)
hipError_t launch_march_gmm_quant(int K, bool half, const Params &P, const QuantArgs &q,
                                  bool spread, uint32_t nblocks, hipStream_t s);
// k_bake_gmm_quant: the same statistic of the resident slices into one whole-volume
// plane at out (launch_bake_gmm's bricks, pitches and limits)
hipError_t launch_bake_gmm_quant(const void *wm, const void *sg, bool half, int K, int nx, int ny,
                                 int z_base, int nzs, const QuantArgs &q, bool spread, float *out,
                                 uint64_t psy, uint64_t psz, hipStream_t s);
// ---- distribution-distance query (method 12, vr_distance.hip) ----
// the target record and the similarity flag of a launch: a kernel argument of
// their own after Params (wave-uniform kernarg: scalar loads, h_i an SGPR operand
// of the subtraction, the flag a uniform select); the first nb entries are used
struct DistTarget {
    float h[32];
    int similarity;
};
// k_march_dist: the march of launch_march_lin with dist_stat against the target per
// corner, metric 0 (L1), 1 (EMD) or 2 (KS); same bin counts and errors (another
// metric: hipErrorInvalidValue); records its name for vr_last_kernel() (M=12)
hipError_t launch_march_dist(const void *vol, bool half, const Params &P, const DistTarget &t,
                             int metric, uint32_t nslots, hipStream_t s);
// k_bake_dist: the same statistic of every voxel into one float plane
// (launch_bake_lin's layout and limits)
hipError_t launch_bake_dist(const void *vol, bool half, const Params &P, const DistTarget &t,
                            int metric, float *out, uint64_t psy, uint64_t psz, hipStream_t s);
// ---- level-crossing query (method 13, vr_crossing.hip) ----
// k_march_cross: the march of launch_march_lin with F_c = lin_stat against the
// crossing weights per corner and the crossing combine 1 - prod F_c - prod (1 - F_c)
// in place of the trilinear filter; same bin counts and errors; records its name
// for vr_last_kernel() (M=13)
hipError_t launch_march_cross(const void *vol, bool half, const Params &P, const BinWeights &w,
                              uint32_t nslots, hipStream_t s);
// k_march_cross_plane: the same march and combine over a plane of F, one float per
// voxel in 16 x 2 x 1 bricks of pitches P.sy / P.sz (P.nb = 1; the plane k_bake_lin
// made of the crossing weights, or a GMM range plane); 32-bit plane indices where
// they fit, 64-bit ones otherwise
hipError_t launch_march_cross_plane(const float *plane, const Params &P, uint32_t nslots,
                                    hipStream_t s);
// ---- user-defined transfer function (vr_transfer.hip) ----
// entries of a table (VR_TF_MAX of include/vr.h); the device copy always holds this many
constexpr int kTfMax = 256;
// k_march_plane_tf: k_march_cross_plane's one-lane march over a plane of one float
// per voxel in 16 x 2 x 1 bricks of pitches P.sy / P.sz (P.nb = 1), classified
// through the first n (1 .. kTfMax) RGBA entries of the device table (kTfMax
// float4, staged into LDS) in place of the built-in nine.  cross: the sample is the
// crossing combine of the 8 corners (M=13), else their trilinear blend (M=0).
// 32-bit plane indices where they fit and VR_TF_WIDE is unset, 64-bit ones otherwise.
hipError_t launch_march_plane_tf(const float *plane, const Params &P, const float4 *table, int n,
                                 bool cross, uint32_t nslots, hipStream_t s);
// ---- 2-D transfer function over two planes (vr_transfer2.hip) ----
// entries of a 2-D table (VR_TF2_MAX of include/vr.h): 16 KiB of LDS as float4; the
// device copy always holds this many
constexpr int kTf2Max = 1024;
// k_march_tf2: k_march_plane_tf's march over two planes pu / pv of one volume (the
// same dims and pitches P.sy / P.sz, P.nb = 1; pu == pv allowed), one footprint per
// step for both, classified through the nu x nv (u fastest, nu * nv <= kTf2Max)
// RGBA entries of the device table at ((su - P.toff) * P.tscale, (sv - voff) *
// vscale).  cu / cv: that axis' sample is the crossing combine of its 8 corners,
// else their trilinear blend (vr_last_kernel's M = cu + 2 cv).  Index widths as
// launch_march_plane_tf.
hipError_t launch_march_tf2(const float *pu, const float *pv, const Params &P, const float4 *table,
                            int nu, int nv, float voff, float vscale, bool cu, bool cv,
                            uint32_t nslots, hipStream_t s);
// ---- ray projections of a baked plane (vr_project.hip) ----
// the modes (VR_PROJ_MAX / MIN / MEAN of include/vr.h; 0 composites: no launch here)
constexpr int kProjMax = 1, kProjMin = 2, kProjMean = 3;
// k_march_proj: launch_march_plane_tf's plane, table, index widths and kernarg segment;
// every ray marched to its end with no opacity test, its samples reduced to their
// maximum, minimum or mean (mode) and that value classified once through the first n
// entries of the device table, read from global memory.  vr_last_kernel:
// k_march_proj_max / _min / _mean, M=13 for cross.
hipError_t launch_march_proj(const float *plane, const Params &P, const float4 *table, int n,
                             bool cross, int mode, uint32_t nslots, hipStream_t s);
// ---- headlight gradient shading of a baked plane (vr_shade.hip) ----
// the light as the kernel takes it (vr_light of include/vr.h): 16 bytes after
// launch_march_plane_tf's kernel arguments; k = shininess_log2, 0 .. kLightMaxLog2
constexpr int kLightMaxLog2 = 7;
struct Light {
    float ka, kd, ks;
    int k;
};
// k_march_lit: launch_march_plane_tf's plane, table, LDS and index widths; every
// classified sample's colour lit by the in-cell gradient of the plane (cross: of F)
// against the ray, col = col * (ka + kd c) + ks c^(2^k), alpha and so every ray's
// length untouched.  vr_last_kernel: k_march_lit, M=13 for cross.
hipError_t launch_march_lit(const float *plane, const Params &P, const float4 *table, int n,
                            const Light &L, bool cross, uint32_t nslots, hipStream_t s);
// ---- gradient-magnitude planes of baked planes (vr_gradient.hip) ----
// k_bake_grad: the central-difference gradient magnitude (one-sided on the faces, in
// units of the normalised coordinates x / nx, y / ny, z / nz) of every voxel of the
// plane src into the plane out, both one float per voxel in 16 x 2 x 1 bricks of
// plane_pitches(nx, ny) = (psy, psz), aprons filled and empty slots +0; the unsigned
// maximum of the magnitudes' bits is folded into the zeroed device word max_bits.
// launch_plane8's limits: a dimension beyond 65535 is hipErrorInvalidValue.
hipError_t launch_bake_grad(const float *src, float *out, uint64_t psy, uint64_t psz, int nx,
                            int ny, int nz, uint32_t *max_bits, hipStream_t s);
// ---- value ranges and histograms of baked planes (vr_histogram.hip) ----
constexpr int kHistMax = 16384;  // VR_HIST_MAX: bins (nu * nv) of a histogram, 64 KiB of LDS
// k_plane_hist<V>: the voxels of box = {x0, x1, y0, y1, z0, z1} (inside the grid, not
// empty) of the plane pu (V = 0: pv NULL, nv 1) or of the planes pu and pv of one grid
// (V = 1), both in 16 x 2 x 1 bricks of plane_pitches(nx, ny) = (psy, psz), counted
// into the zeroed device array counts[nv * nu]: counts[j * nu + i] += 1 for a voxel
// with i = point_axis((u - uoff) * uscale, nu) and j likewise of v; aprons, empty
// slots and padding are never counted.  k_plane_range: the unsigned minimum and
// maximum of the monotone keys (bits ^ 0x80000000 for a non-negative pattern, ~bits
// for a negative one) of the box's voxels that are not NaN into keys[0] / keys[1]
// (preset to 0xFFFFFFFF / 0), and the number that are NaN added to *n_nan.
// launch_plane8's limits: a dimension beyond 65535 is hipErrorInvalidValue, as is a
// box that is empty or leaves the grid, or nu * nv beyond kHistMax.
hipError_t launch_plane_hist(const float *pu, const float *pv, uint64_t psy, uint64_t psz, int nx,
                             int ny, int nz, const int *box, float uoff, float uscale, int nu,
                             float voff, float vscale, int nv, unsigned long long *counts,
                             hipStream_t s);
hipError_t launch_plane_range(const float *p, uint64_t psy, uint64_t psz, int nx, int ny, int nz,
                              const int *box, uint32_t *keys, unsigned long long *n_nan,
                              hipStream_t s);
hipError_t launch_logcheck(unsigned long long *cnt, hipStream_t s);
hipError_t launch_synth(float *vol, const SynthArgs &a, hipStream_t s);
hipError_t launch_unscatter(const uint32_t *packed, const uint32_t *lists, uint32_t ntiles,
                            uint32_t tiles_x, uint32_t *frame, uint32_t W, uint32_t H,
                            hipStream_t s);
hipError_t launch_popcount(const unsigned long long *bits, uint64_t nwords,
                           unsigned long long *total, hipStream_t s);

}  // namespace vr
