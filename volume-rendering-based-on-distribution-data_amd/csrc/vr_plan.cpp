// vr_plan.cpp -- the kernel choice of the record marches (vr_plan.h): every rule,
// in order of precedence, with the measurement behind it.  Pure host code: no
// HIP, no library state.  To change a rule, change it here, add the cases that
// tell the old rule from the new one to tools/record_kernel_choice.py and
// tests/golden/kernel_choice.txt, and run tests/test_plan.py.
#include "vr_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

// k_march_m7wq pixel map default (MarchPlan::wq_map); a build-time tuning knob
#ifndef M7_WQ_MAP
#define M7_WQ_MAP 1
#endif

namespace vr {

namespace {

struct Knobs {
    const char *(*get)(const char *);
    const char *str(const char *key) const { return get ? get(key) : nullptr; }
    bool has(const char *key) const { return str(key) != nullptr; }
    // the knob as an integer (atoi), `unset` if it is not set
    int num(const char *key, int unset) const {
        const char *e = str(key);
        return e ? std::atoi(e) : unset;
    }
    bool off(const char *key) const { return num(key, 1) == 0; }  // set to 0
};

// gather8's 32-bit addressing of a baked plane: pitches and depth fit 24-bit
// multiplies and the byte offset of every element fits 32 bits (a 1024^3 plane,
// 2^30 floats, does: the last element sits at 2^32 - 4)
// a baked plane's index fits the 32-bit form of gather8 (MODE 1: 24-bit
// multiplies, 32-bit sums): pitches and depth < 2^24, plane < 2^32 floats
bool plane_narrow(uint64_t sy, uint64_t sz, uint64_t nz) {
    return sy < (1u << 24) && sz < (1u << 24) && nz < (1u << 24) && sz * nz < (1ull << 32);
}

// The frame's rays, the default choice among the fp32 record marches and the
// launch knobs every frame carries (methods 1/2/3; method 7, f16 and baked
// frames start from the same fields and override some of them below).
void plan_records(const PlanIn &in, const Knobs &K, MarchPlan &p, bool &along_rows) {
    const int nb = in.nb, qm = in.method;
    const uint64_t rays = (uint64_t)in.W * in.H;
    const uint64_t list_rays = (uint64_t)in.n_tiles * kPlanTileRays;
    const uint64_t xy4 = 4ull * (uint64_t)in.nx * (uint64_t)in.ny;
    // VR_BOX_MAX: per-wave LDS box capacity (tuning / ablation knob; 0 disables staging)
    p.box_max = kPlanBoxMax;
    if (K.has("VR_BOX_MAX")) {
        const int v = K.num("VR_BOX_MAX", 0);
        if (v >= 0 && v <= 2048) p.box_max = v;
    }
    // VR_WG_PER_CU: cap resident workgroups per CU through the LDS request (tuning knob)
    p.wg_per_cu = 0;
    if (K.has("VR_WG_PER_CU")) {
        const int v = K.num("VR_WG_PER_CU", 0);
        if (v >= 1 && v <= 32) p.wg_per_cu = v;
    }
    // Kernel choice (measured at 1024^3 x 8).  When the
    // screen x axis runs along the volume's voxel rows (|m[0]| ~ 1, e.g. the
    // runSingleTest view) consecutive lanes read consecutive records and the
    // per-ray pipelined march (path 2) is fastest for mean and variance; the
    // log-heavy entropy decode prefers the wave-staged march (path 4), which
    // decodes every record once per wave-step instead of once per touching
    // ray.  Oblique views use the quad-cooperative gathers (path 0, B == 8),
    // which keep every 4-lane group on one contiguous 64-byte run.
    // VR_PATH overrides (vr_set_tuning): 0 quad, 1 k_march (LDS-staged box /
    // per-ray), 2 per-ray pipelined, 4 wave-staged rows, 7 ray-segmented
    // (VR_SEG lanes per ray).
    along_rows = std::fabs(in.m0) >= 0.95f;
    // (entropy of 1-4 bins: the one-lane pipelined march, round 6 -- 1024^3 x 2
    // 1080p C0 4.66 -> 3.25 ms, x 4 4.51 -> 4.35 against the wave-staged march;
    // profiles/r06/knobs/m3_1024x*.log)
    p.path = along_rows ? (qm == 3 && nb >= 8 ? 4 : 2) : 0;
    // 8-bin entropy of row-aligned views: the LDS-box march with the rolled
    // LDS-column entropy (k_march<8,3>, 128 VGPRs) beats the wave-staged march:
    // 1024^3 C0 4.31 -> 3.52 ms, 512^3 3.10 -> 1.63 (round 4,
    // profiles/r04/variants_1024x8_m3.log, variants_512x8_m3.log).  Rank tile
    // lists too: cost-dealt 1024^3 C0 lists, max over ranks, k_march vs the
    // wave-staged march N = 2 1.99 vs 2.52 ms, N = 4 1.52 vs 1.67, N = 8 1.51 vs
    // 1.51 (round 5, profiles/r05/rank_sim_m3_C0_paths.log)
    if (along_rows && qm == 3 && nb == 8) p.path = 1;
    // ... and of oblique views of a volume coarse for the frame (>= 4 pixels per
    // voxel of the x-y face): 512^3 C1 m3 8.32 -> 5.11 ms; at 1024^3 the quad
    // march stays ahead (8.42 vs 8.61; profiles/r04/variants_*_m3_r4g.log)
    // (16 and 32 bins too, round 6: 512^3 x 16 C1 m3 8.60 -> 5.56 ms, x 32 15.9 ->
    // 10.3; at 1024^3 the quad march stays ahead, 9.05 vs 10.3 and 16.9 vs 19.1;
    // profiles/r06/knobs/wide_*.log, m3_512x32.log)
    if (!along_rows && qm == 3 && (nb == 8 || nb == 16 || nb == 32) && !in.tile_list &&
        rays >= xy4)
        p.path = 1;
    // Views whose screen x runs along the volume's z or y (|M[8]| / |M[4]| >=
    // 0.95) march an axis-rows copy of an owned B <= 8 volume with the per-ray
    // pipelined march (ensure_axis_copy); for the choices below
    // they count as row-aligned (their x-row seg / quad alternatives read the
    // x rows across).  VR_ZROWS=0 keeps them oblique.
    // 8-bin entropy of such views takes the LDS-box march on the x rows instead:
    // the pipelined march decodes all 8 corners' 64 logarithms per step
    // unrolled and spills (1024^3 x 8 side view S m3: 18.8 ms; box 3.38, quad
    // 5.55, wave-staged 5.12; profiles/r06/knobs/side_m3.log)
    const bool axis_dir = std::fabs(in.m8) >= 0.95f || std::fabs(in.m4) >= 0.95f;
    const bool axis_m3 = !along_rows && axis_dir && qm == 3 && nb == 8;
    p.axis = 0;
    if (!along_rows && in.owned && qm >= 1 && qm <= 3 &&
        (nb == 1 || nb == 2 || nb == 4 || nb == 8) && !axis_m3 && !K.off("VR_ZROWS"))
        p.axis = std::fabs(in.m8) >= 0.95f ? 2 : std::fabs(in.m4) >= 0.95f ? 1 : 0;
    const bool row_like = along_rows || p.axis != 0;
    if (p.axis) p.path = 2;
    if (axis_m3) p.path = 1;
    // Side and top views of 16- and 32-bin records (no axis copy: B <= 8 only)
    // likewise take the LDS-box march on the x rows instead of the quad march:
    // 1024^3 x 32 side view m1 13.7 -> 6.9 ms, m3 15.4 -> 7.6, top view m1 7.6 ->
    // 7.0, m3 15.4 -> 7.5; 1024^3 x 16 side m1 6.7 -> 4.9, m3 8.6 -> 4.4; 512^3 x
    // 16 side m1 3.7 -> 1.3, m3 8.2 -> 1.9 (profiles/r06/knobs/wide_*.log)
    if (!along_rows && axis_dir && (nb == 16 || nb == 32) && !in.tile_list && qm >= 1 && qm <= 3)
        p.path = 1;
    // Launches of few rays (a rank's tile list at 4 or 8 GPUs, 1080p) are bound
    // by the per-ray step chain, not by HBM: there the pipelined ray-segmented
    // march (2 lanes per ray, next window gathered before this one decodes,
    // path 7) renders mean / variance row-aligned views faster than the
    // one-lane march (cost-dealt 1024^3x8 C0 lists, max over ranks: N = 8
    // 0.217 ms vs 0.265 for plain 4-lane windows, N = 4 0.410 vs 0.44 one-lane);
    // at 2 GPUs (~1.04 M rays per rank) the one-lane march still wins (0.70 vs
    // 0.81 ms) (tools/rank_sim.py, tools/gpu_seg4.sh).
    // VR_SEG_RAYS overrides the ray-count threshold.
    uint64_t seg_rays = 700000;
    if (const char *e = K.str("VR_SEG_RAYS")) seg_rays = std::strtoull(e, nullptr, 10);
    // Views along the volume's z or y (axis-rows copy) split the rays of such
    // lists the same way, the windows' gathers addressed in the copy
    // (k_march_segp2_zrows: cost-dealt side-view 1024^3 x 8 lists, max over
    // ranks, N = 8 0.399 -> 0.247 ms, N = 4 0.543 -> 0.445; the one-lane march's
    // step chain bound them; profiles/r03/rank_sim_1024x8_S*.log).
    if (row_like && in.tile_list && (qm == 1 || qm == 2) && list_rays <= seg_rays) p.path = 7;
    // Oblique views of a volume coarse for the frame (>= 4 pixels per voxel of
    // the x-y face, e.g. 512^3 at 1080p): neighbouring rays share most records,
    // the launch is bound by the per-ray step chain rather than HBM, and the
    // pipelined 2-lane segmented march beats the quad march (512^3 x 8 C1: m1
    // 2.05 -> 1.77 ms, m2 1.87 -> 1.63; at 1024^3, 2 pixels per voxel, the quad
    // march stays ahead: 3.49 vs 5.23 ms; profiles/r02/paths_512x8.log).
    if (!row_like && nb == 8 && (qm == 1 || qm == 2) && rays >= xy4) p.path = 7;
    // Row-aligned full frames of such a coarse volume: a wave's 64 rays cover
    // ~16 voxel columns, so staging the wave's footprint box in LDS (path 1,
    // each record fetched and decoded once per wave) beats the one-lane
    // pipelined march (512^3 x 8 C0 1080p: m1 1.00 -> 0.88 ms, m2 1.00 -> 0.73;
    // it loses for entropy, oblique views, 1024^3 and launches of <= 262 K
    // rays: profiles/r02/paths_coarse_rows.log).
    // The same holds for 16- and 32-bin records, whose box rows load through the
    // quad-cooperative gathers (512^3 x 32 C0 1080p m1: box 2.97 ms, quad march
    // 6.04; profiles/r02/wide_records.log), entropy included: decoding each record
    // once per wave is what the log-heavy wide decode needs (VR_BOX3=0: quad march).
    const bool wide3 = (nb == 16 || nb == 32) && qm == 3 && !K.off("VR_BOX3");
    // 8-bin mean and variance there take two samples per footprint box
    // (k_march_duo): 512^3 x 8 C0 m1 0.694 -> 0.623 ms, m2 0.571 -> 0.496; three
    // or four per box 0.655 / 0.707; at 1024^3 (VR_PATH=1) the doubled boxes lose,
    // 1.69 -> 2.26 (profiles/r04/variants_*_duo_r4l.log)
    // Side and top views of such a coarse volume too, on the x rows without the
    // axis copy (the face across the view is then y-z or x-z): 512^3 x 8 1080p
    // side view m1 1.14 -> 0.74 ms, m2 1.13 -> 0.55; top view m1 1.08 -> 0.75,
    // m2 1.09 -> 0.54 (profiles/r06/knobs/side_512x8_m*.log)
    const uint64_t face = p.axis == 2   ? (uint64_t)in.ny * in.nz
                          : p.axis == 1 ? (uint64_t)in.nx * in.nz
                                        : (uint64_t)in.nx * in.ny;
    p.duo = 0;
    if (row_like && !in.tile_list && (nb == 8 || nb == 16 || nb == 32) &&
        (qm == 1 || qm == 2 || (wide3 && along_rows)) && rays > seg_rays && rays >= 4ull * face) {
        p.path = 1;
        p.duo = 2;
    }
    // 32-bin records (the reference's own width) are decode-bound at any volume
    // size, and with a 16x4-pixel block per wave the box decodes each record
    // once per wave-step instead of once per touching ray: row-aligned full
    // frames at 1024^3 x 32, 1080p, C0: m1 6.67 -> 6.18 ms, m2 10.42 -> 9.05,
    // m3 41.0 -> 35.0 (16 bins: no gain; profiles/r03/box_map.log)
    if (along_rows && !in.tile_list && nb == 32 && qm >= 1 && qm <= 3 && rays > seg_rays)
        p.path = 1;
    // 16-bin entropy of row-aligned full frames: the box decodes each record
    // once per wave-step with the rolled LDS-column entropy (round 4): 1024^3 x
    // 16 C0 m3 12.3 -> 5.6 ms; oblique views keep the quad march (13.7 vs 14.0)
    // (profiles/r04/variants_1024x16_m3_r4g.log)
    if (along_rows && !in.tile_list && nb == 16 && qm == 3 && rays > seg_rays) p.path = 1;
    // Mid-size row-aligned full frames of such a coarse volume (more rays than the
    // small-frame threshold below, fewer than the segmented one: BASELINE config 2,
    // 256^3 x 4 at 512^2): a round of 4 waves per SIMD whose per-step overheads
    // dominate, so the box march with four samples per box (k_march_duo) beats the
    // one-lane march for 4 and 8 bins: 256^3 x 4 C0 m1 0.129 -> 0.105 ms, m2 0.104
    // -> 0.076; 256^3 x 8 at 512^2 m1 0.271 -> 0.245, m2 0.240 -> 0.144; 384^3 x 4 at
    // 768^2 m1 0.197 -> 0.198, m2 0.176 -> 0.137; 2 bins lose (m2 0.188 -> 0.213)
    // (profiles/r04/variants_midsize_duo_r4ad.log)
    if (along_rows && !in.tile_list && (nb == 4 || nb == 8) && (qm == 1 || qm == 2) &&
        rays > 131072 && rays <= seg_rays && rays >= xy4) {
        p.path = 1;
        p.duo = 4;
    }
    // Small full frames (BASELINE configs 1 and 2: 128^3 x 1 at 256^2, 256^3 x 4
    // at 512^2) cannot fill the GPU with one ray per lane, so the per-ray step
    // chain sets the time, as for a rank's tile list: the pipelined
    // ray-segmented march, 4 lanes per ray up to 128 K rays, else 2.  Measured
    // (profiles/r02/small_frames.log): 128^3 x 1 C0 0.136 -> 0.082 ms, C1
    // 0.180 -> 0.093; 256^3 x 4 C1 0.224 -> 0.147 (its row-aligned view, 262 K
    // rays, takes the box march above).  Oblique views
    // of 8-bin volumes keep the quad march (as for oblique rank lists).
    int small_seg = 0;
    {
        const bool nb_ok = nb == 1 || nb == 2 || nb == 4 || (nb == 8 && row_like);
        const uint64_t limit = row_like ? std::min<uint64_t>(seg_rays, 131072) : seg_rays;
        if (!in.tile_list && rays <= limit && nb_ok && (qm == 1 || qm == 2)) {
            p.path = 7;
            // oblique frames up to 400 K rays on 4-lane windows too (round 4, after
            // the unconditional gathers): 256^3 x 4 C1 at 512^2 0.161 -> 0.135 ms
            // (profiles/r04/variants_256x4_r4g.log)
            small_seg = (rays <= 131072 || (!row_like && rays <= 400000)) ? -4 : -2;
        }
        // Entropy of such frames with 1, 2 or 4 bins (round 4): the wave-staged
        // march (row-aligned) and the one-lane march (oblique) lose to 2-lane
        // windows, and row-aligned coarse frames above 128 K rays to the LDS box:
        // 128^3 x 1 at 256^2 C0 1.066 -> 0.481 ms, C1 0.988 -> 0.514; 256^3 x 4 at
        // 512^2 C0 1.600 -> 1.185 (box), C1 2.299 -> 1.707; 256^3 x 2 at 512^2 C0
        // 1.343 -> 0.783 (box), C1 1.113 -> 1.064 (profiles/r04/variants_midsize_m3_r4ag.log)
        // Round 6, after the cheaper exact log: 2 and 4 bins take the one-lane
        // pipelined march instead (256^3 x 4 at 512^2 C0 1.14 -> 0.99 ms, C1 1.66 ->
        // 1.12; 384^3 x 4 at 768^2 C0 1.84 -> 1.54, C1 2.96 -> 1.65; 256^3 x 2 C0
        // 0.76 -> 0.68, C1 1.04 -> 0.90); one bin keeps the 2-lane windows (128^3
        // x 1 C0 0.47 vs 0.51, C1 0.50 vs 0.80; profiles/r06/knobs/m3_*.log)
        if (!in.tile_list && qm == 3 && !p.axis && (nb == 1 || nb == 2 || nb == 4) &&
            rays <= seg_rays) {
            if (nb != 1) {
                p.path = 2;
            } else if (along_rows && rays > 131072 && rays >= xy4) {
                p.path = 1;
            } else {
                p.path = 7;
                small_seg = -2;
            }
        }
    }
    if (p.path != 2 && p.path != 7) p.axis = 0;  // 7: the segmented march reads the copy too
    if (K.has("VR_DUO")) {  // 0 / 1: one sample per box, 2-4: that many
        const int v = K.num("VR_DUO", 0);
        if (v >= 0 && v <= 4) p.duo = v;
    }
    if (K.has("VR_PATH")) {
        const int v = K.num("VR_PATH", 0);
        if (v == 0 || v == 1 || v == 2 || v == 4 || v == 7) {
            p.path = v;
            p.axis = 0;  // a forced path reads the x rows
        }
    }
    // The quad march (path 0: oblique views, B = 8, methods 1-3) of a rank's tile
    // list of <= 700 K rays (N >= 4 GPUs at 1080p) takes two lanes per ray
    // (k_march_quad2): such a launch is bound by its longest waves' step chains,
    // which halve.  Cost-dealt 1024^3 x 8 C1 lists, max over ranks: N = 8
    // 0.586 -> 0.455 ms, N = 4 0.955 -> 0.880; N = 2 (1 M rays) 1.64 -> 1.68 and
    // the full frame 3.15 -> 3.35 keep one lane per ray (tools/rank_sim.py,
    // profiles/r03/rank_sim_1024x8_C1_quad2.log).  VR_QUAD2=0/1 overrides.
    p.quad2 = in.tile_list && list_rays <= 700000u;
    if (K.has("VR_QUAD2")) p.quad2 = K.num("VR_QUAD2", 0) != 0;
    p.seg_lanes = small_seg ? small_seg : -2;  // VR_SEG=S: S lanes per ray, negative = pipelined windows
    if (K.has("VR_SEG")) {
        const int v = K.num("VR_SEG", 0);
        if (v == 2 || v == 4 || v == -2 || v == -4) p.seg_lanes = v;
    }
    // A wave's rays as a compact pixel block (16 x 4 one lane per ray, (64 / S / 4)
    // x 4 in S-lane windows) instead of a 64- or 64/S-pixel row: its loads touch
    // fewer lines per instruction.  Measured per launch kind (tools/bench_variants.py,
    // tools/rank_sim.py, profiles/r06/segmap/): small full frames on pipelined
    // windows 128^3 x 1 at 256^2 m1 C0 0.075 -> 0.070 ms, C1 0.078 -> 0.077, m3 C0
    // 0.490 -> 0.438 (C1 0.493 vs 0.501: kept as rows), 256^3 x 4 at 512^2 m1 C1
    // 0.143 -> 0.137; row-aligned 2/4-bin entropy on the one-lane march 1024^3 x 2
    // 1080p C0 3.23 -> 3.03, x 4 4.35 -> 4.16 (oblique: 256^3 x 4 C1 1.13 vs 1.22,
    // kept as rows).  Also kept as rows: the 8-bin one-lane march (headline 1.342
    // vs 1.352, side view 1.588 vs 1.628) and the rank lists of records (C0 N = 4
    // 0.376 vs 0.386, N = 8 0.204 vs 0.219).  VR_SEG_MAP=0/1 overrides.
    p.seg_map = (!in.tile_list && p.path == 7 && p.seg_lanes < 0 && (along_rows || qm != 3)) ||
                (p.path == 2 && nb <= 4 && qm == 3 && along_rows && !p.axis);
    if (K.has("VR_SEG_MAP")) p.seg_map = K.num("VR_SEG_MAP", 0) != 0;
    // A rank's list at 8 GPUs (<= 400 K rays, 2-lane windows) is bound by the step
    // chains of its longest tiles: its first 64 slots -- the 8 longest tiles of
    // every XCD sublist -- take 4 lanes per ray in the same launch
    // (k_march_seg_head).  Cost-dealt 1024^3 x 8 lists, max over 8 ranks: C0
    // 0.216 -> 0.202 ms (32 / 96 / 128 slots: 0.204 / 0.204 / 0.207; 8 lanes:
    // 0.212), side view 0.254 -> 0.249-0.263; N = 4 lists (~520 K rays) gain
    // nothing (0.380 both) and keep the plain windows
    // (profiles/r04/rank_sim_C0_head.log, rank_sim_S_head.log).
    // VR_HEAD=slots (0 = off), VR_HEAD_SEG=-2/-4/-8, VR_HEAD_TAIL=1 (one-lane
    // tail, k_march_pipe_head) override.
    p.head_slots = 0;
    if (in.tile_list && p.path == 7 && nb == 8 && (qm == 1 || qm == 2) && list_rays <= 400000u)
        p.head_slots = 64;
    if (K.has("VR_HEAD")) p.head_slots = (uint32_t)K.num("VR_HEAD", 0) & ~7u;
    p.head_lanes = K.num("VR_HEAD_SEG", -4);
    p.head_tail = K.num("VR_HEAD_TAIL", 0);
    if (!in.tile_list) p.head_slots = 0;
}

// Kernel of a baked-statistics frame (measured at 512^3 and 1024^3 x 8, 1080p,
// profiles/r02/baked_paths.log).  A baked step is a few dozen VALU operations
// and 4 pair loads, so the frame is bound by gather issue and line traffic,
// not by decode: row-aligned views take the one-lane pipelined march (path 2,
// 1024^3 C0 0.375 ms); oblique views, whose lanes' loads touch many lines per
// instruction, split each ray over 4 lanes (path 7, VR_SEG 4: 1024^3 C1 2.02
// -> 1.32 ms, 1.11 at 4 workgroups per CU).  A deeper look-ahead ring (2-8 steps in flight per lane) was
// slower everywhere but 512^3 C1 (within 3 %).  VR_PATH (2 / 7) overrides;
// seg_lanes keeps a VR_SEG setting.
void plan_baked(const PlanIn &in, const Knobs &K, MarchPlan &p) {
    // a plane's axis copy (plane_axis 1 / 2) makes a side / top view row-aligned
    const bool along_rows = std::fabs(in.m0) >= 0.95f || p.plane_axis == 1 || p.plane_axis == 2;
    int path = along_rows ? 2 : 7;
    int seg = 4;
    // A rank's tile list (multi-GPU) has few rays, so its longest step chains
    // set the time: row-aligned lists split rays too (cost-dealt 1024^3 C0
    // lists, max over ranks: N = 4 (~520 K rays) pipelined 2-lane windows
    // 0.149 ms vs 0.185 one-lane, N = 8 (~260 K) 4 lanes 0.105 vs 0.165;
    // N = 2 stays one-lane, 0.233 vs 0.281; tools/rank_sim.py --baked).
    if (along_rows && in.tile_list) {
        const uint64_t rays = (uint64_t)in.n_tiles * kPlanTileRays;
        if (rays <= 400000) path = 7;
        else if (rays <= 700000) path = 7, seg = -2;
    }
    if (path == 7 && !K.has("VR_SEG")) p.seg_lanes = seg;
    // compact pixel blocks per wave (plan_records): baked frames gain everywhere
    // but on row-aligned 4-lane windows (1024^3 x 8 1080p C1 0.844 -> 0.817 ms,
    // C0 one-lane 0.310 -> 0.295; rank lists C1 N = 8 0.168 -> 0.153, C0 N = 4
    // 0.133 -> 0.124, C0 N = 8 4-lane 0.093 vs 0.096; profiles/r06/segmap/)
    p.seg_map = !(along_rows && path == 7 && p.seg_lanes > 0);
    // oblique full frames of a fine volume (< 4 pixels per voxel of the x-y
    // face): 4 workgroups per CU, fewer rays' lines in flight per L2 (1024^3
    // C1 1.28 -> 1.11 ms; 2-3 per CU 1.25, 6 1.19); coarse volumes (512^3:
    // 0.67 uncapped vs 0.73) and row-aligned views run uncapped
    if (!along_rows && !in.tile_list && p.wg_per_cu == 0 &&
        (uint64_t)in.W * in.H < 4ull * (uint64_t)in.nx * (uint64_t)in.ny)
        p.wg_per_cu = 4;
    if (K.has("VR_SEG_MAP")) p.seg_map = K.num("VR_SEG_MAP", 0) != 0;
    if (K.has("VR_PATH")) {  // the LDS-box march (1) reads x rows only
        const int v = K.num("VR_PATH", 0);
        if (v == 2 || v == 7) path = v;
    }
    p.path = path;
}

// Method 7 (corner-mean state along the ray, vr_m7.hip); nb: the records' bins,
// 1 over the baked corner means (method -7).
void plan_m7(const PlanIn &in, const Knobs &K, MarchPlan &p, int nb, bool oblique) {
    // the one-lane method-7 marches (k_march_m7_pipe / k_march_m7): a 16x4 pixel
    // block per wave, except 8+-bin row-aligned views of a fine volume (< 4 pixels
    // per voxel of the x-y face), which keep 64-pixel rows: 256^3 x 4 at 512^2 C0
    // 0.322 -> 0.222 ms, C1 0.201 -> 0.175; 512^3 x 8 1080p C0 1.201 -> 1.125;
    // 1024^3 x 4 C0 0.795 -> 0.775, C1 2.67 -> 2.39; 1024^3 x 8 C0 1.447 vs 1.468
    // (rows; profiles/r06/segmap/m7_*.log).  VR_M7_MAP=0/1 overrides.
    p.seg_map = !(nb >= 8 && !oblique &&
                  (uint64_t)in.CW * in.CH < 4ull * (uint64_t)in.nx * (uint64_t)in.ny);
    if (K.has("VR_M7_MAP")) p.seg_map = K.num("VR_M7_MAP", 0) != 0;
    const int B = p.B, wg = p.wg_per_cu;
    if (p.method == -7) {  // method 7 over the baked corner means (plane 3, vr_stats.hip)
        // 4-byte corners: the plain march (the look-ahead gather of
        // k_march_m7_pipe only adds loads), 4 workgroups per CU on row-aligned
        // views, 2 on oblique ones (1024^3 C0 0.68 -> 0.64 ms, C1 2.03 -> 1.67;
        // profiles/r02/baked_m7.log)
        p.kind = Kind::M7;
        p.cap = wg > 0 ? wg : (oblique ? 2 : 4);
        return;
    }
    // oblique views with the method-7 grid equal to the volume: the
    // quad-cooperative march (VR_M7_QUAD=0 disables), 2 workgroups per CU; it
    // reads the micro-brick copy when that can be made (never of an adopted
    // volume, whose records the library does not own)
    if (B == 8 && !K.off("VR_M7_QUAD") && oblique && in.m7x == in.nx && in.m7y == in.ny &&
        in.m7z == in.nz) {
        p.kind = Kind::M7Quad;
        p.cap = wg > 0 ? wg : 2;
        p.brick = in.owned && !(in.denied & kLayoutBrick);
        return;
    }
    // wide records: quad-cooperative refreshes (VR_M7_WQ=0: k_march_m7)
    if ((B == 16 || B == 32) && !K.off("VR_M7_WQ")) {
        p.kind = Kind::M7Wq;
        p.wq_map = K.num("VR_WQ_MAP", M7_WQ_MAP) != 0;
        p.cap = wg;
        return;
    }
    // pipelined corner gathers (VR_M7_PIPE=0: the plain march); oblique views
    // at 2 workgroups per CU (1024^3x8 C1: 8.53 -> 7.45 ms; C0 is fastest
    // uncapped, 1.53 ms; profiles/r02/m7_pipe.log)
    if (B > 0 && B <= 8 && !K.off("VR_M7_PIPE")) {
        p.kind = Kind::M7Pipe;
        p.cap = wg > 0 ? wg : (oblique && B == 8 ? 2 : 0);
        return;
    }
    // oblique views at 3 workgroups per CU when B = 8 (the measured case): fewer
    // corner-mean refreshes in flight, fewer L2 re-reads (1024^3x8 C1 9.94 ->
    // 8.29 ms; row-aligned C0 is fastest uncapped)
    p.kind = Kind::M7;
    p.cap = wg > 0 ? wg : (oblique && B == 8 ? 3 : 0);
}

// The ray-segmented march (path 7, vr_seg.hip) has instances for B <= 8 on 2 or
// 4 lanes per ray, plain (S > 0) or pipelined (S < 0) windows; over an axis-rows
// copy pipelined windows only.  false: no such instance.
bool plan_seg(const PlanIn &in, MarchPlan &p) {
    const int S = p.seg_lanes;
    if (p.method < (p.B == 1 ? -1 : 1) || p.method > 3) return false;
    const uint32_t nslots = in.n_tiles;  // head_slots is 0 without a tile list
    if (p.B == 8 && S == -2 && (p.method == 1 || p.method == 2) && p.head_slots > 0 &&
        p.head_slots < nslots && (p.head_slots & 7u) == 0 &&
        (p.head_lanes == -2 || p.head_lanes == -4 || p.head_lanes == -8)) {
        p.kind = Kind::SegHead;
        return true;
    }
    // axis views: pipelined windows only
    const bool ok = (p.axis && p.method >= 1) ? (S == -2 || S == -4)
                                              : (S == 2 || S == 4 || S == -2 || S == -4);
    if (ok) p.kind = Kind::Seg;
    return ok;
}

// From the path to the kernel family of methods 1/2/3 and the baked 0 / -1 (what
// is compiled for which B; vr_kernels.hip, vr_seg.hip), and the launch's
// occupancy cap.
void plan_kind(const PlanIn &in, const Knobs &K, MarchPlan &p, bool oblique) {
    const int B = p.B, m = p.method;
    p.cap = p.wg_per_cu;
    if (B > 0 && B <= 8) {
        if (p.path == 7) {
            if (plan_seg(in, p)) return;
            p.path = 2;  // no (B, S) instance: the one-lane march
        }
        if (B == 8 && p.path == 0 && m >= 1) {
            p.kind = Kind::Quad;
            p.brick = in.owned && !(in.denied & kLayoutBrick);
            // The quad march uses no LDS; an LDS request caps it at 2 workgroups
            // (2 waves per SIMD) per CU, which trims the oblique view's line
            // re-reads: 1024^3x8 C1 3.73 -> 3.52 ms (3 per CU by registers, 1 per
            // CU 3.91).  VR_WG_PER_CU overrides.
            // A rank's tile list of <= 400 K rays (8 GPUs at 1080p) runs at 1 per
            // CU: its tiles are scattered over the frame, and fewer rays in flight
            // re-read fewer lines (cost-dealt C1 lists, max over 8 ranks: 0.71 ->
            // 0.59 ms; 3 per CU 0.68; tools/rank_sim.py)
            p.cap = p.wg_per_cu > 0 ? p.wg_per_cu
                    : (in.tile_list && (uint64_t)in.n_tiles * 256u <= 400000u) ? 1 : 2;
            return;
        }
        if (p.path == 4 && m >= 1) {
            p.kind = Kind::Ws;
            p.cap = 0;  // its LDS request is the log table alone
            return;
        }
        if (B < 8 && p.path == 0) p.path = 2;  // per-ray pipelined for narrow records
        // baked statistics (vr_stats.hip, bricked planes): paths 2, 7 only
        if (m <= 0) p.path = 2;
        if (p.path == 2) {
            // (views along the volume's y / z march the axis-rows copy: p.axis)
            p.kind = Kind::Pipe;
            return;
        }
    }
    if (B == 16 || B == 32) {
        // wide records, mean / variance: the quad-cooperative march (k_march_wq),
        // except row-aligned views of 16-bin records, whose lane-owned 64-B records
        // already sit side by side (k_march_wide; 1024^3 x 16 C0 2.79 vs 3.90 ms;
        // profiles/r02/wide_records.log).  VR_WIDE=1 / 2 forces one; VR_PATH=1 and
        // coarse row-aligned full frames keep the LDS box (plan_records).  Entropy
        // goes through k_march_wq too (vr_quad.h WQ3); k_march_wide has mean and
        // variance only.
        if (p.path != 1) {
            int kind = (B == 16 && !oblique && m != 3) ? 1 : 2;
            const int v = K.num("VR_WIDE", 0);
            if (v == 1 || v == 2) kind = v;
            if (m == 3) kind = 2;  // k_march_wide: mean and variance only
            // k_march_wq pixels: 16x4 blocks per wave (a quad = a pixel column) beat a
            // 64-pixel row per wave: 1024^3 x 32 C1 12.44 -> 11.77 ms, C0 6.64 -> 6.56,
            // 1024^3 x 16 C1 6.78 -> 6.65 (profiles/r02/wide_records.log); VR_WQ_MAP=0: rows
            p.wq_map = K.num("VR_WQ_MAP", 1) != 0;
            if (kind == 1) {
                p.kind = Kind::Wide;
                // a 16x4 pixel block per wave (1024^3 x 16 1080p C0 m1 2.719 -> 2.673
                // ms, profiles/r06/segmap/wide_1024x16.log); VR_WIDE_MAP=0: rows
                p.seg_map = K.num("VR_WIDE_MAP", 1) != 0;
            } else {
                p.kind = Kind::Wq;
            }
            return;
        }
    }
    // the LDS-box march: a wave takes a 16x4-pixel block, whose footprint box is
    // compact (512^3 x 8 C0 1080p: ~70 voxels per wave-step instead of
    // ~140-210 for a 64-pixel row): m1 0.869 -> 0.723 ms, m2 0.760 -> 0.627
    // (profiles/r03/box_map.log); VR_BOX_MAP=0 keeps the rows
    p.wq_map = K.num("VR_BOX_MAP", 1) != 0;
    // duo samples per footprint box (k_march_duo; plan_records: coarse
    // row-aligned 8-bin full frames, VR_DUO)
    const bool duo = B > 0 && B <= 8 && p.duo >= 2 && p.duo <= 4 && (m == 1 || m == 2) &&
                     p.box_max > 0;
    p.kind = duo ? Kind::Duo : Kind::March;
}

}  // namespace

MarchPlan plan_march(const PlanIn &in) {
    const Knobs K{in.tuning};
    MarchPlan p = {};
    p.kind = Kind::None;
    p.method = in.method;
    p.count = in.count;
    const int nb = in.nb;
    p.B = (nb == 1 || nb == 2 || nb == 4 || nb == 8 || nb == 16 || nb == 32) ? nb : 0;
    bool along_rows = false;
    plan_records(in, K, p, along_rows);
    const bool oblique = !along_rows;
    p.cap = p.wg_per_cu;  // (the quad and method-7 marches set their own below)
    if (in.count) {
        // the footprint-marking pass: the counting instance of the LDS-box march
        // (f16: of the one-lane march, which has no runtime-B form) on the x rows,
        // whatever renders the frame (neither reads a layout copy: axis is unused)
        p.wq_map = !in.f16 && K.num("VR_BOX_MAP", 1) != 0;
        p.kind = (in.method < 1 || in.method > 3) ? Kind::None
                 : !in.f16 ? Kind::March : p.B > 0 ? Kind::PipeH : Kind::None;
        return p;
    }
    if (in.method == 7 && in.baked) {
        // method 7 from the baked corner means (plane 3): the same corner cache
        // and double lerps (K:395-480), 4 bytes per corner refresh
        p.axis = 0;
        p.B = 1;
        p.method = -7;
        plan_m7(in, K, p, 1, oblique);
        return p;
    }
    if (in.baked && in.method >= 1 && in.method <= 6) {
        // one float per corner voxel, the same filter and composite (vr_stats.hip),
        // addressed in the planes' bricks
        p.axis = 0;
        p.B = 1;
        // side / top views of the raw planes: the method's plane with the view's
        // axis in the brick rows (ensure_plane_copy), marched as row-aligned
        if (in.method <= 3 && oblique) {
            int ax = std::fabs(in.m8) >= 0.95f ? 2 : std::fabs(in.m4) >= 0.95f ? 1 : 0;
            // oblique views: the 8 x 2 x 2 brick copy (axis 3)
            if (!ax) ax = 3;
            if (!(in.denied & kLayoutPlane)) {
                p.plane_axis = ax;
                p.layout = kLayoutPlane;
            }
        }
        plan_baked(in, K, p);
        // method 0: the 32-bit plane index (MODE 1), or a plane copy's MODE 4 / 5
        // (32-bit in-slice offsets, 64-bit slice offsets: ensure_plane_copy keeps
        // a slice < 2^32 floats, so a copy never needs -1, which reads x rows);
        // method -1: x-row planes too large for 32-bit indices (MODE 2).
        // VR_PLANE_WIDE=1 (tests) sends every x-row plane to -1.
        const bool wide = K.num("VR_PLANE_WIDE", 0) != 0;
        const bool narrow = p.plane_axis != 0 ||
                            (!wide && plane_narrow(in.plane_sy, in.plane_sz, (uint64_t)in.nz));
        p.method = narrow ? 0 : -1;
        plan_kind(in, K, p, oblique);
        return p;
    }
    if (in.f16) {
        // f16 records: one kernel family for every view, on the x rows (no layout
        // copies, no VR_PATH / VR_SEG / VR_WIDE); method 7
        // reads the baked corner means above
        p.axis = 0;
        if (in.method < 1 || in.method > 3 || p.B == 0) return p;
        // pixels per wave as the fp32 one-lane march's (plan_records): 16 x 4 blocks
        // for row-aligned entropy of narrow records, 64-pixel rows otherwise
        if (!K.has("VR_SEG_MAP")) p.seg_map = nb <= 4 && in.method == 3 && along_rows;
        p.kind = Kind::PipeH;
        return p;
    }
    // views whose screen x runs along the volume's z or y read that axis' rows
    // copy with the per-ray pipelined march (plan_records); if the copy cannot be
    // made (HBM), the oblique view's march on the x rows / bricks
    if (p.axis && (in.denied & kLayoutAxis)) {
        p.axis = 0;
        p.path = 0;
    }
    if (in.method == 7) {
        plan_m7(in, K, p, nb, oblique);
    } else {
        plan_kind(in, K, p, oblique);
    }
    // (brick: the quad marches of oblique views -- methods 1/2/3 on path 0, method
    // 7 when its grid is the volume's -- read the micro-brick copy)
    p.layout = p.axis ? kLayoutAxis : p.brick ? kLayoutBrick : kLayoutNone;
    return p;
}

const char *plan_kernel_name(const MarchPlan &p, char *buf, size_t n) {
    const char *axis = p.axis == 1 ? "_yrows" : p.axis == 2 ? "_zrows" : "";
    // a baked plane's copy (method 0 only: -1 reads x rows)
    const char *plane = p.method != 0       ? ""
                        : p.plane_axis == 1 ? "_plane_yrows"
                        : p.plane_axis == 2 ? "_plane_zrows"
                        : p.plane_axis == 3 ? "_plane8"
                                            : "";
    const char *brick = p.brick ? "_brick" : "";
    char kind[64] = "";
    switch (p.kind) {
    case Kind::None: break;
    case Kind::March: snprintf(kind, sizeof kind, "k_march"); break;
    case Kind::Duo:
        snprintf(kind, sizeof kind, p.duo == 2 ? "k_march_duo" : "k_march_duo%d", p.duo);
        break;
    case Kind::Pipe: snprintf(kind, sizeof kind, "k_march_pipe%s%s", axis, plane); break;
    case Kind::Ws: snprintf(kind, sizeof kind, "k_march_ws"); break;
    case Kind::Quad:
        snprintf(kind, sizeof kind, "k_march_quad%s%s", p.quad2 ? "2" : "", brick);
        break;
    case Kind::Wide: snprintf(kind, sizeof kind, "k_march_wide"); break;
    case Kind::Wq: snprintf(kind, sizeof kind, "k_march_wq"); break;
    case Kind::Seg:
        snprintf(kind, sizeof kind, "k_march_seg%s%d%s%s", p.seg_lanes < 0 ? "p" : "",
                 std::abs(p.seg_lanes), axis, plane);
        break;
    case Kind::SegHead:
        snprintf(kind, sizeof kind, "k_march_segp%d_head_%s%s", -p.head_lanes,
                 p.head_tail == 1 ? "pipe" : "segp2", axis);
        break;
    case Kind::M7: snprintf(kind, sizeof kind, "k_march_m7"); break;
    case Kind::M7Pipe: snprintf(kind, sizeof kind, "k_march_m7_pipe"); break;
    case Kind::M7Quad: snprintf(kind, sizeof kind, "k_march_m7_quad%s", brick); break;
    case Kind::M7Wq: snprintf(kind, sizeof kind, "k_march_m7wq"); break;
    case Kind::PipeH: snprintf(kind, sizeof kind, "k_march_pipe_h"); break;
    }
    snprintf(buf, n, "%s<B=%d,M=%d>", kind, p.B, p.method);
    return buf;
}

}  // namespace vr
