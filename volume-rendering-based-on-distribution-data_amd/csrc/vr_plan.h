// vr_plan.h -- which march kernel renders a frame of methods 1/2/3/7 over record
// volumes (fp32 or f16, baked or not, and the footprint-count passes).
// plan_march() is the only place that chooses: a pure host function of the
// frame's description -- no GPU, no library state, no side effects -- so the
// whole decision table runs on the CPU (tests/test_plan.py).  The launchers
// (launch_plan, vr_kernels.hip) switch on the plan and decide nothing.
// Host-only: no HIP header, compiles with a plain C++17 compiler.
#pragma once

#include <cstddef>
#include <cstdint>

namespace vr {

// vr_device.h's kTileW * kTileH and kBoxMax (vr_api.cpp asserts they agree)
constexpr uint32_t kPlanTileRays = 256;
constexpr int kPlanBoxMax = 1024;

// layout copies a plan can ask for; render_frame tries to make the copy and, if
// it cannot (HBM), plans again with the copy's bit set in PlanIn::denied
enum Layout : unsigned {
    kLayoutNone = 0,
    kLayoutAxis = 1,    // axis-rows copy of the records (MarchPlan::axis 1 = y rows, 2 = z rows)
    kLayoutBrick = 2,   // 2x2 micro-brick copy of 8-bin records (quad marches)
    kLayoutPlane = 4,   // copy of a baked plane (MarchPlan::plane_axis 1 / 2 / 3)
};

struct PlanIn {
    float m0, m4, m8;            // inv_view[0], [4], [8]: screen x along the volume's x / y / z
    uint32_t W, H;               // frame
    uint32_t CW, CH;             // pixels rendered (render_kernel's clip; W, H otherwise)
    bool tile_list;              // a rank's tile list (n_tiles slots) instead of the full frame
    uint32_t n_tiles;
    int method;                  // query method 1, 2, 3 or 7 (4, 5, 6: their baked planes only)
    int nb, nx, ny, nz;          // resident record volume (4, 5, 6: the codec volume)
    bool owned;                  // the library owns the records (it may make an axis copy)
    bool f16;                    // binary16 records
    bool baked;                  // baked statistics planes are resident
    uint64_t plane_sy, plane_sz; // pitches of the baked x-row planes
    int m7x, m7y, m7z;           // method 7's grid
    bool count;                  // the footprint-marking pass (vr_count_footprint)
    unsigned denied;             // Layout bits: copies that could not be made
    const char *(*tuning)(const char *key);  // knob lookup (nullptr value = unset)
};

enum class Kind {
    None,        // nothing compiled renders this (launch: hipErrorInvalidValue)
    March,       // k_march<B,M,COUNT>      LDS box
    Duo,         // k_march_duo<B,M,K>      K = duo samples per box
    Pipe,        // k_march_pipe<B,M,GM>    one lane per ray (+ axis / plane copies)
    Ws,          // k_march_ws<B,M>         wave-staged rows
    Quad,        // k_march_quad(2)<M,BR>   quad-cooperative gathers (B = 8)
    Wide,        // k_march_wide<B,M>       16 / 32 bins, lane-owned records
    Wq,          // k_march_wq<B,M>         16 / 32 bins, quad-cooperative
    Seg,         // k_march_seg<B,M,S,PIPE,GM>  |seg_lanes| lanes per ray
    SegHead,     // k_march_seg_head / k_march_pipe_head: head_lanes for the first head_slots
    M7,          // k_march_m7<B,BK>
    M7Pipe,      // k_march_m7_pipe<B>
    M7Quad,      // k_march_m7_quad<BR>
    M7Wq,        // k_march_m7wq<B>
    PipeH,       // k_march_pipe_h<B,M,COUNT>  f16 records
};

struct MarchPlan {
    Kind kind;
    int B;                   // the kernel's bins template argument (0: runtime bin count)
    int method;              // the kernel's method: 1/2/3/7, or baked 0 (32-bit plane index),
                             // -1 (64-bit), -7 (method 7 over the baked corner means)
    bool count;
    int path;                // the path number behind the kind (Params::path, host-only)
    int seg_lanes;           // lanes per ray of the segmented march, negative = pipelined windows
    int seg_map, wq_map;     // a wave's pixels: 1 = a compact 16x4 block, 0 = a 64-pixel row
    int duo;                 // samples per footprint box
    int quad2;               // the quad march on two lanes per ray
    uint32_t head_slots;     // SegHead: slots of the list on head_lanes lanes per ray
    int head_lanes, head_tail;
    int box_max;             // LDS box capacity (voxels per wave)
    int wg_per_cu;           // VR_WG_PER_CU (or the baked oblique rule), 0 = unset
    int cap;                 // workgroups per CU this launch is capped at (0 = none)
    int axis;                // marches the axis-rows copy: 1 y rows, 2 z rows
    bool brick;              // marches the micro-brick copy
    int plane_axis;          // marches a baked plane's copy: 1 y rows, 2 z rows, 3 8x2x2 bricks
    unsigned layout;         // the Layout copy this plan needs (one bit, or kLayoutNone)
};

MarchPlan plan_march(const PlanIn &in);

// the name vr_last_kernel() reports, "<kind><B=..,M=..>", into buf; returns buf
const char *plan_kernel_name(const MarchPlan &plan, char *buf, size_t n);

}  // namespace vr
