// vr_api.cpp -- host side of libvr.so: module-global device state and the
// C-ABI of include/vr.h (the reference's extern "C" API, K:1889-2406, plus
// the vr_* extensions).  Never exits; errors go to vr_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/vr.h"
#include "vr_internal.h"
#include "vr_phitab.h"

namespace {

struct State {
    float *vol = nullptr;
    int dtype = VR_DTYPE_F32;       // element type of vol's bins (F16: vol addresses halves)
    bool owned = false;
    int nx = 0, ny = 0, nz = 0, nb = 0;
    uint64_t sy = 0, sz = 0;        // record pitch of a voxel row / slice in HBM
    float inv_view[12] = {0};       // __constant__ c_invViewMatrix starts zeroed (K:116)
    hipStream_t stream = nullptr;   // legacy default stream, like the reference
    bool linear_filter = false;     // tex.filterMode = point after initCuda (K:2163)
    std::string err;
    int status = VR_OK;
    // fractal/template codec volume (methods 4/5/6)
    int4 *cb = nullptr;
    float *tpl = nullptr;
    float2 *cerr = nullptr;
    int cnx = 0, cny = 0, cnz = 0, cnb = 0, ntpl = 0, err_slots = 0;
    // flexible blocks (methods 8/9/0): span tables, then the block statistics
    struct Flex {
        int dim = 0, nb = 0, ntpl = 0, nf = 0, ns = 0, nfk = 0, nsk = 0;
        uint64_t *fkeys = nullptr, *skeys = nullptr;
        int32_t *fidx = nullptr, *sidx = nullptr, *scount = nullptr;
        int4 *fcode = nullptr;
        float2 *ferr = nullptr, *shist = nullptr;
        float *tpl = nullptr;
        float4 *blocks = nullptr;
        int nblk = 0;
    } flex;
    // full-frame workgroup -> tile order (frame_order), cached per frame shape
    uint32_t *perm = nullptr;
    size_t perm_cap = 0;
    uint32_t perm_key[22] = {0};
    std::vector<uint32_t> perm_host;
    // adaptive order (frame_order): 0 none, 1 estimate order in use and per-tile
    // costs to be recorded, 2 final; cost_recorded: a render recorded into tile_cost
    int order_state = 0;
    bool cost_recorded = false;
    uint32_t *tile_cost = nullptr;
    size_t tile_cost_cap = 0;
    unsigned long long *wave_clock = nullptr;  // vr_debug_wave_clock (tooling)
    unsigned long long *box_check = nullptr;   // vr_debug_box_check (tooling, -DVR_BOX_CHECK builds)
    // GMM volume (config 5, vr_gmm.hip): planes (w, mu)[voxel][K][2] and
    // sigma[voxel][K] of the resident slices [z_base, z_base + nzs) of an
    // nx x ny x nz volume; dtype F16: the planes address halves (section 14)
    struct Gmm {
        float *wm = nullptr, *sg = nullptr;
        bool owned = false;
        int dtype = VR_DTYPE_F32;
        int nx = 0, ny = 0, nz = 0, K = 0, z_base = 0, nzs = 0;
    } gmm;  // the selected slot's volume (vr_gmm_select)
    // the other slot's volume while not selected (a rank of a two-segment slab
    // chain holds a front and a back z-range)
    Gmm gmm_parked[2];
    int gmm_slot = 0;
    // A baked set of GMM planes (vr_bake_gmm_*, vr_gmm.hip k_bake_gmm*): whole-volume
    // planes of `plane` floats, a statistic of every voxel of an nx x ny x nz
    // volume, filled slab by slab (slice[z]: baked); tied to no slot and to no
    // resident records
    struct GmmStats {
        float *buf = nullptr;
        int nx = 0, ny = 0, nz = 0;
        uint64_t plane = 0, sy = 0, sz = 0;  // plane_pitches
        std::vector<unsigned char> slice;
        int nbaked = 0;
    };
    // The three sets (kGmmPlaneSets below, one row each), each with
    // slice flags of its own and independent of the others: the mean and 16 x
    // variance (two planes), the range probability (method 10, section 18: one plane
    // made of the bounds grq) and the quantile (method 11, section 19: one plane made
    // of the quantile state qq, qmode below)
    enum { kGmmStats, kGmmRange, kGmmQuant, kGmmSets };
    GmmStats gplanes[kGmmSets];
    vr::GmmRange grq = {};
    bool grq_set = false;
    // A baked set of planes of one float per voxel in x-row bricks (plane_pitches),
    // one allocation: `floats` floats a plane, pitches sy / sz; buf nullptr = not
    // baked
    struct Planes {
        float *buf = nullptr;
        uint64_t floats = 0, sy = 0, sz = 0;
    };
    // baked statistics (basicDataProcessing / vr_bake_stats, vr_stats.hip):
    // four planes for the raw volume (methods 1/2/3 and method 7's corner mean)
    // and three for the codec volume (methods 4/5/6); not baked: the march
    // decodes the records at every step
    Planes stats, cstats;
    // The record queries (methods 10-13, kRecordQueries below; DESIGN.md sections
    // 16, 17, 20, 21).  Each has a piece of host state (no HIP call sets or reads
    // it) and qplane[method - 10], the one plane its vr_bake_* made of that state
    // (not baked: the march decodes per step), independent of the other three.
    Planes qplane[4];
    // Gradient-magnitude planes: one optional plane per source
    // method (1-6: slots 0-5, 10-13: slots 6-9; grad_slot), baked from the source's
    // resident plane by vr_bake_gradient and freed before anything frees or replaces
    // that plane; max: the largest magnitude of the plane
    struct Grad {
        Planes p;
        float max = 0.0f;
    } grad[10];
    // method 10, weighted bins: the bin weights (qn = 0: none set)
    vr::BinWeights qw = {};
    int qn = 0;
    // method 11, quantile: the quantiles (qmode 0: none set, 1: Q(q_lo), 2: the
    // spread Q(q_hi) - Q(q_lo))
    vr::QuantArgs qq = {};
    int qmode = 0;
    // method 12, distribution distance: the target record and the similarity flag
    // (dn = 0: none set), and the metric
    vr::DistTarget dt = {};
    int dn = 0, dmetric = 0;
    // method 13, level crossing: the crossing weights (xn = 0: none set), apart
    // from method 10's qw; its plane holds F
    vr::BinWeights xw = {};
    int xn = 0;
    // user-defined transfer function: tf_n RGBA entries
    // (0: none set, the built-in table), the caller's like the weights above and
    // tied to no volume.  Host state; tf_dev is its device copy (kTfMax float4,
    // nullptr: not made), stale while tf_dirty, made and refreshed by the frame
    // that needs it (tf_upload) from the snapshot tf_up; tf_stream: the stream of the
    // last upload or frame that touched it
    float tf[4 * vr::kTfMax] = {0}, tf_up[4 * vr::kTfMax] = {0};
    int tf_n = 0;
    float4 *tf_dev = nullptr;
    bool tf_dirty = false;
    hipStream_t tf_stream = nullptr;
    // 2-D transfer function over two planes: tf2_nu x tf2_nv
    // RGBA entries, u fastest (0 x 0: none set), classified over the frame's plane
    // (u) and the plane of method tf2_mv (v) at (sv - tf2_voff) * tf2_vscale.  At
    // most one of tf_n and tf2_nu is non-zero.  Host state with a device copy of
    // its own (kTf2Max float4), kept exactly as the 1-D table's above
    float tf2[4 * vr::kTf2Max] = {0}, tf2_up[4 * vr::kTf2Max] = {0};
    int tf2_nu = 0, tf2_nv = 0, tf2_mv = 0;
    float tf2_voff = 0.0f, tf2_vscale = 1.0f;
    float4 *tf2_dev = nullptr;
    bool tf2_dirty = false;
    hipStream_t tf2_stream = nullptr;
    // ray projection: VR_PROJ_COMPOSITE (0: every path as
    // without it), VR_PROJ_MAX, _MIN or _MEAN.  The caller's, like the tables: tied to
    // no volume.  Host state; rtf_dev is the device copy of the built-in nine entries
    // (kTfMax float4, nullptr: not made) that a projection without a caller's table
    // classifies through, made by the frame that needs it (rtf_upload).
    int proj = 0;
    float4 *rtf_dev = nullptr;
    bool rtf_dirty = false;
    hipStream_t rtf_stream = nullptr;
    // headlight gradient shading: off, or the four numbers of
    // vr_light.  The caller's, like the tables and the projection: tied to no volume.
    // Host state only; it travels to k_march_lit as a kernel argument.
    bool light_on = false;
    vr_light light = {0.0f, 0.0f, 0.0f, 0};
    // 2x2 (x, y) micro-brick copy of an owned 8-bin volume for the quad march
    // of oblique views (ensure_brick, brick_index); nullptr = not made
    float *brick = nullptr;
    uint64_t bsy = 0, bsz = 0;
    // axis-rows copies of an owned B <= 8 volume for views along y ([0]) and z
    // ([1]) (ensure_axis_copy, axis_copy_strides); nullptr = not made
    struct AxisCopy {
        float *buf = nullptr;
        uint64_t sx = 0, sy = 0, sz = 0, bytes = 0;
    } acopy[2];
    uint64_t brick_bytes = 0;
    // copies of a baked plane (ensure_plane_copy): [axis - 1][plane], axis 1 / 2
    // the y / z-rows copies for views along y or z (k_plane_axis), axis 3 the
    // 8 x 2 x 2 brick copy for oblique views (k_plane8); plane 0-2 = methods 1-3
    struct PlaneCopy {
        float *buf = nullptr;
        uint64_t sy = 0, sz = 0, bytes = 0;
    } pcopy[3][3];
    // layout copies (micro-bricks, axis rows): byte budget (vr_set_layout_budget;
    // UINT64_MAX = the default, layout_budget_bytes) and the cost of the last one
    // made (vr_layout_info)
    uint64_t layout_budget = UINT64_MAX;
    float layout_last_ms = 0.0f;
    uint64_t layout_last_bytes = 0;
    int layout_builds = 0;
    // bumped whenever a resident volume / codec / flexible-block set is
    // released, so an order learned on old data is not reused (the order is a
    // scheduling hint only: any order renders the same image)
    uint32_t volume_epoch = 0;
    // HIP-event time of the kernel of the last vr_plane_range / vr_plane_histogram
    float plane_ms = 0.0f;
};

State g;

// Tuning knobs: kernel-path overrides, occupancy caps and layout experiments
// (tests force every kernel path through them; tools sweep them).  Set only
// through vr_set_tuning; the default build never reads the environment, so a
// variable left set in a shell cannot change which kernel runs.  A build with
// -DVR_TUNING also takes unset knobs from the environment (tooling).
std::map<std::string, std::string> g_tuning;

int fail(int status, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g.err = buf;
    g.status = status;
    return status;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(VR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define VR_HIP(call)                                        \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return hip_fail(e_, #call);   \
    } while (0)

void release_plane_copies();

// The gradient planes.  grad_slot: the slot of source method m
// (1-6, 10-13), -1 for any other number; grad_source: the source of gradient method
// qm (VR_GRADIENT_OF), 0 if qm is none.
int grad_slot(int m) {
    if (m >= 1 && m <= 6) return m - 1;
    if (m >= VR_QUERY_WEIGHTED && m <= VR_QUERY_CROSSING) return m - VR_QUERY_WEIGHTED + 6;
    return -1;
}

int grad_source(int qm) { return grad_slot(qm - VR_QUERY_GRADIENT) >= 0 ? qm - VR_QUERY_GRADIENT : 0; }

// Frees a gradient plane (vr_release_gradient; before its source's plane goes).  A
// tile order learned on it is not reused.
void release_grad(int slot) {
    State::Grad &gd = g.grad[slot];
    if (gd.p.buf) {
        (void)hipFree(gd.p.buf);
        g.volume_epoch++;
    }
    gd = State::Grad();
}

// Frees a baked plane of a record query (vr_release_*; with the records' other
// planes; on any call that sets or clears the state it was baked from).  A tile
// order learned on the plane march is not reused.
void release_planes(State::Planes &p) {
    for (int i = 0; i < 4; i++)  // a query's plane: its gradient plane goes first
        if (&p == &g.qplane[i]) release_grad(6 + i);
    if (p.buf) {
        (void)hipFree(p.buf);
        g.volume_epoch++;
    }
    p = State::Planes();
}

static_assert(VR_QUERY_CROSSING - VR_QUERY_WEIGHTED == 3, "qplane: one plane per method 10-13");
State::Planes &query_plane(int method) { return g.qplane[method - VR_QUERY_WEIGHTED]; }

void release_stats() {
    release_plane_copies();  // copies of the planes go with them
    for (State::Planes &p : g.qplane) release_planes(p);  // derived from the same records
    for (int m = 1; m <= 3; m++) release_grad(grad_slot(m));
    if (g.stats.buf) (void)hipFree(g.stats.buf);
    g.stats = State::Planes();
}

void release_cstats() {
    for (int m = 4; m <= 6; m++) release_grad(grad_slot(m));
    if (g.cstats.buf) (void)hipFree(g.cstats.buf);
    g.cstats = State::Planes();
}

void release_brick() {
    if (g.brick) (void)hipFree(g.brick);
    g.brick = nullptr;
    g.bsy = g.bsz = 0;
    g.brick_bytes = 0;
}

void release_axis_copy(int i) {
    if (g.acopy[i].buf) (void)hipFree(g.acopy[i].buf);
    g.acopy[i] = State::AxisCopy();
}

void release_axis_copy() {
    release_axis_copy(0);
    release_axis_copy(1);
}

void release_plane_copy(int a, int p) {
    if (g.pcopy[a][p].buf) (void)hipFree(g.pcopy[a][p].buf);
    g.pcopy[a][p] = State::PlaneCopy();
}

void release_plane_copies() {
    for (int a = 0; a < 3; a++)
        for (int p = 0; p < 3; p++) release_plane_copy(a, p);
}

uint64_t layout_resident() {
    uint64_t b = g.brick_bytes + g.acopy[0].bytes + g.acopy[1].bytes;
    for (int a = 0; a < 3; a++)
        for (int p = 0; p < 3; p++) b += g.pcopy[a][p].bytes;
    return b;
}

// Room for a layout copy of `bytes`: within the budget (vr_set_layout_budget)
// next to the copies already resident (less `freed`, a copy the caller would
// drop first), and HBM keeps max(4 GiB, 5 %) free after it for the caller.
// The default budget: two copies of the resident record volume (a brick copy
// and one axis copy, or both axis copies) plus three copies of one baked plane,
// each with 1/8 for the copies' padding -- what one view class plus one change
// of view needs, not every copy at once (a third record copy replaces one).
// Plus 64 MiB: a volume a few cells wide pads its 2 x 2 micro-bricks by up to
// 4x, far beyond 1/8, and copies that small cost nothing worth refusing.
// bytes of one bin of the resident record volume
uint64_t elem_bytes() { return g.dtype == VR_DTYPE_F16 ? 2 : sizeof(float); }
bool is_f16() { return g.vol && g.dtype == VR_DTYPE_F16; }

uint64_t layout_budget_bytes() {
    if (g.layout_budget != UINT64_MAX) return g.layout_budget;
    const uint64_t rec = g.vol ? g.sz * (uint64_t)g.nz * g.nb * elem_bytes() : 0;
    const uint64_t plane = g.stats.buf ? g.stats.floats * sizeof(float) : 0;
    return 2 * (rec + rec / 8) + 3 * (plane + plane / 8) + (64ull << 20);
}

bool layout_room(uint64_t bytes, uint64_t freed = 0) {
    const uint64_t have = layout_resident() - freed;
    const uint64_t budget = layout_budget_bytes();
    if (budget < have || budget - have < bytes) return false;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return (uint64_t)free_b + freed >= bytes + std::max<uint64_t>(4ull << 30, total_b / 20);
}

void release_volume() {
    release_stats();
    release_brick();
    release_axis_copy();
    g.volume_epoch++;
    if (g.vol && g.owned) (void)hipFree(g.vol);
    g.vol = nullptr;
    g.dtype = VR_DTYPE_F32;
    g.owned = false;
    g.nx = g.ny = g.nz = g.nb = 0;
    g.sy = g.sz = 0;
}

// Row / slice pitch (in records) of the resident volume.  VR_PAD="px,pz" adds
// px records to every row and pz records to every slice (layout experiments).
void choose_pitch(int nx, int ny, uint64_t &sy, uint64_t &sz) {
    long px = 0, pz = 0;
    if (const char *e = vr::tuning("VR_PAD")) {
        char *end = nullptr;
        px = std::strtol(e, &end, 10);
        if (end && *end == ',') pz = std::strtol(end + 1, nullptr, 10);
        if (px < 0 || px > 4096) px = 0;
        if (pz < 0 || pz > (1 << 20)) pz = 0;
    }
    sy = (uint64_t)nx + (uint64_t)px;
    sz = sy * (uint64_t)ny + (uint64_t)pz;
}

float entropy_norm(int nb) {
    // K:769: log((float)nBins) / log(2.0f) with the float overloads of log
    const float a = (float)std::log((double)(float)nb);
    const float b = (float)std::log((double)2.0f);
    return a / b;
}

uint32_t tiles_x(uint32_t w) { return (w + vr::kTileW - 1) / vr::kTileW; }
uint32_t tiles_y(uint32_t h) { return (h + vr::kTileH - 1) / vr::kTileH; }

void release_codec() {
    release_cstats();
    g.volume_epoch++;
    if (g.cb) (void)hipFree(g.cb);
    if (g.tpl) (void)hipFree(g.tpl);
    if (g.cerr) (void)hipFree(g.cerr);
    g.cb = nullptr;
    g.tpl = nullptr;
    g.cerr = nullptr;
    g.cnx = g.cny = g.cnz = g.cnb = g.ntpl = g.err_slots = 0;
}

void release_flex_blocks() {
    g.volume_epoch++;
    if (g.flex.blocks) (void)hipFree(g.flex.blocks);
    g.flex.blocks = nullptr;
    g.flex.nblk = 0;
}

void release_flex() {
    release_flex_blocks();
    void *ptrs[] = {g.flex.fkeys, g.flex.skeys, g.flex.fidx, g.flex.sidx, g.flex.scount,
                    g.flex.fcode, g.flex.ferr, g.flex.shist, g.flex.tpl};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    g.flex = State::Flex();
}

bool is_flex_method(int m) { return m == 8 || m == 9 || m == 0; }

bool lin_bins(int n) { return n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 32; }

// The record queries: methods 10-13 on a resident record volume (vr_query.h holds
// their device loops, each query's .hip file its functor and launchers).  What
// differs between them on the host, one row each, in method order; everything
// else -- the checks, the plane's life, the frame launch -- is written once below.
struct RecordQuery {
    int method;
    const char *name;     // of the query, in messages
    const char *state;    // what its setters set, in messages
    const char *setters;
    const char *bake;     // the bake's entry point and kernel, in messages
    // bins of the state set: 0 none set, -1 set and bound to no bin count
    int (*bins)();
    // the per-step march and the bake of the plane, from the records and the state
    hipError_t (*march)(const vr::Params &P, uint32_t nslots);
    hipError_t (*bake_launch)(const vr::Params &P, float *out, uint64_t psy, uint64_t psz);
    // a frame from the plane: false, the plan's plane march (the same eight floats
    // into the same filter as per step); true, k_march_cross_plane (method 13
    // combines the eight corners, it does not blend them)
    bool cross_plane;
};

const RecordQuery kRecordQueries[] = {
    {VR_QUERY_WEIGHTED, "weighted-bin", "bin weights", "vr_set_bin_weights / vr_set_query_range",
     "vr_bake_weighted(k_bake_lin)", [] { return g.qn; },
     [](const vr::Params &P, uint32_t nslots) {
         return vr::launch_march_lin(g.vol, is_f16(), P, g.qw, nslots, g.stream);
     },
     [](const vr::Params &P, float *out, uint64_t psy, uint64_t psz) {
         return vr::launch_bake_lin(g.vol, is_f16(), P, g.qw, out, psy, psz, g.stream);
     },
     false},
    {VR_QUERY_QUANTILE, "quantile", "a quantile", "vr_set_quantile / vr_set_quantile_spread",
     "vr_bake_quantile(k_bake_quant)", [] { return g.qmode ? -1 : 0; },
     [](const vr::Params &P, uint32_t nslots) {
         return vr::launch_march_quant(g.vol, is_f16(), P, g.qq, g.qmode == 2, nslots, g.stream);
     },
     [](const vr::Params &P, float *out, uint64_t psy, uint64_t psz) {
         return vr::launch_bake_quant(g.vol, is_f16(), P, g.qq, g.qmode == 2, out, psy, psz,
                                      g.stream);
     },
     false},
    {VR_QUERY_DISTANCE, "distance", "a target",
     "vr_set_query_target / vr_set_query_target_region", "vr_bake_distance(k_bake_dist)",
     [] { return g.dn; },
     [](const vr::Params &P, uint32_t nslots) {
         return vr::launch_march_dist(g.vol, is_f16(), P, g.dt, g.dmetric, nslots, g.stream);
     },
     [](const vr::Params &P, float *out, uint64_t psy, uint64_t psz) {
         return vr::launch_bake_dist(g.vol, is_f16(), P, g.dt, g.dmetric, out, psy, psz, g.stream);
     },
     false},
    // (the plane of F is method 10's statistic of the crossing weights: k_bake_lin)
    {VR_QUERY_CROSSING, "level-crossing", "crossing weights",
     "vr_set_isovalue / vr_set_crossing_weights", "vr_bake_crossing(k_bake_lin)",
     [] { return g.xn; },
     [](const vr::Params &P, uint32_t nslots) {
         return vr::launch_march_cross(g.vol, is_f16(), P, g.xw, nslots, g.stream);
     },
     [](const vr::Params &P, float *out, uint64_t psy, uint64_t psz) {
         return vr::launch_bake_lin(g.vol, is_f16(), P, g.xw, out, psy, psz, g.stream);
     },
     true},
};

// the row of method m; nullptr: not a record query
const RecordQuery *record_query(int m) {
    for (const RecordQuery &q : kRecordQueries)
        if (q.method == m) return &q;
    return nullptr;
}

// What a frame of query q and the bake of its plane both need: a record volume
// of a compiled bin count, and the query's state, set for that bin count.
int query_ready(const RecordQuery &q) {
    if (!g.vol)
        return fail(VR_ERR_STATE, "the %s query (queryMethod %d) needs a record volume (initCuda / "
                                  "vr_init_distribution*)", q.name, q.method);
    if (!lin_bins(g.nb))
        return fail(VR_ERR_UNSUPPORTED, "the %s query on records of %d bins (compiled: "
                                        "1,2,4,8,16,32)", q.name, g.nb);
    const int n = q.bins();
    if (n == 0)
        return fail(VR_ERR_STATE, "the %s query (queryMethod %d) needs %s (%s)", q.name, q.method,
                    q.state, q.setters);
    if (n > 0 && n != g.nb)
        return fail(VR_ERR_STATE, "the %s query: %s of %d bins set, the resident records have %d "
                                  "bins", q.name, q.state, n, g.nb);
    return VR_OK;
}

int check_method(int m) {
    if (m == 1 || m == 2 || m == 3 || m == 7 || m == 4 || m == 5 || m == 6) return VR_OK;
    if (const RecordQuery *q = record_query(m)) return query_ready(*q);
    if (const int src = grad_source(m)) {  // a gradient method has no per-step march
        if (!g.grad[grad_slot(src)].p.buf)
            return fail(VR_ERR_UNSUPPORTED, "queryMethod %d renders the gradient plane of method %d "
                                            "only: vr_bake_gradient(%d) first", m, src, src);
        return VR_OK;
    }
    if (is_flex_method(m)) {
        if (!g.flex.blocks)
            return fail(VR_ERR_STATE,
                        "queryMethod %d needs the flexible-block statistics (span tables via "
                        "initCuda / vr_init_flex, then dataProcessing / vr_flex_process)", m);
        return VR_OK;
    }
    return fail(VR_ERR_ARG, "unknown queryMethod %d", m);
}

// Host estimate of the samples a ray takes before leaving the volume (the
// slab test of K:136-156 on the pixel's ray; early termination ignored).
float est_steps(const float *M, uint32_t W, uint32_t H, float x, float y) {
    const float u = (x / (float)W) * 2.0f - 1.0f, v = (y / (float)H) * 2.0f - 1.0f;
    const float inv = 1.0f / std::sqrt(u * u + v * v + 4.0f);
    const float ax = u * inv, ay = v * inv, az = -2.0f * inv;
    const float d[3] = {ax * M[0] + ay * M[1] + az * M[2], ax * M[4] + ay * M[5] + az * M[6],
                        ax * M[8] + ay * M[9] + az * M[10]};
    const float o[3] = {M[3], M[7], M[11]};
    float tn = -1e30f, tf = 1e30f;
    for (int k = 0; k < 3; k++) {
        const float a = (-1.0f - o[k]) / d[k], b = (1.0f - o[k]) / d[k];
        tn = std::max(tn, std::min(a, b));
        tf = std::min(tf, std::max(a, b));
    }
    tn = std::max(tn, 0.0f);
    return tf > tn ? (tf - tn) / vr::kTStep : 0.0f;
}

// Full-frame tile order.  Workgroup b runs on XCD b % 8, and each XCD has its
// own L2.  Tiles are grouped in bx x by blocks (neighbouring tiles share the
// records along their common edges, so a block keeps that sharing inside one
// L2); block (i, j) goes to XCD (i + 3 j) % 8, a diagonal lattice that gives
// every XCD an evenly spread eighth of any region spanning a few blocks -- so
// the hit region, and with it the ray-marching work, is split evenly (a raster
// split hands the frame's empty top and bottom strips to whole XCDs).  Each
// XCD takes its blocks longest-ray first (longest-processing-time order on
// the view's ray lengths): a tile's march is a chain of dependent gathers, so
// the frame ends no earlier than its longest tile started plus that tile's
// length.  VR_XBLOCK="bx,by" (default 1,4 = 64x16 pixels; "0" = plain raster
// order).
//
// Adaptive refinement: the estimate ignores early ray termination and the
// volume's content, so the first render of a view also records every tile's
// measured cost (per wave: its longest ray's samples + 2, record_tile_cost),
// and the next render of the same view re-deals the blocks by those costs
// (lists_from_costs).  VR_NO_ADAPT keeps the estimate order.

// Interleave the 8 per-XCD lists into the workgroup order (entry b runs on
// XCD b % 8) and upload it as g.perm.
int upload_perm(const std::vector<std::vector<uint32_t>> &lists) {
    std::vector<uint32_t> &h = g.perm_host;
    h.clear();
    size_t longest = 0;
    for (auto &l : lists) longest = std::max(longest, l.size());
    for (size_t i = 0; i < longest; i++)
        for (auto &l : lists)
            if (i < l.size()) h.push_back(l[i]);
    if (h.size() > g.perm_cap) {  // grow; otherwise rewrite in stream order
        if (g.perm) (void)hipFree(g.perm);
        g.perm = nullptr;
        g.perm_cap = 0;
        VR_HIP(hipMalloc(&g.perm, h.size() * sizeof(uint32_t)));
        g.perm_cap = h.size();
    }
    VR_HIP(hipMemcpyAsync(g.perm, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          g.stream));
    return VR_OK;
}

// Measured-cost deal: blocks sorted by total cost, each given to the least
// loaded XCD that still has room (every XCD keeps the same number of blocks,
// +-1, so the interleaved order keeps entry b on XCD b % 8); an XCD's blocks
// stay in dealing order, i.e. most expensive first.
void lists_from_costs(const std::vector<uint32_t> &cost, uint32_t tx, uint32_t ty, uint32_t bx,
                      uint32_t by, std::vector<std::vector<uint32_t>> &lists) {
    const uint32_t nbx = (tx + bx - 1) / bx, nby = (ty + by - 1) / by;
    struct Blk { uint64_t cost; uint32_t i, j; };
    std::vector<Blk> blk;
    blk.reserve((size_t)nbx * nby);
    for (uint32_t j = 0; j < nby; j++)
        for (uint32_t i = 0; i < nbx; i++) {
            uint64_t c = 0;
            for (uint32_t y = j * by; y < std::min(ty, j * by + by); y++)
                for (uint32_t x = i * bx; x < std::min(tx, i * bx + bx); x++)
                    c += cost[(size_t)y * tx + x];
            blk.push_back({c, i, j});
        }
    std::stable_sort(blk.begin(), blk.end(), [](const Blk &a, const Blk &b) { return a.cost > b.cost; });
    // every XCD ends with lo or lo + 1 blocks, exactly `extra` of them with lo + 1
    const size_t lo = blk.size() / 8, extra = blk.size() % 8;
    size_t n_plus = 0;
    uint64_t load[8] = {0};
    size_t count[8] = {0};
    lists.assign(8, {});
    for (const Blk &b : blk) {
        int best = -1;
        for (int x8 = 0; x8 < 8; x8++) {
            const bool room = count[x8] < lo || (count[x8] == lo && n_plus < extra);
            if (room && (best < 0 || load[x8] < load[best])) best = x8;
        }
        n_plus += count[best] == lo;
        load[best] += b.cost;
        count[best]++;
        for (uint32_t y = b.j * by; y < std::min(ty, b.j * by + by); y++)
            for (uint32_t x = b.i * bx; x < std::min(tx, b.i * bx + bx); x++)
                lists[best].push_back(y * tx + x);
    }
}

int frame_order(const vr_render_desc *d, uint32_t tx, uint32_t ty, const uint32_t *&perm,
                uint32_t **record) {
    uint32_t bx = 1, by = 4;
    if (const char *e = vr::tuning("VR_XBLOCK")) {
        char *end = nullptr;
        const long a = std::strtol(e, &end, 10);
        long b = a;
        if (end && *end == ',') b = std::strtol(end + 1, nullptr, 10);
        if (a <= 0 || b <= 0) { perm = nullptr; return VR_OK; }
        bx = (uint32_t)std::min(a, 64L);
        by = (uint32_t)std::min(b, 64L);
    }
    // everything that changes the samples each ray takes keys the order
    uint32_t key[22] = {d->width, d->height, bx, by};
    std::memcpy(key + 4, d->inv_view, sizeof d->inv_view);
    key[16] = vr::tuning("VR_NO_LPT") ? 1u : 0u;
    key[17] = (uint32_t)d->query_method;
    std::memcpy(key + 18, &d->density, sizeof(float));
    std::memcpy(key + 19, &d->transfer_offset, sizeof(float));
    std::memcpy(key + 20, &d->transfer_scale, sizeof(float));
    key[21] = g.volume_epoch;
    const size_t ntile = (size_t)tx * ty;
    if (g.perm && std::memcmp(key, g.perm_key, sizeof key) == 0) {
        perm = g.perm;
        if (g.order_state == 1 && record) {
            if (!g.cost_recorded) {  // no frame of this view has recorded yet
                VR_HIP(hipMemsetAsync(g.tile_cost, 0, ntile * sizeof(uint32_t), g.stream));
                *record = g.tile_cost;
                return VR_OK;
            }
            // the frame after the recording one: re-deal the tiles by the costs
            std::vector<uint32_t> cost(ntile);
            VR_HIP(hipMemcpyAsync(cost.data(), g.tile_cost, ntile * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, g.stream));
            VR_HIP(hipStreamSynchronize(g.stream));
            g.order_state = 2;
            bool any = false;
            for (uint32_t c : cost) any |= c != 0;
            if (any) {  // kernels other than the per-ray pipelined march record nothing
                std::vector<std::vector<uint32_t>> lists;
                lists_from_costs(cost, tx, ty, bx, by, lists);
                int rc = upload_perm(lists);
                if (rc != VR_OK) return rc;
                perm = g.perm;
            }
        }
        return VR_OK;
    }
    const uint32_t nbx = (tx + bx - 1) / bx, nby = (ty + by - 1) / by;
    struct Blk { float cost; uint32_t i, j; };
    std::vector<std::vector<Blk>> blocks(8);
    for (uint32_t byi = 0; byi < nby; byi++) {
        for (uint32_t bxi = 0; bxi < nbx; bxi++) {
            float c = 0.0f;
            for (uint32_t y = byi * by; y < std::min(ty, byi * by + by); y++)
                for (uint32_t x = bxi * bx; x < std::min(tx, bxi * bx + bx); x++)
                    for (int k = 0; k < 3; k++)
                        c = std::max(c, est_steps(d->inv_view, d->width, d->height,
                                                  (float)(x * vr::kTileW + k * (vr::kTileW - 1) / 2),
                                                  (float)(y * vr::kTileH + vr::kTileH / 2)));
            blocks[(bxi + 3 * byi) & 7].push_back({c, bxi, byi});
        }
    }
    std::vector<std::vector<uint32_t>> lists(8);
    for (int x8 = 0; x8 < 8; x8++) {
        std::vector<Blk> &bl = blocks[x8];
        if (!key[16])
            std::stable_sort(bl.begin(), bl.end(),
                             [](const Blk &a, const Blk &b) { return a.cost > b.cost; });
        for (const Blk &b : bl)
            for (uint32_t y = b.j * by; y < std::min(ty, b.j * by + by); y++)
                for (uint32_t x = b.i * bx; x < std::min(tx, b.i * bx + bx); x++)
                    lists[x8].push_back(y * tx + x);
    }
    g.order_state = 0;  // until the new order is in place
    int rc = upload_perm(lists);
    if (rc != VR_OK) return rc;
    std::memcpy(g.perm_key, key, sizeof key);
    perm = g.perm;
    g.order_state = (key[16] || vr::tuning("VR_NO_ADAPT")) ? 2 : 1;
    g.cost_recorded = false;
    if (g.order_state == 1) {
        if (ntile > g.tile_cost_cap) {
            if (g.tile_cost) (void)hipFree(g.tile_cost);
            g.tile_cost = nullptr;
            g.tile_cost_cap = 0;
            VR_HIP(hipMalloc(&g.tile_cost, ntile * sizeof(uint32_t)));
            g.tile_cost_cap = ntile;
        }
        if (record) {
            VR_HIP(hipMemsetAsync(g.tile_cost, 0, ntile * sizeof(uint32_t), g.stream));
            *record = g.tile_cost;
        }
    }
    return VR_OK;
}

// LDS bytes per CU and per workgroup of the current device (160 KiB each on
// gfx950), read once per device; the occupancy caps are sized from them
// (vr_march.h cap_lds).
void device_lds(int &per_cu, int &per_wg) {
    static int cached_dev = -1, cu = 160 * 1024, wg = 64 * 1024;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev != cached_dev) {
        int a = 0, b = 0;
        if (hipDeviceGetAttribute(&a, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) ==
                hipSuccess && a > 0)
            cu = a;
        if (hipDeviceGetAttribute(&b, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) ==
                hipSuccess && b > 0)
            wg = b;
        cached_dev = dev;
    }
    per_cu = cu;
    per_wg = wg;
}

// the voxel grid a frame's Params describe: dims, bins per record and the
// record pitches of a row / slice
struct FrameVol {
    int nx, ny, nz, nb;
    uint64_t sy, sz;
};

// Params of a frame over the grid v (fill_params: the resident record or codec
// volume; vr_render_gmm_baked: the GMM planes); the codec and flexible-block
// methods add their tables
int fill_frame_params(const vr_render_desc *d, const FrameVol &v, vr::Params &P, uint32_t &nslots,
                      bool for_render) {
    const bool codec = d->query_method >= 4 && d->query_method <= 6;
    const bool flex = is_flex_method(d->query_method);
    if (!d->d_output) return fail(VR_ERR_ARG, "d_output is null");
    if (d->width == 0 || d->height == 0) return fail(VR_ERR_ARG, "empty image");
    int rc = check_method(d->query_method);
    if (rc != VR_OK) return rc;
    if (d->query_method == 7 &&
        (d->volume_size.width == 0 || d->volume_size.height == 0 || d->volume_size.depth == 0))
        return fail(VR_ERR_ARG, "method 7 needs a non-empty volumeSize");
    std::memset(&P, 0, sizeof P);
    std::memcpy(P.m, d->inv_view, sizeof P.m);
    P.W = d->width;
    P.H = d->height;
    P.CW = d->width;
    P.CH = d->height;
    P.density = d->density;
    P.brightness = d->brightness;
    P.toff = d->transfer_offset;
    P.tscale = d->transfer_scale;
    P.nx = v.nx; P.ny = v.ny; P.nz = v.nz;
    P.sy = v.sy; P.sz = v.sz;
    P.nb = v.nb;
    if (codec) {
        P.cb = g.cb;
        P.tpl = g.tpl;
        P.err = g.cerr;
        P.ntpl = g.ntpl;
        P.err_slots = g.err_slots;
        // template tables up to 32 KiB are staged in LDS (VR_CODEC_LDS=0 disables)
        const size_t tb = (size_t)g.ntpl * g.cnb * sizeof(float);
        const char *el = vr::tuning("VR_CODEC_LDS");
        P.tpl_lds = (tb <= 32768 && !(el && std::atoi(el) == 0)) ? (int)tb : 0;
    }
    if (flex) {
        P.flex = g.flex.blocks;
        P.nflex = g.flex.nblk;
        P.nb = g.flex.nb;
    }
    P.m7x = (int)d->volume_size.width;
    P.m7y = (int)d->volume_size.height;
    P.m7z = (int)d->volume_size.depth;
    P.enorm = entropy_norm(P.nb);
    P.tiles_x = tiles_x(d->width);
    P.tile_list = d->d_tile_list;
    P.perm = nullptr;
    uint32_t *record = nullptr;
    if (!d->d_tile_list) {
        int rc = frame_order(d, tiles_x(d->width), tiles_y(d->height), P.perm,
                             for_render ? &record : nullptr);
        if (rc != VR_OK) return rc;
    }
    P.out = d->d_output;
    P.out_f = d->d_output_f;
    P.out_n = d->d_steps;
    P.mark = nullptr;
    // VR_WG_PER_CU / VR_SEG_MAP for the codec and flexible-block launches; the
    // record marches take theirs, with every other launch knob, from the plan
    // (plan_input / apply_plan below, vr_plan.cpp)
    P.wg_per_cu = 0;
    if (const char *e = vr::tuning("VR_WG_PER_CU")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 32) P.wg_per_cu = v;
    }
    if (const char *e = vr::tuning("VR_SEG_MAP")) P.seg_map = std::atoi(e) != 0;
    P.oblique = std::fabs(d->inv_view[0]) >= 0.95f ? 0 : 1;
    device_lds(P.lds_cu, P.lds_wg);
    P.wave_clock = g.wave_clock;
    P.box_check = g.box_check;
    P.tile_cost = record;
    const uint64_t all = (uint64_t)tiles_x(d->width) * tiles_y(d->height);
    if (d->d_tile_list) {
        nslots = d->n_tiles;
    } else {
        if (all > 0xFFFFFFFFull) return fail(VR_ERR_ARG, "image too large");
        nslots = (uint32_t)all;
    }
    P.n_tiles = nslots;
    return VR_OK;
}

int fill_params(const vr_render_desc *d, vr::Params &P, uint32_t &nslots,
                bool for_render = false) {
    if (!d) return fail(VR_ERR_ARG, "null render descriptor");
    // a gradient method: its plane or a refusal, and the grid of its source's family
    // (a resident gradient plane has a resident source, so a resident volume)
    const int gsrc = grad_source(d->query_method);
    if (gsrc) {
        const int rc = check_method(d->query_method);
        if (rc != VR_OK) return rc;
    }
    const bool codec = (d->query_method >= 4 && d->query_method <= 6) || (gsrc >= 4 && gsrc <= 6);
    if (codec && !g.cb)
        return fail(VR_ERR_STATE, "queryMethod %d needs a codec volume (initCuda's codebook / "
                                  "vr_init_codec)", d->query_method);
    const bool flex = is_flex_method(d->query_method);
    if (!codec && !flex && !g.vol)
        return fail(VR_ERR_STATE, "no volume resident (initCuda / vr_init_* first)");
    // the codec volume: dense voxel order, its own bin count
    const FrameVol v = codec ? FrameVol{g.cnx, g.cny, g.cnz, g.cnb, (uint64_t)g.cnx,
                                        (uint64_t)g.cnx * (uint64_t)g.cny}
                             : FrameVol{g.nx, g.ny, g.nz, g.nb, g.sy, g.sz};
    return fill_frame_params(d, v, P, nslots, for_render);
}

// Bakes n planes of the P.nx x P.ny x P.nz grid into dst: launch(buf, plane floats,
// psy, psz) fills a zeroed buffer on the library's stream.  Synchronous: a later
// frame may run on another stream.  On a failure nothing changes (dst keeps what
// it held, the march keeps decoding per step): the stream drains before the
// buffer is freed, and a launch that has no kernel for the grid or the bin count
// (hipErrorInvalidValue) is VR_ERR_UNSUPPORTED.  `what` names the entry point and
// kernel, `vols` the volumes, in messages.
template <typename Launch>
int bake_planes(State::Planes &dst, int n, const vr::Params &P, const char *what,
                const char *vols, Launch launch) {
    State::Planes p;
    vr::plane_pitches((uint32_t)P.nx, (uint32_t)P.ny, p.sy, p.sz);
    p.floats = p.sz * (uint64_t)P.nz;
    // (4 floats of padding: a march fetches them beside a row's last voxel and
    // reads them with weight 0, so they must be there and hold finite floats)
    const size_t bytes = ((uint64_t)n * p.floats + 4) * sizeof(float);
    VR_HIP(hipMalloc(&p.buf, bytes));
    hipError_t e = hipMemsetAsync(p.buf, 0, bytes, g.stream);
    if (e == hipSuccess) e = launch(p.buf, p.floats, p.sy, p.sz);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(g.stream);
        (void)hipFree(p.buf);
        if (e == hipErrorInvalidValue)
            return fail(VR_ERR_UNSUPPORTED, "baking %s with %d bins, %d x %d x %d voxels (compiled: "
                                            "1,2,4,8,16,32 bins; at most 65535 rows and slices)",
                        vols, P.nb, P.nx, P.ny, P.nz);
        return hip_fail(e, what);
    }
    dst = p;
    return VR_OK;
}

// Bakes the statistics planes of the resident raw and codec volumes (whichever
// are resident and not yet baked).
int bake_stats() {
    if (!g.vol && !g.cb) return fail(VR_ERR_STATE, "no volume resident (initCuda / vr_init_* first)");
    vr::Params P;
    if (g.vol && !g.stats.buf) {
        std::memset(&P, 0, sizeof P);
        P.nx = g.nx; P.ny = g.ny; P.nz = g.nz;
        P.sy = g.sy; P.sz = g.sz;
        P.nb = g.nb;
        P.enorm = entropy_norm(g.nb);
        const int rc = bake_planes(
            g.stats, 4, P, "basicDataProcessing(k_bake_raw)", "record volumes",
            [&](float *out, uint64_t plane, uint64_t psy, uint64_t psz) {
                return vr::launch_bake_raw(g.vol, is_f16(), P, out, plane, psy, psz, g.stream);
            });
        if (rc != VR_OK) return rc;
    }
    if (g.cb && !g.cstats.buf) {
        std::memset(&P, 0, sizeof P);
        P.nx = g.cnx; P.ny = g.cny; P.nz = g.cnz;
        P.sy = (uint64_t)g.cnx;
        P.sz = (uint64_t)g.cnx * (uint64_t)g.cny;
        P.nb = g.cnb;
        P.enorm = entropy_norm(g.cnb);
        P.cb = g.cb;
        P.tpl = g.tpl;
        P.err = g.cerr;
        P.ntpl = g.ntpl;
        P.err_slots = g.err_slots;
        const int rc = bake_planes(
            g.cstats, 3, P, "basicDataProcessing(k_bake_codec)", "codec volumes",
            [&](float *out, uint64_t plane, uint64_t psy, uint64_t psz) {
                return vr::launch_bake_codec(P, out, plane, psy, psz, g.stream);
            });
        if (rc != VR_OK) return rc;
    }
    return VR_OK;
}

// vr_bake_*: the plane of query q from the records and q's state.  A plane that
// is there was baked from this state (any change drops it): nothing to do.
int bake_query(const RecordQuery &q) {
    const int rc = query_ready(q);
    if (rc != VR_OK) return rc;
    State::Planes &dst = query_plane(q.method);
    if (dst.buf) return VR_OK;
    vr::Params P;
    std::memset(&P, 0, sizeof P);
    P.nx = g.nx; P.ny = g.ny; P.nz = g.nz;
    P.sy = g.sy; P.sz = g.sz;
    P.nb = g.nb;
    const int rb = bake_planes(dst, 1, P, q.bake, "record volumes",
                               [&](float *out, uint64_t, uint64_t psy, uint64_t psz) {
                                   return q.bake_launch(P, out, psy, psz);
                               });
    if (rb == VR_OK) g.volume_epoch++;  // a tile order learned on the per-step march is not reused
    return rb;
}

// ---- synthetic volume tables ----
uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

double u01(uint64_t h) { return (double)(h >> 11) * 0x1.0p-53; }

void blob_axis(int n, double c, double s, float *out) {
    for (int i = 0; i < n; i++) {
        const double q = ((double)i + 0.5) / (double)n;
        out[i] = (float)std::exp(-(q - c) * (q - c) / (2.0 * s * s));
    }
}

// Oblique views of an 8-bin volume (the quad march, path 0) read a 2x2 (x, y)
// micro-brick copy of the records: a footprint's four (x, y) corners share
// one 128-B line when x0 and y0 are even, so a wave step touches fewer lines
// than in x rows.  Made on the first such frame of an owned
// volume (a caller-owned buffer adopted by vr_init_distribution may change
// behind the library's back), only if HBM keeps max(4 GiB, 5 %) free after it; without
// it the quad march reads the x rows.  VR_BRICK=0 (vr_set_tuning) disables it.
bool ensure_brick() {
    if (const char *e = vr::tuning("VR_BRICK"))
        if (std::atoi(e) == 0) return false;
    if (g.brick) return true;
    if (!g.vol || !g.owned || g.nb != 8 || is_f16()) return false;  // fp32 records only
    const uint64_t nxp = (uint64_t)g.nx + (g.nx & 1), nyp = (uint64_t)g.ny + (g.ny & 1);
    const uint64_t bsy = 2 * nxp, bsz = nxp * nyp;
    const uint64_t bytes = bsz * (uint64_t)g.nz * 8 * sizeof(float);
    if (!layout_room(bytes)) return false;
    float *buf = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    vr::Params P;
    std::memset(&P, 0, sizeof P);
    P.nx = g.nx; P.ny = g.ny; P.nz = g.nz;
    P.sy = g.sy; P.sz = g.sz;
    // synchronous, like the statistics bake: a later frame may run on another
    // stream (vr_set_stream) and must never see a partly written copy
    const auto t0 = std::chrono::steady_clock::now();
    if (vr::launch_brick8(g.vol, P, buf, bsy, bsz, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        return false;
    }
    g.layout_last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g.layout_last_bytes = bytes;
    g.layout_builds++;
    g.brick = buf;
    g.bsy = bsy;
    g.bsz = bsz;
    g.brick_bytes = bytes;
    return true;
}

// Views whose screen x runs along the volume's z or y axis (|M[8]| or |M[4]|
// >= 0.95: side views, e.g. the display() camera at yaw 90 deg, and top views
// at pitch and yaw 90 deg) see the x rows across: a wave's 64 rays sit at
// consecutive z (y), each reading its own lines.  A copy of the records with
// that axis contiguous (axis_copy_strides) gives them what x rows give the
// runSingleTest view -- consecutive lanes on consecutive records -- and the
// per-ray pipelined march reads it (1024^3 x 8, yaw 90: 3.01 -> 1.63 ms,
// DESIGN.md 2).  Both axis copies stay resident when the layout budget holds
// them (vr_set_layout_budget); otherwise a view along the other axis replaces
// the copy.  Made on the first such frame of an owned volume with B <= 8 (as
// ensure_brick: synchronous, timed into vr_layout_info) by k_axis_copy, an
// LDS-tiled transpose; VR_ZROWS=0 (vr_set_tuning) disables it.
bool ensure_axis_copy(int axis) {
    if (const char *e = vr::tuning("VR_ZROWS"))
        if (std::atoi(e) == 0) return false;
    const int i = axis - 1, other = 1 - i;
    if (g.acopy[i].buf) return true;
    if (!g.vol || !g.owned || !(g.nb == 1 || g.nb == 2 || g.nb == 4 || g.nb == 8)) return false;
    if (is_f16()) return false;  // fp32 records only
    uint64_t sx = 0, sy = 0, sz = 0;
    vr::axis_copy_strides(axis, (uint64_t)g.nx, (uint64_t)g.ny, (uint64_t)g.nz, sx, sy, sz);
    const uint64_t bytes = (uint64_t)g.nx * g.ny * (uint64_t)g.nz * (uint64_t)g.nb * sizeof(float);
    // keep the other axis' copy when both fit; drop it only if that makes room
    // (checked before anything is released)
    if (!layout_room(bytes)) {
        if (!g.acopy[other].buf || !layout_room(bytes, g.acopy[other].bytes)) return false;
        release_axis_copy(other);
    }
    float *buf = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    vr::Params P;
    std::memset(&P, 0, sizeof P);
    P.nx = g.nx; P.ny = g.ny; P.nz = g.nz; P.nb = g.nb;
    P.sy = g.sy; P.sz = g.sz;
    const auto t0 = std::chrono::steady_clock::now();
    if (vr::launch_axis_copy(g.vol, P, buf, sx, sy, sz, g.stream) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        return false;
    }
    g.layout_last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g.layout_last_bytes = bytes;
    g.layout_builds++;
    g.acopy[i].buf = buf;
    g.acopy[i].sx = sx;
    g.acopy[i].sy = sy;
    g.acopy[i].sz = sz;
    g.acopy[i].bytes = bytes;
    return true;
}

// Baked frames of views whose screen x runs along the volume's y or z (side
// and top views) read the planes' 16 x 2 x 1 bricks across: a wave's 64 rays
// sit at consecutive z (y), each on its own lines.  The plane the method
// filters gets a copy with that axis in the brick rows (k_plane_axis), the
// axis-rows idea of ensure_axis_copy for planes: one per axis, made on the
// first such frame within the layout budget, dropped with the planes.
// Axis 3 (round 5): oblique views get the plane in 8 x 2 x 2 bricks
// (k_plane8, gather8 MODE 6), whose lines also hold a footprint's z pair
// (per 64x4-tile line floor at 1024^3 C1: 3.77 -> 3.47 GB);
// VR_PLANE8=0 keeps such views on the 16 x 2 x 1 plane.
// Each (axis, method plane) keeps its own copy while the layout budget holds
// them, so a client alternating methods on one view class builds each copy
// once (one copy per axis was rebuilt -- hipMalloc, k_plane8, a
// stream sync, ~4.6 GB at 1024^3 -- on every method change); only when the
// budget is short are this axis' other planes' copies dropped for the new one.
bool ensure_plane_copy(int plane, int axis) {
    if (const char *e = vr::tuning(axis == 3 ? "VR_PLANE8" : "VR_ZROWS"))
        if (std::atoi(e) == 0) return false;
    const int i = axis - 1;
    if (!g.stats.buf || plane < 0 || plane > 2) return false;
    if (g.pcopy[i][plane].buf) return true;
    const uint32_t nf = axis == 2 ? g.nz : g.ny, np = axis == 2 ? g.ny : g.nx;
    uint64_t ns = axis == 2 ? (uint64_t)g.nx : (uint64_t)g.nz;
    if (nf >= (1u << 16) || np > 65535 || ns > 65535 || g.nx > 65535) return false;
    uint64_t dsy = 0, dsz = 0;
    if (axis == 3) {
        vr::plane8_pitches(g.nx, g.ny, dsy, dsz);
        ns = (uint64_t)(g.nz + 1) / 2;  // slice pairs
    } else {
        vr::plane_pitches(nf, np, dsy, dsz);
    }
    // gather8 MODE 4/5/6: 32-bit offsets inside a slice (pair)
    if (dsz >= (1ull << 32)) return false;
    const uint64_t bytes = (dsz * ns + 4) * sizeof(float);
    if (!layout_room(bytes, 0)) {  // room only without this axis' other planes' copies
        uint64_t freed = 0;
        for (int p = 0; p < 3; p++) freed += g.pcopy[i][p].bytes;
        if (!layout_room(bytes, freed)) return false;
        for (int p = 0; p < 3; p++) release_plane_copy(i, p);
    }
    float *buf = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const float *src = g.stats.buf + (uint64_t)plane * g.stats.floats;
    if (hipMemsetAsync(buf, 0, bytes, g.stream) != hipSuccess ||
        (axis == 3 ? vr::launch_plane8(src, g.stats.sy, g.stats.sz, buf, dsy, dsz, g.nx, g.ny,
                                       g.nz, g.stream)
                   : vr::launch_plane_axis(src, g.stats.sy, g.stats.sz, buf, dsy, dsz, g.nx,
                                           g.ny, g.nz, axis, g.stream)) != hipSuccess ||
        hipStreamSynchronize(g.stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(buf);
        return false;
    }
    g.layout_last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g.layout_last_bytes = bytes;
    g.layout_builds++;
    g.pcopy[i][plane].buf = buf;
    g.pcopy[i][plane].sy = dsy;
    g.pcopy[i][plane].sz = dsz;
    g.pcopy[i][plane].bytes = bytes;
    return true;
}

}  // namespace

namespace vr {
int record_error(int status, const char *msg) { return fail(status, "%s", msg); }
const char *tuning(const char *key) {
    auto it = g_tuning.find(key);
    if (it != g_tuning.end()) return it->second.c_str();
#ifdef VR_TUNING
    return std::getenv(key);
#else
    return nullptr;
#endif
}
// Span index: sorted keys and, per key, the entry the reference's linear scan
// (K:1352-1372) returns -- its `break` leaves only the x loop, so among equal
// spans the last 64-entry row holding one wins, and its first entry.  Entries
// with a coordinate outside [0, 1023] can never match a sub-span and are left out.
void build_span_index(const vr_int4 *lo, const vr_int4 *hi, int n,
                             std::vector<uint64_t> &keys, std::vector<int32_t> &idx) {
    std::vector<std::pair<uint64_t, int32_t>> kv;
    kv.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        const int c[6] = {lo[i].x, lo[i].y, lo[i].z, hi[i].x, hi[i].y, hi[i].z};
        bool ok = true;
        for (int q = 0; q < 6; q++) ok = ok && c[q] >= 0 && c[q] < 1024;
        if (ok) kv.push_back({vr::span_key(c[0], c[1], c[2], c[3], c[4], c[5]), i});
    }
    std::sort(kv.begin(), kv.end());
    keys.clear();
    idx.clear();
    for (size_t a = 0; a < kv.size();) {
        size_t b = a;
        while (b < kv.size() && kv[b].first == kv[a].first) b++;
        const int32_t last_row = kv[b - 1].second / 64;
        size_t pick = a;
        while (kv[pick].second / 64 != last_row) pick++;
        keys.push_back(kv[a].first);
        idx.push_back(kv[pick].second);
        a = b;
    }
}

template <typename T>
hipError_t upload(T *&dst, const T *src, size_t n) {
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc(&dst, n * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

}  // namespace vr

extern "C" {

const char *vr_version(void) { return "vrdd-amd 0.1 (gfx950)"; }

const char *vr_last_kernel(void) { return vr::last_march_kernel(); }

// Measured read ceiling: the resident record volume streamed
// once per rep by k_stream_read on the library's stream, timed with HIP events.
int vr_stream_read(int reps, float *ms, uint64_t *bytes) {
    if (!ms || reps < 1) return fail(VR_ERR_ARG, "vr_stream_read: ms null or reps < 1");
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident");
    const uint64_t nbytes = (g.sz * (uint64_t)g.nz * (uint64_t)g.nb * elem_bytes()) & ~(uint64_t)15;
    hipDevice_t dev;
    int dev_id = 0, cus = 0;
    VR_HIP(hipGetDevice(&dev_id));
    (void)dev;
    VR_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id));
    const uint32_t nblocks = (uint32_t)(cus > 0 ? cus : 256) * 8u;  // 8 workgroups per CU
    uint32_t *d = nullptr;
    VR_HIP(hipMalloc(&d, nblocks * sizeof(uint32_t)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best = 0.0f, sum = 0.0f;
    // one untimed pass first (clocks, address translation)
    if (e == hipSuccess) e = vr::launch_stream_read(g.vol, nbytes, d, nblocks, g.stream);
    for (int r = 0; r < reps && e == hipSuccess; r++) {
        e = hipEventRecord(e0, g.stream);
        if (e == hipSuccess) e = vr::launch_stream_read(g.vol, nbytes, d, nblocks, g.stream);
        if (e == hipSuccess) e = hipEventRecord(e1, g.stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float t = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        if (e == hipSuccess) {
            best = (r == 0 || t < best) ? t : best;
            sum += t;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "vr_stream_read");
    ms[0] = best;
    ms[1] = sum / (float)reps;
    if (bytes) *bytes = nbytes;
    return VR_OK;
}

int vr_selftest_logf(uint64_t *counts) {
    if (!counts) return fail(VR_ERR_ARG, "null pointer");
    unsigned long long *d = nullptr;
    VR_HIP(hipMalloc(&d, 2 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), g.stream);
    if (e == hipSuccess) e = vr::launch_logcheck(d, g.stream);
    unsigned long long h[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "vr_selftest_logf");
    counts[0] = h[0];
    counts[1] = h[1];
    return VR_OK;
}

const char *vr_last_error(void) { return g.err.c_str(); }
int vr_last_status(void) { return g.status; }
void vr_clear_error(void) {
    g.err.clear();
    g.status = VR_OK;
}

uint32_t vr_tiles_x(uint32_t width) { return tiles_x(width); }
uint32_t vr_tiles_y(uint32_t height) { return tiles_y(height); }

int vr_set_tuning(const char *key, const char *value) {
    if (!key || !*key) return fail(VR_ERR_ARG, "vr_set_tuning: empty key");
    if (value) g_tuning[key] = value;
    else g_tuning.erase(key);
    g.perm_key[0] = 0;  // knobs such as VR_XBLOCK / VR_NO_LPT shape the frame order
    return VR_OK;
}

void vr_clear_tuning(void) {
    g_tuning.clear();
    g.perm_key[0] = 0;
}

int vr_set_stream(void *stream) {
    g.stream = (hipStream_t)stream;
    return VR_OK;
}

int vr_init_codec(const vr_int4 *codebook, vr_extent dims, const float *templates,
                  int ntemplates, const vr_float2 *errors, int err_slots, int nbins, int where) {
    if (!codebook || !templates || (!errors && err_slots > 0))
        return fail(VR_ERR_ARG, "vr_init_codec: null array");
    if (where != 0 && where != 1) return fail(VR_ERR_ARG, "vr_init_codec: where must be 0 or 1");
    if (dims.width == 0 || dims.height == 0 || dims.depth == 0 || nbins <= 0 ||
        ntemplates <= 0 || err_slots < 0 || dims.width > 65535 || dims.height > 65535 ||
        dims.depth > 65535)
        return fail(VR_ERR_ARG, "vr_init_codec: bad sizes");
    if (nbins != 1 && nbins != 2 && nbins != 4 && nbins != 8 && nbins != 16 && nbins != 32)
        return fail(VR_ERR_UNSUPPORTED, "vr_init_codec: %d bins (compiled: 1,2,4,8,16,32)", nbins);
    const uint64_t nvox = (uint64_t)dims.width * dims.height * dims.depth;
    release_codec();
    const hipMemcpyKind kind = where == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const size_t bcb = nvox * sizeof(int4), btp = (size_t)ntemplates * nbins * sizeof(float);
    const size_t ber = nvox * (size_t)err_slots * sizeof(float2);
    VR_HIP(hipMalloc(&g.cb, bcb));
    VR_HIP(hipMalloc(&g.tpl, btp));
    if (ber) VR_HIP(hipMalloc(&g.cerr, ber));
    hipError_t e = hipMemcpy(g.cb, codebook, bcb, kind);
    if (e == hipSuccess) e = hipMemcpy(g.tpl, templates, btp, kind);
    if (e == hipSuccess && ber) e = hipMemcpy(g.cerr, errors, ber, kind);
    unsigned long long *bad = nullptr, hbad = 0;
    if (e == hipSuccess) e = hipMalloc(&bad, sizeof hbad);
    if (e == hipSuccess) e = hipMemset(bad, 0, sizeof hbad);
    if (e == hipSuccess) e = vr::launch_codec_check(g.cb, nvox, ntemplates, nbins, err_slots, bad, 0);
    if (e == hipSuccess) e = hipMemcpy(&hbad, bad, sizeof hbad, hipMemcpyDeviceToHost);
    if (bad) (void)hipFree(bad);
    if (e != hipSuccess) {
        release_codec();
        return hip_fail(e, "vr_init_codec");
    }
    if (hbad) {
        release_codec();
        return fail(VR_ERR_ARG,
                    "vr_init_codec: %llu codebook entries out of range (template id < %d, "
                    "0 <= shift < %d, 0 <= NE <= %d)", hbad, ntemplates, nbins, err_slots);
    }
    g.cnx = (int)dims.width;
    g.cny = (int)dims.height;
    g.cnz = (int)dims.depth;
    g.cnb = nbins;
    g.ntpl = ntemplates;
    g.err_slots = err_slots;
    return VR_OK;
}

int vr_init_flex(const vr_flex_tables *t) {
    if (!t) return fail(VR_ERR_ARG, "vr_init_flex: null tables");
    if (t->dim < 1 || t->dim > vr::kFlexMaxDim)
        return fail(VR_ERR_ARG, "vr_init_flex: dim %d outside [1, %d]", t->dim, vr::kFlexMaxDim);
    if (t->nbins < 1 || t->nbins > vr::kFlexMaxBins)
        return fail(VR_ERR_ARG, "vr_init_flex: nbins %d outside [1, %d]", t->nbins,
                    vr::kFlexMaxBins);
    if (t->n_fractal < 0 || t->n_simple < 0 || (t->n_fractal > 0 && t->ntemplates < 1))
        return fail(VR_ERR_ARG, "vr_init_flex: bad table sizes");
    if ((t->n_fractal > 0 && (!t->fractal_low || !t->fractal_high || !t->fractal_code ||
                              !t->fractal_errors || !t->templates)) ||
        (t->n_simple > 0 && (!t->simple_low || !t->simple_high || !t->simple_count ||
                             !t->simple_hist)))
        return fail(VR_ERR_ARG, "vr_init_flex: null array");
    const int nb = t->nbins;
    for (int i = 0; i < t->n_fractal; i++) {  // K:1377-1385 (the reference only prints)
        const vr_int4 c = t->fractal_code[i];
        if (c.x < 0 || c.x >= t->ntemplates || c.y < 0 || c.y >= nb || c.w < 0 || c.w > nb)
            return fail(VR_ERR_ARG,
                        "vr_init_flex: fractal entry %d out of range (template %d of %d, shift %d, "
                        "NE %d, %d bins)", i, c.x, t->ntemplates, c.y, c.w, nb);
    }
    for (int i = 0; i < t->n_simple; i++)
        if (t->simple_count[i] < 0 || t->simple_count[i] > nb)
            return fail(VR_ERR_ARG, "vr_init_flex: simple entry %d has %d bins", i,
                        t->simple_count[i]);
    std::vector<uint64_t> fk, sk;
    std::vector<int32_t> fi, si;
    vr::build_span_index(t->fractal_low, t->fractal_high, t->n_fractal, fk, fi);
    vr::build_span_index(t->simple_low, t->simple_high, t->n_simple, sk, si);
    release_flex();
    State::Flex &f = g.flex;
    hipError_t e = vr::upload(f.fkeys, fk.data(), fk.size());
    if (e == hipSuccess) e = vr::upload(f.fidx, fi.data(), fi.size());
    if (e == hipSuccess) e = vr::upload(f.skeys, sk.data(), sk.size());
    if (e == hipSuccess) e = vr::upload(f.sidx, si.data(), si.size());
    if (e == hipSuccess)
        e = vr::upload(f.fcode, reinterpret_cast<const int4 *>(t->fractal_code), (size_t)t->n_fractal);
    if (e == hipSuccess)
        e = vr::upload(f.ferr, reinterpret_cast<const float2 *>(t->fractal_errors),
                   (size_t)t->n_fractal * nb);
    if (e == hipSuccess) e = vr::upload(f.scount, t->simple_count, (size_t)t->n_simple);
    if (e == hipSuccess)
        e = vr::upload(f.shist, reinterpret_cast<const float2 *>(t->simple_hist),
                   (size_t)t->n_simple * nb);
    if (e == hipSuccess && t->n_fractal > 0)
        e = vr::upload(f.tpl, t->templates, (size_t)t->ntemplates * nb);
    if (e != hipSuccess) {
        release_flex();
        return hip_fail(e, "vr_init_flex");
    }
    f.dim = t->dim;
    f.nb = nb;
    f.ntpl = t->ntemplates;
    f.nf = t->n_fractal;
    f.ns = t->n_simple;
    f.nfk = (int)fk.size();
    f.nsk = (int)sk.size();
    return VR_OK;
}

int vr_flex_process(int block) {
    State::Flex &f = g.flex;
    if (f.dim == 0) return fail(VR_ERR_STATE, "vr_flex_process: no span tables (vr_init_flex)");
    if (block < 1 || block > f.dim)
        return fail(VR_ERR_ARG, "vr_flex_process: block %d outside [1, %d]", block, f.dim);
    const int nblk = (f.dim + block - 1) / block;  // K:906-931
    const size_t nblocks = (size_t)nblk * nblk * nblk;
    release_flex_blocks();
    vr::FlexTables T;
    T.dim = f.dim;
    T.nb = f.nb;
    T.fkeys = f.fkeys;
    T.fidx = f.fidx;
    T.nfk = f.nfk;
    T.fcode = f.fcode;
    T.ferr = f.ferr;
    T.skeys = f.skeys;
    T.sidx = f.sidx;
    T.nsk = f.nsk;
    T.scount = f.scount;
    T.shist = f.shist;
    T.tpl = f.tpl;
    float *ch = nullptr;
    unsigned int *missing = nullptr, hmiss = 0;
    float4 *blocks = nullptr;
    hipError_t e = hipMalloc(&ch, nblocks * 8 * f.nb * sizeof(float) + 256);
    if (e == hipSuccess) e = hipMalloc(&blocks, nblocks * sizeof(float4));
    if (e == hipSuccess) {
        missing = reinterpret_cast<unsigned int *>(ch + nblocks * 8 * f.nb);
        e = hipMemsetAsync(missing, 0, sizeof(unsigned int), g.stream);
    }
    if (e == hipSuccess) e = vr::launch_flex_corners(T, block, nblk, ch, missing, g.stream);
    if (e == hipSuccess) e = vr::launch_flex_blocks(f.nb, nblk, ch, blocks, g.stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&hmiss, missing, sizeof hmiss, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (ch) (void)hipFree(ch);
    if (e != hipSuccess) {
        if (blocks) (void)hipFree(blocks);
        return hip_fail(e, "vr_flex_process");
    }
    if (hmiss) {
        (void)hipFree(blocks);
        return fail(VR_ERR_ARG, "vr_flex_process: a sub-span of some block corner has no table "
                                "entry (the reference reads an uninitialised codebook entry)");
    }
    f.blocks = blocks;
    f.nblk = nblk;
    return nblk;
}

int vr_flex_info(int *nblk, int *nbins, const float **d_blocks) {
    if (nblk) *nblk = g.flex.nblk;
    if (nbins) *nbins = g.flex.nb;
    if (d_blocks) *d_blocks = reinterpret_cast<const float *>(g.flex.blocks);
    return g.flex.blocks ? VR_OK : fail(VR_ERR_STATE, "no flexible-block statistics resident");
}

// vr_init_distribution / vr_init_distribution_f16: bins of `elem` bytes each
static int init_records(const void *bins, vr_extent dims, int nbins, int where, int dtype) {
    const size_t elem = dtype == VR_DTYPE_F16 ? 2 : sizeof(float);
    if (!bins) return fail(VR_ERR_ARG, "null distribution pointer");
    if (nbins < 1) return fail(VR_ERR_ARG, "nbins must be >= 1 (got %d)", nbins);
    if (dims.width == 0 || dims.height == 0 || dims.depth == 0)
        return fail(VR_ERR_ARG, "empty volume");
    if (dims.width > 65536 || dims.height > 65536 || dims.depth > 65536)
        return fail(VR_ERR_ARG, "volume dimension > 65536");
    if (dtype == VR_DTYPE_F16) {
        if (nbins != 1 && nbins != 2 && nbins != 4 && nbins != 8 && nbins != 16 && nbins != 32)
            return fail(VR_ERR_UNSUPPORTED, "f16 volumes with %d bins (compiled: 1,2,4,8,16,32)",
                        nbins);
        // a record is read in loads of up to 16 bytes (vr_half.h load_rec_h)
        const size_t align = std::min<size_t>(16, 2 * (size_t)nbins);
        if (where == 2 && reinterpret_cast<uintptr_t>(bins) % align != 0)
            return fail(VR_ERR_ARG, "an adopted f16 volume of %d bins must be aligned to %zu bytes",
                        nbins, align);
    }
    release_volume();
    const int nx = (int)dims.width, ny = (int)dims.height, nz = (int)dims.depth;
    uint64_t sy, sz;
    if (where == 2) {  // adopted buffer keeps its dense AoS layout
        sy = (uint64_t)nx;
        sz = sy * (uint64_t)ny;
        g.vol = static_cast<float *>(const_cast<void *>(bins));
        g.owned = false;
    } else {
        choose_pitch(nx, ny, sy, sz);
        const size_t rec = (size_t)nbins * elem;
        char *d = nullptr;
        const char *src = static_cast<const char *>(bins);
        VR_HIP(hipMalloc(&d, sz * (size_t)nz * rec));
        const hipMemcpyKind kind = where == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        hipError_t e = hipSuccess;
        if (sy == (uint64_t)nx && sz == sy * (uint64_t)ny) {
            e = hipMemcpy(d, src, sz * (size_t)nz * rec, kind);
        } else {  // one pitched 2-D copy per slice
            for (int z = 0; z < nz && e == hipSuccess; z++)
                e = hipMemcpy2D(d + (size_t)z * sz * rec, sy * rec,
                                src + (size_t)z * ny * nx * rec, (size_t)nx * rec,
                                (size_t)nx * rec, (size_t)ny, kind);
        }
        if (e != hipSuccess) {
            (void)hipFree(d);
            return hip_fail(e, "hipMemcpy(volume)");
        }
        g.vol = reinterpret_cast<float *>(d);
        g.owned = true;
    }
    g.dtype = dtype;
    g.sy = sy;
    g.sz = sz;
    g.nx = nx;
    g.ny = ny;
    g.nz = nz;
    g.nb = nbins;
    return VR_OK;
}

int vr_init_distribution(const float *bins, vr_extent dims, int nbins, int where) {
    return init_records(bins, dims, nbins, where, VR_DTYPE_F32);
}

int vr_init_distribution_f16(const void *bins, vr_extent dims, int nbins, int where) {
    return init_records(bins, dims, nbins, where, VR_DTYPE_F16);
}

int vr_volume_dtype(void) {
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident");
    return g.dtype;
}

// The resident fp32 records narrowed to f16 on the device (k_narrow_f16) into a
// new library-owned buffer of the same record pitches; the fp32 buffer goes
// only once the new one is complete, so a failure leaves the volume as it was.
int vr_convert_f16(void) {
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident");
    if (g.dtype == VR_DTYPE_F16) return fail(VR_ERR_STATE, "the resident volume is f16 already");
    if (g.nb != 1 && g.nb != 2 && g.nb != 4 && g.nb != 8 && g.nb != 16 && g.nb != 32)
        return fail(VR_ERR_UNSUPPORTED, "f16 volumes with %d bins (compiled: 1,2,4,8,16,32)", g.nb);
    const uint64_t n = g.sz * (uint64_t)g.nz * (uint64_t)g.nb;
    void *buf = nullptr;
    VR_HIP(hipMalloc(&buf, n * 2));
    hipError_t e = vr::launch_narrow_f16(g.vol, buf, n, g.stream);
    // synchronous, like the statistics bake: a later frame may run on another stream
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return hip_fail(e, "vr_convert_f16(k_narrow_f16)");
    }
    release_stats();
    release_brick();
    release_axis_copy();
    g.volume_epoch++;  // the records changed: an order learned on them is not reused
    if (g.owned) (void)hipFree(g.vol);
    g.vol = static_cast<float *>(buf);
    g.owned = true;
    g.dtype = VR_DTYPE_F16;
    return VR_OK;
}

// the section-5 blob field tables (host), shared by both synthesizers
void blob_tables(int nx, int ny, int nz, uint64_t seed, vr::SynthArgs &a, std::vector<float> &gx,
                 std::vector<float> &gy, std::vector<float> &gz) {
    gx.assign((size_t)vr::kSynthBlobs * nx, 0.0f);
    gy.assign((size_t)vr::kSynthBlobs * ny, 0.0f);
    gz.assign((size_t)vr::kSynthBlobs * nz, 0.0f);
    for (int k = 0; k < vr::kSynthBlobs; k++) {
        double r[5];
        for (int j = 0; j < 5; j++)
            r[j] = u01(splitmix64(seed + 0x100u + 8u * (uint64_t)k + (uint64_t)j));
        a.amp[k] = (float)(0.3 + 0.7 * r[0]);
        const double s = 0.05 + 0.15 * r[4];
        blob_axis(nx, 0.2 + 0.6 * r[1], s, gx.data() + (size_t)k * nx);
        blob_axis(ny, 0.2 + 0.6 * r[2], s, gy.data() + (size_t)k * ny);
        blob_axis(nz, 0.2 + 0.6 * r[3], s, gz.data() + (size_t)k * nz);
    }
}

int vr_synthesize_codec(vr_extent dims, int nbins, int ntemplates, int slots, uint64_t seed) {
    if (nbins != 1 && nbins != 2 && nbins != 4 && nbins != 8 && nbins != 16 && nbins != 32)
        return fail(VR_ERR_UNSUPPORTED, "codec volumes with %d bins (compiled: 1,2,4,8,16,32)", nbins);
    if (ntemplates < 1 || slots < 0 || slots > nbins)
        return fail(VR_ERR_ARG, "vr_synthesize_codec: bad template count or slots");
    if (dims.width == 0 || dims.height == 0 || dims.depth == 0 || dims.width > 65535 ||
        dims.height > 65535 || dims.depth > 65535)
        return fail(VR_ERR_ARG, "vr_synthesize_codec: bad dims");
    const int nx = (int)dims.width, ny = (int)dims.height, nz = (int)dims.depth;
    const uint64_t nvox = (uint64_t)nx * ny * nz;
    vr::SynthArgs a{};
    std::vector<float> gx, gy, gz;
    blob_tables(nx, ny, nz, seed, a, gx, gy, gz);
    // templates: discretised Gaussians of mean (t + 0.5) / T, sigma 0.06 (double, normalised)
    std::vector<float> tpl((size_t)ntemplates * nbins);
    for (int t = 0; t < ntemplates; t++) {
        const double mu = ((double)t + 0.5) / (double)ntemplates;
        std::vector<double> e(nbins);
        double sum = 0.0;
        for (int b = 0; b < nbins; b++) {
            const double dd = ((double)b + 0.5) / (double)nbins - mu;
            e[b] = std::exp(-dd * dd / (2.0 * 0.06 * 0.06));
            sum += e[b];
        }
        for (int b = 0; b < nbins; b++) tpl[(size_t)t * nbins + b] = (float)(e[b] / sum);
    }
    release_codec();
    float *dgx = nullptr, *dgy = nullptr, *dgz = nullptr;
    hipError_t e = hipMalloc(&g.cb, nvox * sizeof(int4));
    if (e == hipSuccess && slots) e = hipMalloc(&g.cerr, nvox * (size_t)slots * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&g.tpl, tpl.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgx, gx.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgy, gy.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgz, gz.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(g.tpl, tpl.data(), tpl.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgx, gx.data(), gx.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgy, gy.data(), gy.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgz, gz.data(), gz.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        a.gx = dgx; a.gy = dgy; a.gz = dgz;
        a.nx = nx; a.ny = ny; a.nz = nz; a.nb = nbins; a.seed = seed;
        e = vr::launch_synth_codec(g.cb, g.cerr, a, ntemplates, slots, g.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (dgx) (void)hipFree(dgx);
    if (dgy) (void)hipFree(dgy);
    if (dgz) (void)hipFree(dgz);
    if (e != hipSuccess) {
        release_codec();
        return hip_fail(e, "vr_synthesize_codec");
    }
    g.cnx = nx; g.cny = ny; g.cnz = nz; g.cnb = nbins; g.ntpl = ntemplates; g.err_slots = slots;
    return VR_OK;
}

int vr_codec_info(vr_extent *dims, int *nbins, int *ntemplates, int *slots, const void **codebook,
                  const float **templates, const void **errors) {
    if (!g.cb) return fail(VR_ERR_STATE, "no codec volume resident");
    if (dims) {
        dims->width = (size_t)g.cnx;
        dims->height = (size_t)g.cny;
        dims->depth = (size_t)g.cnz;
    }
    if (nbins) *nbins = g.cnb;
    if (ntemplates) *ntemplates = g.ntpl;
    if (slots) *slots = g.err_slots;
    if (codebook) *codebook = g.cb;
    if (templates) *templates = g.tpl;
    if (errors) *errors = g.cerr;
    return VR_OK;
}

int vr_synthesize(vr_extent dims, int nbins, uint64_t seed) {
    if (nbins < 1) return fail(VR_ERR_ARG, "nbins must be >= 1 (got %d)", nbins);
    if (dims.width == 0 || dims.height == 0 || dims.depth == 0)
        return fail(VR_ERR_ARG, "empty volume");
    if (dims.width > 65536 || dims.height > 65536 || dims.depth > 65536)
        return fail(VR_ERR_ARG, "volume dimension > 65536");
    const int nx = (int)dims.width, ny = (int)dims.height, nz = (int)dims.depth;
    const size_t nvox = dims.width * dims.height * dims.depth;
    vr::SynthArgs a{};
    std::vector<float> gx, gy, gz;
    blob_tables(nx, ny, nz, seed, a, gx, gy, gz);
    std::vector<float> tab;
    if (nbins > 1) {
        tab.resize((size_t)vr::kSynthG * vr::kSynthQ * nbins);
        std::vector<double> e(nbins);
        for (int gi = 0; gi < vr::kSynthG; gi++) {
            const double sig = 0.02 + 0.1 * (double)gi / 15.0;
            for (int q = 0; q < vr::kSynthQ; q++) {
                const double mu = ((double)q + 0.5) / (double)vr::kSynthQ;
                double sum = 0.0;
                for (int b = 0; b < nbins; b++) {
                    const double dd = ((double)b + 0.5) / (double)nbins - mu;
                    e[b] = std::exp(-dd * dd / (2.0 * sig * sig));
                    sum += e[b];
                }
                float *row = tab.data() + ((size_t)gi * vr::kSynthQ + q) * nbins;
                for (int b = 0; b < nbins; b++) row[b] = (float)(e[b] / sum);
            }
        }
    }
    release_volume();
    uint64_t sy, sz;
    choose_pitch(nx, ny, sy, sz);
    float *vol = nullptr, *dgx = nullptr, *dgy = nullptr, *dgz = nullptr, *dtab = nullptr;
    auto cleanup = [&]() {
        if (dgx) (void)hipFree(dgx);
        if (dgy) (void)hipFree(dgy);
        if (dgz) (void)hipFree(dgz);
        if (dtab) (void)hipFree(dtab);
    };
    (void)nvox;
    hipError_t e = hipMalloc(&vol, sz * (size_t)nz * (size_t)nbins * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(volume)");
    e = hipMalloc(&dgx, gx.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgy, gy.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgz, gz.size() * 4);
    if (e == hipSuccess && !tab.empty()) e = hipMalloc(&dtab, tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(dgx, gx.data(), gx.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgy, gy.data(), gy.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgz, gz.data(), gz.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && dtab)
        e = hipMemcpy(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        a.gx = dgx; a.gy = dgy; a.gz = dgz; a.table = dtab;
        a.nx = nx; a.ny = ny; a.nz = nz; a.nb = nbins; a.seed = seed;
        a.sy = sy; a.sz = sz;
        e = vr::launch_synth(vol, a, g.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    cleanup();
    if (e != hipSuccess) {
        (void)hipFree(vol);
        return hip_fail(e, "vr_synthesize");
    }
    g.vol = vol;
    g.owned = true;
    g.nx = nx; g.ny = ny; g.nz = nz; g.nb = nbins;
    g.sy = sy; g.sz = sz;
    return VR_OK;
}

int vr_set_layout_budget(uint64_t bytes) {
    g.layout_budget = bytes;
    // copies already resident beyond a lowered budget are dropped (the next
    // frame that wants one makes it again if it fits)
    if (layout_resident() > layout_budget_bytes()) {
        release_brick();
        release_axis_copy();
        release_plane_copies();
    }
    return VR_OK;
}

int vr_layout_info(uint64_t *resident_bytes, int *builds, float *last_build_ms,
                   uint64_t *last_build_bytes) {
    if (resident_bytes) *resident_bytes = layout_resident();
    if (builds) *builds = g.layout_builds;
    if (last_build_ms) *last_build_ms = g.layout_last_ms;
    if (last_build_bytes) *last_build_bytes = g.layout_last_bytes;
    return VR_OK;
}

int vr_volume_layout(size_t *row_pitch, size_t *slice_pitch) {
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident");
    if (row_pitch) *row_pitch = (size_t)g.sy;
    if (slice_pitch) *slice_pitch = (size_t)g.sz;
    return VR_OK;
}

int vr_volume_info(vr_extent *dims, int *nbins, const float **d_bins) {
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident");
    if (dims) {
        dims->width = (size_t)g.nx;
        dims->height = (size_t)g.ny;
        dims->depth = (size_t)g.nz;
    }
    if (nbins) *nbins = g.nb;
    if (d_bins) *d_bins = g.vol;
    return VR_OK;
}

}  // extern "C"

namespace {

static_assert(vr::kPlanTileRays == vr::kTileW * vr::kTileH && vr::kPlanBoxMax == vr::kBoxMax,
              "vr_plan.h repeats vr_device.h's tile size and box capacity");

// What plan_march() reads of any frame: the view, the image with the rendered
// rectangle (P: with the clip applied), the tile list and the tuning knobs.
vr::PlanIn plan_frame(const vr_render_desc *d, const vr::Params &P) {
    vr::PlanIn in = {};
    in.m0 = d->inv_view[0];
    in.m4 = d->inv_view[4];
    in.m8 = d->inv_view[8];
    in.W = d->width;
    in.H = d->height;
    in.CW = P.CW;
    in.CH = P.CH;
    in.tile_list = d->d_tile_list != nullptr;
    in.n_tiles = d->n_tiles;
    in.tuning = vr::tuning;
    return in;
}

// ... and of a frame of methods 1/2/3/7 over the resident record volume (P:
// fill_params' result).
vr::PlanIn plan_input(const vr_render_desc *d, const vr::Params &P, bool count) {
    vr::PlanIn in = plan_frame(d, P);
    in.method = d->query_method;
    // (methods 4/5/6 come here only for their baked planes: the codec volume's)
    const bool codec = d->query_method >= 4 && d->query_method <= 6;
    in.nb = P.nb;
    in.nx = P.nx;
    in.ny = P.ny;
    in.nz = P.nz;
    in.owned = !codec && g.owned;
    in.f16 = !codec && is_f16();
    in.baked = (codec ? g.cstats.buf : g.stats.buf) != nullptr;
    in.plane_sy = codec ? g.cstats.sy : g.stats.sy;
    in.plane_sz = codec ? g.cstats.sz : g.stats.sz;
    in.m7x = P.m7x;
    in.m7y = P.m7y;
    in.m7z = P.m7z;
    in.count = count;
    return in;
}

// The plan's launch knobs into the Params the kernels (and, for the host-only
// fields path / duo / quad2 / axis_view, nobody) read.
void apply_plan(const vr::MarchPlan &pl, vr::Params &P) {
    P.path = pl.path;
    P.duo = pl.duo;
    P.quad2 = pl.quad2;
    P.axis_view = pl.axis;
    P.plane_axis = pl.plane_axis;
    P.seg_lanes = pl.seg_lanes;
    P.seg_map = pl.seg_map;
    P.wq_map = pl.wq_map;
    P.head_slots = pl.head_slots;
    P.head_lanes = pl.head_lanes;
    P.head_tail = pl.head_tail;
    P.box_max = pl.box_max;
    P.wg_per_cu = pl.wg_per_cu;
}

// A frame from a baked plane of one float per voxel of P's grid, in x-row bricks
// of pitches psy / psz: the weighted, quantile and distance planes of the records
// and the planes of a GMM volume (vr_render_gmm_baked).  The plan's plane march on
// the bricks themselves -- such a plane has no layout copies.
int launch_plane_frame(const vr_render_desc *desc, vr::Params &P, uint32_t nslots,
                       const float *plane, uint64_t psy, uint64_t psz, hipError_t &e) {
    vr::PlanIn in = plan_frame(desc, P);
    // any plane statistic (a variance plane too: the plan of a baked frame tells
    // methods 1 and 2 apart nowhere)
    in.method = 1;
    in.nb = 1;
    in.nx = P.nx;
    in.ny = P.ny;
    in.nz = P.nz;
    in.owned = false;
    in.f16 = false;
    in.baked = true;
    in.plane_sy = psy;
    in.plane_sz = psz;
    in.count = false;
    in.denied = vr::kLayoutAxis | vr::kLayoutBrick | vr::kLayoutPlane;
    const vr::MarchPlan pl = vr::plan_march(in);
    if (pl.layout != vr::kLayoutNone || pl.method > 0)
        return fail(VR_ERR_UNSUPPORTED, "no plane march for this frame of a baked plane");
    apply_plan(pl, P);
    P.nb = 1;
    P.sy = psy;
    P.sz = psz;
    e = vr::launch_plan(pl, plane, P, nslots, g.stream);
    return VR_OK;
}

// The march of a frame of record query q (check_method has passed).  Per step:
// q's kernel on the x rows of the records, whatever the view -- no plan, no layout
// copy.  With q's baked plane resident (vr_bake_*): the plane march plan_march
// names for one float per voxel in x-row bricks (launch_plane_frame)
// -- the same eight floats into the same filter, so the same frame bit for bit.
// Method 13 combines its eight corners where the others blend them: its plane of
// F goes to k_march_cross_plane, the one-lane march for every view, no plan.
int launch_query(const RecordQuery &q, const vr_render_desc *desc, vr::Params &P,
                 uint32_t nslots, hipError_t &e) {
    const State::Planes &pl = query_plane(q.method);
    if (!pl.buf) {
        e = q.march(P, nslots);
        return VR_OK;
    }
    if (!q.cross_plane) return launch_plane_frame(desc, P, nslots, pl.buf, pl.sy, pl.sz, e);
    P.nb = 1;
    P.sy = pl.sy;
    P.sz = pl.sz;
    e = vr::launch_march_cross_plane(pl.buf, P, nslots, g.stream);
    return VR_OK;
}

// ---- frames under a user-defined transfer function ----

// What has no plane march under a custom table is refused, never rendered with the
// built-in one (a count too: early termination depends on the table).
int tf_refuse(const char *what) {
    return fail(VR_ERR_UNSUPPORTED, "%s: a custom transfer function renders baked planes only "
                                    "(bake the statistic first, or clear the table with "
                                    "%s)", what,
                g.tf2_nu ? "vr_set_transfer_function_2d(NULL, 0, 0, 0, 0, 0)"
                         : "vr_set_transfer_function(NULL, 0)");
}

// a 1-D or a 2-D table is set (at most one is)
bool tf_set() { return g.tf_n || g.tf2_nu; }

// The device copy of the table, made or refreshed for the frame about to use it.
// Frames already queued may still read the old copy: the stream that last read it
// drains first (the render stream; the device if the stream was changed since).
// The copy itself is ordered on the render stream, before the frame's launch.
int table_upload(float4 *&dev, bool &dirty, hipStream_t &last, const float *host, float *snap,
                 size_t bytes) {
    if (!dev) {
        VR_HIP(hipMalloc(&dev, bytes));
        dirty = true;
        last = g.stream;
    }
    if (dirty) {
        VR_HIP(last == g.stream ? hipStreamSynchronize(g.stream) : hipDeviceSynchronize());
        // (from a snapshot the setter never writes: the copy may still be in flight
        // when the table is set again; the drain above has finished the last one)
        std::memcpy(snap, host, bytes);
        last = g.stream;
        VR_HIP(hipMemcpyAsync(dev, snap, bytes, hipMemcpyHostToDevice, g.stream));
        dirty = false;
    }
    return VR_OK;
}

int tf_upload() {
    return table_upload(g.tf_dev, g.tf_dirty, g.tf_stream, g.tf, g.tf_up, sizeof g.tf);
}

// (the 2-D table's copy, a buffer of its own: section 23)
int tf2_upload() {
    return table_upload(g.tf2_dev, g.tf2_dirty, g.tf2_stream, g.tf2, g.tf2_up, sizeof g.tf2);
}

void release_tf_device() {
    if (g.tf_dev) (void)hipFree(g.tf_dev);
    g.tf_dev = nullptr;
    g.tf_dirty = false;
    if (g.tf2_dev) (void)hipFree(g.tf2_dev);
    g.tf2_dev = nullptr;
    g.tf2_dirty = false;
    if (g.rtf_dev) (void)hipFree(g.rtf_dev);
    g.rtf_dev = nullptr;
    g.rtf_dirty = false;
}

// A frame of P's grid from `plane` (one float per voxel in x-row bricks of pitches
// psy / psz) under the table: k_march_plane_tf on the bricks themselves, whatever
// the view -- no plan, no layout copy.  cross: the plane holds F (method 13).
int launch_tf_frame(vr::Params &P, uint32_t nslots, const float *plane, uint64_t psy, uint64_t psz,
                    bool cross) {
    const int rc = tf_upload();
    if (rc != VR_OK) return rc;
    P.nb = 1;
    P.sy = psy;
    P.sz = psz;
    const hipError_t e =
        vr::launch_march_plane_tf(plane, P, g.tf_dev, g.tf_n, cross, nslots, g.stream);
    if (e != hipSuccess) return hip_fail(e, "launch(k_march_plane_tf)");
    g.tf_stream = g.stream;
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

// vr_render's frame under the table: the resident baked plane of the method
// (statistics planes: methods 1/2/3, codec planes: 4/5/6, a record query's plane:
// 10-13), or a refusal
// The baked plane a table frame of method qm reads.  family: 0 the record volume's
// planes (1/2/3, 10-13), 1 the codec planes (4/5/6), -1 no plane march
struct TfPlane {
    const State::Planes *pl = nullptr;
    int k = 0, family = -1;
    bool cross = false;
    const float *ptr() const { return pl->buf + (uint64_t)k * pl->floats; }
};

TfPlane tf_plane(int qm) {
    TfPlane t;
    if (qm >= 1 && qm <= 3) {
        t.pl = &g.stats;
        t.k = qm - 1;
        t.family = 0;
    } else if (qm >= 4 && qm <= 6) {
        t.pl = &g.cstats;
        t.k = qm - 4;
        t.family = 1;
    } else if (const RecordQuery *q = record_query(qm)) {
        t.pl = &query_plane(qm);
        t.cross = q->cross_plane;
        t.family = 0;
    } else if (const int src = grad_source(qm)) {
        // the gradient plane of src, of src's family; |grad F| is blended, not combined
        t.pl = &g.grad[grad_slot(src)].p;
        t.family = src >= 4 && src <= 6 ? 1 : 0;
    }
    return t;
}

int render_tf_frame(const vr_render_desc *desc, vr::Params &P, uint32_t nslots, bool dry) {
    const TfPlane u = tf_plane(desc->query_method);
    if (!u.pl || !u.pl->buf) return tf_refuse("vr_render");
    if (dry) return VR_OK;
    return launch_tf_frame(P, nslots, u.ptr(), u.pl->sy, u.pl->sz, u.cross);
}

// ---- frames under a 2-D transfer function ----

// A frame of P's grid from the planes pu / pv of one volume (both in x-row bricks
// of pitches psy / psz) under the 2-D table: k_march_tf2 on the bricks themselves.
int launch_tf2_frame(vr::Params &P, uint32_t nslots, const float *pu, const float *pv, uint64_t psy,
                     uint64_t psz, bool cu, bool cv) {
    const int rc = tf2_upload();
    if (rc != VR_OK) return rc;
    P.nb = 1;
    P.sy = psy;
    P.sz = psz;
    const hipError_t e = vr::launch_march_tf2(pu, pv, P, g.tf2_dev, g.tf2_nu, g.tf2_nv, g.tf2_voff,
                                              g.tf2_vscale, cu, cv, nslots, g.stream);
    if (e != hipSuccess) return hip_fail(e, "launch(k_march_tf2)");
    g.tf2_stream = g.stream;
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

// vr_render's frame under the 2-D table: the planes of the frame's method (u) and
// of the table's second method (v), both resident and of one family, or a refusal
int render_tf2_frame(const vr_render_desc *desc, vr::Params &P, uint32_t nslots, bool dry) {
    const TfPlane u = tf_plane(desc->query_method), v = tf_plane(g.tf2_mv);
    if (!u.pl || !v.pl || u.family != v.family || !u.pl->buf || !v.pl->buf)
        return tf_refuse("vr_render");
    // (planes of one volume share one brick layout; anything else is a bug here)
    if (u.pl->floats != v.pl->floats || u.pl->sy != v.pl->sy || u.pl->sz != v.pl->sz)
        return fail(VR_ERR_STATE, "the planes of methods %d and %d differ in size or pitches",
                    desc->query_method, g.tf2_mv);
    if (dry) return VR_OK;
    return launch_tf2_frame(P, nslots, u.ptr(), v.ptr(), u.pl->sy, u.pl->sz, u.cross, v.cross);
}

// ---- ray projections of baked planes ----

// What has no plane march under a projection is refused, never composited.
int proj_refuse(const char *what) {
    static const char *const kName[] = {"", "maximum", "minimum", "mean"};
    if (g.tf2_nu)
        return fail(VR_ERR_UNSUPPORTED, "%s: the %s projection classifies one plane, and a 2-D "
                                        "transfer function is set (clear the table with "
                                        "vr_set_transfer_function_2d(NULL, 0, 0, 0, 0, 0), or the "
                                        "projection with vr_set_projection(0))", what,
                    kName[g.proj]);
    return fail(VR_ERR_UNSUPPORTED, "%s: the %s projection renders baked planes only (bake the "
                                    "statistic first, or clear the projection with "
                                    "vr_set_projection(0))", what, kName[g.proj]);
}

// the built-in nine entries (K:2323-2326; tf_entry, vr_device.h) as a table, for a
// projection with no caller's table: the kernel needs no second classifier
int rtf_upload() {
    static float rtf[4 * vr::kTfMax] = {0, 0, 0, 0, 1, 0, 0, 1, 1, 0.5f, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1,
                                        0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0};
    static float snap[4 * vr::kTfMax];
    return table_upload(g.rtf_dev, g.rtf_dirty, g.rtf_stream, rtf, snap, sizeof rtf);
}

// A frame of P's grid from `plane` (launch_tf_frame's arguments) under the
// projection: k_march_proj on the bricks themselves, whatever the view -- no plan,
// no layout copy -- classified through the caller's 1-D table or the built-in one.
int launch_proj_frame(vr::Params &P, uint32_t nslots, const float *plane, uint64_t psy,
                      uint64_t psz, bool cross) {
    const int rc = g.tf_n ? tf_upload() : rtf_upload();
    if (rc != VR_OK) return rc;
    P.nb = 1;
    P.sy = psy;
    P.sz = psz;
    const hipError_t e =
        vr::launch_march_proj(plane, P, g.tf_n ? g.tf_dev : g.rtf_dev, g.tf_n ? g.tf_n : 9, cross,
                              g.proj, nslots, g.stream);
    if (e != hipSuccess) return hip_fail(e, "launch(k_march_proj)");
    (g.tf_n ? g.tf_stream : g.rtf_stream) = g.stream;
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

// vr_render's frame under the projection: the plane a table frame reads (tf_plane)
int render_proj_frame(const vr_render_desc *desc, vr::Params &P, uint32_t nslots, bool dry) {
    if (g.tf2_nu) return proj_refuse("vr_render");
    const TfPlane u = tf_plane(desc->query_method);
    if (!u.pl || !u.pl->buf) return proj_refuse("vr_render");
    if (dry) return VR_OK;
    return launch_proj_frame(P, nslots, u.ptr(), u.pl->sy, u.pl->sz, u.cross);
}

// ---- headlight gradient shading of baked planes ----

// What has no lit plane march is refused, never rendered unlit.
int light_refuse(const char *what) {
    if (g.proj)
        return fail(VR_ERR_UNSUPPORTED, "%s: the light shades composited samples, and a "
                                        "projection classifies once per ray (clear the projection "
                                        "with vr_set_projection(0), or the light with "
                                        "vr_set_light(NULL))", what);
    if (g.tf2_nu)
        return fail(VR_ERR_UNSUPPORTED, "%s: the light shades one plane, and a 2-D transfer "
                                        "function is set (clear the table with "
                                        "vr_set_transfer_function_2d(NULL, 0, 0, 0, 0, 0), or the "
                                        "light with vr_set_light(NULL))", what);
    return fail(VR_ERR_UNSUPPORTED, "%s: the light shades frames of baked planes only (bake the "
                                    "statistic first, or clear the light with "
                                    "vr_set_light(NULL))", what);
}

// A frame of P's grid from `plane` (launch_tf_frame's arguments) under the light:
// k_march_lit on the bricks themselves, whatever the view -- no plan, no layout copy
// -- classified through the caller's 1-D table or the built-in one (rtf_upload).
int launch_lit_frame(vr::Params &P, uint32_t nslots, const float *plane, uint64_t psy, uint64_t psz,
                     bool cross) {
    const int rc = g.tf_n ? tf_upload() : rtf_upload();
    if (rc != VR_OK) return rc;
    P.nb = 1;
    P.sy = psy;
    P.sz = psz;
    const vr::Light L = {g.light.ambient, g.light.diffuse, g.light.specular,
                         g.light.shininess_log2};
    const hipError_t e =
        vr::launch_march_lit(plane, P, g.tf_n ? g.tf_dev : g.rtf_dev, g.tf_n ? g.tf_n : 9, L, cross,
                             nslots, g.stream);
    if (e != hipSuccess) return hip_fail(e, "launch(k_march_lit)");
    (g.tf_n ? g.tf_stream : g.rtf_stream) = g.stream;
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

// vr_render's frame under the light: the plane a table frame reads (tf_plane)
int render_lit_frame(const vr_render_desc *desc, vr::Params &P, uint32_t nslots, bool dry) {
    if (g.proj || g.tf2_nu) return light_refuse("vr_render");
    const TfPlane u = tf_plane(desc->query_method);
    if (!u.pl || !u.pl->buf) return light_refuse("vr_render");
    if (dry) return VR_OK;
    return launch_lit_frame(P, nslots, u.ptr(), u.pl->sy, u.pl->sz, u.cross);
}

// A gradient method has no per-step march, so nothing to count.
int grad_refuse(const char *what) {
    return fail(VR_ERR_UNSUPPORTED, "%s: a gradient method renders its baked plane only "
                                    "(vr_bake_gradient) and has no per-step march to count", what);
}

// One frame of vr_render / render_kernel; clip_w x clip_h is the top-left
// rectangle of pixels the launch covers (render_kernel's gridSize x blockSize,
// K:2397 + K:282-286; the whole image otherwise).
int render_frame(const vr_render_desc *desc, uint32_t clip_w, uint32_t clip_h) {
    vr::Params P;
    uint32_t nslots = 0;
    int rc = fill_params(desc, P, nslots, true);
    if (rc != VR_OK) return rc;
    P.CW = std::min(clip_w, P.W);
    P.CH = std::min(clip_h, P.H);
    if (P.CW < P.W || P.CH < P.H) {
        // the launch keeps the whole frame's tiles and order; pixels outside
        // the rectangle leave at once (miss-free: nothing written), and the
        // frame records no tile costs for the adaptive order
        if (desc->d_tile_list) return fail(VR_ERR_ARG, "a clipped render takes the whole frame");
        if (P.CW == 0 || P.CH == 0) return VR_OK;
        P.tile_cost = nullptr;
    }
    // VR_DRY (tooling: tools/host_cost.py): the host work of a frame (parameters
    // and the kernel choice) without its layout copies and its launch, to time
    // what a frame costs the issuing thread
    const char *ed = vr::tuning("VR_DRY");
    const bool dry = ed && std::atoi(ed) != 0;
    if (g.light_on) return render_lit_frame(desc, P, nslots, dry);
    if (g.proj) return render_proj_frame(desc, P, nslots, dry);
    if (g.tf_n) return render_tf_frame(desc, P, nslots, dry);
    if (g.tf2_nu) return render_tf2_frame(desc, P, nslots, dry);
    hipError_t e;
    const int qm = desc->query_method;
    if (is_flex_method(qm)) {
        if (dry) return VR_OK;
        e = vr::launch_march_flex(qm, P, nslots, g.stream);
    } else if (grad_source(qm)) {
        // a gradient plane (resident: check_method) under the built-in table, as a
        // record query's plane
        if (dry) return VR_OK;
        const TfPlane u = tf_plane(qm);
        rc = launch_plane_frame(desc, P, nslots, u.ptr(), u.pl->sy, u.pl->sz, e);
        if (rc != VR_OK) return rc;
    } else if (qm >= 4 && qm <= 6 && !g.cstats.buf) {
        if (dry) return VR_OK;
        // the one-lane codec march of a row-aligned view: a 16x4 pixel block per
        // wave (1024^3 x 8 1080p C0 m4 2.91 -> 2.88 ms, m5 5.26 -> 5.17, m6 7.07 ->
        // 6.90; profiles/r06/segmap/codec_*.log); VR_CODEC_MAP=0/1 overrides
        P.seg_map = std::fabs(desc->inv_view[0]) >= 0.95f;
        if (const char *em = vr::tuning("VR_CODEC_MAP")) P.seg_map = std::atoi(em) != 0;
        e = vr::launch_march_codec(P.nb, qm, P, nslots, false, g.stream);
        if (e == hipErrorInvalidValue)
            return fail(VR_ERR_UNSUPPORTED, "codec volumes with %d bins (compiled: 1,2,4,8,16,32)",
                        P.nb);
    } else if (const RecordQuery *q = record_query(qm)) {
        if (dry) return VR_OK;
        rc = launch_query(*q, desc, P, nslots, e);
        if (rc != VR_OK) return rc;
    } else {
        // records (fp32 / f16) and baked planes: vr_plan.cpp chooses the march
        if (qm == 7 && is_f16() && !g.stats.buf)
            return fail(VR_ERR_UNSUPPORTED, "method 7 on an f16 volume reads the baked corner "
                                            "means: basicDataProcessing / vr_bake_stats first");
        vr::PlanIn in = plan_input(desc, P, false);
        vr::MarchPlan pl = vr::plan_march(in);
        if (dry) return VR_OK;
        // the layout copy the plan marches; if it cannot be made (HBM), the plan
        // without it
        while (pl.layout != vr::kLayoutNone) {
            const bool made = pl.layout == vr::kLayoutAxis    ? ensure_axis_copy(pl.axis)
                              : pl.layout == vr::kLayoutBrick ? ensure_brick()
                                                              : ensure_plane_copy(qm - 1, pl.plane_axis);
            if (made) break;
            in.denied |= pl.layout;
            pl = vr::plan_march(in);
        }
        apply_plan(pl, P);
        const void *vol = g.vol;
        if (pl.method == -7) {  // the baked corner means (plane 3)
            vol = g.stats.buf + 3 * g.stats.floats;
            P.nb = 1;
            P.sy = g.stats.sy;
            P.sz = g.stats.sz;
        } else if (pl.method <= 0) {
            // the method's baked plane, addressed in its bricks, or its copy for the view
            P.nb = 1;
            if (pl.plane_axis) {
                const State::PlaneCopy &c = g.pcopy[pl.plane_axis - 1][qm - 1];
                vol = c.buf;
                P.sy = c.sy;
                P.sz = c.sz;
            } else if (qm <= 3) {
                vol = g.stats.buf + (uint64_t)(qm - 1) * g.stats.floats;
                P.sy = g.stats.sy;
                P.sz = g.stats.sz;
            } else {
                vol = g.cstats.buf + (uint64_t)(qm - 4) * g.cstats.floats;
                P.sy = g.cstats.sy;
                P.sz = g.cstats.sz;
            }
        } else if (pl.axis) {
            const State::AxisCopy &c = g.acopy[pl.axis - 1];
            P.avol = c.buf;
            P.asx = c.sx;
            P.asy = c.sy;
            P.asz = c.sz;
        } else if (pl.brick) {
            P.bvol = g.brick;
            P.bsy = g.bsy;
            P.bsz = g.bsz;
        }
        e = vr::launch_plan(pl, vol, P, nslots, g.stream);
    }
    if (e != hipSuccess) return hip_fail(e, "launch(k_march)");
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_render(const vr_render_desc *desc) { return render_frame(desc, UINT32_MAX, UINT32_MAX); }

int vr_debug_wave_clock(uint64_t *d_buf) {
    g.wave_clock = reinterpret_cast<unsigned long long *>(d_buf);
    return VR_OK;
}

// tooling: 6 x u64 device counters of the LDS-box marches (k_march /
// k_march_duo staged reads; layout in vr.h: [0] violations, [1] worst overrun,
// [2] out-of-volume box voxels, [3] decoded voxels, [4] lane slots, [5] spare),
// zeroed here on the library's stream and accumulated by every later launch;
// counted only by a -DVR_BOX_CHECK build, which reports whether it was built
// so (return 1) -- the default build returns 0
int vr_debug_box_check(uint64_t *d_buf) {
    if (d_buf) VR_HIP(hipMemsetAsync(d_buf, 0, 6 * sizeof(uint64_t), g.stream));
    g.box_check = reinterpret_cast<unsigned long long *>(d_buf);
#ifdef VR_BOX_CHECK
    return 1;
#else
    return 0;
#endif
}

int64_t vr_count_footprint(const vr_render_desc *desc) {
    if (g.light_on) return light_refuse("vr_count_footprint");
    if (g.proj) return proj_refuse("vr_count_footprint");
    if (tf_set()) return tf_refuse("vr_count_footprint");
    if (desc && grad_source(desc->query_method)) return grad_refuse("vr_count_footprint");
    if (desc && record_query(desc->query_method))  // no counting instance of their marches
        return fail(VR_ERR_UNSUPPORTED, "footprint count is defined for methods 1/2/3");
    vr::Params P;
    uint32_t nslots = 0;
    int rc = fill_params(desc, P, nslots);
    if (rc != VR_OK) return rc;
    if (desc->query_method < 1 || desc->query_method > 3)
        return fail(VR_ERR_UNSUPPORTED, "footprint count is defined for methods 1/2/3");
    const uint64_t nvox = (uint64_t)g.nx * g.ny * g.nz;
    const uint64_t nwords = (nvox + 63) / 64;
    unsigned long long *bits = nullptr, *total = nullptr;
    VR_HIP(hipMalloc(&bits, nwords * 8 + 8));
    total = bits + nwords;
    hipError_t e = hipMemsetAsync(bits, 0, nwords * 8 + 8, g.stream);
    P.mark = bits;
    if (e == hipSuccess) {  // the counting instance of the LDS-box march (f16: of the one-lane march)
        const vr::MarchPlan pl = vr::plan_march(plan_input(desc, P, true));
        apply_plan(pl, P);
        e = vr::launch_plan(pl, g.vol, P, nslots, g.stream);
    }
    if (e == hipSuccess) e = vr::launch_popcount(bits, nwords, total, g.stream);
    unsigned long long u = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&u, total, 8, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    (void)hipFree(bits);
    if (e != hipSuccess) return hip_fail(e, "vr_count_footprint");
    return (int64_t)u;
}

int64_t vr_footprint_bytes(const vr_render_desc *desc) {
    if (g.light_on) return light_refuse("vr_footprint_bytes");
    if (g.proj) return proj_refuse("vr_footprint_bytes");
    if (tf_set()) return tf_refuse("vr_footprint_bytes");
    if (desc && grad_source(desc->query_method)) return grad_refuse("vr_footprint_bytes");
    if (desc && record_query(desc->query_method))
        return fail(VR_ERR_UNSUPPORTED, "footprint bytes are defined for methods 1-6");
    vr::Params P;
    uint32_t nslots = 0;
    int rc = fill_params(desc, P, nslots);
    if (rc != VR_OK) return rc;
    const int m = desc->query_method;
    if (m == 7 || m < 1 || m > 6)
        return fail(VR_ERR_UNSUPPORTED, "footprint bytes are defined for methods 1-6");
    if (m <= 3) {
        const int64_t u = vr_count_footprint(desc);
        return u < 0 ? u : u * (int64_t)g.nb * (int64_t)elem_bytes();
    }
    const uint64_t nvox = (uint64_t)P.nx * P.ny * P.nz;
    const uint64_t nwords = (nvox + 63) / 64;
    unsigned long long *bits = nullptr;
    VR_HIP(hipMalloc(&bits, nwords * 8 + 8));
    unsigned long long *total = bits + nwords;
    hipError_t e = hipMemsetAsync(bits, 0, nwords * 8 + 8, g.stream);
    P.mark = bits;
    if (e == hipSuccess) e = vr::launch_march_codec(P.nb, m, P, nslots, true, g.stream);
    if (e == hipSuccess) e = vr::launch_codec_bytes(bits, nvox, g.cb, total, g.stream);
    unsigned long long b = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&b, total, 8, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    (void)hipFree(bits);
    if (e != hipSuccess) return hip_fail(e, "vr_footprint_bytes");
    return (int64_t)b + (int64_t)g.ntpl * g.cnb * 4;  // + the template table, read once
}

int vr_unscatter_tiles(const uint32_t *d_packed, const uint32_t *d_tile_lists, uint32_t n_ranks,
                       uint32_t n_slots, uint32_t *d_frame, uint32_t width, uint32_t height) {
    if (!d_packed || !d_tile_lists || !d_frame) return fail(VR_ERR_ARG, "null pointer");
    const uint64_t n = (uint64_t)n_ranks * n_slots;
    if (n > 0x7FFFFFFFull) return fail(VR_ERR_ARG, "too many tiles");
    hipError_t e = vr::launch_unscatter(d_packed, d_tile_lists, (uint32_t)n, tiles_x(width),
                                        d_frame, width, height, g.stream);
    if (e != hipSuccess) return hip_fail(e, "launch(k_unscatter)");
    return VR_OK;
}

// ---------------- GMM volumes (config 5) ----------

}  // extern "C"

namespace {

void release_gmm_volume(State::Gmm &v) {
    if (v.owned) {
        if (v.wm) (void)hipFree(v.wm);
        if (v.sg) (void)hipFree(v.sg);
    }
    v = State::Gmm{};
}

// the selected slot's GMM volume
void release_gmm() {
    g.volume_epoch++;
    release_gmm_volume(g.gmm);
}

// both slots' (freeCudaBuffers)
void release_all_gmm() {
    release_gmm();
    release_gmm_volume(g.gmm_parked[0]);
    release_gmm_volume(g.gmm_parked[1]);
    g.gmm_slot = 0;
}

// Frees a baked set of GMM planes: vr_release_gmm_*; the range plane on any change
// of the range, the quantile plane on any set or clear of the quantile;
// freeCudaBuffers: all
int release_gmm_set(int set) {
    State::GmmStats &b = g.gplanes[set];
    if (b.buf) {
        (void)hipFree(b.buf);
        g.volume_epoch++;  // a tile order learned on these planes is not reused
    }
    b = State::GmmStats{};
    return VR_OK;
}

int check_gmm_shape(vr_extent dims, int K, int z_base, int nzs) {
    if (K != 8 && K != 16 && K != 32)
        return fail(VR_ERR_UNSUPPORTED, "GMM volumes with %d components (compiled: 8, 16, 32)", K);
    if (dims.width == 0 || dims.height == 0 || dims.depth == 0 || dims.width > 65536 ||
        dims.height > 65536 || dims.depth > 65536)
        return fail(VR_ERR_ARG, "GMM volume: bad dims");
    // a slice must stay below 2^31 voxels: the march offsets corners by 32-bit slice strides
    if ((uint64_t)dims.width * dims.height >= (1ull << 31))
        return fail(VR_ERR_ARG, "GMM volume: a slice of %zu x %zu voxels is too large", dims.width,
                    dims.height);
    if (z_base < 0 || nzs < 1 || (size_t)z_base + (size_t)nzs > dims.depth)
        return fail(VR_ERR_ARG, "GMM volume: resident slices [%d, %d) outside [0, %zu)", z_base,
                    z_base + nzs, dims.depth);
    return VR_OK;
}

bool gmm_f16() { return g.gmm.dtype == VR_DTYPE_F16; }

// The statistics of a GMM volume: the plane sets g.gplanes and the queryMethods
// that read them (vr_gmm.hip holds the kernels, one march and one bake body for
// all).  What differs between them on the host, one row each, in the order of
// State::kGmmStats ...; everything else -- the checks, the planes' life, the frame
// launches -- is written once below.
struct GmmPlaneSet {
    uint64_t nplanes;
    const char *planes;           // the set, in messages
    const char *bake, *release;   // its entry points and its bake kernel, in messages
    const char *bake_kernel;
    // the host state a bake or a per-step frame needs set (nullptr: none), and what
    // sets it, in messages.  (Not a `[] { ... }`: the compiler gives the n-th lambda
    // of one signature in each table of this file one name, and so one body.)
    bool (*ready)(const State &s);
    const char *state, *setters;
    // the per-step march and the bake of the selected slot's resident slices
    hipError_t (*march)(int method, const vr::Params &P, uint32_t nblocks);
    hipError_t (*bake_launch)(float *out, uint64_t plane, uint64_t psy, uint64_t psz);
};

const GmmPlaneSet kGmmPlaneSets[State::kGmmSets] = {
    {2, "planes", "vr_bake_gmm_stats", "vr_release_gmm_stats", "launch(k_bake_gmm)", nullptr,
     nullptr, nullptr,
     [](int method, const vr::Params &P, uint32_t nblocks) {
         return vr::launch_march_gmm(g.gmm.K, method, gmm_f16(), P, nblocks, false, g.stream);
     },
     [](float *out, uint64_t plane, uint64_t psy, uint64_t psz) {
         const State::Gmm &v = g.gmm;
         return vr::launch_bake_gmm(v.wm, v.sg, gmm_f16(), v.K, v.nx, v.ny, v.z_base, v.nzs, out,
                                    plane, psy, psz, g.stream);
     }},
    {1, "range plane", "vr_bake_gmm_range", "vr_release_gmm_range", "launch(k_bake_gmm_range)",
     [](const State &s) { return s.grq_set; }, "range", "vr_set_gmm_range",
     [](int, const vr::Params &P, uint32_t nblocks) {
         return vr::launch_march_gmm_range(g.gmm.K, gmm_f16(), P, g.grq, nblocks, g.stream);
     },
     [](float *out, uint64_t, uint64_t psy, uint64_t psz) {
         const State::Gmm &v = g.gmm;
         return vr::launch_bake_gmm_range(v.wm, v.sg, gmm_f16(), v.K, v.nx, v.ny, v.z_base, v.nzs,
                                          g.grq, out, psy, psz, g.stream);
     }},
    {1, "quantile plane", "vr_bake_gmm_quantile", "vr_release_gmm_quantile",
     "launch(k_bake_gmm_quant)", [](const State &s) { return s.qmode != 0; }, "quantile",
     "vr_set_quantile / vr_set_quantile_spread",
     [](int, const vr::Params &P, uint32_t nblocks) {
         return vr::launch_march_gmm_quant(g.gmm.K, gmm_f16(), P, g.qq, g.qmode == 2, nblocks,
                                           g.stream);
     },
     [](float *out, uint64_t, uint64_t psy, uint64_t psz) {
         const State::Gmm &v = g.gmm;
         return vr::launch_bake_gmm_quant(v.wm, v.sg, gmm_f16(), v.K, v.nx, v.ny, v.z_base, v.nzs,
                                          g.qq, g.qmode == 2, out, psy, psz, g.stream);
     }},
};

// the set queryMethod m reads; -1: none.  (Method 13 has no per-step GMM march: it
// reads the range plane, as the plane of F = P(v < theta), in vr_render_gmm_baked.)
int gmm_plane_set(int m) {
    switch (m) {
    case 1:
    case 2: return State::kGmmStats;
    case VR_QUERY_WEIGHTED:
    case VR_QUERY_CROSSING: return State::kGmmRange;
    case VR_QUERY_QUANTILE: return State::kGmmQuant;
    default: return -1;
    }
}

// Parameters of a GMM launch: the reference's ray / transfer / composite
// inputs from the descriptor, the resident slices, and the slab.
// count: a footprint count (no instance of the range probability or the quantile
// is built)
int fill_gmm_params(const vr_render_desc *d, const vr_gmm_slab *slab, vr::Params &P,
                    uint32_t &nblocks, bool count) {
    if (!d) return fail(VR_ERR_ARG, "null render descriptor");
    if (!g.gmm.wm) return fail(VR_ERR_STATE, "no GMM volume resident (vr_init_gmm / vr_synthesize_gmm)");
    const int set = d->query_method == VR_QUERY_CROSSING ? -1 : gmm_plane_set(d->query_method);
    if (set < 0 || (count && set != State::kGmmStats))
        return fail(VR_ERR_UNSUPPORTED, count
                    ? "GMM footprint counts support queryMethod 1 (mean) and 2 (variance)"
                    : "GMM volumes support queryMethod 1 (mean), 2 (variance), 10 (range "
                      "probability) and 11 (quantile)");
    const GmmPlaneSet &ps = kGmmPlaneSets[set];
    if (ps.ready && !ps.ready(g))
        return fail(VR_ERR_STATE, "queryMethod %d on a GMM volume needs a %s (%s)",
                    d->query_method, ps.state, ps.setters);
    if (!d->d_output) return fail(VR_ERR_ARG, "d_output is null");
    if (d->width == 0 || d->height == 0) return fail(VR_ERR_ARG, "empty image");
    if ((uint64_t)d->width * d->height > 0xFFFFFFFFull) return fail(VR_ERR_ARG, "image too large");
    if (d->d_tile_list) return fail(VR_ERR_UNSUPPORTED, "GMM renders take whole frames or alive lists");
    std::memset(&P, 0, sizeof P);
    std::memcpy(P.m, d->inv_view, sizeof P.m);
    P.W = d->width;
    P.H = d->height;
    P.CW = d->width;
    P.CH = d->height;
    P.density = d->density;
    P.brightness = d->brightness;
    P.toff = d->transfer_offset;
    P.tscale = d->transfer_scale;
    P.nx = g.gmm.nx; P.ny = g.gmm.ny; P.nz = g.gmm.nz;
    P.gwm = g.gmm.wm;
    P.gsg = g.gmm.sg;
    P.gk = g.gmm.K;
    P.z_base = g.gmm.z_base;
    P.nzs = g.gmm.nzs;
    P.tiles_x = tiles_x(d->width);
    P.out = d->d_output;
    P.out_f = d->d_output_f;
    P.out_n = d->d_steps;
    device_lds(P.lds_cu, P.lds_wg);
    if (const char *e = vr::tuning("VR_WG_PER_CU")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 32) P.wg_per_cu = v;
    }
    // lockstep batches (path 1, default): a wave's rays stay adjacent and at the
    // same step, so their corner loads share lines (1024^3 x 16, 1080p: C0
    // 4.89 -> 4.20 ms, C1 7.88 -> 7.38); VR_GMM_LOCKSTEP=0 refills groups one by one
    P.path = 1;
    if (const char *e = vr::tuning("VR_GMM_LOCKSTEP")) P.path = std::atoi(e) ? 1 : 0;
    const int zr_hi = g.gmm.z_base + g.gmm.nzs;  // resident slices end (exclusive)
    if (!slab) {
        if (g.gmm.z_base != 0 || g.gmm.nzs != g.gmm.nz)
            return fail(VR_ERR_STATE, "only slices [%d, %d) of the GMM volume are resident: "
                        "render it slab by slab (vr_render_gmm with a vr_gmm_slab)",
                        g.gmm.z_base, zr_hi);
        P.z_lo = 0;
        P.z_hi = g.gmm.nz;
    } else {
        if (slab->z_lo < 0 || slab->z_hi > g.gmm.nz || slab->z_lo >= slab->z_hi)
            return fail(VR_ERR_ARG, "slab [%d, %d) outside the volume's [0, %d)", slab->z_lo,
                        slab->z_hi, g.gmm.nz);
        // a footprint with z0 in [z_lo, z_hi) reads slices z0 and min(z0 + 1, nz - 1)
        const int need_hi = std::min(slab->z_hi + 1, g.gmm.nz);
        if (slab->z_lo < g.gmm.z_base || need_hi > zr_hi)
            return fail(VR_ERR_ARG, "slab [%d, %d) needs slices [%d, %d); resident: [%d, %d)",
                        slab->z_lo, slab->z_hi, slab->z_lo, need_hi, g.gmm.z_base, zr_hi);
        if (!slab->d_rays_out || !slab->d_n_rays_out)
            return fail(VR_ERR_ARG, "a slab launch needs d_rays_out and d_n_rays_out");
        if (slab->n_rays_in && !slab->d_rays_in) return fail(VR_ERR_ARG, "d_rays_in is null");
        if ((uint64_t)slab->n_rays_in > (uint64_t)d->width * d->height)
            return fail(VR_ERR_ARG, "%u alive rays in for a %ux%u frame", slab->n_rays_in,
                        d->width, d->height);
        // an alive-list entry holds the pixel in 23 bits (vr_gmm.hip GmmRay)
        if ((uint64_t)d->width * d->height > (1ull << 23))
            return fail(VR_ERR_ARG, "slab chains address at most 2^23 pixels (%ux%u)",
                        d->width, d->height);
        // slabs must be taken in the order every ray crosses them: the sign of
        // a ray's z step is that of the linear form u M8 + v M9 - 2 M10, so the
        // four frame corners decide whether it is the same for the whole frame
        const float *M = d->inv_view;
        int pos = 0, neg = 0;
        for (int c = 0; c < 4; c++) {
            const float u = (c & 1) ? ((float)(d->width - 1) / (float)d->width) * 2.0f - 1.0f : -1.0f;
            const float v = (c & 2) ? ((float)(d->height - 1) / (float)d->height) * 2.0f - 1.0f : -1.0f;
            const float dz = u * M[8] + v * M[9] - 2.0f * M[10];
            pos += dz > 0.0f;
            neg += dz < 0.0f;
        }
        if (pos && neg)
            return fail(VR_ERR_UNSUPPORTED, "rays of this view cross z-slabs in both directions: "
                        "slab-chained rendering needs one crossing order");
        P.z_lo = slab->z_lo;
        P.z_hi = slab->z_hi;
        P.rays_in = reinterpret_cast<const uint32_t *>(slab->d_rays_in);
        P.n_rays_in = slab->d_rays_in ? slab->n_rays_in : 0;
        P.rays_out = reinterpret_cast<uint32_t *>(slab->d_rays_out);
        P.n_rays_out = slab->d_n_rays_out;
    }
    if (P.rays_in || (slab && slab->d_rays_in)) {
        nblocks = (uint32_t)(((uint64_t)P.n_rays_in + 255) / 256);
        P.n_tiles = nblocks;
    } else {
        nblocks = tiles_x(d->width) * tiles_y(d->height);
        P.n_tiles = nblocks;
        int rc = frame_order(d, tiles_x(d->width), tiles_y(d->height), P.perm, nullptr);
        if (rc != VR_OK) return rc;
    }
    return VR_OK;
}

// the widest loads k_march_gmm_h makes of a lane's chunk (vr_gmm.hip gmm_gather)
constexpr size_t kGmmHalfAlignWm = 16, kGmmHalfAlignSigma = 8;

// vr_init_gmm / vr_init_gmm_f16: elements of `elem` bytes
int init_gmm_planes(const void *wm, const void *sigma, vr_extent dims, int ncomp, int z_base,
                    int nslices, int where, int dtype) {
    const char *fn = dtype == VR_DTYPE_F16 ? "vr_init_gmm_f16" : "vr_init_gmm";
    const size_t elem = dtype == VR_DTYPE_F16 ? 2 : sizeof(float);
    int rc = check_gmm_shape(dims, ncomp, z_base, nslices);
    if (rc != VR_OK) return rc;
    if (!wm || !sigma) return fail(VR_ERR_ARG, "%s: null plane", fn);
    if (where < 0 || where > 2) return fail(VR_ERR_ARG, "%s: where must be 0, 1 or 2", fn);
    if (dtype == VR_DTYPE_F16 && where == 2 &&
        ((reinterpret_cast<uintptr_t>(wm) & (kGmmHalfAlignWm - 1)) ||
         (reinterpret_cast<uintptr_t>(sigma) & (kGmmHalfAlignSigma - 1))))
        return fail(VR_ERR_ARG, "an adopted f16 GMM volume must be aligned to %zu (wm) and %zu "
                    "(sigma) bytes", kGmmHalfAlignWm, kGmmHalfAlignSigma);
    const uint64_t nvox = (uint64_t)dims.width * dims.height * (uint64_t)nslices;
    const size_t bwm = nvox * (size_t)ncomp * 2 * elem, bsg = nvox * (size_t)ncomp * elem;
    release_gmm();
    State::Gmm m;
    m.nx = (int)dims.width; m.ny = (int)dims.height; m.nz = (int)dims.depth;
    m.K = ncomp; m.z_base = z_base; m.nzs = nslices;
    m.dtype = dtype;
    if (where == 2) {
        m.wm = static_cast<float *>(const_cast<void *>(wm));
        m.sg = static_cast<float *>(const_cast<void *>(sigma));
        m.owned = false;
    } else {
        hipError_t e = hipMalloc(&m.wm, bwm);
        if (e == hipSuccess) e = hipMalloc(&m.sg, bsg);
        const hipMemcpyKind k = where == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        if (e == hipSuccess) e = hipMemcpy(m.wm, wm, bwm, k);
        if (e == hipSuccess) e = hipMemcpy(m.sg, sigma, bsg, k);
        if (e != hipSuccess) {
            if (m.wm) (void)hipFree(m.wm);
            if (m.sg) (void)hipFree(m.sg);
            return hip_fail(e, fn);
        }
        m.owned = true;
    }
    g.gmm = m;
    return VR_OK;
}

int synthesize_gmm(vr_extent dims, int ncomp, uint64_t seed, int z_base, int nslices, int dtype) {
    const char *fn = dtype == VR_DTYPE_F16 ? "vr_synthesize_gmm_f16" : "vr_synthesize_gmm";
    const size_t elem = dtype == VR_DTYPE_F16 ? 2 : sizeof(float);
    int rc = check_gmm_shape(dims, ncomp, z_base, nslices);
    if (rc != VR_OK) return rc;
    const int nx = (int)dims.width, ny = (int)dims.height, nz = (int)dims.depth;
    const uint64_t nvox = (uint64_t)nx * ny * (uint64_t)nslices;
    vr::SynthArgs a{};
    std::vector<float> gx, gy, gz;
    blob_tables(nx, ny, nz, seed, a, gx, gy, gz);
    release_gmm();
    State::Gmm m;
    float *dgx = nullptr, *dgy = nullptr, *dgz = nullptr;
    hipError_t e = hipMalloc(&m.wm, nvox * (size_t)ncomp * 2 * elem);
    if (e == hipSuccess) e = hipMalloc(&m.sg, nvox * (size_t)ncomp * elem);
    if (e == hipSuccess) e = hipMalloc(&dgx, gx.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgy, gy.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&dgz, gz.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(dgx, gx.data(), gx.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgy, gy.data(), gy.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dgz, gz.data(), gz.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        a.gx = dgx; a.gy = dgy; a.gz = dgz;
        a.nx = nx; a.ny = ny; a.nz = nz; a.nb = ncomp; a.seed = seed;
        e = vr::launch_synth_gmm(m.wm, m.sg, dtype == VR_DTYPE_F16, a, ncomp, z_base, nslices,
                                 g.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (dgx) (void)hipFree(dgx);
    if (dgy) (void)hipFree(dgy);
    if (dgz) (void)hipFree(dgz);
    if (e != hipSuccess) {
        if (m.wm) (void)hipFree(m.wm);
        if (m.sg) (void)hipFree(m.sg);
        return hip_fail(e, fn);
    }
    m.nx = nx; m.ny = ny; m.nz = nz; m.K = ncomp; m.z_base = z_base; m.nzs = nslices;
    m.owned = true;
    m.dtype = dtype;
    g.gmm = m;
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_init_gmm(const float *wm, const float *sigma, vr_extent dims, int ncomp, int z_base,
                int nslices, int where) {
    return init_gmm_planes(wm, sigma, dims, ncomp, z_base, nslices, where, VR_DTYPE_F32);
}

int vr_init_gmm_f16(const void *wm, const void *sigma, vr_extent dims, int ncomp, int z_base,
                    int nslices, int where) {
    return init_gmm_planes(wm, sigma, dims, ncomp, z_base, nslices, where, VR_DTYPE_F16);
}

int vr_synthesize_gmm(vr_extent dims, int ncomp, uint64_t seed, int z_base, int nslices) {
    return synthesize_gmm(dims, ncomp, seed, z_base, nslices, VR_DTYPE_F32);
}

int vr_synthesize_gmm_f16(vr_extent dims, int ncomp, uint64_t seed, int z_base, int nslices) {
    return synthesize_gmm(dims, ncomp, seed, z_base, nslices, VR_DTYPE_F16);
}

// The selected slot's fp32 planes narrowed to f16 on the device (k_narrow_f16)
// into new library-owned buffers; the fp32 planes go only once both new ones
// are complete, so a failure leaves the volume as it was.
int vr_convert_gmm_f16(void) {
    if (!g.gmm.wm) return fail(VR_ERR_STATE, "no GMM volume resident");
    if (gmm_f16()) return fail(VR_ERR_STATE, "the resident GMM volume is f16 already");
    const uint64_t n = (uint64_t)g.gmm.nx * g.gmm.ny * (uint64_t)g.gmm.nzs * (uint64_t)g.gmm.K;
    void *hwm = nullptr, *hsg = nullptr;
    hipError_t e = hipMalloc(&hwm, n * 4);
    if (e == hipSuccess) e = hipMalloc(&hsg, n * 2);
    if (e == hipSuccess) e = vr::launch_narrow_f16(g.gmm.wm, hwm, n * 2, g.stream);
    if (e == hipSuccess) e = vr::launch_narrow_f16(g.gmm.sg, hsg, n, g.stream);
    // synchronous, like vr_convert_f16: a later frame may run on another stream
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) {
        if (hwm) (void)hipFree(hwm);
        if (hsg) (void)hipFree(hsg);
        return hip_fail(e, "vr_convert_gmm_f16(k_narrow_f16)");
    }
    g.volume_epoch++;  // the records changed: an order learned on them is not reused
    if (g.gmm.owned) {
        (void)hipFree(g.gmm.wm);
        (void)hipFree(g.gmm.sg);
    }
    g.gmm.wm = static_cast<float *>(hwm);
    g.gmm.sg = static_cast<float *>(hsg);
    g.gmm.owned = true;
    g.gmm.dtype = VR_DTYPE_F16;
    return VR_OK;
}

int vr_gmm_dtype(void) {
    if (!g.gmm.wm) return fail(VR_ERR_STATE, "no GMM volume resident");
    return g.gmm.dtype;
}

int vr_gmm_info(vr_extent *dims, int *ncomp, int *z_base, int *nslices, const float **d_wm,
                const float **d_sigma) {
    if (!g.gmm.wm) return fail(VR_ERR_STATE, "no GMM volume resident");
    if (dims) {
        dims->width = (size_t)g.gmm.nx;
        dims->height = (size_t)g.gmm.ny;
        dims->depth = (size_t)g.gmm.nz;
    }
    if (ncomp) *ncomp = g.gmm.K;
    if (z_base) *z_base = g.gmm.z_base;
    if (nslices) *nslices = g.gmm.nzs;
    if (d_wm) *d_wm = g.gmm.wm;
    if (d_sigma) *d_sigma = g.gmm.sg;
    return VR_OK;
}

int vr_gmm_select(int slot) {
    if (slot != 0 && slot != 1) return fail(VR_ERR_ARG, "GMM slot %d (0 or 1)", slot);
    if (slot == g.gmm_slot) return VR_OK;
    g.gmm_parked[g.gmm_slot] = g.gmm;
    g.gmm = g.gmm_parked[slot];
    g.gmm_parked[slot] = State::Gmm{};
    g.gmm_slot = slot;
    g.volume_epoch++;  // (the tile order is keyed on what is resident)
    return VR_OK;
}

int vr_free_gmm(void) {
    release_gmm();
    return VR_OK;
}

int vr_render_gmm(const vr_render_desc *desc, const vr_gmm_slab *slab) {
    if (g.light_on) return light_refuse("vr_render_gmm");
    if (g.proj) return proj_refuse("vr_render_gmm");
    if (tf_set()) return tf_refuse("vr_render_gmm");
    vr::Params P;
    uint32_t nblocks = 0;
    int rc = fill_gmm_params(desc, slab, P, nblocks, false);
    if (rc != VR_OK) return rc;
    // the alive-list counter starts from 0 on the stream the launch runs on
    // (a caller zeroing it on another stream raced the launch)
    hipError_t e = slab ? hipMemsetAsync(slab->d_n_rays_out, 0, sizeof(uint32_t), g.stream)
                        : hipSuccess;
    if (e == hipSuccess)
        e = kGmmPlaneSets[gmm_plane_set(desc->query_method)].march(desc->query_method, P, nblocks);
    if (e != hipSuccess) return hip_fail(e, gmm_f16() ? "launch(k_march_gmm_h)" : "launch(k_march_gmm)");
    return VR_OK;
}

int64_t vr_gmm_count_footprint(const vr_render_desc *desc) {
    return vr_gmm_count_footprint_slab(desc, nullptr);
}

int64_t vr_gmm_count_footprint_slab(const vr_render_desc *desc, const vr_gmm_slab *slab) {
    if (g.light_on) return light_refuse("vr_gmm_count_footprint");
    if (g.proj) return proj_refuse("vr_gmm_count_footprint");
    if (tf_set()) return tf_refuse("vr_gmm_count_footprint");
    vr::Params P;
    uint32_t nblocks = 0;
    int rc = fill_gmm_params(desc, slab, P, nblocks, true);
    if (rc != VR_OK) return rc;
    // one bit per resident voxel (gmm_vox indexes the resident slices)
    const uint64_t nvox = (uint64_t)g.gmm.nx * g.gmm.ny * (uint64_t)g.gmm.nzs;
    const uint64_t nwords = (nvox + 63) / 64;
    unsigned long long *bits = nullptr;
    VR_HIP(hipMalloc(&bits, nwords * 8 + 8));
    unsigned long long *total = bits + nwords;
    hipError_t e = hipMemsetAsync(bits, 0, nwords * 8 + 8, g.stream);
    if (e == hipSuccess && slab)
        e = hipMemsetAsync(slab->d_n_rays_out, 0, sizeof(uint32_t), g.stream);
    P.mark = bits;
    P.out = nullptr;  // count launch writes no pixels
    P.out_f = nullptr;
    P.out_n = nullptr;
    if (e == hipSuccess) e = vr::launch_march_gmm(g.gmm.K, desc->query_method, gmm_f16(), P, nblocks, true, g.stream);
    if (e == hipSuccess) e = vr::launch_popcount(bits, nwords, total, g.stream);
    unsigned long long u = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&u, total, 8, hipMemcpyDeviceToHost, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    (void)hipFree(bits);
    if (e != hipSuccess) return hip_fail(e, "vr_gmm_count_footprint");
    return (int64_t)u;
}

}  // extern "C"

namespace {

// vr_bake_gmm_*: the selected slot's resident slices decoded once per voxel into the
// set's whole-volume planes (its bake kernel, queued on the library stream).  The
// first call allocates and zeroes the planes; if it fails, nothing has changed.
int bake_gmm_planes(int set) {
    const GmmPlaneSet &ps = kGmmPlaneSets[set];
    State::GmmStats &b = g.gplanes[set];
    const State::Gmm &v = g.gmm;
    if (!v.wm) return fail(VR_ERR_STATE, "no GMM volume resident (vr_init_gmm / vr_synthesize_gmm)");
    if (ps.ready && !ps.ready(g)) return fail(VR_ERR_STATE, "no %s set (%s)", ps.state, ps.setters);
    if (b.buf && (b.nx != v.nx || b.ny != v.ny || b.nz != v.nz))
        return fail(VR_ERR_STATE, "the GMM planes hold a %d x %d x %d volume, the resident records "
                    "are of %d x %d x %d: %s first", b.nx, b.ny, b.nz, v.nx, v.ny, v.nz, ps.release);
    if (v.nx > 65535 || v.ny > 65535 || v.nzs > 65535)
        return fail(VR_ERR_UNSUPPORTED, "baking GMM volumes beyond 65535 voxels per axis");
    uint64_t psy = b.sy, psz = b.sz, plane = b.plane;
    float *buf = b.buf;
    if (!buf) {
        vr::plane_pitches((uint32_t)v.nx, (uint32_t)v.ny, psy, psz);
        plane = psz * (uint64_t)v.nz;
        VR_HIP(hipMalloc(&buf, (ps.nplanes * plane + 4) * sizeof(float)));
        // (the planes' padding is read with weight 0: it must hold finite floats)
        const hipError_t e = hipMemsetAsync(buf, 0, (ps.nplanes * plane + 4) * sizeof(float), g.stream);
        if (e != hipSuccess) {
            (void)hipFree(buf);
            return hip_fail(e, ps.bake);
        }
    }
    const hipError_t e = ps.bake_launch(buf, plane, psy, psz);
    if (e != hipSuccess) {
        if (!b.buf) {  // the planes this call allocated, once their memset has run
            (void)hipStreamSynchronize(g.stream);
            (void)hipFree(buf);
        }
        return hip_fail(e, ps.bake_kernel);
    }
    if (!b.buf) {
        b.buf = buf;
        b.nx = v.nx; b.ny = v.ny; b.nz = v.nz;
        b.plane = plane;
        b.sy = psy;
        b.sz = psz;
        b.slice.assign((size_t)v.nz, 0);
        b.nbaked = 0;
        g.volume_epoch++;
    }
    for (int z = v.z_base; z < v.z_base + v.nzs; z++) {
        b.nbaked += !b.slice[(size_t)z];
        b.slice[(size_t)z] = 1;
    }
    return VR_OK;
}

// vr_gmm_*_info of a set
int gmm_planes_info(int set, vr_extent *dims, const float **d_planes, uint64_t *plane_floats,
                    int *slices_baked) {
    const State::GmmStats &b = g.gplanes[set];
    if (dims) {
        dims->width = (size_t)b.nx;
        dims->height = (size_t)b.ny;
        dims->depth = (size_t)b.nz;
    }
    if (d_planes) *d_planes = b.buf;
    if (plane_floats) *plane_floats = b.plane;
    if (slices_baked) *slices_baked = b.nbaked;
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_bake_gmm_stats(void) { return bake_gmm_planes(State::kGmmStats); }

// ---- range probability of GMM volumes ----
// host state only: no HIP call (the plane a set or clear drops is freed, if any)
int vr_set_gmm_range(float lo, float hi) {
    if (lo != lo || hi != hi || lo > hi)
        return fail(VR_ERR_ARG, "vr_set_gmm_range: bounds [%g, %g) (NaN or lo > hi)", (double)lo,
                    (double)hi);
    release_gmm_set(State::kGmmRange);
    g.grq = vr::GmmRange{lo, hi};
    g.grq_set = true;
    return VR_OK;
}

int vr_clear_gmm_range(void) {
    release_gmm_set(State::kGmmRange);
    g.grq = vr::GmmRange{};
    g.grq_set = false;
    return VR_OK;
}

int vr_gmm_range(float *lo, float *hi) {
    if (!g.grq_set) return fail(VR_ERR_STATE, "no range set (vr_set_gmm_range)");
    if (lo) *lo = g.grq.lo;
    if (hi) *hi = g.grq.hi;
    return VR_OK;
}

int vr_gmm_phi_table(const float **c, int *nseg, float *h, float *zmax) {
    if (c) *c = vr::gmm_phi_table_host();
    if (nseg) *nseg = vr::kPhiSeg;
    if (h) *h = vr::kPhiH;
    if (zmax) *zmax = vr::kPhiZMax;
    return VR_OK;
}

int vr_bake_gmm_range(void) { return bake_gmm_planes(State::kGmmRange); }

int vr_release_gmm_range(void) { return release_gmm_set(State::kGmmRange); }

int vr_gmm_range_info(vr_extent *dims, const float **d_plane, uint64_t *plane_floats,
                      int *slices_baked) {
    return gmm_planes_info(State::kGmmRange, dims, d_plane, plane_floats, slices_baked);
}

// ---- quantile of GMM volumes: the quantile itself is the
// state of vr_set_quantile / vr_set_quantile_spread / vr_clear_quantile ----
int vr_gmm_quantile_steps(void) { return vr::kGmmQuantSteps; }

int vr_bake_gmm_quantile(void) { return bake_gmm_planes(State::kGmmQuant); }

int vr_release_gmm_quantile(void) { return release_gmm_set(State::kGmmQuant); }

int vr_gmm_quantile_info(vr_extent *dims, const float **d_plane, uint64_t *plane_floats,
                         int *slices_baked) {
    return gmm_planes_info(State::kGmmQuant, dims, d_plane, plane_floats, slices_baked);
}

int vr_release_gmm_stats(void) { return release_gmm_set(State::kGmmStats); }

int vr_gmm_stats_info(vr_extent *dims, const float **d_planes, uint64_t *plane_floats,
                      int *slices_baked) {
    return gmm_planes_info(State::kGmmStats, dims, d_planes, plane_floats, slices_baked);
}

// A frame of method 1 / 2 from the baked GMM planes: vr_render's plane march
// (plan_march with baked planes and no layout copies) on plane method - 1;
// method 10: the same march on the range plane; method 11: on the quantile plane.
// Method 13: k_march_cross_plane on the range plane, read as the plane of
// F = P(v < theta) it is after vr_set_gmm_range(-inf, theta).
int vr_render_gmm_baked(const vr_render_desc *desc) {
    if (!desc) return fail(VR_ERR_ARG, "null render descriptor");
    const int set = gmm_plane_set(desc->query_method);
    if (set < 0)
        return fail(VR_ERR_UNSUPPORTED, "baked GMM frames support queryMethod 1 (mean), 2 "
                    "(variance), 10 (range probability), 11 (quantile) and 13 (level "
                    "crossing)");
    // the plane of the set: method - 1 of the mean / variance pair, the only one of
    // the others (the plane march is planned as method 1 for those: each is one
    // float per voxel like the mean's)
    const int plane = set == State::kGmmStats ? desc->query_method - 1 : 0;
    const GmmPlaneSet &ps = kGmmPlaneSets[set];
    const State::GmmStats &b = g.gplanes[set];
    if (g.light_on && (g.proj || g.tf2_nu || !b.buf)) return light_refuse("vr_render_gmm_baked");
    if (g.proj && g.tf2_nu) return proj_refuse("vr_render_gmm_baked");
    // (under a 2-D table a plane that is not resident is the table's refusal)
    if (!b.buf && g.tf2_nu) return tf_refuse("vr_render_gmm_baked");
    if (!b.buf) return fail(VR_ERR_STATE, "no baked GMM %s (%s first)", ps.planes, ps.bake);
    if (b.nbaked != b.nz)
        return fail(VR_ERR_STATE, "%d of the GMM planes' %d slices are baked", b.nbaked, b.nz);
    // a 2-D table: the v plane, in the methods' GMM meaning, complete and of u's shape
    const float *pv = nullptr;
    if (g.tf2_nu) {
        const int vset = gmm_plane_set(g.tf2_mv);
        if (vset < 0) return tf_refuse("vr_render_gmm_baked");  // (a codec method: no GMM plane)
        const State::GmmStats &c = g.gplanes[vset];
        if (!c.buf) return tf_refuse("vr_render_gmm_baked");
        if (c.nbaked != c.nz)
            return fail(VR_ERR_STATE, "%d of the GMM planes' %d slices are baked", c.nbaked, c.nz);
        if (c.nx != b.nx || c.ny != b.ny || c.nz != b.nz || c.sy != b.sy || c.sz != b.sz)
            return fail(VR_ERR_STATE, "the GMM planes of methods %d and %d hold volumes of "
                        "different dimensions", desc->query_method, g.tf2_mv);
        pv = c.buf + (vset == State::kGmmStats ? (uint64_t)(g.tf2_mv - 1) * c.plane : 0);
    }
    vr::Params P;
    uint32_t nslots = 0;
    const FrameVol v = {b.nx, b.ny, b.nz, 1, b.sy, b.sz};
    vr_render_desc as_plane = *desc;  // (methods 10 / 11 here are not the record volumes' queries)
    as_plane.query_method = plane + 1;
    int rc = fill_frame_params(&as_plane, v, P, nslots, true);
    if (rc != VR_OK) return rc;
    const float *pl = b.buf + (uint64_t)plane * b.plane;
    if (g.light_on)  // the light: k_march_lit for every method here
        return launch_lit_frame(P, nslots, pl, b.sy, b.sz, desc->query_method == VR_QUERY_CROSSING);
    if (g.proj)  // a projection: k_march_proj for every method here
        return launch_proj_frame(P, nslots, pl, b.sy, b.sz, desc->query_method == VR_QUERY_CROSSING);
    if (g.tf_n)  // a custom transfer function: k_march_plane_tf for every method here
        return launch_tf_frame(P, nslots, pl, b.sy, b.sz, desc->query_method == VR_QUERY_CROSSING);
    if (g.tf2_nu)  // a 2-D one: k_march_tf2 on the two planes
        return launch_tf2_frame(P, nslots, pl, pv, b.sy, b.sz,
                                desc->query_method == VR_QUERY_CROSSING,
                                g.tf2_mv == VR_QUERY_CROSSING);
    hipError_t e;
    if (desc->query_method == VR_QUERY_CROSSING) {
        // no plan: the one-lane march on the x-row bricks for every view
        e = vr::launch_march_cross_plane(pl, P, nslots, g.stream);
        if (e != hipSuccess) return hip_fail(e, "launch(k_march_cross_plane)");
    } else {
        rc = launch_plane_frame(desc, P, nslots, pl, b.sy, b.sz, e);
        if (rc != VR_OK) return rc;
        if (e != hipSuccess) return hip_fail(e, "launch(k_march)");
    }
    if (P.tile_cost) g.cost_recorded = true;
    return VR_OK;
}

// ---------------- reference entry points (K:1889-2406) ------------------

void render_kernel(vr_dim3 gridSize, vr_dim3 blockSize, uint32_t *d_output, uint32_t imageW,
                   uint32_t imageH, float density, float brightness, float transferOffset,
                   float transferScale, int queryMethod, vr_extent volumeSize) {
    // d_render covers x = blockIdx.x * blockDim.x + threadIdx.x < imageW (and
    // the same in y, K:282-286): a grid smaller than the image leaves the
    // pixels beyond gridSize x blockSize untouched, a larger one is cut at the
    // image.  A launch the reference's CUDA launch would refuse fails the same
    // way (cudaErrorInvalidConfiguration, reported by getLastCudaError, C:214):
    // an empty grid or block, more than 1024 threads per block, a block
    // dimension beyond (1024, 1024, 64) or a grid beyond (2^31 - 1, 65535, 65535).
    const uint64_t threads = (uint64_t)blockSize.x * blockSize.y * blockSize.z;
    if (gridSize.x == 0 || gridSize.y == 0 || gridSize.z == 0 || threads == 0 || threads > 1024 ||
        blockSize.x > 1024 || blockSize.y > 1024 || blockSize.z > 64 ||
        gridSize.x > 0x7FFFFFFFu || gridSize.y > 65535 || gridSize.z > 65535) {
        fail(VR_ERR_ARG, "render_kernel: invalid launch configuration grid (%u,%u,%u) block (%u,%u,%u)",
             gridSize.x, gridSize.y, gridSize.z, blockSize.x, blockSize.y, blockSize.z);
        return;
    }
    const uint64_t cw = (uint64_t)gridSize.x * blockSize.x, ch = (uint64_t)gridSize.y * blockSize.y;
    vr_render_desc d;
    std::memset(&d, 0, sizeof d);
    d.d_output = d_output;
    d.width = imageW;
    d.height = imageH;
    std::memcpy(d.inv_view, g.inv_view, sizeof d.inv_view);
    d.density = density;
    d.brightness = brightness;
    d.transfer_offset = transferOffset;
    d.transfer_scale = transferScale;
    d.query_method = queryMethod;
    d.volume_size = volumeSize;
    (void)render_frame(&d, (uint32_t)std::min<uint64_t>(cw, UINT32_MAX),
                       (uint32_t)std::min<uint64_t>(ch, UINT32_MAX));
}

void copyInvViewMatrix(float *invViewMatrix, size_t sizeofMatrix) {
    if (!invViewMatrix) {
        fail(VR_ERR_ARG, "copyInvViewMatrix: null matrix");
        return;
    }
    if (sizeofMatrix > sizeof g.inv_view) {
        fail(VR_ERR_ARG, "copyInvViewMatrix: %zu bytes > 48", sizeofMatrix);
        return;
    }
    std::memcpy(g.inv_view, invViewMatrix, sizeofMatrix);
}

void initCuda(void *h_histogram, vr_extent volumeSize, vr_extent histogramSize,
              vr_int4 *h_codebook, vr_extent codebookSize, float *h_templates,
              vr_extent templatesSize, vr_float2 *h_errorsbook, vr_extent errorsbookSize,
              vr_int4 *h_codebookSpanLow, vr_int4 *h_codebookSpanHigh,
              vr_int4 *h_flexibleCodebook, vr_float2 *h_flexibleErrorsbook,
              vr_int4 *h_simpleLow, vr_int4 *h_simpleHigh, int *h_simpleCount,
              vr_float2 *h_simpleHistogram, float *h_flexibleTemplates) {
    const size_t nvox = volumeSize.width * volumeSize.height * volumeSize.depth;
    if (histogramSize.width == 0 || histogramSize.height * histogramSize.depth != nvox) {
        fail(VR_ERR_ARG,
             "initCuda: histogramSize (%zu,%zu,%zu) does not hold one record per voxel of "
             "(%zu,%zu,%zu)",
             histogramSize.width, histogramSize.height, histogramSize.depth, volumeSize.width,
             volumeSize.height, volumeSize.depth);
        return;
    }
    if (vr_init_distribution((const float *)h_histogram, volumeSize, (int)histogramSize.width,
                             0) != VR_OK)
        return;
    g.linear_filter = false;
    // codec arrays (methods 4/5/6, K:1920-2050): codebook (X,Y,Z) int4, templates
    // (nBins, nTemplates, layers) -- layer 0 is used, the reference reads layer 1
    // of a 1-layer array (K:792-793) --, errorsbook (slots, rows, layers) with one
    // row of `slots` (bin, error) pairs per voxel
    if (h_codebook && h_templates && h_errorsbook) {
        if (codebookSize.width != volumeSize.width || codebookSize.height != volumeSize.height ||
            codebookSize.depth != volumeSize.depth || templatesSize.width != histogramSize.width ||
            errorsbookSize.height * errorsbookSize.depth != nvox) {
            fail(VR_ERR_ARG, "initCuda: codebook/templates/errorsbook sizes do not match the volume");
            return;
        }
        (void)vr_init_codec(h_codebook, codebookSize, h_templates, (int)templatesSize.height,
                            h_errorsbook, (int)errorsbookSize.width, (int)templatesSize.width, 0);
    }
    // flexible-block span tables (methods 8/9/0, K:2052-2320) with the
    // reference's fixed sizes: 64x64x32 fractal and simple entries
    // (flexibleVolumeSize, K:99), 64 bins, 469 templates (K:98, 101), a 64^3
    // raw volume (K:106)
    if (h_codebookSpanLow && h_codebookSpanHigh && h_flexibleCodebook && h_flexibleErrorsbook &&
        h_simpleLow && h_simpleHigh && h_simpleCount && h_simpleHistogram && h_flexibleTemplates) {
        vr_flex_tables t;
        t.dim = 64;
        t.nbins = 64;
        t.n_fractal = t.n_simple = 64 * 64 * 32;
        t.fractal_low = h_codebookSpanLow;
        t.fractal_high = h_codebookSpanHigh;
        t.fractal_code = h_flexibleCodebook;
        t.fractal_errors = h_flexibleErrorsbook;
        t.simple_low = h_simpleLow;
        t.simple_high = h_simpleHigh;
        t.simple_count = h_simpleCount;
        t.simple_hist = h_simpleHistogram;
        t.templates = h_flexibleTemplates;
        t.ntemplates = 469;
        (void)vr_init_flex(&t);
    }
}

void freeCudaBuffers(void) {
    release_volume();
    release_codec();
    release_flex();
    release_all_gmm();
    for (int set = 0; set < State::kGmmSets; set++) release_gmm_set(set);
    release_tf_device();  // the table itself is the caller's and stays set
}

void setTextureFilterMode(bool bLinearFilter) { g.linear_filter = bLinearFilter; }

void basicDataProcessing(void) {
    // d_basicDataProcessing (K:1798-1887) fills originalQueryTex / fractalQueryTex
    // once; here the planes of vr_stats.hip.  Errors go to vr_last_error(); a
    // failed bake leaves the per-step decode in place.
    (void)bake_stats();
}

int vr_bake_stats(void) { return bake_stats(); }

int vr_release_stats(void) {
    release_stats();
    release_cstats();
    release_brick();  // the layout copies are derived from the records too
    release_axis_copy();
    return VR_OK;
}

// ---------------- the record queries (methods 10-13): shared pieces ----------------

namespace {

// vr_release_*
int release_query(int method) {
    release_planes(query_plane(method));
    return VR_OK;
}

// vr_*_info
int query_info(int method, const float **d_plane, uint64_t *plane_floats) {
    const State::Planes &p = query_plane(method);
    if (d_plane) *d_plane = p.buf;
    if (plane_floats) *plane_floats = p.floats;
    return VR_OK;
}

// w[i]: the part of [lo, hi) inside bin i of the n bins of [0, 1), in bin widths
void interval_weights(float lo, float hi, int n, float *w) {
    const double l = (double)lo, h = (double)hi, dn = (double)n;
    for (int i = 0; i < n; i++) {
        const double a = std::max(l, (double)i / dn), b = std::min(h, ((double)i + 1.0) / dn);
        w[i] = (float)(dn * std::max(0.0, b - a));
    }
}

}  // namespace

// ---------------- weighted-bin query (method 10) ----------

int vr_set_bin_weights(const float *w, int n) {
    if (!w) {  // clear
        release_planes(query_plane(VR_QUERY_WEIGHTED));
        g.qn = 0;
        g.qw = vr::BinWeights{};
        return VR_OK;
    }
    if (!lin_bins(n))
        return fail(VR_ERR_UNSUPPORTED, "%d bin weights (supported: 1,2,4,8,16,32)", n);
    for (int i = 0; i < n; i++)
        if (!std::isfinite(w[i])) return fail(VR_ERR_ARG, "bin weight %d is not finite", i);
    release_planes(query_plane(VR_QUERY_WEIGHTED));  // a plane baked with other weights
    g.qw = vr::BinWeights{};
    std::memcpy(g.qw.w, w, (size_t)n * sizeof(float));
    g.qn = n;
    return VR_OK;
}

int vr_bin_weights(float *w, int *n) {
    if (g.qn == 0) return fail(VR_ERR_STATE, "no bin weights set");
    if (w) std::memcpy(w, g.qw.w, (size_t)g.qn * sizeof(float));
    if (n) *n = g.qn;
    return VR_OK;
}

int vr_set_query_range(float lo, float hi, int n) {
    if (!lin_bins(n))
        return fail(VR_ERR_UNSUPPORTED, "%d bin weights (supported: 1,2,4,8,16,32)", n);
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi)
        return fail(VR_ERR_ARG, "vr_set_query_range: bounds must be finite with lo <= hi");
    float w[32];
    interval_weights(lo, hi, n, w);
    return vr_set_bin_weights(w, n);
}

int vr_bake_weighted(void) { return bake_query(*record_query(VR_QUERY_WEIGHTED)); }
int vr_release_weighted(void) { return release_query(VR_QUERY_WEIGHTED); }
int vr_weighted_info(const float **d_plane, uint64_t *plane_floats) {
    return query_info(VR_QUERY_WEIGHTED, d_plane, plane_floats);
}

// ---------------- quantile query (method 11) ----------------

namespace {
bool quantile_ok(float q) { return std::isfinite(q) && q >= 0.0f && q <= 1.0f; }
}  // namespace

int vr_set_quantile(float q) {
    if (!quantile_ok(q)) return fail(VR_ERR_ARG, "vr_set_quantile: q must be in [0, 1]");
    release_planes(query_plane(VR_QUERY_QUANTILE));  // a plane baked for another quantile
    release_gmm_set(State::kGmmQuant);
    g.qq = vr::QuantArgs{q, q};
    g.qmode = 1;
    return VR_OK;
}

int vr_set_quantile_spread(float q_lo, float q_hi) {
    if (!quantile_ok(q_lo) || !quantile_ok(q_hi) || q_lo > q_hi)
        return fail(VR_ERR_ARG, "vr_set_quantile_spread: 0 <= q_lo <= q_hi <= 1 required");
    release_planes(query_plane(VR_QUERY_QUANTILE));
    release_gmm_set(State::kGmmQuant);
    g.qq = vr::QuantArgs{q_lo, q_hi};
    g.qmode = 2;
    return VR_OK;
}

int vr_clear_quantile(void) {
    release_planes(query_plane(VR_QUERY_QUANTILE));
    release_gmm_set(State::kGmmQuant);
    g.qq = vr::QuantArgs{};
    g.qmode = 0;
    return VR_OK;
}

int vr_quantile(float *q_lo, float *q_hi, int *spread) {
    if (g.qmode == 0) return fail(VR_ERR_STATE, "no quantile set");
    if (q_lo) *q_lo = g.qq.q_lo;
    if (q_hi) *q_hi = g.qq.q_hi;
    if (spread) *spread = g.qmode == 2;
    return VR_OK;
}

int vr_bake_quantile(void) { return bake_query(*record_query(VR_QUERY_QUANTILE)); }
int vr_release_quantile(void) { return release_query(VR_QUERY_QUANTILE); }
int vr_quantile_info(const float **d_plane, uint64_t *plane_floats) {
    return query_info(VR_QUERY_QUANTILE, d_plane, plane_floats);
}

// ---------------- distribution-distance query (method 12) ----

int vr_set_query_target(const float *h, int n, int metric, int similarity) {
    if (!h) {  // clear
        release_planes(query_plane(VR_QUERY_DISTANCE));
        g.dn = 0;
        g.dmetric = 0;
        g.dt = vr::DistTarget{};
        return VR_OK;
    }
    if (!lin_bins(n))
        return fail(VR_ERR_UNSUPPORTED, "a target of %d bins (supported: 1,2,4,8,16,32)", n);
    if (metric < VR_DIST_L1 || metric > VR_DIST_KS)
        return fail(VR_ERR_ARG, "unknown distance metric %d (VR_DIST_L1 / _EMD / _KS)", metric);
    for (int i = 0; i < n; i++)
        if (!std::isfinite(h[i])) return fail(VR_ERR_ARG, "target bin %d is not finite", i);
    release_planes(query_plane(VR_QUERY_DISTANCE));  // a plane baked against another target
    vr::DistTarget t = {};
    std::memcpy(t.h, h, (size_t)n * sizeof(float));  // (h may be g.dt.h itself)
    t.similarity = similarity != 0;
    g.dt = t;
    g.dn = n;
    g.dmetric = metric;
    return VR_OK;
}

int vr_query_target(float *h, int *n, int *metric, int *similarity) {
    if (g.dn == 0) return fail(VR_ERR_STATE, "no query target set");
    if (h) std::memcpy(h, g.dt.h, (size_t)g.dn * sizeof(float));
    if (n) *n = g.dn;
    if (metric) *metric = g.dmetric;
    if (similarity) *similarity = g.dt.similarity;
    return VR_OK;
}

int vr_set_query_target_region(int x0, int y0, int z0, int x1, int y1, int z1, int metric,
                               int similarity) {
    constexpr int64_t kMaxVoxels = 4096;
    if (!g.vol) return fail(VR_ERR_STATE, "no volume resident (initCuda / vr_init_* first)");
    if (x0 < 0 || y0 < 0 || z0 < 0 || x1 > g.nx || y1 > g.ny || z1 > g.nz || x0 >= x1 ||
        y0 >= y1 || z0 >= z1)
        return fail(VR_ERR_ARG, "vr_set_query_target_region: the box must be non-empty and inside "
                                "the %d x %d x %d volume", g.nx, g.ny, g.nz);
    const int64_t bx = x1 - x0, by = y1 - y0, bz = z1 - z0;
    if (bx * by * bz > kMaxVoxels)
        return fail(VR_ERR_ARG, "vr_set_query_target_region: a box of %lld voxels (at most %lld)",
                    (long long)(bx * by * bz), (long long)kMaxVoxels);
    if (!lin_bins(g.nb))
        return fail(VR_ERR_UNSUPPORTED, "a target of %d bins (supported: 1,2,4,8,16,32)", g.nb);
    if (metric < VR_DIST_L1 || metric > VR_DIST_KS)
        return fail(VR_ERR_ARG, "unknown distance metric %d (VR_DIST_L1 / _EMD / _KS)", metric);
    // the box's records to the host, row by row of each slice, once the library
    // stream has drained (a bake or a conversion may still be writing)
    const size_t rec = (size_t)g.nb * elem_bytes();
    std::vector<char> box((size_t)(bx * by * bz) * rec);
    VR_HIP(hipStreamSynchronize(g.stream));
    const char *src = reinterpret_cast<const char *>(g.vol);
    for (int64_t z = 0; z < bz; z++) {
        const uint64_t first = (uint64_t)(z0 + z) * g.sz + (uint64_t)y0 * g.sy + (uint64_t)x0;
        VR_HIP(hipMemcpy2D(box.data() + (size_t)(z * by * bx) * rec, (size_t)bx * rec,
                           src + first * rec, g.sy * rec, (size_t)bx * rec, (size_t)by,
                           hipMemcpyDeviceToHost));
    }
    // each bin summed in double, voxel after voxel (x fastest, then y, then z),
    // divided by the count in double and rounded once to float
    double sum[32] = {};
    const int64_t nvox = bx * by * bz;
    for (int64_t v = 0; v < nvox; v++) {
        const char *r = box.data() + (size_t)v * rec;
        for (int i = 0; i < g.nb; i++) {
            if (g.dtype == VR_DTYPE_F16) {
                _Float16 hv;
                std::memcpy(&hv, r + 2 * (size_t)i, 2);
                sum[i] += (double)(float)hv;  // widened exactly
            } else {
                float fv;
                std::memcpy(&fv, r + 4 * (size_t)i, 4);
                sum[i] += (double)fv;
            }
        }
    }
    float h[32] = {};
    for (int i = 0; i < g.nb; i++) h[i] = (float)(sum[i] / (double)nvox);
    return vr_set_query_target(h, g.nb, metric, similarity);
}

int vr_bake_distance(void) { return bake_query(*record_query(VR_QUERY_DISTANCE)); }
int vr_release_distance(void) { return release_query(VR_QUERY_DISTANCE); }
int vr_distance_info(const float **d_plane, uint64_t *plane_floats) {
    return query_info(VR_QUERY_DISTANCE, d_plane, plane_floats);
}

// ---------------- level-crossing query (method 13) ----------

int vr_set_crossing_weights(const float *w, int n) {
    if (!w) {  // clear
        release_planes(query_plane(VR_QUERY_CROSSING));
        g.xn = 0;
        g.xw = vr::BinWeights{};
        return VR_OK;
    }
    if (!lin_bins(n))
        return fail(VR_ERR_UNSUPPORTED, "%d crossing weights (supported: 1,2,4,8,16,32)", n);
    for (int i = 0; i < n; i++)
        if (!std::isfinite(w[i])) return fail(VR_ERR_ARG, "crossing weight %d is not finite", i);
    release_planes(query_plane(VR_QUERY_CROSSING));  // a plane baked with other weights
    vr::BinWeights t = {};
    std::memcpy(t.w, w, (size_t)n * sizeof(float));  // (w may be g.xw.w itself)
    g.xw = t;
    g.xn = n;
    return VR_OK;
}

int vr_crossing_weights(float *w, int *n) {
    if (g.xn == 0) return fail(VR_ERR_STATE, "no crossing weights set");
    if (w) std::memcpy(w, g.xw.w, (size_t)g.xn * sizeof(float));
    if (n) *n = g.xn;
    return VR_OK;
}

int vr_set_isovalue(float theta, int n) {
    if (!lin_bins(n))
        return fail(VR_ERR_UNSUPPORTED, "%d crossing weights (supported: 1,2,4,8,16,32)", n);
    if (!std::isfinite(theta)) return fail(VR_ERR_ARG, "vr_set_isovalue: theta must be finite");
    float w[32];
    interval_weights(0.0f, theta, n, w);  // [0, theta)
    return vr_set_crossing_weights(w, n);
}

int vr_bake_crossing(void) { return bake_query(*record_query(VR_QUERY_CROSSING)); }
int vr_release_crossing(void) { return release_query(VR_QUERY_CROSSING); }
int vr_crossing_info(const float **d_plane, uint64_t *plane_floats) {
    return query_info(VR_QUERY_CROSSING, d_plane, plane_floats);
}

// ---------------- user-defined transfer function ----------

static_assert(VR_TF_MAX == vr::kTfMax, "vr.h repeats vr_internal.h's table size");

int vr_set_transfer_function(const float *rgba, int n) {
    if (!rgba) {  // clear: the built-in table
        g.tf_n = 0;
        g.volume_epoch++;  // a tile order learned under the table is not reused
        return VR_OK;
    }
    if (n < 1 || n > VR_TF_MAX)
        return fail(VR_ERR_ARG, "a transfer function of %d entries (1 .. %d)", n, VR_TF_MAX);
    for (int i = 0; i < 4 * n; i++)
        if (!std::isfinite(rgba[i]))
            return fail(VR_ERR_ARG, "transfer function entry %d, channel %d is not finite", i / 4,
                        i % 4);
    float t[4 * VR_TF_MAX] = {0};
    std::memcpy(t, rgba, (size_t)n * 4 * sizeof(float));  // (rgba may be g.tf itself)
    std::memcpy(g.tf, t, sizeof g.tf);
    g.tf_n = n;
    g.tf_dirty = true;  // uploaded by the next frame that uses it
    g.tf2_nu = g.tf2_nv = 0;  // at most one of the two tables is set (section 23)
    g.volume_epoch++;
    return VR_OK;
}

int vr_transfer_function(float *rgba, int *n) {
    if (rgba && g.tf_n) std::memcpy(rgba, g.tf, (size_t)g.tf_n * 4 * sizeof(float));
    if (n) *n = g.tf_n;
    return VR_OK;
}

// ---------------- ray projections ----------

static_assert(VR_PROJ_MAX == vr::kProjMax && VR_PROJ_MIN == vr::kProjMin &&
                  VR_PROJ_MEAN == vr::kProjMean,
              "vr.h repeats vr_internal.h's projection modes");

int vr_set_projection(int mode) {
    if (mode < VR_PROJ_COMPOSITE || mode > VR_PROJ_MEAN)
        return fail(VR_ERR_ARG, "projection mode %d (0 composite, 1 maximum, 2 minimum, 3 mean)",
                    mode);
    if (mode != g.proj) g.volume_epoch++;  // the rays end elsewhere: the tile order starts afresh
    g.proj = mode;
    return VR_OK;
}

int vr_projection(void) { return g.proj; }

// ---------------- headlight gradient shading ----------

static_assert(sizeof(vr_light) == 16 && sizeof(vr::Light) == 16, "the light is 16 bytes");

// Host state only.  The volume epoch is not bumped: opacity is not lit, every ray ends
// where it ended, and the adaptive tile order recorded without the light stays valid.
int vr_set_light(const vr_light *l) {
    if (!l) {
        g.light_on = false;
        return VR_OK;
    }
    const float k[3] = {l->ambient, l->diffuse, l->specular};
    static const char *const kName[3] = {"ambient", "diffuse", "specular"};
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(k[i]) || k[i] < 0.0f)
            return fail(VR_ERR_ARG, "vr_set_light: %s must be finite and >= 0", kName[i]);
    if (l->shininess_log2 < 0 || l->shininess_log2 > vr::kLightMaxLog2)
        return fail(VR_ERR_ARG, "vr_set_light: shininess_log2 %d (0 .. %d: the highlight "
                                "exponent is 2^k)", l->shininess_log2, vr::kLightMaxLog2);
    g.light = *l;
    g.light_on = true;
    return VR_OK;
}

int vr_light_state(vr_light *out) {
    if (!g.light_on) return 0;
    if (out) *out = g.light;
    return 1;
}

// ---------------- 2-D transfer function ----------

static_assert(VR_TF2_MAX == vr::kTf2Max, "vr.h repeats vr_internal.h's table size");

int vr_set_transfer_function_2d(const float *rgba, int nu, int nv, int method_v, float v_offset,
                                float v_scale) {
    if (!rgba) {  // clear (the other arguments are not read); the 1-D table stays
        g.tf2_nu = g.tf2_nv = 0;
        g.volume_epoch++;  // a tile order learned under the table is not reused
        return VR_OK;
    }
    if (nu < 1 || nv < 1 || nu > 256 || nv > 256 || nu * nv > VR_TF2_MAX)
        return fail(VR_ERR_ARG, "a 2-D transfer function of %d x %d entries (1 .. 256 each, %d in "
                    "all)", nu, nv, VR_TF2_MAX);
    const bool mv_ok = (method_v >= 1 && method_v <= 6) ||
                       (method_v >= VR_QUERY_WEIGHTED && method_v <= VR_QUERY_CROSSING) ||
                       grad_source(method_v);
    if (!mv_ok)
        return fail(VR_ERR_ARG, "method_v %d has no baked plane (1-6, 10-13, or the gradient "
                                "plane of one of those: 32 + its number)", method_v);
    if (!std::isfinite(v_offset) || !std::isfinite(v_scale))
        return fail(VR_ERR_ARG, "v_offset / v_scale is not finite");
    const int n = nu * nv;
    for (int i = 0; i < 4 * n; i++)
        if (!std::isfinite(rgba[i]))
            return fail(VR_ERR_ARG, "transfer function entry (%d, %d), channel %d is not finite",
                        (i / 4) % nu, (i / 4) / nu, i % 4);
    float t[4 * VR_TF2_MAX] = {0};  // (rgba may be g.tf2 itself)
    std::memcpy(t, rgba, (size_t)n * 4 * sizeof(float));
    std::memcpy(g.tf2, t, sizeof g.tf2);
    g.tf2_nu = nu;
    g.tf2_nv = nv;
    g.tf2_mv = method_v;
    g.tf2_voff = v_offset;
    g.tf2_vscale = v_scale;
    g.tf2_dirty = true;  // uploaded by the next frame that uses it
    g.tf_n = 0;          // at most one of the two tables is set
    g.volume_epoch++;
    return VR_OK;
}

int vr_transfer_function_2d(float *rgba, int *nu, int *nv, int *method_v, float *v_offset,
                            float *v_scale) {
    const bool set = g.tf2_nu != 0;
    if (rgba && set) std::memcpy(rgba, g.tf2, (size_t)g.tf2_nu * g.tf2_nv * 4 * sizeof(float));
    if (nu) *nu = g.tf2_nu;
    if (nv) *nv = g.tf2_nv;
    if (set) {
        if (method_v) *method_v = g.tf2_mv;
        if (v_offset) *v_offset = g.tf2_voff;
        if (v_scale) *v_scale = g.tf2_vscale;
    }
    return VR_OK;
}

// ---------------- gradient-magnitude planes ----------

// The plane of |grad s| of the resident plane s of source method `method`, by
// k_bake_grad, and its maximum.  A plane that is there was baked from this source
// (whatever frees or replaces the source frees it first): nothing to do.
int vr_bake_gradient(int method) {
    const int slot = grad_slot(method);
    if (slot < 0)
        return fail(VR_ERR_ARG, "vr_bake_gradient: method %d has no baked plane (1-6, 10-13)",
                    method);
    const TfPlane s = tf_plane(method);
    if (!s.pl->buf) {
        const RecordQuery *q = record_query(method);
        return fail(VR_ERR_STATE, "vr_bake_gradient(%d): the plane of method %d is not resident "
                                  "(%s first)", method, method,
                    q ? q->bake : "basicDataProcessing / vr_bake_stats");
    }
    State::Grad &gd = g.grad[slot];
    if (gd.p.buf) return VR_OK;
    vr::Params P;
    std::memset(&P, 0, sizeof P);
    if (s.family == 1) {
        P.nx = g.cnx; P.ny = g.cny; P.nz = g.cnz;
    } else {
        P.nx = g.nx; P.ny = g.ny; P.nz = g.nz;
    }
    P.nb = 1;
    uint32_t *d_max = nullptr;  // the maximum's bits: folded by the kernel, read back below
    VR_HIP(hipMalloc(&d_max, sizeof(uint32_t)));
    State::Planes p;
    int rc = VR_OK;
    hipError_t e = hipMemsetAsync(d_max, 0, sizeof(uint32_t), g.stream);
    if (e != hipSuccess) rc = hip_fail(e, "vr_bake_gradient");
    if (rc == VR_OK)
        rc = bake_planes(p, 1, P, "vr_bake_gradient(k_bake_grad)", "gradient planes",
                         [&](float *out, uint64_t, uint64_t psy, uint64_t psz) {
                             // (the planes of one grid share one brick layout)
                             if (psy != s.pl->sy || psz != s.pl->sz) return hipErrorInvalidValue;
                             return vr::launch_bake_grad(s.ptr(), out, psy, psz, P.nx, P.ny, P.nz,
                                                         d_max, g.stream);
                         });
    uint32_t bits = 0;
    if (rc == VR_OK) {  // (bake_planes has drained the stream)
        e = hipMemcpy(&bits, d_max, sizeof bits, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            (void)hipFree(p.buf);
            rc = hip_fail(e, "vr_bake_gradient");
        }
    }
    (void)hipFree(d_max);
    if (rc != VR_OK) return rc;
    gd.p = p;
    std::memcpy(&gd.max, &bits, sizeof bits);
    g.volume_epoch++;  // as bake_query: a tile order learned without the plane is not reused
    return VR_OK;
}

int vr_release_gradient(int method) {
    const int slot = grad_slot(method);
    if (slot < 0)
        return fail(VR_ERR_ARG, "vr_release_gradient: method %d has no baked plane (1-6, 10-13)",
                    method);
    release_grad(slot);
    return VR_OK;
}

int vr_gradient_info(int method, const float **d_plane, uint64_t *plane_floats, float *max) {
    const int slot = grad_slot(method);
    if (slot < 0)
        return fail(VR_ERR_ARG, "vr_gradient_info: method %d has no baked plane (1-6, 10-13)",
                    method);
    const State::Grad &gd = g.grad[slot];
    if (d_plane) *d_plane = gd.p.buf;
    if (plane_floats) *plane_floats = gd.p.floats;
    if (max) *max = gd.max;
    return VR_OK;
}

// ---------------- value ranges and histograms of baked planes ----

}  // extern "C"

namespace {

// A resident plane for vr_plane_range / vr_plane_histogram: tf_plane's, or a refusal
// (VR_ERR_ARG: the method names no plane; VR_ERR_STATE: not resident, with its bake),
// and the grid of its family.
int stat_plane(const char *what, const char *arg, int method, TfPlane &t, int (&dims)[3]) {
    t = tf_plane(method);
    if (!t.pl)
        return fail(VR_ERR_ARG, "%s: %s %d has no baked plane (1-6, 10-13, or the gradient plane "
                                "of one of those: 32 + its number)", what, arg, method);
    if (!t.pl->buf) {
        if (const int src = grad_source(method))
            return fail(VR_ERR_STATE, "%s: the gradient plane of method %d is not resident "
                                      "(vr_bake_gradient(%d) first)", what, src, src);
        const RecordQuery *q = record_query(method);
        return fail(VR_ERR_STATE, "%s: the plane of method %d is not resident (%s first)", what,
                    method, q ? q->bake : "basicDataProcessing / vr_bake_stats");
    }
    dims[0] = t.family == 1 ? g.cnx : g.nx;
    dims[1] = t.family == 1 ? g.cny : g.ny;
    dims[2] = t.family == 1 ? g.cnz : g.nz;
    if (dims[0] > 65535 || dims[1] > 65535 || dims[2] > 65535)
        return fail(VR_ERR_UNSUPPORTED, "%s: a grid of %d x %d x %d voxels (65535 at most along "
                                        "an axis)", what, dims[0], dims[1], dims[2]);
    return VR_OK;
}

// what a box must be whatever the grid: three non-empty ranges of non-negative voxels
int box_sane(const char *what, const int *box) {
    if (box)
        for (int a = 0; a < 3; a++)
            if (box[2 * a] < 0 || box[2 * a] >= box[2 * a + 1])
                return fail(VR_ERR_ARG, "%s: the box [%d, %d) x [%d, %d) x [%d, %d) is empty or "
                                        "starts below 0", what, box[0], box[1], box[2], box[3],
                            box[4], box[5]);
    return VR_OK;
}

// box (NULL: the whole grid) as six ints inside the grid, or VR_ERR_ARG
int box_in_grid(const char *what, const int *box, const int (&dims)[3], int (&out)[6]) {
    for (int a = 0; a < 3; a++) {
        out[2 * a] = box ? box[2 * a] : 0;
        out[2 * a + 1] = box ? box[2 * a + 1] : dims[a];
        if (out[2 * a + 1] > dims[a])
            return fail(VR_ERR_ARG, "%s: the box [%d, %d) x [%d, %d) x [%d, %d) leaves the grid of "
                                    "%d x %d x %d voxels", what, box[0], box[1], box[2], box[3],
                        box[4], box[5], dims[0], dims[1], dims[2]);
    }
    return VR_OK;
}

// Runs `launch` on the library's stream between two events and waits for it; the
// kernel's time goes to g.plane_ms (vr_plane_kernel_ms).
template <typename Launch>
int timed_launch(const char *what, Launch launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, g.stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipEventRecord(e1, g.stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) (void)hipStreamSynchronize(g.stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return hip_fail(e, what);
    g.plane_ms = ms;
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_plane_range(int method, const int *box, float *min, float *max, uint64_t *n_nan) {
    const char *const what = "vr_plane_range";
    int rc = box_sane(what, box);
    if (rc != VR_OK) return rc;
    TfPlane t;
    int dims[3], b[6];
    if ((rc = stat_plane(what, "method", method, t, dims)) != VR_OK) return rc;
    if ((rc = box_in_grid(what, box, dims, b)) != VR_OK) return rc;
    // the scratch: the two keys, preset to the identities of min and max, and the count
    struct Words {
        uint32_t keys[2];
        unsigned long long nan;
    } h = {{0xFFFFFFFFu, 0u}, 0ull}, *d = nullptr;
    VR_HIP(hipMalloc(&d, sizeof h));
    hipError_t e = hipMemcpyAsync(d, &h, sizeof h, hipMemcpyHostToDevice, g.stream);
    rc = e == hipSuccess ? VR_OK : hip_fail(e, what);
    if (rc == VR_OK)
        rc = timed_launch("vr_plane_range(k_plane_range)", [&] {
            return vr::launch_plane_range(t.ptr(), t.pl->sy, t.pl->sz, dims[0], dims[1], dims[2], b,
                                          d->keys, &d->nan, g.stream);
        });
    if (rc == VR_OK) {  // (timed_launch has drained the stream)
        e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, what);
    } else {
        (void)hipStreamSynchronize(g.stream);
    }
    (void)hipFree(d);
    if (rc != VR_OK) return rc;
    uint32_t lo = 0x7FC00000u, hi = 0x7FC00000u;  // every voxel NaN: NaN
    if (h.keys[0] <= h.keys[1]) {
        lo = (h.keys[0] & 0x80000000u) ? h.keys[0] ^ 0x80000000u : ~h.keys[0];
        hi = (h.keys[1] & 0x80000000u) ? h.keys[1] ^ 0x80000000u : ~h.keys[1];
    }
    if (min) std::memcpy(min, &lo, sizeof lo);
    if (max) std::memcpy(max, &hi, sizeof hi);
    if (n_nan) *n_nan = h.nan;
    return VR_OK;
}

int vr_plane_histogram(int method_u, float u_offset, float u_scale, int nu, int method_v,
                       float v_offset, float v_scale, int nv, const int *box, uint64_t *counts) {
    const char *const what = "vr_plane_histogram";
    if (!counts) return fail(VR_ERR_ARG, "%s: counts is null", what);
    if (nu < 1 || nv < 1 || (int64_t)nu * nv > VR_HIST_MAX)
        return fail(VR_ERR_ARG, "%s: a histogram of %d x %d bins (1 or more each, %d in all)", what,
                    nu, nv, VR_HIST_MAX);
    if (method_v == 0 && nv != 1)
        return fail(VR_ERR_ARG, "%s: nv = %d without a v plane (method_v 0 takes nv = 1)", what, nv);
    if (!std::isfinite(u_offset) || !std::isfinite(u_scale) ||
        (method_v != 0 && (!std::isfinite(v_offset) || !std::isfinite(v_scale))))
        return fail(VR_ERR_ARG, "%s: a window (offset / scale) is not finite", what);
    int rc = box_sane(what, box);
    if (rc != VR_OK) return rc;
    // both methods name planes, of one family, before either has to be resident
    const TfPlane named_u = tf_plane(method_u), named_v = method_v ? tf_plane(method_v) : named_u;
    if (!named_u.pl)
        return fail(VR_ERR_ARG, "%s: method_u %d has no baked plane (1-6, 10-13, or the gradient "
                                "plane of one of those: 32 + its number)", what, method_u);
    if (!named_v.pl)
        return fail(VR_ERR_ARG, "%s: method_v %d has no baked plane (0: none; 1-6, 10-13, or the "
                                "gradient plane of one of those: 32 + its number)", what, method_v);
    if (named_u.family != named_v.family)
        return fail(VR_ERR_UNSUPPORTED, "%s: methods %d and %d are planes of different volumes (the "
                                        "record volume's: 1-3, 10-13; the codec volume's: 4-6)",
                    what, method_u, method_v);
    TfPlane u, v;
    int dims[3], b[6];
    if ((rc = stat_plane(what, "method_u", method_u, u, dims)) != VR_OK) return rc;
    if (method_v && (rc = stat_plane(what, "method_v", method_v, v, dims)) != VR_OK) return rc;
    if (method_v && (u.pl->floats != v.pl->floats || u.pl->sy != v.pl->sy || u.pl->sz != v.pl->sz))
        return fail(VR_ERR_STATE, "the planes of methods %d and %d differ in size or pitches",
                    method_u, method_v);
    if ((rc = box_in_grid(what, box, dims, b)) != VR_OK) return rc;
    const size_t bytes = (size_t)nu * (size_t)nv * sizeof(unsigned long long);
    unsigned long long *d = nullptr;
    VR_HIP(hipMalloc(&d, bytes));
    hipError_t e = hipMemsetAsync(d, 0, bytes, g.stream);
    rc = e == hipSuccess ? VR_OK : hip_fail(e, what);
    if (rc == VR_OK)
        rc = timed_launch("vr_plane_histogram(k_plane_hist)", [&] {
            return vr::launch_plane_hist(u.ptr(), method_v ? v.ptr() : nullptr, u.pl->sy, u.pl->sz,
                                         dims[0], dims[1], dims[2], b, u_offset, u_scale, nu,
                                         v_offset, v_scale, nv, d, g.stream);
        });
    if (rc == VR_OK) {  // (timed_launch has drained the stream)
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counts are 64-bit");
        e = hipMemcpy(counts, d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, what);
    } else {
        (void)hipStreamSynchronize(g.stream);
    }
    (void)hipFree(d);
    return rc;
}

int vr_plane_kernel_ms(float *ms) {
    if (!ms) return fail(VR_ERR_ARG, "vr_plane_kernel_ms: ms is null");
    *ms = g.plane_ms;
    return VR_OK;
}

int vr_stats_info(const float **d_raw, uint64_t *raw_plane, const float **d_codec,
                  uint64_t *codec_plane) {
    if (d_raw) *d_raw = g.stats.buf;
    if (raw_plane) *raw_plane = g.stats.floats;
    if (d_codec) *d_codec = g.cstats.buf;
    if (codec_plane) *codec_plane = g.cstats.floats;
    return VR_OK;
}

void dataProcessing(void) {
    (void)vr_flex_process(6);  // blockSize = 6, K:1737
}

}  // extern "C"
