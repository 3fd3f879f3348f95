/*
 * vr.h -- C-ABI of libvr.so, the MI355X (gfx950) drop-in for the d_render path
 * of ykou/Volume-Rendering-Based-on-Distribution-Data.
 *
 * Citations: K = volumeRender_kernel.cu, C = volumeRender.cpp (reference).
 *
 * Part 1 -- the reference's own extern "C" entry points (declared C:156-170),
 * same names, argument order and meaning.  vr_dim3 / vr_extent are
 * layout-identical to dim3 (3 x uint32) and cudaExtent/hipExtent (3 x size_t),
 * so a caller written against the reference header links unchanged.
 *
 * Part 2 -- extensions (vr_*): explicit-parameter render with tile lists for
 * the multi-GPU image split, on-device synthetic volumes, the footprint counter
 * used for the roofline, GMM volumes (fp32 / f16 records, z-slab chains, baked
 * mean / variance planes), and error reporting.  The library never calls exit():
 * failures are recorded for vr_last_error() (the reference's checkCudaErrors
 * printed and exited, C:201-216).
 *
 * Threading: like the reference, all state is module-global and the entry
 * points are not thread-safe (K:22-88, 116).  One process drives one GPU.
 */
#ifndef VR_H
#define VR_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint32_t x, y, z; } vr_dim3;                /* == dim3       */
typedef struct { size_t width, height, depth; } vr_extent;   /* == cudaExtent */
typedef struct { int32_t x, y, z, w; } vr_int4;               /* == int4       */
typedef struct { float x, y; } vr_float2;                     /* == float2     */

/* ---------------- Part 1: reference entry points ------------------------- */

/* Replaces render_kernel, K:2387-2401.  Launches the per-ray march into the
 * caller-owned device buffer d_output (imageW*imageH packed RGBA8, row-major,
 * A<<24|B<<16|G<<8|R).  Miss pixels are not written (caller zeroes, C:208).
 * gridSize/blockSize keep their meaning -- pixels with x < gridSize.x*blockSize.x
 * and y < gridSize.y*blockSize.y are rendered (K:282-286), the rest of the
 * image is left untouched; an empty grid/block or more than 1024 threads per
 * block is an invalid launch (VR_ERR_ARG, nothing rendered) -- but not their
 * geometry: the library picks its own gfx950 launch (64x4-pixel tiles, one
 * 64-pixel row per wave).
 * volumeSize is used exactly where the reference uses it: the method-7 corner
 * grid (K:322-352).  queryMethod: 1 mean, 2 variance, 3 entropy,
 * 7 software-interpolated mean, 4/5/6 fractal-codec mean / variance / entropy
 * (needs the codec arrays of initCuda or vr_init_codec), 8/9/0 flexible-block
 * entropy / mean / variance (needs dataProcessing or vr_flex_process after the
 * span tables of initCuda or vr_init_flex).  Asynchronous on the library stream (default: null stream),
 * like the reference's default-stream launch. */
void render_kernel(vr_dim3 gridSize, vr_dim3 blockSize, uint32_t *d_output,
                   uint32_t imageW, uint32_t imageH, float density, float brightness,
                   float transferOffset, float transferScale, int queryMethod,
                   vr_extent volumeSize);

/* Replaces copyInvViewMatrix, K:2403-2406: 3 rows of float4 (48 bytes). */
void copyInvViewMatrix(float *invViewMatrix, size_t sizeofMatrix);

/* Replaces initCuda, K:1893-2358 (declared C:157-163 with arg 1 as void*).
 * h_histogram: fp32 records, record r = bins [r*B, r*B+B) where
 * B = histogramSize.width and r = x + X*(y + Y*z) -- the reference's layered
 * layout (bin, r % height, r / height) is exactly this AoS order (K:363-364).
 * histogramSize.height*depth must equal volumeSize.width*height*depth.
 * Args 4-9 (codebook, templates, errorsbook and their sizes) make the codec
 * volume of methods 4/5/6 resident when all three arrays are non-null (see
 * vr_init_codec); the flexible-block span tables (args 10-18) are made
 * resident when all nine are non-null, with the reference's fixed sizes
 * (64x64x32 fractal and simple entries, 64 bins, 469 templates, 64^3 raw
 * volume, K:93-106; see vr_init_flex). */
void initCuda(void *h_histogram, vr_extent volumeSize, vr_extent histogramSize,
              vr_int4 *h_codebook, vr_extent codebookSize, float *h_templates,
              vr_extent templatesSize, vr_float2 *h_errorsbook, vr_extent errorsbookSize,
              vr_int4 *h_codebookSpanLow, vr_int4 *h_codebookSpanHigh,
              vr_int4 *h_flexibleCodebook, vr_float2 *h_flexibleErrorsbook,
              vr_int4 *h_simpleLow, vr_int4 *h_simpleHigh, int *h_simpleCount,
              vr_float2 *h_simpleHistogram, float *h_flexibleTemplates);

/* Replaces freeCudaBuffers, K:2360-2385. */
void freeCudaBuffers(void);

/* Replaces setTextureFilterMode, K:1889-1891.  In the reference it switches the
 * filter of the integer index volume `tex`, which methods 1/2/3 never sample;
 * the flag is stored and has no effect on any supported method. */
void setTextureFilterMode(bool bLinearFilter);

/* Replaces basicDataProcessing, K:1798-1887.  The reference pre-bakes per-voxel
 * mean/variance/entropy of the raw volume (originalQueryTex, K:722-773) and of
 * the codec volume (fractalQueryTex, K:775-871) into float4 textures.  Here the
 * same statistics are baked once into three float planes per resident volume
 * (vr_bake_stats); frames of methods 1-7 then read the planes instead of
 * decoding the corner records at every step -- bit-identical output, 4 bytes
 * per corner voxel read instead of a whole record.  Without it (or after
 * vr_release_stats) the march decodes the records per step.  Errors (no
 * volume, out of memory) go to vr_last_error(); the per-step decode stays. */
void basicDataProcessing(void);

/* Replaces dataProcessing, K:1735-1796: the flexible-block pre-pass of
 * methods 8/9/0 with the reference's block edge of 6 voxels (K:1737), i.e.
 * vr_flex_process(6). */
void dataProcessing(void);

/* ---------------- Part 2: extensions ------------------------------------- */

#define VR_OK 0
#define VR_ERR_ARG -1
#define VR_ERR_STATE -2
#define VR_ERR_HIP -3
#define VR_ERR_UNSUPPORTED -4

/* Baked statistics (basicDataProcessing).  vr_bake_stats bakes the planes of
 * the resident raw and codec volumes that are not baked yet: 4 planes for the
 * raw volume (mean, variance, entropy and method 7's undivided corner mean)
 * and 3 for the codec volume (methods 4/5/6).  A plane is laid out in
 * 16 x 2 x 1 bricks whose x runs overlap by one voxel: with
 * sy = ((X - 1) / 15 + 1) * 32 and sz = ((Y + 1) / 2) * sy floats, voxel
 * (x, y, z) sits at z * sz + (y / 2) * sy + (y % 2) * 16 + (x / 15) * 32 +
 * x % 15 (and, for x = 15 k > 0, also at offset 15 of brick k - 1); a plane
 * holds sz * Z floats.  Re-uploading or releasing a volume drops its planes; a volume
 * modified in place through vr_volume_info's pointer must be re-baked
 * (vr_release_stats, then vr_bake_stats).  vr_stats_info: device pointers
 * (nullptr = not baked) and plane lengths in floats.
 * Layout copy: the first oblique-view frame of a library-owned 8-bin volume
 * makes a second, 2x2 (x, y) micro-brick copy of its records (DESIGN.md 2;
 * as many bytes as the volume, made synchronously, only while HBM keeps
 * max(4 GiB, 5 %) free after it).  Views whose screen x runs along the volume's
 * z or y axis (|M[8]| or |M[4]| >= 0.95) of an owned volume with 1, 2, 4 or 8
 * bins get an axis-rows copy (that axis contiguous) on the same terms, one
 * axis (both a y and a z copy when they fit; one is dropped for the other only
 * when that makes room).  vr_release_stats drops the copies with the planes, so
 * after an in-place modification the next frame that needs one rebuilds it. */
int vr_bake_stats(void);
int vr_release_stats(void);
int vr_stats_info(const float **d_raw, uint64_t *raw_plane, const float **d_codec,
                  uint64_t *codec_plane);

/* Layout copies (the micro-brick and axis-rows copies above) are made only
 * within a byte budget: vr_set_layout_budget(bytes) caps their total HBM
 * (default UINT64_MAX = two record-volume copies plus three baked-plane
 * copies, 1/8 padding each, plus 64 MiB for small volumes' padding: one view
 * class and one change of view; a baked plane's copy is kept per (view axis,
 * method) while the budget holds it, so alternating methods builds each once;
 * 0 = never make
 * one, every view marches the records' x rows) and drops resident copies that
 * exceed a lowered budget.  vr_layout_info: bytes resident in copies, copies
 * made since load, and the time and size of the last one made (each is built
 * synchronously inside the first frame that needs it, so that frame costs
 * last_build_ms more). */
int vr_set_layout_budget(uint64_t bytes);
int vr_layout_info(uint64_t *resident_bytes, int *builds, float *last_build_ms,
                   uint64_t *last_build_bytes);

/* last error message ("" if none); vr_clear_error resets it */
const char *vr_last_error(void);
int vr_last_status(void);
void vr_clear_error(void);

/* Volume residency.  bins: fp32 AoS records as in initCuda.
 * where: 0 = host pointer (copied), 1 = device pointer (copied),
 *        2 = device pointer adopted (not freed by the library). */
int vr_init_distribution(const float *bins, vr_extent dims, int nbins, int where);

/* Generate the seeded synthetic distribution volume of DESIGN.md section 5
 * directly in HBM (library-owned). */
int vr_synthesize(vr_extent dims, int nbins, uint64_t seed);

/* f16 record volumes: the bins stored as IEEE binary16,
 * half the HBM bytes per voxel.  f16 -> f32 widening is exact, so an f16 volume
 * renders bit-identically to the fp32 volume of the same records widened.
 *
 * vr_init_distribution_f16: as vr_init_distribution (same AoS layout, `where`
 * values and pitches) with 2-byte elements.  nbins must be one of 1, 2, 4, 8,
 * 16, 32 (VR_ERR_UNSUPPORTED otherwise); an adopted pointer (where == 2) must
 * be aligned to min(16, 2 * nbins) bytes (VR_ERR_ARG otherwise).
 *
 * vr_convert_f16: narrows the resident fp32 record volume to f16 on the device
 * (round to nearest even, subnormals kept) into a new library-owned buffer
 * with the same record pitches, then releases the fp32 one (freed if the
 * library owned it, forgotten if it was adopted); peak memory 1.5x the fp32
 * volume.  Baked planes and layout copies are dropped, as by a re-upload.
 * VR_ERR_STATE if no volume is resident or it is f16 already,
 * VR_ERR_UNSUPPORTED for other bin counts than the six above.
 *
 * vr_volume_dtype: VR_DTYPE_F32 / VR_DTYPE_F16 of the resident record volume,
 * VR_ERR_STATE without one.
 *
 * What an f16 volume serves: methods 1/2/3 per step through one kernel family
 * (k_march_pipe_h, every view on the x rows; no micro-brick or axis-rows copy
 * is made, VR_PATH / VR_SEG / VR_WIDE do not apply, VR_WG_PER_CU does);
 * vr_bake_stats and with it baked methods 1/2/3/7; tile lists, d_output_f,
 * d_steps, clipped renders; vr_count_footprint, vr_footprint_bytes (U * nbins
 * * 2), vr_stream_read (the real byte size).  Method 7 on an unbaked f16 volume
 * is VR_ERR_UNSUPPORTED (bake first).  Codec and flexible-block volumes are
 * separate state and always fp32; GMM volumes have their own f16 entry points
 * (vr_init_gmm_f16 below). */
#define VR_DTYPE_F32 0
#define VR_DTYPE_F16 1
int vr_init_distribution_f16(const void *bins, vr_extent dims, int nbins, int where);
int vr_convert_f16(void);
int vr_volume_dtype(void);

/* Fractal/template codec volume for methods 4/5/6 (the initCuda arrays of
 * K:1893-1900, as the reference's loaders fill them, C:558-675):
 *   codebook  dims.width*height*depth x (template id, shift, flip, NE), voxel
 *             order x + X*(y + Y*z);
 *   templates ntemplates x nbins floats;
 *   errors    err_slots (bin id, value) pairs per voxel, the first NE used.
 * where: 0 = host arrays, 1 = device arrays (copied).  Entries are validated
 * (template id < ntemplates, 0 <= shift < nbins, 0 <= NE <= err_slots);
 * error bin ids outside [0, nbins) are skipped at decode.  nbins must be one
 * of 1, 2, 4, 8, 16, 32.  initCuda calls this when its codebook, templates and
 * errorsbook arguments are non-null. */
int vr_init_codec(const vr_int4 *codebook, vr_extent dims, const float *templates,
                  int ntemplates, const vr_float2 *errors, int err_slots, int nbins, int where);

/* Generate the seeded synthetic codec volume of DESIGN.md section 5 in HBM
 * (the section-5 scalar field encoded against ntemplates templates, `slots`
 * error pairs per voxel). */
int vr_synthesize_codec(vr_extent dims, int nbins, int ntemplates, int slots, uint64_t seed);

/* shape and device arrays of the resident codec volume (codebook int4 per
 * voxel, templates [ntemplates][nbins] fp32, errors [voxel][slots] float2) */
int vr_codec_info(vr_extent *dims, int *nbins, int *ntemplates, int *slots,
                  const void **codebook, const float **templates, const void **errors);

/* Flexible-block span tables (methods 8/9/0): an integral histogram of a cubic
 * dim^3 raw volume stored as dyadic spans, as the reference's loaders fill
 * initCuda's arguments 10-18 (C:709-997):
 *   fractal_*  spans of >= 8 voxels, 1-based inclusive low/high (x, y, z, -);
 *              code (template id, shift, flip, NE); errors nbins (bin id,
 *              value) pairs per entry, the first NE used (C:773-877);
 *   simple_*   spans of < 8 voxels, 0-based inclusive low/high; count and
 *              nbins (bin id, frequency) pairs per entry (C:879-949);
 *   templates  ntemplates x nbins floats (C:951-997).
 * Entry i of a table stands where the reference's 64x64x32 lookup texture
 * holds it (x = i % 64, y = i / 64 % 64, z = i / 4096); a span listed twice
 * resolves like the reference's scan (K:1352-1372: the last 64-entry row
 * holding it, first entry in that row).  Validated: 1 <= dim <= 126,
 * 1 <= nbins <= 64, template id < ntemplates, 0 <= shift < nbins,
 * 0 <= NE <= nbins, 0 <= count <= nbins.  Host arrays, copied. */
typedef struct {
    int dim;
    int nbins;
    int n_fractal;
    const vr_int4 *fractal_low, *fractal_high, *fractal_code;
    const vr_float2 *fractal_errors;
    int n_simple;
    const vr_int4 *simple_low, *simple_high;
    const int32_t *simple_count;
    const vr_float2 *simple_hist;
    const float *templates;
    int ntemplates;
} vr_flex_tables;

int vr_init_flex(const vr_flex_tables *tables);

/* The dataProcessing pre-pass (K:1735-1796) with blocks of `block` voxels per
 * axis (the last one cut at dim): per-block mean / variance / entropy of the
 * span-table histogram (K:1033-1126), resident for methods 8/9/0.  Returns the
 * blocks per axis, or a negative status (VR_ERR_ARG if some sub-span a block
 * corner needs has no table entry).  Synchronous. */
int vr_flex_process(int block);

/* blocks per axis, bins and device array (blocks^3 x float4 (mean, variance,
 * entropy, 0), block (x, y, z) at x + n*(y + n*z)) of the resident statistics */
int vr_flex_info(int *nblk, int *nbins, const float **d_blocks);

/* dims, bin count and device pointer of the resident volume (for an f16 volume,
 * vr_volume_dtype, *d_bins addresses 2-byte halves despite its type) */
int vr_volume_info(vr_extent *dims, int *nbins, const float **d_bins);

/* Record pitch of a voxel row and of a slice of the resident volume in HBM
 * (record (x,y,z) starts at d_bins + (z*slice_pitch + y*row_pitch + x)*nbins). */
int vr_volume_layout(size_t *row_pitch, size_t *slice_pitch);

/* Stream for all subsequent launches (hipStream_t; NULL = null stream). */
int vr_set_stream(void *stream);

/* Tuning knobs (tests and tools): kernel-path overrides ("VR_PATH" 0 quad,
 * 1 LDS-box, 2 per-ray pipelined, 4 wave-staged, 7 ray-segmented; "VR_SEG"
 * lanes per ray 2/4, pipelined -2/-4), occupancy caps ("VR_WG_PER_CU"),
 * layout experiments ("VR_PAD", "VR_BRICK", ...).
 * value NULL removes a knob; vr_clear_tuning removes all.  Every knob only
 * changes which kernel computes a frame, never its pixels.  The library reads
 * no environment variables (a build with -DVR_TUNING also takes unset knobs
 * from the environment, for tooling). */
int vr_set_tuning(const char *key, const char *value);
void vr_clear_tuning(void);

/* Explicit-parameter render.  With d_tile_list == NULL the whole frame is
 * rendered into d_output[y*width + x].  Otherwise the n_tiles 64x4-pixel
 * tiles named by d_tile_list (tile id = ty*ceil(width/64) + tx, device array)
 * are rendered into a packed buffer: tile slot s occupies
 * d_output[s*256 .. s*256+255] in row-major 64x4 order.  Entries of
 * 0xFFFFFFFF in the tile list are padding and are skipped.  Entry s is
 * rendered by workgroup s, which runs on XCD s % 8 (each XCD has its own L2):
 * order the list so every 8th entry forms an equally loaded, spatially
 * compact set (tiles.py tile_lists does).  Full frames use the library's own
 * XCD-balanced order.
 * In tile-list mode miss pixels are written as 0, so packed buffers need no
 * clearing between frames (full frames keep the reference's behaviour: misses
 * untouched).
 * d_output_f (optional) receives the saturated float RGBA of every written
 * pixel, d_steps (optional) the samples taken (-1 for a miss; written for
 * every pixel inside the image). */
typedef struct {
    uint32_t *d_output;
    float *d_output_f;
    int32_t *d_steps;
    uint32_t width, height;
    float inv_view[12];
    float density, brightness, transfer_offset, transfer_scale;
    int query_method;
    vr_extent volume_size;          /* method-7 grid (render_kernel's volumeSize) */
    const uint32_t *d_tile_list;
    uint32_t n_tiles;
} vr_render_desc;

int vr_render(const vr_render_desc *desc);

/* U of SURVEY.md 8(d): distinct voxel records in the union of the trilinear
 * footprints of all samples taken (methods 1/2/3).  Synchronous; allocates a
 * bitset of voxels/8 bytes.  Returns U, or a negative status. */
int64_t vr_count_footprint(const vr_render_desc *desc);

/* Algorithmic bytes of one launch's volume reads: methods
 * 1/2/3: U * nbins * 4 (f16 volume: * 2); methods 4/5/6: 16 bytes of codebook and 8 bytes per
 * used error pair for every distinct voxel the footprints touch, plus the
 * template table once.  Synchronous.  Returns bytes or a negative status. */
int64_t vr_footprint_bytes(const vr_render_desc *desc);

/* Rank-0 assembly of the multi-GPU frame: d_packed holds n_ranks x n_slots
 * tiles (each 256 uint32) gathered from the ranks, d_tile_lists the matching
 * n_ranks x n_slots tile ids (0xFFFFFFFF = padding); every listed tile is
 * copied into d_frame (width x height, pixels outside the image dropped). */
int vr_unscatter_tiles(const uint32_t *d_packed, const uint32_t *d_tile_lists,
                       uint32_t n_ranks, uint32_t n_slots, uint32_t *d_frame,
                       uint32_t width, uint32_t height);

/* tiles (64 wide, 4 high) across / down a width x height frame */
uint32_t vr_tiles_x(uint32_t width);
uint32_t vr_tiles_y(uint32_t height);

/* name and template arguments of the march kernel the last vr_render /
 * render_kernel call launched (e.g. "k_march_quad<B=8,M=1>"), "" before any */
const char *vr_last_kernel(void);

/* Tooling: while d_buf is non-null, every launch of the per-ray pipelined,
 * quad and ray-segmented marches overwrites 3 uint64 per wave (no zeroing
 * needed, nothing accumulates): wall clock at the
 * wave's start and end (100 MHz) and __smid() (CU id, XCC id in the high
 * bits), at d_buf[(slot*4 + wave)*3] (pipelined, quad), d_buf[(slot*8 +
 * half*4 + wave)*3] (k_march_quad2) or d_buf[(slot*16 + part*4 + wave)*3]
 * (segmented).  d_buf must hold 48 * n_slots values.  nullptr turns it off. */
int vr_debug_wave_clock(uint64_t *d_buf);

/* Tooling: d_buf = 6 x uint64 of device memory, zeroed by this call on the
 * library's stream (vr_set_stream); while it is non-null, every launch of the
 * staged marches (k_march, k_march_duo) of a library built with -DVR_BOX_CHECK
 * accumulates into it: d_buf[0] = reads whose box index or footprint falls
 * outside the wave's box (each such read is skipped), d_buf[1] = the largest
 * box index + 1 - box voxels seen, d_buf[2] = box voxels of a box whose far
 * corner lies outside the volume; and the decode work: d_buf[3] = box voxels
 * decoded, d_buf[4] = lane slots spent on them (64 per group); d_buf[5] is
 * unused.  Returns 1 for a checking build, 0 for the default build (which
 * counts nothing). */
int vr_debug_box_check(uint64_t *d_buf);

/* Device self-test: compares the entropy decode's fast float logarithms (the
 * series form and the table form, vr_device.h) with (float)log((double)x) for
 * every positive finite float (synchronous, a few seconds).  counts[0] =
 * mismatches of either (must be 0), counts[1] = inputs either form left to the
 * double-log fallback (summed). */
int vr_selftest_logf(uint64_t counts[2]);

/* Measured read ceiling of this device (bench.py reports the
 * march's traffic against it beside the 8 TB/s peak): the resident record
 * volume (all B * 4 bytes of every record, pitches included, rounded down to
 * 16 B) is streamed once untimed and then reps times by a coalesced 16-B-per-
 * lane read kernel on the library's stream.  ms[0] = fastest pass, ms[1] =
 * mean; *bytes (optional) = bytes per pass.  Synchronous. */
int vr_stream_read(int reps, float ms[2], uint64_t *bytes);

/* ---- the reference's input files ---- */

/* Parse a codebook file (loadCodebook's format, C:558-642): int nSteps,
 * int nBlocks, per block int spanId, int templateId, int shift, 1-byte flip,
 * int NE, NE int bin ids, NE double errors.  Writes min(nBlocks, max_blocks)
 * entries: codebook 4 x int32 per block, errors nbins (bin, value) float pairs
 * per block (unused pairs 0).  Either output may be NULL.  Returns nBlocks,
 * -1 if unreadable/truncated, -2 if a block has NE > nbins. */
long long vr_parse_codebook(const char *path, int nbins, long long max_blocks, int32_t *codebook,
                            float *errors);

/* Parse a templates file (loadTemplates' format, C:645-675): int nTemplates,
 * per template 6 doubles (ignored) + nbins doubles.  Writes
 * min(nTemplates, max_templates) x nbins floats (may be NULL).  Returns
 * nTemplates or -1. */
long long vr_parse_templates(const char *path, int nbins, long long max_templates,
                             float *templates);

/* Load the reference's input files and make them resident, as its main()
 * does (C:1156-1203): the raw fp32 histogram volume (nBlocks x nbins), and
 * optionally the codebook + templates files for methods 4/5/6.
 * histogram_path may be NULL; codebook/templates both NULL or both given. */
int vr_load_reference_files(const char *histogram_path, const char *codebook_path,
                            const char *templates_path, vr_extent dims, int nbins);

/* Flexible-block input files (methods 8/9/0), the formats of loadSpanList,
 * loadFractalHistogram, loadSimpleHistogram and loadFlexibleTemplates
 * (C:709-997; layouts in vr_io.cpp).  Each parser writes min(count, max)
 * entries (outputs may be NULL) and returns the file's entry count, -1 if
 * unreadable or truncated, -2 if an entry is rejected the way the reference's
 * loader rejects it, -3 (fractal) if a spanId lies past the span list.
 *   span list: low/high int4 (x, y, z, 0);
 *   fractal spans: low/high = the span list's entry spanId, code int4
 *     (template id, shift, flip, NE), errors nbins (bin, value) float pairs;
 *   simple spans: low/high int4, count, hist nbins (bin, freq) float pairs. */
long long vr_parse_span_list(const char *path, long long max, int32_t *low, int32_t *high);
long long vr_parse_fractal_histogram(const char *path, const int32_t *span_low,
                                     const int32_t *span_high, long long nspans, int nbins,
                                     long long max, int32_t *low, int32_t *high, int32_t *code,
                                     float *errors);
long long vr_parse_simple_histogram(const char *count_path, const char *binid_path,
                                    const char *binfreq_path, int nbins, long long max,
                                    int32_t *low, int32_t *high, int32_t *count, float *hist);

/* Parse all six flexible-block files (flexible templates in the templates
 * format, values in [0, 1]) and make the span tables resident (vr_init_flex)
 * for a dim^3 raw volume, as main() does (C:1170-1203). */
int vr_load_flex_files(const char *span_list_path, const char *fractal_path,
                       const char *simple_count_path, const char *simple_binid_path,
                       const char *simple_binfreq_path, const char *templates_path, int dim,
                       int nbins);

/* ---- GMM distribution volumes (BASELINE config 5) ----
 * An extension: the reference holds histograms only.  Each voxel is a K-component
 * Gaussian mixture in two planes:
 *   wm     (w_k, mu_k) float pairs, [voxel][K][2]  (8K bytes per voxel)
 *   sigma  sigma_k floats,          [voxel][K]     (4K bytes per voxel)
 * voxel order x + X*(y + Y*(z - z_base)) over the resident slices
 * [z_base, z_base + nslices) of an X x Y x Z volume (dims).  K: 8, 16 or 32.
 * The march is the reference's (K:282-717) with the per-step statistic decoded
 * from the 8 corner mixtures: queryMethod 1 samples the mean sum w mu,
 * queryMethod 2 samples 16 x the variance sum w (sigma^2 + mu^2) - mean^2
 * (canonical evaluation order in vr_gmm.hip).  where: 0 host, 1 device (copied),
 * 2 device (adopted, not freed).  A new GMM volume replaces the previous one. */
int vr_init_gmm(const float *wm, const float *sigma, vr_extent dims, int ncomp, int z_base,
                int nslices, int where);

/* Generate slices [z_base, z_base + nslices) of the seeded synthetic GMM volume
 * of DESIGN.md 11.1 (a dims-sized volume) directly in HBM. */
int vr_synthesize_gmm(vr_extent dims, int ncomp, uint64_t seed, int z_base, int nslices);

/* f16 GMM volumes: the same two planes with IEEE
 * binary16 elements -- wm 4K bytes and sigma 2K bytes per voxel, same voxel
 * order, z_base / nslices, slots and `where` values.  f16 -> f32 widening is
 * exact and the statistic's evaluation order is fixed, so an f16 GMM volume
 * renders bit-identically to the fp32 volume of the same records widened.
 * Each slot carries its own element type: an fp32 volume in slot 0 and an f16
 * volume in slot 1 may be resident together.
 *
 * vr_init_gmm_f16: as vr_init_gmm with 2-byte elements.  An adopted pointer
 * (where == 2) must be aligned to the widest load the march (k_march_gmm_h, 4
 * components per lane) makes of it: 16 bytes for wm and 8 bytes for sigma
 * (VR_ERR_ARG otherwise).
 *
 * vr_synthesize_gmm_f16: the synthetic volume of vr_synthesize_gmm generated
 * directly as halves, each value the fp32 generator's rounded to nearest even
 * (what synthesize-then-narrow gives, without the fp32 planes ever existing).
 *
 * vr_convert_gmm_f16: narrows the selected slot's resident fp32 planes to f16
 * on the device (round to nearest even, subnormals kept) into new
 * library-owned buffers, then releases the fp32 planes (freed if the library
 * owned them, forgotten if adopted); peak memory 1.5x the fp32 volume.
 * VR_ERR_STATE if the slot holds no volume or it is f16 already.
 *
 * vr_gmm_dtype: VR_DTYPE_F32 / VR_DTYPE_F16 of the selected slot's volume,
 * VR_ERR_STATE without one.
 *
 * Every call on the selected slot honours its element type: vr_render_gmm
 * (whole frames and slab launches; queryMethod 1 and 2, 10 once a range is
 * set -- vr_set_gmm_range below -- and 11 once a quantile is set --
 * vr_set_quantile --, anything else VR_ERR_UNSUPPORTED as for
 * fp32), vr_gmm_count_footprint(_slab), vr_gmm_info,
 * vr_free_gmm, freeCudaBuffers.  The alive list of a slab chain is the same
 * 36-byte entry, so slabs of either type may hand rays to each other. */
int vr_init_gmm_f16(const void *wm, const void *sigma, vr_extent dims, int ncomp, int z_base,
                    int nslices, int where);
int vr_synthesize_gmm_f16(vr_extent dims, int ncomp, uint64_t seed, int z_base, int nslices);
int vr_convert_gmm_f16(void);
int vr_gmm_dtype(void);

/* dims, component count, resident slices and device pointers of the selected
 * slot's volume (for an f16 volume, d_wm and d_sigma address halves). */
int vr_gmm_info(vr_extent *dims, int *ncomp, int *z_base, int *nslices, const float **d_wm,
                const float **d_sigma);
int vr_free_gmm(void);
/* Two GMM volumes may be resident, in slots 0 and 1 (a rank of a two-segment
 * slab chain holds a front and a back z-range): every vr_*gmm*
 * call acts on the selected slot (0 until changed); vr_free_gmm frees only it,
 * freeCudaBuffers both. */
int vr_gmm_select(int slot);

/* Slab of a slab-chained render (out-of-core and multi-GPU sort-last, DESIGN.md
 * 11.2).  The launch takes the samples whose trilinear footprint starts in
 * slices [z_lo, z_hi) (it reads slices z_lo .. min(z_hi, Z-1), which must be
 * resident).  Rays come from the camera (d_rays_in == NULL: whole frame) or
 * from the alive list of the previous slab (n_rays_in entries of 36 bytes:
 * float sum[4], t, pos[3]; uint32 pixel | samples taken << 23; slab launches
 * need width*height <= 2^23).  Rays that end in
 * the slab are written to the frame (d_output etc., pixel y*width + x); rays that
 * leave it alive are appended to d_rays_out (capacity: n_rays_in, or
 * width*height) and counted in *d_n_rays_out (device memory; the call sets it
 * to 0 on the library's stream before its launch, so the caller reads it
 * after synchronising with that stream; entries past the capacity would be
 * dropped, never written).
 * Slabs must be rendered in the order the view's rays cross them (every ray of
 * the frame must step the same way in z, else VR_ERR_UNSUPPORTED); the chain
 * then reproduces the whole-volume render bit for bit. */
typedef struct {
    int z_lo, z_hi;
    const void *d_rays_in;
    uint32_t n_rays_in;
    void *d_rays_out;
    uint32_t *d_n_rays_out;
} vr_gmm_slab;

/* Render the resident GMM volume: slab == NULL renders the whole frame (all
 * slices must be resident); otherwise one slab of a chain.  desc: as for
 * vr_render (d_tile_list must be NULL). */
int vr_render_gmm(const vr_render_desc *desc, const vr_gmm_slab *slab);

/* U for a whole-volume GMM render: distinct voxels in the union of the
 * footprints of all samples taken (algorithmic bytes = U * 8K for the mean,
 * U * 12K for the variance; an f16 volume: U * 4K and U * 6K).  Synchronous. */
int64_t vr_gmm_count_footprint(const vr_render_desc *desc);
/* U of one slab of a chain (slab as for vr_render_gmm: the samples whose
 * footprint starts in the slab, from its camera rays or its alive list in).
 * The counting launch also writes the slab's alive list out (as a render
 * would) but no pixels.  Synchronous. */
int64_t vr_gmm_count_footprint_slab(const vr_render_desc *desc, const vr_gmm_slab *slab);

/* Baked GMM statistics.  The mean and the 16 x variance
 * vr_render_gmm decodes from the 8 corner mixtures of every sample are pure
 * functions of one voxel, so they can be decoded once per voxel into two float
 * planes -- plane 0 the mean (queryMethod 1), plane 1 16 x the variance
 * (queryMethod 2), each the bits the march's decode produces -- and a frame
 * rendered from the planes with the plane march of vr_render: bit-identical to
 * vr_render_gmm, 4 bytes per corner voxel read instead of 8K / 12K (f16: 4K / 6K).
 * The planes are whole-volume (X x Y x Z) in the layout of vr_bake_stats:
 * 16 x 2 x 1 bricks, sy = ((X - 1) / 15 + 1) * 32, sz = ((Y + 1) / 2) * sy,
 * voxel (x, y, z) at z * sz + (y / 2) * sy + (y % 2) * 16 + (x / 15) * 32 + x % 15
 * (and, for x = 15 k > 0, also at offset 15 of brick k - 1), sz * Z floats each,
 * plane 1 directly after plane 0.
 *
 * vr_bake_gmm_stats: bakes the selected slot's resident slices
 * [z_base, z_base + nslices), fp32 or f16, into the planes.  The first call
 * allocates both planes for the volume's dims (zeroed); later calls must come
 * from a volume of the same dims (VR_ERR_STATE otherwise).  One pass over the
 * records fills both planes.  The kernel is queued on the library stream like
 * vr_render_gmm, so an adopted buffer must stay unchanged until that stream has
 * passed it; which slices are baked is recorded at once.  Baking a slice again
 * is allowed and rewrites the same values.  VR_ERR_STATE: no GMM volume in the
 * selected slot.  VR_ERR_HIP: the planes could not be allocated; nothing has
 * changed.  VR_ERR_UNSUPPORTED: more than 65535 voxels along x or y, or more
 * than 65535 resident slices.
 * The planes belong to no slot and to no resident records: they survive
 * vr_init_gmm*, vr_synthesize_gmm*, vr_convert_gmm_f16, vr_free_gmm and
 * vr_gmm_select, so a volume that never fits in HBM is baked slab by slab
 * (make a slab resident, bake, free, next slab; any order, overlaps allowed)
 * and then rendered with no records resident.  The library cannot see that
 * records changed: A CALLER WHO CHANGES THE VOLUME'S RECORDS (new data of the
 * same dims, or records modified in place) MUST CALL vr_release_gmm_stats
 * BEFORE BAKING AGAIN, or frames mix old and new slices.
 *
 * vr_release_gmm_stats: frees the planes (freeCudaBuffers does too).
 *
 * vr_gmm_stats_info: the planes' dims, the device pointer of plane 0 (NULL: no
 * planes), a plane's length in floats and the number of distinct slices baked;
 * any argument may be NULL.
 *
 * vr_render_gmm_baked: a whole frame of queryMethod 1 or 2 (10: from the range
 * plane of vr_bake_gmm_range below; 11: from the quantile plane of
 * vr_bake_gmm_quantile below; others: VR_ERR_UNSUPPORTED) from the planes; VR_ERR_STATE unless all Z slices are
 * baked.  No GMM records need be resident, and vr_render_gmm is unaffected by
 * the planes: it keeps decoding the records per step.  desc: everything
 * vr_render takes -- d_output_f, d_steps and d_tile_list / n_tiles (padding
 * entries, misses written as 0), which gives GMM volumes the image-tile
 * multi-GPU split vr_render_gmm refuses.  The march reads the x-row bricks for
 * every view (no layout copies of GMM planes); vr_last_kernel names the plane
 * march, "<B=1,M=0>" (M=-1: planes beyond 32-bit indices).  Asynchronous on
 * the library stream. */
int vr_bake_gmm_stats(void);
int vr_release_gmm_stats(void);
int vr_gmm_stats_info(vr_extent *dims, const float **d_planes, uint64_t *plane_floats,
                      int *slices_baked);
int vr_render_gmm_baked(const vr_render_desc *desc);

/* The weighted-bin query: queryMethod 10 samples
 * s = sum_i w_i * p_i, a fixed linear functional of a voxel's bins -- the
 * probability of a value range, the CDF at an isovalue, a tail mass, a custom
 * moment; only the weights differ.  Arithmetic: float, acc = 0, then for i = 0 ..
 * B-1 in order acc = acc + p_i * w_i with a separate multiply and add (never
 * fused), no division or normalisation, subnormal products kept; numpy float32
 * restates it bit for bit.  Record volumes only (fp32 or f16, owned or adopted)
 * with 1, 2, 4, 8, 16 or 32 bins; vr_render and render_kernel take the method
 * like 1/2/3 (tile lists, d_output_f, d_steps, clipped coverage).  Every view
 * marches the x rows of the records with k_march_lin (vr_last_kernel:
 * "k_march_lin<B=..,M=10>"); no layout copy is used or made.
 * vr_render / render_kernel with queryMethod 10: VR_ERR_STATE without a record
 * volume, without weights, or with a weight count other than the volume's bins;
 * VR_ERR_UNSUPPORTED for records of any other bin count.  vr_count_footprint
 * and vr_footprint_bytes: VR_ERR_UNSUPPORTED.
 *
 * vr_set_bin_weights: n weights (n in 1, 2, 4, 8, 16, 32, else
 * VR_ERR_UNSUPPORTED; every weight finite, else VR_ERR_ARG), copied; w == NULL
 * clears them.  Host state only: no device call, so it works without a GPU and
 * before any volume is resident.  Setting or clearing weights drops the baked
 * weighted plane.
 * vr_bin_weights: the weights (w: room for 32 floats, or NULL) and their count;
 * VR_ERR_STATE if none are set.
 * vr_set_query_range: the weights of P(lo <= v < hi) on the normalised value
 * axis [0, 1], bin i covering [i / n, (i + 1) / n):
 * w_i = (float)(n * max(0, min(hi, (i + 1) / n) - max(lo, i / n))) evaluated in
 * double (a fully covered bin: exactly 1).  lo > hi or a non-finite bound:
 * VR_ERR_ARG; n as for vr_set_bin_weights.
 *
 * vr_bake_weighted: the statistic of every voxel, decoded once with the same
 * arithmetic, into one float plane in the layout of vr_bake_stats (16 x 2 x 1
 * bricks, the pitches and index formula given at vr_bake_gmm_stats; zeroed
 * padding).  While the plane is resident a queryMethod-10 frame is rendered from
 * it by the plane march of vr_render (vr_last_kernel "<B=1,M=0>"; M=-1: a
 * plane beyond 32-bit indices), bit-identical to the per-step frame.
 * Synchronous.  VR_ERR_STATE: no record volume, no weights, or a weight count
 * other than the volume's bins; VR_ERR_UNSUPPORTED: more than 65535 rows or
 * slices.  The plane is dropped by any change of the weights, a new upload or
 * release of the volume, vr_convert_f16, vr_release_stats, freeCudaBuffers and
 * vr_release_weighted.
 * vr_weighted_info: the plane's device pointer (NULL: not baked) and its length
 * in floats; either argument may be NULL. */
#define VR_QUERY_WEIGHTED 10
int vr_set_bin_weights(const float *w, int n);
int vr_bin_weights(float *w, int *n);
int vr_set_query_range(float lo, float hi, int n);
int vr_bake_weighted(void);
int vr_release_weighted(void);
int vr_weighted_info(const float **d_plane, uint64_t *plane_floats);

/* The quantile query: queryMethod 11 samples the inverse
 * of a voxel's CDF -- s = Q(q), the value on the normalised axis [0, 1] where the
 * CDF reaches q (the median, a percentile), or the spread s = Q(q_hi) - Q(q_lo)
 * (the interquartile range).  Bin i covers [i / B, (i + 1) / B) with its mass
 * spread uniformly, the conventions of vr_set_query_range.  Arithmetic: float,
 *   c_-1 = 0, c_i = c_{i-1} + p_i for i = 0 .. B-1 in order; T = c_{B-1};
 *   tau = q * T; k = the smallest i with c_i >= tau and p_i > 0, B-1 if none;
 *   frac = p_k > 0 ? (tau - c_{k-1}) / p_k : 0 (a correctly rounded IEEE division,
 *   subnormal quotients kept), then frac > 0 ? (frac > 1 ? 1 : frac) : 0;
 *   Q = (k + frac) * (1 / B); Q = T > 0 ? Q : 0 (an empty record: 0);
 * the spread is one float subtraction of two such values taken from the same
 * prefix sums.  The record is not normalised; Q(0) is the lower edge of its
 * support and Q(1) the upper edge; a record with negative bins gets whatever
 * these lines give.  numpy float32 restates it bit for bit.  Record volumes only
 * (fp32 or f16, owned or adopted) with 1, 2, 4, 8, 16 or 32 bins; vr_render and
 * render_kernel take the method like 1/2/3/10 (tile lists, d_output_f, d_steps,
 * clipped coverage).  Every view marches the x rows of the records with
 * k_march_quant (vr_last_kernel: "k_march_quant<B=..,M=11>"); no layout copy is
 * used or made.
 * vr_render / render_kernel with queryMethod 11: VR_ERR_STATE without a record
 * volume or without a quantile set; VR_ERR_UNSUPPORTED for records of any other
 * bin count.  vr_count_footprint and vr_footprint_bytes: VR_ERR_UNSUPPORTED.
 *
 * vr_set_quantile: a single quantile q.  vr_set_quantile_spread: the spread
 * between q_lo and q_hi.  q finite and in [0, 1], q_lo <= q_hi, else VR_ERR_ARG
 * and the state stays as it was.  Host state only: no device call, so they work
 * without a GPU and before any volume is resident.  vr_clear_quantile: none set.
 * Each of the three drops the baked quantile plane, and the quantile plane of
 * GMM volumes (vr_bake_gmm_quantile below), which is made of the same state.
 * vr_quantile: what is set (a single quantile: *q_lo == *q_hi, *spread = 0; the
 * spread: *spread = 1); any argument may be NULL; VR_ERR_STATE if none is set.
 *
 * vr_bake_quantile: the statistic of every voxel, decoded once with the same
 * arithmetic, into one float plane in the layout of vr_bake_stats (as
 * vr_bake_weighted; a plane of its own, resident beside the weighted plane or
 * without it).  While it is resident a queryMethod-11 frame is rendered from it
 * by the plane march of vr_render (vr_last_kernel "<B=1,M=0>"; M=-1: a plane
 * beyond 32-bit indices), bit-identical to the per-step frame.  Synchronous.
 * VR_ERR_STATE: no record volume or no quantile set; VR_ERR_UNSUPPORTED: another
 * bin count, more than 65535 rows or slices.  The plane is dropped by any call
 * that sets or clears the quantile, a new upload or release of the volume,
 * vr_convert_f16, vr_release_stats, freeCudaBuffers and vr_release_quantile.
 * vr_quantile_info: the plane's device pointer (NULL: not baked) and its length
 * in floats; either argument may be NULL. */
#define VR_QUERY_QUANTILE 11
int vr_set_quantile(float q);
int vr_set_quantile_spread(float q_lo, float q_hi);
int vr_clear_quantile(void);
int vr_quantile(float *q_lo, float *q_hi, int *spread);
int vr_bake_quantile(void);
int vr_release_quantile(void);
int vr_quantile_info(const float **d_plane, uint64_t *plane_floats);

/* The distribution-distance query: queryMethod 12 samples
 * how far a voxel's record p is from one target record h -- pick a material by
 * its histogram, or by pointing at an example region, and see where else it
 * occurs.  Three metrics, float throughout (f16 records widened first, which is
 * exact), every operation separate (never fused), in bin order, subnormals kept,
 * nothing normalised:
 *   VR_DIST_L1  (0): a = 0;        for i = 0 .. B-1: d = p_i - h_i;
 *                    a = a + |d|;                         D = a * 0.5f
 *   VR_DIST_EMD (1): a = 0; e = 0; for i = 0 .. B-1: d = p_i - h_i; e = e + d;
 *                    a = a + |e|;                         D = a * (1.0f / B)
 *   VR_DIST_KS  (2): a = 0; e = 0; for i = 0 .. B-1: d = p_i - h_i; e = e + d;
 *                    a = fmaxf(a, |e|);                   D = a
 *   s = similarity ? 1.0f - D : D
 * L1 is the total-variation distance of normalised records.  EMD is the
 * Wasserstein-1 distance on the normalised value axis [0, 1] (bin spacing 1 / B,
 * an exact scale); all B prefix differences are summed, so for unnormalised
 * records the last term charges the difference of the totals.  KS is the largest
 * CDF gap; fmaxf returns its other operand for a NaN.  Records with NaN or
 * infinite fields get whatever these lines give.  numpy float32 restates all of
 * it bit for bit.  Record volumes only (fp32 or f16, owned or adopted) with 1, 2,
 * 4, 8, 16 or 32 bins; vr_render and render_kernel take the method like
 * 1/2/3/10/11 (tile lists, d_output_f, d_steps, clipped coverage).  Every view
 * marches the x rows of the records with k_march_dist (vr_last_kernel:
 * "k_march_dist<B=..,M=12>"); no layout copy is used or made.
 * vr_render / render_kernel with queryMethod 12: VR_ERR_STATE without a record
 * volume, without a target, or with a target count other than the volume's bins;
 * VR_ERR_UNSUPPORTED for records of any other bin count.  vr_count_footprint and
 * vr_footprint_bytes: VR_ERR_UNSUPPORTED.  vr_render_gmm and vr_render_gmm_baked
 * with queryMethod 12: VR_ERR_UNSUPPORTED.
 *
 * vr_set_query_target: a target of n bins (n in 1, 2, 4, 8, 16, 32, else
 * VR_ERR_UNSUPPORTED; every h_i finite and metric in 0 .. 2, else VR_ERR_ARG; an
 * error leaves the state as it was), copied; similarity != 0: frames of 1 - D;
 * h == NULL clears the state.  Host state only: no device call, so it works
 * without a GPU and before any volume is resident.
 * vr_query_target: the target (h: room for 32 floats), its count, the metric and
 * the flag; any argument may be NULL; VR_ERR_STATE if nothing is set.
 * vr_set_query_target_region: query by example -- the target becomes the mean
 * record of the box [x0, x1) x [y0, y1) x [z0, z1) of the resident record volume.
 * The box must be non-empty, inside the volume and of at most 4096 voxels, else
 * VR_ERR_ARG; VR_ERR_STATE without a record volume.  The records are copied to
 * the host synchronously after the library stream has drained (pitches honoured,
 * f16 widened); each bin is summed in double, voxel after voxel, x fastest, then
 * y, then z, divided by the voxel count in double and rounded once to float.  The
 * state is then that of vr_set_query_target, and vr_query_target reads it back.
 * Every call that sets or clears the target drops the baked distance plane.
 *
 * vr_bake_distance: the statistic of every voxel, decoded once with the same
 * arithmetic, into one float plane in the layout of vr_bake_stats (as
 * vr_bake_weighted; a plane of its own, resident beside the weighted and quantile
 * planes or without them).  While it is resident a queryMethod-12 frame is
 * rendered from it by the plane march of vr_render (vr_last_kernel "<B=1,M=0>";
 * M=-1: a plane beyond 32-bit indices), bit-identical to the per-step frame.
 * Synchronous.  VR_ERR_STATE: no record volume, no target, or a target count
 * other than the volume's bins; VR_ERR_UNSUPPORTED: more than 65535 rows or
 * slices.  The plane is dropped by any call that sets or clears the target, a
 * new upload or release of the volume, vr_convert_f16, vr_release_stats,
 * freeCudaBuffers and vr_release_distance.
 * vr_distance_info: the plane's device pointer (NULL: not baked) and its length
 * in floats; either argument may be NULL. */
#define VR_QUERY_DISTANCE 12
#define VR_DIST_L1 0
#define VR_DIST_EMD 1
#define VR_DIST_KS 2
int vr_set_query_target(const float *h, int n, int metric, int similarity);
int vr_query_target(float *h, int *n, int *metric, int *similarity);
int vr_set_query_target_region(int x0, int y0, int z0, int x1, int y1, int z1, int metric,
                               int similarity);
int vr_bake_distance(void);
int vr_release_distance(void);
int vr_distance_info(const float **d_plane, uint64_t *plane_floats);

/* The level-crossing query: queryMethod 13 samples the
 * probability that the isosurface v = theta passes through the cell a sample lies
 * in -- the level-crossing probability of probabilistic marching cubes.  It is the
 * first query that is a joint function of the 8 corner distributions of a cell
 * and not a blend of per-voxel numbers.  ASSUMPTION OF THE METHOD: the 8 corners
 * are independent.  With F_c = P(v_c < theta) the surface crosses the cell unless
 * all corners lie on one side of it: P = 1 - prod F_c - prod (1 - F_c).
 * Arithmetic.  At a sample the footprint gives the 8 clamped corners the other
 * queries fetch, c = 0 .. 7 with x = c & 1, y = c & 2, z = c & 4.  For each,
 *   F_c = sum w_i p_i          method 10's arithmetic (a = 0; a = a + w_i * p_i in
 *                              bin order) against the crossing weights w
 * (f16 records widened first, which is exact), then in float, every operation
 * separate (never fused), subnormals kept, nothing clamped:
 *   lo = F_0;  hi = 1.0f - F_0
 *   for c = 1 .. 7:  lo = lo * F_c;  hi = hi * (1.0f - F_c)
 *   s = (1.0f - lo) - hi
 * The filter weights of the footprint are not used: the sample is constant inside
 * a cell, like a nearest-cell fetch.  In the outermost half-voxel shell of the
 * volume the clamp makes corners coincide; the lines above run over the 8 fetched
 * values as they are, so a coincident corner enters twice (or four or eight
 * times).  s may come out a few ulp below 0; the transfer function clamps its
 * argument as for every method.  numpy float32 restates all of it bit for bit.
 * Record volumes only (fp32 or f16, owned or adopted) with 1, 2, 4, 8, 16 or 32
 * bins; vr_render and render_kernel take the method like 1/2/3/10/11/12 (tile
 * lists, d_output_f, d_steps, clipped coverage).  Every view marches the x rows of
 * the records with k_march_cross (vr_last_kernel: "k_march_cross<B=..,M=13>"); no
 * layout copy is used or made.
 * vr_render / render_kernel with queryMethod 13: VR_ERR_STATE without a record
 * volume, without crossing weights, or with a weight count other than the
 * volume's bins; VR_ERR_UNSUPPORTED for records of any other bin count.
 * vr_count_footprint and vr_footprint_bytes: VR_ERR_UNSUPPORTED.  vr_render_gmm
 * with queryMethod 13: VR_ERR_UNSUPPORTED (no per-step GMM march is built).
 *
 * vr_set_crossing_weights: the weights w of the event whose probability F is (n
 * in 1, 2, 4, 8, 16, 32, else VR_ERR_UNSUPPORTED; every weight finite, else
 * VR_ERR_ARG; an error leaves the state as it was), copied; w == NULL clears
 * them.  Any per-voxel probability that is linear in the bins may stand for F;
 * the isovalue is the common case.  Host state only: no device call.  The state
 * is apart from method 10's weights, the quantile and the distance target.
 * vr_crossing_weights: the weights (w: room for 32 floats) and their count; either
 * argument may be NULL; VR_ERR_STATE if none are set.
 * vr_set_isovalue: w_i = (float)(n * max(0, min(theta, (i + 1) / n) - i / n))
 * evaluated in double with theta the float received -- bit for bit the weights
 * vr_set_query_range(0, theta, n) makes, so F is the histogram's CDF at theta on
 * the normalised value axis [0, 1]; theta <= 0 gives F = 0 everywhere, theta >= 1
 * the record's total.  theta must be finite, else VR_ERR_ARG.
 * Every call that sets or clears the crossing weights drops the crossing plane.
 *
 * vr_bake_crossing: F of every voxel, decoded once by method 10's bake kernel
 * (k_bake_lin) with the crossing weights, into one float plane in the layout of
 * vr_bake_stats -- a plane of its own, resident beside the weighted, quantile and
 * distance planes or without them.  While it is resident a queryMethod-13 frame
 * is k_march_cross_plane on it (vr_last_kernel "k_march_cross_plane<B=1,M=13>"),
 * bit-identical to the per-step frame.  Synchronous.  VR_ERR_STATE: no record
 * volume, no weights, or a weight count other than the volume's bins;
 * VR_ERR_UNSUPPORTED: more than 65535 rows or slices.  The plane is dropped by
 * any call that sets or clears the crossing weights, a new upload or release of
 * the volume, vr_convert_f16, vr_release_stats, freeCudaBuffers and
 * vr_release_crossing; the weights are the caller's and survive all of these
 * except a call that sets or clears them.
 * vr_crossing_info: the plane's device pointer (NULL: not baked) and its length
 * in floats; either argument may be NULL.
 *
 * GMM volumes: vr_render_gmm_baked with queryMethod 13 runs k_march_cross_plane
 * over the resident GMM range plane (vr_bake_gmm_range).  Baked with
 * vr_set_gmm_range(-inf, theta) that plane holds the mixture's CDF at theta, so
 * the frame is the level-crossing probability of the GMM volume.  VR_ERR_STATE
 * without a complete range plane. */
#define VR_QUERY_CROSSING 13
int vr_set_crossing_weights(const float *w, int n);
int vr_crossing_weights(float *w, int *n);
int vr_set_isovalue(float theta, int n);
int vr_bake_crossing(void);
int vr_release_crossing(void);
int vr_crossing_info(const float **d_plane, uint64_t *plane_floats);

/* The range probability of GMM volumes: queryMethod 10
 * (VR_QUERY_WEIGHTED) on a GMM volume samples the mixture's mass in [lo, hi),
 *   s = sum_k w_k (Phi((hi - mu_k) / sigma_k) - Phi((lo - mu_k) / sigma_k)),
 * the meaning vr_set_query_range gives the method on histogram volumes; lo = -inf
 * is the CDF at hi, hi = +inf the exceedance of lo.  lo and hi are on the axis mu
 * lives on and nothing is clamped to [0, 1].
 * Arithmetic: float throughout, f16 records widened first (exact), every
 * multiply and add separate (no fma anywhere), so numpy float32 restates it bit
 * for bit.  Per component k:
 *   r   = 1.0f / sigma_k                         (IEEE division)
 *   ok  = sigma_k > 0 and r is finite
 *   eh  = ok ? E((hi - mu_k) * r) : (mu_k < hi ? 0.5f : -0.5f)
 *   el  = ok ? E((lo - mu_k) * r) : (mu_k < lo ? 0.5f : -0.5f)
 *   t_k = w_k * (eh - el)
 * so a component with sigma = 0 (or with a reciprocal that overflows) is a Dirac
 * that counts exactly when lo <= mu < hi.  Lane s of the voxel's L = K / 4 lanes
 * forms p = t_4s; p = p + t_4s+1; p = p + t_4s+2; p = p + t_4s+3, and the lanes'
 * p are summed by the pairwise tree of vr_gmm.hip (T(p)).
 * Records with NaN or infinite fields get whatever these lines give.
 * E(z) = Phi(z) - 1/2 is odd and read from a table of cubic segments:
 *   a = fmin(|z|, ZMAX)                          (a NaN z takes ZMAX)
 *   i = (int)(a * (1 / h));  t = a - (float)i * h    (h a power of two: both exact)
 *   e = c0[i] + t * (c1[i] + t * (c2[i] + t * c3[i]))
 *   E = copysign(e, z)
 * with h = 1/16, ZMAX = 5 and 80 segments, plus the row i = 80 = (0.5, 0, 0, 0)
 * that a = ZMAX reads: E(0) = 0 and E(+-inf) = +-0.5 exactly.  |E - E_true| <=
 * 2.9e-7 < 2^-18 for every z (largest at the clamp), so with sum w = 1 a voxel's
 * probability is within 2^-16 of the true value.  The table is not strictly
 * monotone: at some segment joints it dips by 1 ulp (3e-8), so a very narrow
 * range can give about -3e-8; the transfer function clamps.
 * vr_gmm_phi_table: the constants the kernels use -- *c: four arrays c0 .. c3 of
 * *nseg + 1 floats each, one after the other (host memory, never freed), *h,
 * *zmax; any argument may be NULL.  No device call.
 *
 * vr_set_gmm_range: the bounds.  NaN or lo > hi: VR_ERR_ARG, the state stays as
 * it was; +-inf is allowed.  Host state only: no device call, so it works
 * without a GPU and before any volume is resident.  vr_clear_gmm_range: none
 * set.  Both drop the baked range plane.  vr_gmm_range: the bounds (either
 * argument may be NULL); VR_ERR_STATE if none are set.
 *
 * vr_render_gmm with queryMethod 10: VR_ERR_STATE without a range; fp32 and f16
 * volumes, both slots, whole frames and slabs (the alive list is the one of
 * methods 1/2).  vr_last_kernel: "k_march_gmm_range<B=K,M=10>" /
 * "k_march_gmm_range_h<...>".  vr_gmm_count_footprint(_slab) with queryMethod
 * 10: VR_ERR_UNSUPPORTED.
 *
 * vr_bake_gmm_range: the statistic of the selected slot's resident slices,
 * decoded once per voxel with the same arithmetic, into one whole-volume float
 * plane of its own in the layout and pitches given at vr_bake_gmm_stats, with
 * its own per-slice flags: the first call allocates it (zeroed), later calls
 * must come from a volume of the same dims, and a volume that never fits is
 * baked slab by slab.  Queued on the library stream.  VR_ERR_STATE: no GMM
 * volume in the selected slot, no range set, or other dims; VR_ERR_UNSUPPORTED
 * and VR_ERR_HIP as for vr_bake_gmm_stats.  The plane is independent of the
 * mean / variance planes: either may be resident without the other and neither
 * call touches the other's plane.  It survives vr_init_gmm*, vr_synthesize_gmm*,
 * vr_convert_gmm_f16, vr_free_gmm and vr_gmm_select, and is dropped by
 * vr_set_gmm_range, vr_clear_gmm_range, vr_release_gmm_range and
 * freeCudaBuffers.  As for vr_bake_gmm_stats: A CALLER WHO CHANGES THE VOLUME'S
 * RECORDS (new data of the same dims, or records modified in place) MUST CALL
 * vr_release_gmm_range BEFORE BAKING AGAIN, or frames mix old and new slices.
 * vr_gmm_range_info: as vr_gmm_stats_info, for the one range plane.
 *
 * vr_render_gmm_baked with queryMethod 10: a whole frame from the range plane by
 * the plane march ("<B=1,M=0>"), bit-identical to the per-step frame; tile
 * lists, d_output_f and d_steps as for methods 1/2.  VR_ERR_STATE: no range
 * plane, or not all slices baked. */
int vr_set_gmm_range(float lo, float hi);
int vr_clear_gmm_range(void);
int vr_gmm_range(float *lo, float *hi);
int vr_gmm_phi_table(const float **c, int *nseg, float *h, float *zmax);
int vr_bake_gmm_range(void);
int vr_release_gmm_range(void);
int vr_gmm_range_info(vr_extent *dims, const float **d_plane, uint64_t *plane_floats,
                      int *slices_baked);

/* The quantile of GMM volumes: queryMethod 11
 * (VR_QUERY_QUANTILE) on a GMM volume samples the value at which the voxel's
 * mixture CDF reaches q -- the median, a percentile --, or the spread
 * Q(q_hi) - Q(q_lo) (the interquartile range).  The quantile is the state of
 * vr_set_quantile / vr_set_quantile_spread / vr_clear_quantile / vr_quantile
 * above; there is no setter of its own.  Q lives on the axis mu lives on and
 * nothing is clamped to [0, 1].  A mixture's quantile has no closed form: it is
 * a bisection of N = vr_gmm_quantile_steps() = 20 steps over the support.
 * Arithmetic: float throughout, f16 records widened first (exact), every
 * multiply and add separate (no fma anywhere), E and ZMAX the table of the range
 * probability above, so numpy float32 restates it bit for bit.  Per voxel, lane
 * s of its L = K / 4 lanes holding components 4s .. 4s + 3 and T the pairwise
 * tree of vr_gmm.hip:
 *   r_k  = 1.0f / sigma_k                        (IEEE division)
 *   ok_k = sigma_k > 0 and r_k is finite         (else a Dirac at mu_k)
 *   W    = T(p), p = w_4s; p = p + w_4s+1; p = p + w_4s+2; p = p + w_4s+3
 *   a0   = fmin over k with w_k > 0 of (mu_k - ZMAX * sigma_k)
 *   b0   = fmax over k with w_k > 0 of (mu_k + ZMAX * sigma_k)
 *   C(x) = T(p), p = c_4s; p = p + c_4s+1; ..., c_k = w_k * (0.5f + e_k),
 *          e_k = ok_k ? E((x - mu_k) * r_k) : (mu_k < x ? 0.5f : -0.5f)
 *   tau  = q * W;  lo = a0;  hi = b0
 *   N times: mid = (lo + hi) * 0.5f;  if C(mid) < tau then lo = mid else hi = mid
 *   Q(q) = (some w_k > 0) ? hi : 0.0f
 * and the spread is two searches on the same r, W, a0, b0, then one float
 * subtraction.  All components enter W and C; only those of positive weight set
 * the bracket.  Q(0) is the lower edge a0 of the support or a float next to it,
 * Q(1) is at or next to b0; a Dirac at mu returns a value within
 * (b0 - a0) 2^-N above mu; a record with no positive weight returns 0; records
 * with NaN or infinite fields, or negative weights, get whatever these lines
 * give (which of a0 = +0 and a0 = -0 a tie between the two yields is not fixed).
 * The search leaves Q within (b0 - a0) 2^-N of the table CDF's crossing.
 *
 * vr_render_gmm with queryMethod 11: VR_ERR_STATE without a quantile set; fp32
 * and f16 volumes, both slots, whole frames and slabs (the alive list is the one
 * of methods 1/2).  vr_last_kernel: "k_march_gmm_quant<B=K,M=11>" /
 * "k_march_gmm_quant_h<...>".  vr_gmm_count_footprint(_slab) with queryMethod
 * 11: VR_ERR_UNSUPPORTED.  The per-step march repeats the search at all 8
 * corners of every sample: frames are meant to come from the plane.
 *
 * vr_bake_gmm_quantile: the statistic of the selected slot's resident slices,
 * decoded once per voxel with the same arithmetic, into one whole-volume float
 * plane of its own in the layout and pitches given at vr_bake_gmm_stats, with
 * its own per-slice flags: the first call allocates it (zeroed), later calls
 * must come from a volume of the same dims, and a volume that never fits is
 * baked slab by slab.  Queued on the library stream.  VR_ERR_STATE: no GMM
 * volume in the selected slot, no quantile set, or other dims;
 * VR_ERR_UNSUPPORTED and VR_ERR_HIP as for vr_bake_gmm_stats.  The plane is
 * independent of the mean / variance planes and of the range plane: any of the
 * three may be resident without the others and no call on one touches another.
 * It survives vr_init_gmm*, vr_synthesize_gmm*, vr_convert_gmm_f16, vr_free_gmm
 * and vr_gmm_select, and is dropped by vr_set_quantile, vr_set_quantile_spread,
 * vr_clear_quantile, vr_release_gmm_quantile and freeCudaBuffers.  As for
 * vr_bake_gmm_stats: A CALLER WHO CHANGES THE VOLUME'S RECORDS (new data of the
 * same dims, or records modified in place) MUST CALL vr_release_gmm_quantile
 * BEFORE BAKING AGAIN, or frames mix old and new slices.
 * vr_gmm_quantile_info: as vr_gmm_stats_info, for the one quantile plane.
 *
 * vr_render_gmm_baked with queryMethod 11: a whole frame from the quantile plane
 * by the plane march ("<B=1,M=0>"), bit-identical to the per-step frame; tile
 * lists, d_output_f and d_steps as for methods 1/2.  VR_ERR_STATE: no quantile
 * plane, or not all slices baked. */
int vr_gmm_quantile_steps(void);
int vr_bake_gmm_quantile(void);
int vr_release_gmm_quantile(void);
int vr_gmm_quantile_info(vr_extent *dims, const float **d_plane, uint64_t *plane_floats,
                         int *slices_baked);

/* A user-defined transfer function for frames from baked planes (DESIGN.md
 * section 22).  Every frame is classified through the reference's nine-entry
 * rainbow (K:2323-2326) unless a table is set here: n RGBA entries, 1 <= n <=
 * VR_TF_MAX, sampled exactly as the built-in nine are -- linear filter,
 * normalised coordinate x = (sample - transfer_offset) * transfer_scale clamped
 * to [0, 1], entry i centred at (i + 1/2) / n, 8-bit fractional weight, indices
 * clamped to [0, n - 1] -- with every operation a separate float one.  The table's
 * values are not clamped (the packed pixel saturates, as always); compositing is
 * unchanged.  A table of the reference's nine entries gives the built-in frames
 * bit for bit.
 *
 * vr_set_transfer_function: n entries of r, g, b, a, copied; rgba == NULL clears
 * the table (n ignored).  n outside 1 .. VR_TF_MAX or a value that is not finite:
 * VR_ERR_ARG, the state stays as it was.  Host state only: no device call, so it
 * works without a GPU; the device copy is made or refreshed by the next frame that
 * uses it (one synchronisation of the render stream then, nothing extra in later
 * frames).  The table is the caller's, like the bin weights: it survives new
 * volumes, vr_convert_f16, vr_release_*, and freeCudaBuffers (which frees only the
 * device copy); only a NULL call clears it.  It drops no baked plane.
 * vr_transfer_function: the table (rgba: room for 4 * VR_TF_MAX floats, or NULL)
 * and its entry count, *n = 0 when the built-in table is in use; either argument
 * may be NULL.
 *
 * While a table is set a frame comes from a baked plane or not at all:
 *   vr_render / render_kernel, methods 1/2/3 with vr_bake_stats' planes resident,
 *     4/5/6 with the codec planes resident, 10/11/12 with the query's plane
 *     resident: k_march_plane_tf on that plane in its x-row bricks, whatever the
 *     view (vr_last_kernel "k_march_plane_tf<B=1,M=0>"); no plan is consulted and
 *     no layout copy is made or used;
 *   method 13 with the crossing plane resident, and vr_render_gmm_baked with
 *     queryMethod 13: the same kernel with the crossing combine ("<B=1,M=13>");
 *   vr_render_gmm_baked with queryMethod 1, 2, 10, 11: as the first case;
 *   everything else -- every per-step march, method 7, methods 8/9/0,
 *     vr_render_gmm, vr_count_footprint, vr_footprint_bytes,
 *     vr_gmm_count_footprint(_slab) -- is VR_ERR_UNSUPPORTED: bake first, or clear
 *     the table.  Nothing falls back to the built-in table.
 * Tile lists, d_output_f, d_steps and clipped coverage work as in every other
 * frame.  Tuning key VR_TF_WIDE=1 forces the instance with 64-bit plane indices
 * (chosen by itself for planes beyond 32-bit indices).
 *
 * At most one of this table and the 2-D table below is set: a successful
 * vr_set_transfer_function(non-NULL) clears the 2-D table; a NULL call clears only
 * this one.
 *
 * The order of the checks, where more than one refusal applies to a frame (it holds
 * for both tables, the projection and the light below).  vr_render / render_kernel:
 * first a gradient method whose plane is not resident (VR_ERR_UNSUPPORTED); then the
 * volume the method reads (VR_ERR_STATE without it); then a record query's own state
 * (methods 10-13: VR_ERR_STATE without it or with another bin count, as without a
 * table); only then the light, the projection and the tables, in that order, each with
 * its VR_ERR_UNSUPPORTED.  vr_render_gmm: the light, the projection and the tables
 * first (VR_ERR_UNSUPPORTED), then the volume, the method and its state as without
 * them.  vr_render_gmm_baked: a method without a GMM plane set (VR_ERR_UNSUPPORTED);
 * then the light (with a projection or a 2-D table set, or with the plane set not
 * baked: VR_ERR_UNSUPPORTED), a projection with a 2-D table, a 2-D table with the
 * plane set not baked (both VR_ERR_UNSUPPORTED); then, as without any of them and so
 * under a 1-D table or a projection too, VR_ERR_STATE for a plane set that is not baked
 * or not complete; last the 2-D table's v plane set. */
#define VR_TF_MAX 256
int vr_set_transfer_function(const float *rgba, int n);
int vr_transfer_function(float *rgba, int *n);

/* A 2-D transfer function over two baked planes of one volume (DESIGN.md section
 * 23): colour by one statistic, opacity by another, inside one march.  The table
 * has nu x nv RGBA float entries, entry (i, j) at rgba[4 * (j * nu + i)] (u
 * fastest), 1 <= nu, nv <= 256 and nu * nv <= VR_TF2_MAX.  At every sample the
 * march forms two numbers from the same footprint: su from the plane of the
 * frame's query_method ("u"), sv from the plane of method_v ("v"), each the
 * trilinear blend of its eight corners (method 13: the crossing combine of them,
 * as in the one-plane frames).  Then, with lin_axis (linear filter, coordinate
 * clamped to [0, 1], NaN as 0, entry i centred at (i + 1/2) / n, 8-bit weight,
 * indices clamped) and lerpq(p, q, t) = (1 - t) * p + t * q:
 *
 *   xu = (su - transfer_offset) * transfer_scale ;  lin_axis(xu, nu, i0, i1, a)
 *   xv = (sv - v_offset)        * v_scale        ;  lin_axis(xv, nv, j0, j1, b)
 *   for c in r, g, b, a:
 *       r0    = lerpq(tab[j0][i0].c, tab[j0][i1].c, a)
 *       r1    = lerpq(tab[j1][i0].c, tab[j1][i1].c, a)
 *       col.c = lerpq(r0, r1, b)
 *
 * every operation a separate float one, nothing in the table clamped, subnormals
 * kept; compositing is unchanged (col.a *= density, premultiply, over, exit at
 * 0.95).  numpy float32 restates it bit for bit.
 *
 * Collapse to the 1-D table: lerpq(r, r, b) is not r in general, but it is when
 * every table value is m / 256 with an integer 0 <= m <= 256 (a and b are multiples
 * of 2^-8, so r0 is a multiple of 2^-16 no larger than 1 and both products of the
 * second lerp are exact).  A table whose rows all hold the same such 8-bit 1-D
 * table, with any nv including 1, therefore gives the one-plane frame of
 * vr_set_transfer_function with that 1-D table bit for bit, whatever plane v is;
 * with the reference's nine entries as rows it gives the built-in frames.  The
 * property holds for 8-bit values only: rows of arbitrary floats differ from the
 * 1-D frame in the last bit of some samples.
 *
 * vr_set_transfer_function_2d: nu * nv entries, copied; rgba == NULL clears the
 * table (the other arguments are not read).  nu or nv outside 1 .. 256, nu * nv >
 * VR_TF2_MAX, a table value, v_offset or v_scale that is not finite, or a method_v
 * outside {1, 2, 3, 4, 5, 6, 10, 11, 12, 13}: VR_ERR_ARG, the state stays as it
 * was.  Host state only, kept exactly as the 1-D table is: no device call (works
 * without a GPU), uploaded by the next frame that uses it into a device buffer of
 * its own, the caller's (survives new volumes, vr_convert_f16, vr_release_* and
 * freeCudaBuffers, which frees only the device copy), drops no baked plane.
 * At most one of the two tables is set: a successful
 * vr_set_transfer_function_2d(non-NULL) clears the 1-D table; a NULL call clears
 * only the 2-D one.
 * vr_transfer_function_2d: the table (rgba: room for 4 * VR_TF2_MAX floats, or
 * NULL), its shape and the v axis; *nu = *nv = 0 when none is set (the other
 * outputs are then left alone); every argument may be NULL.
 *
 * While a 2-D table is set:
 *   vr_render / render_kernel with query_method u: u and method_v both from
 *     {1, 2, 3, 10, 11, 12, 13} (vr_bake_stats' planes and the record queries'
 *     planes) or both from {4, 5, 6} (the codec planes), each the plane the 1-D
 *     route takes, both resident: k_march_tf2 on the two planes in their x-row
 *     bricks, whatever the view (vr_last_kernel "k_march_tf2<B=2,M=c>" with
 *     c = (u is 13) + 2 * (method_v is 13)); u == method_v is allowed;
 *   vr_render_gmm_baked with u and method_v from {1, 2, 10, 11, 13} in their GMM
 *     meaning (10 and 13 both read the range plane, 13 combined), every plane set
 *     used complete (else VR_ERR_STATE, as without a table) and of the same
 *     dimensions (else VR_ERR_STATE);
 *   a plane that is not resident, or a u / method_v pair of different families:
 *     VR_ERR_UNSUPPORTED with the 1-D table's message (bake first, or clear);
 *   everything else is VR_ERR_UNSUPPORTED exactly as under a 1-D table.  Nothing
 *     falls back to the built-in table or to the 1-D route.
 * Tile lists, d_output_f, d_steps, clipped coverage and VR_TF_WIDE work as under
 * the 1-D table.  VR_TF2_MAX is 1024 because the table is staged in LDS as float4
 * (16 KiB a workgroup). */
#define VR_TF2_MAX 1024
int vr_set_transfer_function_2d(const float *rgba, int nu, int nv, int method_v, float v_offset,
                                float v_scale);
int vr_transfer_function_2d(float *rgba, int *nu, int *nv, int *method_v, float *v_offset,
                            float *v_scale);

/* ---- ray projections of baked planes ----
 * What is done with the samples along a ray.  VR_PROJ_COMPOSITE (the default) is
 * the front-to-back emission-absorption integral with early termination, every
 * path exactly as without this state.  Under the other three a ray is set up and
 * stepped as ever (sample i at pos, t += 0.01, the ray ends when t > tfar or after
 * 500 samples) but no opacity test is made, and its n samples are reduced in
 * float32, in step order:
 *     VR_PROJ_MAX   acc = -inf; acc = (s > acc) ? s : acc   (a NaN sample is skipped)
 *     VR_PROJ_MIN   acc = +inf; acc = (s < acc) ? s : acc
 *     VR_PROJ_MEAN  sum = 0; sum = sum + s; acc = sum / (float)n
 * The ray's one value is then classified as a sample is, x = (acc -
 * transfer_offset) * transfer_scale through the table of vr_set_transfer_function
 * if one is set, else the built-in nine entries, and the pixel is (r a, g a, b a,
 * a) times brightness, clamped and packed as ever; d_steps receives n.  density is
 * not read: it is the opacity of one step, and a projection has no steps to weigh.
 *
 * vr_set_projection: one of the four modes; anything else is VR_ERR_ARG and the
 * state stays as it was.  Host state only: no device call, so it may be set before
 * a volume is resident.  Like the table it is the caller's: it survives new volumes,
 * vr_convert_f16, every vr_release_* and freeCudaBuffers; only
 * vr_set_projection(VR_PROJ_COMPOSITE) clears it.  Changing it starts the adaptive
 * tile order afresh.  vr_projection: the mode.
 *
 * With a projection set, vr_render / render_kernel and vr_render_gmm_baked serve
 * exactly the frames a 1-D table serves -- the resident baked plane of methods
 * 1/2/3, 4/5/6 and 10-13 (13: the crossing combine of the 8 corners), of GMM
 * methods 1, 2, 10, 11 and 13 -- marched in the plane's own bricks for every view
 * (k_march_proj; vr_last_kernel: k_march_proj_max / _min / _mean<B=1,M=0 or 13>);
 * tile lists, d_output_f, d_steps, clipped coverage, VR_TF_WIDE and VR_WG_PER_CU as
 * under the table.  Everything else -- a plane that is not baked, methods 7 and
 * 8/9/0, vr_render_gmm and slab chains, vr_count_footprint, vr_footprint_bytes,
 * vr_gmm_count_footprint(_slab), and any frame while a 2-D table is set (a
 * projection classifies one plane) -- is VR_ERR_UNSUPPORTED: bake first, or clear
 * the projection.  Nothing falls back to compositing. */
#define VR_PROJ_COMPOSITE 0
#define VR_PROJ_MAX 1
#define VR_PROJ_MIN 2
#define VR_PROJ_MEAN 3
int vr_set_projection(int mode);
int vr_projection(void);

/* ---- headlight gradient shading of baked planes ----
 * A light at the eye that gives the surfaces of a baked-plane frame their shape.
 * Off (the default) leaves every path exactly as without this state.  On, a ray is
 * set up, stepped and ended as under a 1-D table (the same positions, the 500-sample
 * cap, the 0.95 opacity test; d_steps receives the same counts), and at every sample
 * the gradient of the trilinear interpolant inside the sample's cell is formed from
 * the 8 corner values s0..s7 the step holds (corner j: x = j & 1, y = j & 2,
 * z = j & 4; ax, ay, az the footprint's weights; float32, one operation at a time):
 *     gx = lerp(lerp(s1 - s0, s3 - s2, ay), lerp(s5 - s4, s7 - s6, ay), az)
 *     gy = lerp(c10 - c00, c11 - c01, az)      c00..c11, c0, c1: the blend's own
 *     gz = c1 - c0                             intermediates
 *     G  = (gx nx, gy ny, gz nz)               nx, ny, nz: the volume's dimensions
 *     c  = |G . d| / sqrt(G . G)  clamped to at most 1; 1 where G . G is not > 0
 *     p  = c squared shininess_log2 times      (c ^ (2 ^ shininess_log2))
 * with d the ray's direction, and the table's colour is lit before it is weighted by
 * its opacity: rgb = rgb * (ambient + diffuse * c) + specular * p.  Alpha is not lit,
 * so rays end where they end without the light.  For a plane of F (method 13) the
 * sample stays the crossing combine and the gradient is that of F, the normal of the
 * probabilistic isosurface.  (ambient, diffuse, specular) = (1, 0, 0) gives the
 * unlit frame bit for bit.
 *
 * vr_set_light: NULL turns the light off.  A coefficient that is not finite or is
 * negative, or shininess_log2 outside 0..7, is VR_ERR_ARG and the state stays as it
 * was.  Host state only: no device call, so it may be set before a volume is
 * resident.  Like the tables it is the caller's: it survives new volumes,
 * vr_convert_f16, every vr_release_* and freeCudaBuffers; only vr_set_light(NULL)
 * clears it.  The adaptive tile order is kept: rays have not changed length.
 * vr_light_state: 1 and *out filled (out may be NULL) if a light is set, 0 if not.
 *
 * With the light on, vr_render / render_kernel and vr_render_gmm_baked serve exactly
 * the frames a 1-D table serves -- the resident baked plane of methods 1/2/3, 4/5/6
 * and 10-13, of GMM methods 1, 2, 10, 11 and 13 -- classified through the table of
 * vr_set_transfer_function if one is set, else the built-in nine entries
 * (k_march_lit; vr_last_kernel: k_march_lit<B=1,M=0 or 13>); tile lists, d_output_f,
 * d_steps, clipped coverage, VR_TF_WIDE and VR_WG_PER_CU as under the table.
 * Everything else -- a plane that is not baked, methods 7 and 8/9/0, vr_render_gmm
 * and slab chains, vr_count_footprint, vr_footprint_bytes,
 * vr_gmm_count_footprint(_slab), any frame while a 2-D table is set and any frame
 * while a projection is set (a projection classifies once per ray) -- is
 * VR_ERR_UNSUPPORTED: bake first, or clear the light.  Nothing falls back to an
 * unlit frame. */
typedef struct {
    float ambient, diffuse, specular;
    int shininess_log2;
} vr_light;
int vr_set_light(const vr_light *l);
int vr_light_state(vr_light *out);

/* library version string */
const char *vr_version(void);

/* ---- value ranges and histograms of baked planes ----
 * What a window (transfer_offset / transfer_scale, v_offset / v_scale) and a table are
 * designed from: the value range of a resident baked plane, and the 1-D histogram of
 * one plane or the joint 2-D histogram of two planes of one volume, binned exactly
 * into the cells of the table a frame will use.  A method is whatever has a baked
 * plane: 1-6, 10-13 and VR_GRADIENT_OF(m); for method 13 the plane holds F and the
 * figures are those of F.  box: six ints x0, x1, y0, y1, z0, z1, the voxels
 * [x0, x1) x [y0, y1) x [z0, z1) of the plane's grid; NULL: the whole volume.
 *
 * The bin of plane value s under the window (offset, scale) of an axis of n entries,
 * float32, one operation at a time:
 *     x = (s - offset) * scale
 *     i = min((int)floorf(clamp01(x) * (float)n), n - 1)      clamp01(NaN) = 0
 * the texel cell [i / n, (i + 1) / n) of table entry i, around the coordinate
 * (i + 0.5) / n at which the table's linear filter returns entry i alone.  Values
 * outside the window land in the edge bins, as the table clamps them; a NaN lands in
 * bin 0.  counts[j * nu + i] (u fastest, the 2-D table's order) is the number of
 * voxels of the box with u bin i of nu and v bin j of nv; without a v plane
 * (method_v 0) nv is 1.  Every voxel of the box is counted once -- the copies and the
 * padding of the brick layout never -- so the counts sum to the box's voxels.  A
 * histogram counts voxels; a frame classifies samples interpolated between them.
 *
 * vr_plane_range: the minimum and maximum over the box's voxels that are not NaN and
 * the number that are (any of the three pointers may be NULL), ordered by bit pattern
 * so that -0 < +0; if every voxel is NaN, min and max are NaN (0x7FC00000).
 *
 * Both calls are synchronous on the library's stream, run one kernel (k_plane_range,
 * k_plane_hist), keep nothing on the device and change no state: tables, projection,
 * light and planes are as before.  VR_ERR_ARG: a method that names no plane; nu or
 * nv < 1 or nu * nv > VR_HIST_MAX; method_v 0 with nv != 1; a window that is not
 * finite; a box that is empty or leaves the grid; counts NULL.  VR_ERR_STATE: a plane
 * that is not resident (the message names its bake).  VR_ERR_UNSUPPORTED: u and v
 * planes of different volumes (record and codec), as the 2-D table refuses them, and
 * dimensions beyond 65535.  vr_plane_kernel_ms: the time of the last such kernel by
 * HIP events, for measurements. */
#define VR_HIST_MAX 16384
int vr_plane_range(int method, const int *box /* 6 ints or NULL */,
                   float *min, float *max, uint64_t *n_nan);
int vr_plane_histogram(int method_u, float u_offset, float u_scale, int nu,
                       int method_v /* 0: none */, float v_offset, float v_scale, int nv,
                       const int *box, uint64_t *counts /* host, nu * nv */);
int vr_plane_kernel_ms(float *ms);

/* ---- gradient-magnitude planes of baked planes ----
 * A boundary axis for frames from baked planes: |grad s| of a resident baked plane s,
 * baked once per voxel by central differences (one-sided on the volume's faces; an
 * axis of one voxel contributes 0) and then blended like any other statistic.  With
 * nx x ny x nz the plane's grid, float32, one operation at a time:
 *     xm = x > 0 ? x - 1 : 0      xp = x + 1 < nx ? x + 1 : nx - 1      (y, z alike)
 *     Gx = (s(xp, y, z) - s(xm, y, z)) * (xp - xm == 2 ? nx * 0.5f : nx)
 *     m  = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz)
 * in units of change per unit of the normalised coordinate x / nx (section 25's G).
 * For method 13 the plane holds F and the gradient is that of F.
 *
 * The gradient plane of source method m (1-6, 10-13) is query method
 * VR_GRADIENT_OF(m) = 32 + m.  vr_render / render_kernel serve it from its plane
 * wherever a baked plane is served: under the 1-D table, as u or as method_v of the
 * 2-D table, under a projection, under the light, and with none of these set through
 * the plane march with the built-in table, as a record query's plane.  It has no
 * per-step march: with its plane not resident every frame of it is
 * VR_ERR_UNSUPPORTED (vr_bake_gradient first), and vr_count_footprint /
 * vr_footprint_bytes of it always are.  GMM planes have no gradient planes:
 * vr_render_gmm_baked with a gradient method, as the frame's or as method_v, is
 * VR_ERR_UNSUPPORTED.
 *
 * vr_bake_gradient(m): VR_ERR_ARG for an m that is no source, VR_ERR_STATE if m's
 * plane is not resident (bake it first); nothing to do if the gradient plane is
 * there; dimensions beyond 65535 are VR_ERR_UNSUPPORTED.  Whatever frees or replaces
 * a source's plane -- vr_release_stats, the query's vr_release_* and setters, a new
 * volume, freeCudaBuffers -- frees its gradient plane first, so a plane that is there
 * was baked from the source that is there.  vr_release_gradient(m) frees the gradient
 * plane alone.  vr_gradient_info: the plane's device pointer (NULL: not baked), its
 * length in floats (the layout of the source's plane) and the largest magnitude of
 * the volume, e.g. for v_scale = 1 / max of a 2-D table. */
int vr_bake_gradient(int method);
int vr_release_gradient(int method);
int vr_gradient_info(int method, const float **d_plane, uint64_t *plane_floats, float *max);
#define VR_QUERY_GRADIENT 32
#define VR_GRADIENT_OF(m) (VR_QUERY_GRADIENT + (m))   /* m in 1..6, 10..13 */

#ifdef __cplusplus
}
#endif
#endif /* VR_H */
