/*
 * ref_driver.cpp -- runs the reference's d_basicDataProcessing and d_render on the
 * host, from the generated copy of the reference's kernel text that
 * oracle/ref/build_ref.py writes (VR_REF_KERNEL_TEXT) and the shim headers in
 * oracle/ref/shim/.  Called through ctypes (oracle/reference.py).
 *
 * TEST INFRASTRUCTURE ONLY.  Our own text; K:line cites volumeRender_kernel.cu,
 * C:line volumeRender.cpp.  The driver does what the reference's host code does
 * around the two kernels: it binds the arrays with the modes initCuda and
 * basicDataProcessing set, and plays the launches thread by thread.
 */
/* standard headers first: the shim renames log for the text that follows */
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include VR_REF_KERNEL_TEXT

thread_local uint3 threadIdx;
thread_local uint3 blockIdx;
thread_local dim3 blockDim;
thread_local float vr_shim_sat_out[4];
thread_local unsigned vr_shim_sat_calls;
int vr_shim_weight_trunc = 0;

namespace {

/* the reference's hard-coded volume (K:90, K:105, K:727-729) */
const int VX = 50, VY = 50, VZ = 10;

std::vector<VolumeType> g_index;
std::vector<float> g_hist, g_templates;
std::vector<int4> g_codebook;
std::vector<float2> g_errors;
std::vector<float4> g_flex;
float4 g_orig_query[nBlocks], g_fractal_query[nBlocks];

/* K:2323-2326 */
const float4 g_transfer[9] = {
    {0.0f, 0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f, 1.0f}, {1.0f, 0.5f, 0.0f, 1.0f},
    {1.0f, 1.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 1.0f, 1.0f},
    {0.0f, 0.0f, 1.0f, 1.0f}, {1.0f, 0.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f},
};

template <class Tex>
void modes(Tex &t, bool normalized, int filter) {
    t.normalized = normalized;
    t.filterMode = filter;
    t.addressMode[0] = t.addressMode[1] = cudaAddressModeClamp;
}

}  // namespace

extern "C" {

int ref_nbins(void) { return nBins; }

void ref_set_weight_trunc(int on) { vr_shim_weight_trunc = on; }

/* initCuda, K:1893-2358, for the arrays the two kernels read.
 * hist: nBlocks records of nBins floats (histogramSize = (nBins, 2500, 10), C:87);
 * codebook: nBlocks x (template id, shift, flip, NE); templates: ntemplates x nBins
 * (templatesSize = (nBins, T, 1), C:89); errors: nBlocks x err_slots (bin id, value)
 * pairs (errorsbookSize = (slots, 2500, 10), C:90).  codebook == NULL binds a
 * codec that decodes to all-zero records (template 0 of one zero template,
 * NE = 0), since d_basicDataProcessing always decodes. */
void ref_init(const float *hist, const int32_t *codebook, const float *templates,
              int ntemplates, const float *errors, int err_slots) {
    g_index.resize(nBlocks);
    for (int i = 0; i < nBlocks; i++) g_index[i] = (VolumeType)i; /* K:1903-1906 */
    g_hist.assign(hist, hist + (size_t)nBlocks * nBins);
    g_codebook.assign(nBlocks, int4{0, 0, 0, 0});
    if (codebook) {
        std::memcpy(g_codebook.data(), codebook, sizeof(int4) * nBlocks);
        g_templates.assign(templates, templates + (size_t)ntemplates * nBins);
        g_errors.resize((size_t)nBlocks * err_slots);
        if (err_slots) std::memcpy(g_errors.data(), errors, sizeof(float2) * g_errors.size());
    } else {
        ntemplates = 1;
        err_slots = 1;
        g_templates.assign(nBins, 0.0f);
        g_errors.assign(nBlocks, float2{0.0f, 0.0f});
    }
    if (err_slots < 1) { /* a texture has at least one texel; NE = 0 never reads it */
        err_slots = 1;
        g_errors.assign(nBlocks, float2{0.0f, 0.0f});
    }
    tex.bind(g_index.data(), VX, VY, VZ);
    modes(tex, true, cudaFilterModePoint); /* K:2161-2165 */
    histogramTex.bind(g_hist.data(), nBins, VX * VY, VZ);
    modes(histogramTex, false, cudaFilterModePoint); /* K:2168-2171 */
    codebookTex.bind(g_codebook.data(), VX, VY, VZ);
    modes(codebookTex, false, cudaFilterModePoint); /* K:2175-2178 */
    templatesTex.bind(g_templates.data(), nBins, ntemplates, 1);
    modes(templatesTex, false, cudaFilterModePoint); /* K:2181-2184 */
    errorsbookTex.bind(g_errors.data(), err_slots, VX * VY, VZ);
    modes(errorsbookTex, false, cudaFilterModePoint); /* K:2187-2190 */
    transferTex.bind(g_transfer, 9);
    modes(transferTex, true, cudaFilterModeLinear); /* K:2337-2339 */
}

/* basicDataProcessing, K:1798-1887: the launch of K:1799-1801, the two symbol
 * copies and the bindings of the query textures.  orig / fractal: nBlocks x 4
 * floats out (may be NULL). */
void ref_basic_data_processing(float *orig, float *fractal) {
    const dim3 bSize(5, 5, 5), tSize(10, 10, 2);
    blockDim = tSize;
    for (unsigned bz = 0; bz < bSize.z; bz++)
        for (unsigned by = 0; by < bSize.y; by++)
            for (unsigned bx = 0; bx < bSize.x; bx++)
                for (unsigned tz = 0; tz < tSize.z; tz++)
                    for (unsigned ty = 0; ty < tSize.y; ty++)
                        for (unsigned tx = 0; tx < tSize.x; tx++) {
                            blockIdx = uint3{bx, by, bz};
                            threadIdx = uint3{tx, ty, tz};
                            d_basicDataProcessing();
                        }
    std::memcpy(g_orig_query, originalHistogramData, sizeof(g_orig_query));   /* K:1805 */
    std::memcpy(g_fractal_query, fractalHistogramData, sizeof(g_fractal_query)); /* K:1807 */
    originalQueryTex.bind(g_orig_query, VX, VY, VZ);
    modes(originalQueryTex, true, cudaFilterModeLinear); /* K:1865-1869 */
    fractalQueryTex.bind(g_fractal_query, VX, VY, VZ);
    modes(fractalQueryTex, true, cudaFilterModeLinear); /* K:1872-1876 */
    if (orig) std::memcpy(orig, g_orig_query, sizeof(g_orig_query));
    if (fractal) std::memcpy(fractal, g_fractal_query, sizeof(g_fractal_query));
}

/* bindToTex, K:1572-1696, from a block table the caller computed: blocks is
 * nblk^3 float4 (mean, variance, entropy, 0), block (z * nblk + y) * nblk + x.
 * flexBlockTex addresses nMaxBlockDim^3 texels (K:102), zero outside the table
 * (K:1640-1647); only the table is stored. */
void ref_bind_flex(const float *blocks, int nblk) {
    g_flex.resize((size_t)nblk * nblk * nblk);
    std::memcpy(g_flex.data(), blocks, sizeof(float4) * g_flex.size());
    flexBlockTex.bind(g_flex.data(), nblk, nblk, nblk);
    flexBlockTex.width = flexBlockTex.height = flexBlockTex.depth = nMaxBlockDim;
    modes(flexBlockTex, false, cudaFilterModeLinear); /* K:1681-1686 */
    nFlexBlock = nblk * nblk * nblk;
    nFlexBlockX = nFlexBlockY = nFlexBlockZ = nblk;
}

/* copyInvViewMatrix, K:2403-2406 */
void ref_set_inv_view(const float *m12) { std::memcpy(&c_invViewMatrix, m12, sizeof(float) * 12); }

/* render_kernel, K:2387-2401, with the 16 x 16 blocks and the grid of C:122 /
 * C:145-148; d_output is prefilled by the caller (a miss writes nothing, K:302).
 * out_f (may be NULL): imageW * imageH * 4 floats, the saturated float RGBA that
 * rgbaFloatToInt packed for every pixel written (the shim's __saturatef keeps
 * them); pixels of rays that miss are left as they are. */
void ref_render(uint32_t *d_output, float *out_f, unsigned imageW, unsigned imageH, float density,
                float brightness, float transferOffset, float transferScale, int queryMethod,
                int vx, int vy, int vz) {
    const dim3 blockSize(16, 16);
    const dim3 gridSize((imageW + blockSize.x - 1) / blockSize.x,
                        (imageH + blockSize.y - 1) / blockSize.y);
    const int nblocks = (int)(gridSize.x * gridSize.y);
#pragma omp parallel for schedule(dynamic, 1)
    for (int b = 0; b < nblocks; b++) {
        blockDim = blockSize;
        blockIdx = uint3{(unsigned)b % gridSize.x, (unsigned)b / gridSize.x, 0};
        for (unsigned ty = 0; ty < blockSize.y; ty++)
            for (unsigned tx = 0; tx < blockSize.x; tx++) {
                threadIdx = uint3{tx, ty, 0};
                vr_shim_sat_calls = 0;
                d_render(d_output, imageW, imageH, density, brightness, transferOffset,
                         transferScale, queryMethod, make_int3(vx, vy, vz), flexBlockSurfObj);
                const unsigned x = blockIdx.x * blockSize.x + tx, y = blockIdx.y * blockSize.y + ty;
                if (out_f && vr_shim_sat_calls == 4 && x < imageW && y < imageH)
                    std::memcpy(out_f + ((size_t)y * imageW + x) * 4, vr_shim_sat_out,
                                sizeof(vr_shim_sat_out));
            }
    }
}

}  // extern "C"

#ifdef VR_REF_SELFCHECK_MAIN
/* Stand-alone run for host sanitizers (python oracle/ref/build_ref.py --selfcheck
 * builds this with -fsanitize=address,undefined and runs it): random records and
 * codec entries within the decode's documented ranges, both pre-pass planes,
 * then one small frame of every method on an oblique and an inside-the-box view. */
int main() {
    std::mt19937 rng(20261015u);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const int T = 7, slots = nBins;
    std::vector<float> hist((size_t)nBlocks * nBins), tpl((size_t)T * nBins);
    std::vector<int32_t> cb((size_t)nBlocks * 4);
    std::vector<float> err((size_t)nBlocks * slots * 2);
    for (auto &v : hist) v = uni(rng) / nBins;
    for (auto &v : tpl) v = uni(rng) / nBins;
    for (int i = 0; i < nBlocks; i++) {
        cb[4 * i + 0] = (int)(rng() % T);
        cb[4 * i + 1] = (int)(rng() % nBins);
        cb[4 * i + 2] = (int)(rng() % 2);
        cb[4 * i + 3] = (int)(rng() % (slots + 1));
        for (int s = 0; s < slots; s++) {
            err[((size_t)i * slots + s) * 2] = (float)(rng() % nBins);
            err[((size_t)i * slots + s) * 2 + 1] = (uni(rng) - 0.5f) * 0.1f;
        }
    }
    ref_init(hist.data(), cb.data(), tpl.data(), T, err.data(), slots);
    ref_basic_data_processing(nullptr, nullptr);
    std::vector<float> blocks(4 * 4 * 4 * 4);
    for (auto &v : blocks) v = uni(rng);
    ref_bind_flex(blocks.data(), 4);
    const float views[2][12] = {
        {0.70710677f, 0.0f, -0.70710677f, -2.828427f, -0.35355338f, 0.8660254f, -0.35355338f,
         -1.4142135f, 0.61237246f, 0.5f, 0.61237246f, 2.4494898f},
        {1.0f, 0.0f, 0.0f, 0.1f, 0.0f, 1.0f, 0.0f, -0.2f, 0.0f, 0.0f, 1.0f, 0.5f}};
    const int W = 40, H = 24, methods[] = {1, 2, 3, 7, 4, 5, 6, 8, 9, 0};
    std::vector<uint32_t> out((size_t)W * H);
    std::vector<float> out_f((size_t)W * H * 4);
    unsigned long long sum = 0;
    for (auto &view : views) {
        ref_set_inv_view(view);
        for (int m : methods) {
            ref_render(out.data(), out_f.data(), W, H, 0.5f, 1.0f, 0.1f, 4.0f, m, 20, 30, 7);
            for (uint32_t p : out) sum += p;
        }
    }
    std::printf("ref selfcheck: %d bins, 20 frames rendered, checksum %llu\n", nBins, sum);
    return 0;
}
#endif
