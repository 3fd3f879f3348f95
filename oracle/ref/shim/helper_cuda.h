/*
 * helper_cuda.h -- host stand-in for the CUDA names the reference's two kernels
 * (d_render, d_basicDataProcessing) and their helpers use, so that the text of
 * those kernels compiles as plain host C++ (oracle/ref/build_ref.py).
 *
 * TEST INFRASTRUCTURE ONLY.  Our own text: nothing here is taken from the CUDA
 * toolkit or from the reference.  The texture fetches are written from the CUDA
 * C programming guide's "Texture Fetching" appendix.
 *
 * Readings this shim has to choose where the guide or the hardware leave the
 * arithmetic open.  They are the canonical readings of oracle/vr_oracle.c:
 *   - rsqrtf(x) is 1.0f / sqrtf(x);
 *   - the float overload log(float) is (float)log((double)x);
 *   - linear-filter weights are held with 8 fractional bits, rounded to
 *     nearest (vr_shim_weight_trunc != 0: truncated, a wrong-on-purpose
 *     reading for the canary of tests/test_reference_text.py);
 *   - a linear fetch blends (1 - a) * T0 + a * T1 along x, then y, then z, in
 *     float (the appendix gives the blend as one sum of products and does not
 *     fix an order);
 *   - a NaN coordinate fetches as coordinate 0.
 */
#ifndef VR_REF_SHIM_HELPER_CUDA_H
#define VR_REF_SHIM_HELPER_CUDA_H

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#define __global__
#define __device__
#define __host__
#define __constant__

/* ---- vector types ---- */
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };

static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline float4 make_float4(float x, float y, float z, float w) {
    return float4{x, y, z, w};
}

struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

/* one host thread plays one CUDA thread at a time */
extern thread_local uint3 threadIdx;
extern thread_local uint3 blockIdx;
extern thread_local dim3 blockDim;

/* ---- runtime types the text names but the two kernels never touch ---- */
struct cudaArray;
typedef unsigned long long cudaTextureObject_t;
typedef unsigned long long cudaSurfaceObject_t;

struct cudaExtent { size_t width, height, depth; };
static inline cudaExtent make_cudaExtent(size_t w, size_t h, size_t d) {
    return cudaExtent{w, h, d};
}

/* ---- intrinsics ---- */
/* __saturatef also keeps its last four results, in call order: rgbaFloatToInt
 * saturates sum.x, .y, .z, .w and packs them, so after a d_render call that
 * wrote a pixel they are the float frame the reference computes and never
 * stores.  Storing a value is no arithmetic: the kernel's results are untouched. */
extern thread_local float vr_shim_sat_out[4];
extern thread_local unsigned vr_shim_sat_calls;
static inline float __saturatef(float x) {
    float r = !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); /* NaN -> 0 */
    vr_shim_sat_out[vr_shim_sat_calls++ & 3u] = r;
    return r;
}
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }

/* log: the float overload under the canonical reading; the double one is libm's */
static inline float vr_shim_log(float x) { return (float)::log((double)x); }
static inline double vr_shim_log(double x) { return ::log(x); }
#define log vr_shim_log

/* ---- textures ---- */
enum cudaTextureReadMode { cudaReadModeElementType = 0, cudaReadModeNormalizedFloat = 1 };
enum cudaTextureFilterMode { cudaFilterModePoint = 0, cudaFilterModeLinear = 1 };
enum cudaTextureAddressMode { cudaAddressModeWrap = 0, cudaAddressModeClamp = 1 };
#define cudaTextureType1D 0x01
#define cudaTextureType2D 0x02
#define cudaTextureType3D 0x03
#define cudaTextureType2DLayered 0xF2

/* A texture reference bound to a host array.  width/height/depth are the
 * extents the fetch addresses (depth = layers of a layered texture); the array
 * itself holds only [0, bw) x [0, bh) x [0, bd) of them, x fastest, and every
 * texel outside that reads as zero (bw = width etc. for an ordinary binding). */
template <class T, int dim = cudaTextureType1D, int mode = cudaReadModeElementType>
struct texture {
    const T *data = nullptr;
    int width = 0, height = 1, depth = 1;
    int bw = 0, bh = 1, bd = 1;
    int normalized = 0;
    int filterMode = cudaFilterModePoint;
    int addressMode[3] = {cudaAddressModeClamp, cudaAddressModeClamp, cudaAddressModeClamp};

    void bind(const T *p, int w, int h = 1, int d = 1) {
        data = p;
        width = bw = w;
        height = bh = h;
        depth = bd = d;
    }
    T texel(int i, int j, int k) const {
        if (i >= bw || j >= bh || k >= bd) return T{};
        return data[((size_t)k * (size_t)bh + (size_t)j) * (size_t)bw + (size_t)i];
    }
};

extern int vr_shim_weight_trunc;

/* texel-space coordinate of one axis: x = N * u for a normalised texture */
static inline float vr_shim_texel_space(float u, int n, int normalized) {
    return normalized ? u * (float)n : u;
}

static inline int vr_shim_clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

/* point filter, clamp: texel floor(x), out-of-range coordinates to the edge */
static inline int vr_shim_point(float u, int n, int normalized) {
    float x = vr_shim_texel_space(u, n, normalized);
    if (!(x > 0.0f)) return 0; /* also NaN */
    if (x >= (float)n) return n - 1;
    return vr_shim_clampi((int)floorf(x), n);
}

/* linear filter, clamp: xB = x - 0.5, i = floor(xB), a = frac(xB) in 1.8 fixed
 * point; texels i and i + 1, each clamped to the edge */
static inline void vr_shim_linear(float u, int n, int normalized, int *i0, int *i1, float *a) {
    float x = vr_shim_texel_space(u, n, normalized);
    if (!(x > 0.0f)) x = 0.0f; /* clamp addressing; also NaN */
    if (x > (float)n) x = (float)n;
    float xb = x - 0.5f;
    float fl = floorf(xb);
    float fr = xb - fl;
    float q = vr_shim_weight_trunc ? floorf(fr * 256.0f) : nearbyintf(fr * 256.0f);
    *a = q / 256.0f;
    *i0 = vr_shim_clampi((int)fl, n);
    *i1 = vr_shim_clampi((int)fl + 1, n);
}

static inline float vr_shim_mix(float t0, float t1, float a) { return (1.0f - a) * t0 + a * t1; }
static inline float4 vr_shim_mix(float4 t0, float4 t1, float a) {
    return float4{vr_shim_mix(t0.x, t1.x, a), vr_shim_mix(t0.y, t1.y, a),
                  vr_shim_mix(t0.z, t1.z, a), vr_shim_mix(t0.w, t1.w, a)};
}
/* integer texels are never fetched with a linear filter */
template <class T> static inline T vr_shim_mix(T t0, T, float) { return t0; }

template <class T, int dim, int mode>
static inline T tex1D(const texture<T, dim, mode> &t, float x) {
    if (t.filterMode == cudaFilterModePoint)
        return t.texel(vr_shim_point(x, t.width, t.normalized), 0, 0);
    int i0, i1;
    float a;
    vr_shim_linear(x, t.width, t.normalized, &i0, &i1, &a);
    return vr_shim_mix(t.texel(i0, 0, 0), t.texel(i1, 0, 0), a);
}

template <class T, int dim, int mode>
static inline T tex3D(const texture<T, dim, mode> &t, float x, float y, float z) {
    if (t.filterMode == cudaFilterModePoint)
        return t.texel(vr_shim_point(x, t.width, t.normalized),
                       vr_shim_point(y, t.height, t.normalized),
                       vr_shim_point(z, t.depth, t.normalized));
    int i0, i1, j0, j1, k0, k1;
    float a, b, c;
    vr_shim_linear(x, t.width, t.normalized, &i0, &i1, &a);
    vr_shim_linear(y, t.height, t.normalized, &j0, &j1, &b);
    vr_shim_linear(z, t.depth, t.normalized, &k0, &k1, &c);
    T r00 = vr_shim_mix(t.texel(i0, j0, k0), t.texel(i1, j0, k0), a);
    T r10 = vr_shim_mix(t.texel(i0, j1, k0), t.texel(i1, j1, k0), a);
    T r01 = vr_shim_mix(t.texel(i0, j0, k1), t.texel(i1, j0, k1), a);
    T r11 = vr_shim_mix(t.texel(i0, j1, k1), t.texel(i1, j1, k1), a);
    return vr_shim_mix(vr_shim_mix(r00, r10, b), vr_shim_mix(r01, r11, b), c);
}

/* layered: x, y filtered within the layer, the layer an integer clamped to range */
template <class T, int dim, int mode>
static inline T tex2DLayered(const texture<T, dim, mode> &t, float x, float y, int layer) {
    int k = vr_shim_clampi(layer, t.depth);
    if (t.filterMode == cudaFilterModePoint)
        return t.texel(vr_shim_point(x, t.width, t.normalized),
                       vr_shim_point(y, t.height, t.normalized), k);
    int i0, i1, j0, j1;
    float a, b;
    vr_shim_linear(x, t.width, t.normalized, &i0, &i1, &a);
    vr_shim_linear(y, t.height, t.normalized, &j0, &j1, &b);
    T r0 = vr_shim_mix(t.texel(i0, j0, k), t.texel(i1, j0, k), a);
    T r1 = vr_shim_mix(t.texel(i0, j1, k), t.texel(i1, j1, k), a);
    return vr_shim_mix(r0, r1, b);
}

#endif
