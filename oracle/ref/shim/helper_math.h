/*
 * helper_math.h -- the vector operators the reference's two kernels use, as the
 * CUDA samples' header of this name defines them: component-wise float
 * arithmetic, dot products summed left to right, normalize through rsqrtf.
 * TEST INFRASTRUCTURE ONLY; our own text (see helper_cuda.h).
 */
#ifndef VR_REF_SHIM_HELPER_MATH_H
#define VR_REF_SHIM_HELPER_MATH_H

#include "helper_cuda.h"

static inline float3 make_float3(float s) { return float3{s, s, s}; }
static inline float3 make_float3(float4 a) { return float3{a.x, a.y, a.z}; }
static inline float4 make_float4(float s) { return float4{s, s, s, s}; }

static inline float3 operator+(float3 a, float3 b) { return float3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static inline float3 operator-(float3 a, float3 b) { return float3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline float3 operator*(float3 a, float3 b) { return float3{a.x * b.x, a.y * b.y, a.z * b.z}; }
static inline float3 operator/(float3 a, float3 b) { return float3{a.x / b.x, a.y / b.y, a.z / b.z}; }
static inline float3 operator*(float3 a, float b) { return float3{a.x * b, a.y * b, a.z * b}; }
static inline float3 operator*(float b, float3 a) { return float3{b * a.x, b * a.y, b * a.z}; }
static inline void operator+=(float3 &a, float3 b) {
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
}

static inline float4 operator+(float4 a, float4 b) {
    return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
static inline float4 operator*(float4 a, float b) { return float4{a.x * b, a.y * b, a.z * b, a.w * b}; }
static inline void operator*=(float4 &a, float b) {
    a.x *= b;
    a.y *= b;
    a.z *= b;
    a.w *= b;
}

static inline float dot(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline float dot(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

static inline float3 normalize(float3 v) {
    float invLen = rsqrtf(dot(v, v));
    return v * invLen;
}

static inline float3 fminf(float3 a, float3 b) {
    return float3{fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)};
}
static inline float3 fmaxf(float3 a, float3 b) {
    return float3{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)};
}

#endif
