// nrs_vec.cuh -- the three-float vector of the device code, its reductions in the reference's (Eigen's) order, the small scalar helpers,
// and the address-space casts of global and constant memory.
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_internal.h"

namespace nrs {

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk3(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 operator*(float s, f3 a) { return {s * a.x, s * a.y, s * a.z}; }
// Eigen evaluates fixed-size reductions (dot, squaredNorm, the inner sums of small matrix products) with its complete unroller
// (Eigen/src/Core/Redux.h, redux_novec_unroller: split at len / 2), so a 3-term sum is x0 + (x1 + x2), not (x0 + x1) + x2.
// The reference's own sources compiled against that model pin this (oracle/ref_render.cpp, tests/test_ref_pin.py).
__device__ __forceinline__ float sum3(float a, float b, float c) { return a + (b + c); }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return sum3(a.x * b.x, a.y * b.y, a.z * b.z); }
// M * v, M column-major 3x3 (Eigen's coefficient-based product: every row in the reduction order above)
__device__ __forceinline__ f3 mat3_mul(const float* M, f3 v) {
	return {sum3(M[0] * v.x, M[3] * v.y, M[6] * v.z), sum3(M[1] * v.x, M[4] * v.y, M[7] * v.z), sum3(M[2] * v.x, M[5] * v.y, M[8] * v.z)};
}
__device__ __forceinline__ f3 cross3(f3 a, f3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__device__ __forceinline__ bool box_contains(const Box3& b, f3 p) { // BoundingBox::contains, bounding_box.cuh:243
	return p.x >= b.mn[0] && p.x <= b.mx[0] && p.y >= b.mn[1] && p.y <= b.mx[1] && p.z >= b.mn[2] && p.z <= b.mx[2];
}

__device__ __forceinline__ float clampf_(float v, float lo, float hi) { return v < lo ? lo : (hi < v ? hi : v); }
__device__ __forceinline__ float signf_(float x) { return copysignf(1.0f, x); }
__device__ __forceinline__ int clampi_(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float fractf_(float x) { return x - floorf(x); }

#define NRS_GLOBAL __attribute__((address_space(1)))
#define NRS_CONSTANT __attribute__((address_space(4)))
// The operator tables are reached through pointers that sit in a device-memory struct (DeviceEdit): left alone, the compiler cannot tell their address
// space and emits FLAT loads (an aperture check per access, both wait counters) with one 64-bit address computation per dword.  They are global memory:
// gp() casts them so (global_load), and a vertex / matrix column is one 12-byte load.
template <typename T>
__device__ __forceinline__ const NRS_GLOBAL T* gp(const T* p) { return (const NRS_GLOBAL T*)p; }
__device__ __forceinline__ f3 ld3(const float* __restrict__ a, uint32_t i) {
	typedef float f3a __attribute__((ext_vector_type(3), aligned(4)));
	const f3a v = *(const NRS_GLOBAL f3a*)(gp(a) + 3 * (size_t)i);
	return {v.x, v.y, v.z};
}

} // namespace nrs
