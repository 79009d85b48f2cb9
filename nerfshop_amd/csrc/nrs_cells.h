// nrs_cells.h -- the 64-bit fixed-point cells that gradients and errors are summed in without a float atomic (the sum does not depend on the order of arrival), each
// rule stated ONCE for the kernels and for the host code behind the C-ABI: the SIGNED cell of the environment map and of per-image exposure (include/nrs.h, "the
// environment map", DEPOSIT), and the error map's UNSIGNED cell (include/nrs.h, "the training error map", deviation 1).  The two rules differ in their bits and stay
// apart; only the add is common.  Plain C++ with <math.h> only; every expression is float32 in the written order (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NRS_CELLS_FN __host__ __device__ __forceinline__
#else
#define NRS_CELLS_FN inline
#endif

namespace nrs {

// ---- the signed cell: 0 -- nothing to add -- unless finite and non-zero; clamped to +-512, scaled by 2^32 (exact), rounded to nearest even ----------------------
constexpr float kSignedCellClamp = 512.0f;       // 2^21 rays x 512 x 2^32 = 2^62: a cell never wraps
constexpr float kSignedCellScale = 4294967296.0f; // 2^32
NRS_CELLS_FN long long signed_cell_quantise(float p) {
	if (!(fabsf(p) <= 3.402823466e38f) || p == 0.0f) return 0ll; // NaN, +-inf, +-0
	return (long long)rintf(fminf(fmaxf(p, -kSignedCellClamp), kSignedCellClamp) * kSignedCellScale);
}
NRS_CELLS_FN float signed_cell_to_float(long long cell) { return (float)((double)cell * 0x1p-32); }
// a whole array, as a step reads it: the gradient the cells hold
inline void signed_cells_to_float(const int64_t* cells, size_t n, float* out) {
	for (size_t i = 0; i < n; ++i) out[i] = signed_cell_to_float((long long)cells[i]);
}

// ---- the error map's cell: 0 unless v > 0 (NaN too); clamped to 1024, scaled by 2^32 (exact), truncated; back through float32 ------------------------------------
NRS_CELLS_FN uint64_t error_cell_quantise(float v) { return v > 0.0f ? (uint64_t)(fminf(v, 1024.0f) * 4294967296.0f) : 0ull; }
NRS_CELLS_FN float error_cell_to_float(uint64_t cell) { return (float)cell * 0x1p-32f; }

#if defined(__HIPCC__)
// ---- the add, for both: it returns nothing; a deposit that quantises to zero is not sent -------------------------------------------------------------------------
template <class Cell>
__device__ __forceinline__ void cell_add(Cell* cell, Cell q) {
	static_assert(sizeof(Cell) == 8, "a 64-bit cell");
	(void)__hip_atomic_fetch_add(cell, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void signed_cell_deposit(unsigned long long* cell, float p) {
	const long long q = signed_cell_quantise(p);
	if (q) cell_add(cell, (unsigned long long)q);
}
__device__ __forceinline__ void error_cell_deposit(uint64_t* cell, float v) {
	const uint64_t q = error_cell_quantise(v);
	if (q) cell_add(cell, q);
}
#endif

} // namespace nrs
