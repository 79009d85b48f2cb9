// nrs_occupancy.hip -- the occupancy grid on the device (gfx950, wave64).
//
//   grid -> bitfield     update_density_grid_mean_and_bitfield.
//   occ_accel_*          the marching accelerator (OccAccel) derived from the bitfield.
//   grid_refresh / grid_ema   the deformed-space occupancy refresh: the operators, hash grid + density MLP on MFMA, max-splat.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_launch.h"
#include "nrs_occupancy.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"
#include "nrs_edit_warp.cuh"
#include "nrs_shade.cuh"
#include "nrs_hashgrid.cuh"
#include "nrs_mlp.cuh"

namespace nrs {

// ---- density grid -> bitfield (tn:514-555, 3642-3657) ----------------------------------------------------------------------
// mean of max(v, 0) / n over cascade 0 (tn:3650), in double, in a fixed two-stage order: deterministic.
constexpr uint32_t kMeanBlocks = 256;
__global__ __launch_bounds__(256) void grid_mean_partial_kernel(const float* __restrict__ grid, double* __restrict__ partial) {
	__shared__ double part[256];
	double acc = 0.0;
	const uint32_t per = kGridVol / kMeanBlocks; // 8192 contiguous cells per block
	const float* g = grid + (size_t)blockIdx.x * per;
	for (uint32_t i = threadIdx.x; i < per; i += 256) acc += (double)(fmaxf(g[i], 0.f) / (float)kGridVol);
	part[threadIdx.x] = acc;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}
__global__ __launch_bounds__(256) void grid_mean_final_kernel(const double* __restrict__ partial, float* __restrict__ mean_out) {
	__shared__ double part[256];
	part[threadIdx.x] = partial[threadIdx.x];
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0) mean_out[0] = (float)part[0];
}
__global__ void grid_to_bitfield_kernel(uint32_t n_elements, const float* __restrict__ grid, uint8_t* __restrict__ bitfield, const float* __restrict__ mean) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	const float thresh = fminf(0.01f, *mean); // NERF_MIN_OPTICAL_THICKNESS
	uint8_t bits = 0;
	#pragma unroll
	for (uint32_t j = 0; j < 8; ++j) bits |= grid[(size_t)i * 8 + j] > thresh ? (uint8_t)(1u << j) : 0;
	bitfield[i] = bits;
}
__global__ void bitfield_max_pool_kernel(uint32_t n_elements, const uint8_t* __restrict__ prev_level, uint8_t* __restrict__ next_level) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	uint8_t bits = 0;
	#pragma unroll
	for (uint32_t j = 0; j < 8; ++j) bits |= prev_level[i * 8 + j] > 0 ? (uint8_t)(1u << j) : 0;
	const uint32_t x = morton3D_invert(i >> 0) + kGrid / 8, y = morton3D_invert(i >> 1) + kGrid / 8, z = morton3D_invert(i >> 2) + kGrid / 8;
	next_level[morton3D(x, y, z)] |= bits;
}

int launch_grid_to_bitfield(const float* d_grid, uint8_t* d_bitfield, float* d_scratch_mean, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	// d_scratch_mean: [0] the mean (float), [2..] kMeanBlocks doubles of partial sums
	double* partial = reinterpret_cast<double*>(d_scratch_mean + 2);
	hipLaunchKernelGGL(grid_mean_partial_kernel, dim3(kMeanBlocks), dim3(256), 0, s, d_grid, partial);
	hipLaunchKernelGGL(grid_mean_final_kernel, dim3(1), dim3(256), 0, s, partial, d_scratch_mean);
	const uint32_t n = kGridVol / 8 * kCascades;
	hipLaunchKernelGGL(grid_to_bitfield_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, d_grid, d_bitfield, d_scratch_mean);
	for (uint32_t level = 1; level < kCascades; ++level) {
		const uint32_t ne = kGridVol / 64;
		hipLaunchKernelGGL(bitfield_max_pool_kernel, dim3((ne + 255) / 256), dim3(256), 0, s, ne, d_bitfield + (size_t)(level - 1) * kGridVol / 8,
		                   d_bitfield + (size_t)level * kGridVol / 8);
	}
	NRS_LAUNCH_CHECK("grid_to_bitfield launch");
	return NRS_OK;
}

// ---- the marching accelerator (OccAccel) from the bitfield, on the device --------------------------------------------------
// Two flavours at once (slot 0: any step parameters; slot 1: cone_angle == 0 && min_mip == 0, where a cell of cascade L >= 1 can only
// be consulted from the shell 2^(L-2) <= max|pos - 0.5| (cn:163-168), so blocks that lie inside that shell's hole are ignored: this is
// what keeps the OR-pooled coarse cascades of an aabb_scale-1 scene from blowing box and mask up to their resolution).
// One thread per 8 bytes of the bitfield = 8 Morton 2x2x2 blocks; a block's world bounds, inflated by 1/16 cell of its cascade, feed
//   pass 1: min / max per axis (wave reduction, then atomicMin / atomicMax on order-preserving integer keys: exact, order-independent),
//   pass 2: box, cell and 1 / cell of the kCoarse^3 look-ahead mask (one thread; the host downloads exactly these numbers),
//   pass 3: the mask bits every relevant block's extent overlaps (atomicOr, skipped when the bit is already visible).
struct OccAccelOut { float mn[3], mx[3], cell[3], inv_cell[3]; };
__device__ __forceinline__ uint32_t float_key(float f) { const uint32_t u = __float_as_uint(f); return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ bool accel_block_relevant(uint32_t level, const uint32_t c[3], float s, float margin) {
	if (level == 0) return true;
	float far = 0.f;
	for (int k = 0; k < 3; ++k) {
		const float a = ((float)c[k] / (float)kGrid - 0.5f) * s - margin, b = ((float)(c[k] + 2u) / (float)kGrid - 0.5f) * s + margin; // pos - 0.5
		far = fmaxf(far, fmaxf(fabsf(a), fabsf(b)));
	}
	return far >= ldexpf(1.0f, (int)level - 2);
}
__global__ void __launch_bounds__(256) occ_accel_bounds_kernel(const uint64_t* __restrict__ bitfield, uint32_t* __restrict__ keys) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x; // kCascades * kGridVol / 64 words exactly
	const uint64_t w = bitfield[i];
	const float inf = __builtin_huge_valf();
	float mn[2][3] = {{inf, inf, inf}, {inf, inf, inf}}, mx[2][3] = {{-inf, -inf, -inf}, {-inf, -inf, -inf}};
	if (w) {
		const uint32_t level = i / (kGridVol / 64), byte0 = (i % (kGridVol / 64)) * 8;
		const float s = ldexpf(1.0f, (int)level), margin = s / (float)kGrid / 16.f;
		for (uint32_t j = 0; j < 8; ++j) {
			if (!((w >> (8 * j)) & 0xffu)) continue;
			const uint32_t m = (byte0 + j) * 8;
			const uint32_t c[3] = {morton3D_invert(m), morton3D_invert(m >> 1), morton3D_invert(m >> 2)};
			const bool exact = accel_block_relevant(level, c, s, margin);
			for (int k = 0; k < 3; ++k) {
				const float lo = ((float)c[k] / (float)kGrid - 0.5f) * s + 0.5f - margin, hi = ((float)(c[k] + 2u) / (float)kGrid - 0.5f) * s + 0.5f + margin;
				mn[0][k] = fminf(mn[0][k], lo); mx[0][k] = fmaxf(mx[0][k], hi);
				if (exact) { mn[1][k] = fminf(mn[1][k], lo); mx[1][k] = fmaxf(mx[1][k], hi); }
			}
		}
	}
	if (!__ballot(w != 0)) return;
	for (int f = 0; f < 2; ++f)
		for (int k = 0; k < 3; ++k) {
			float a = mn[f][k], b = mx[f][k];
			for (int o = 32; o; o >>= 1) { a = fminf(a, __shfl_xor(a, o)); b = fmaxf(b, __shfl_xor(b, o)); }
			if ((threadIdx.x & 63) == 0) {
				if (a < inf) atomicMin(&keys[f * 6 + k], float_key(a));
				if (b > -inf) atomicMax(&keys[f * 6 + 3 + k], float_key(b));
			}
		}
}
__global__ void occ_accel_box_kernel(const uint32_t* __restrict__ keys, OccAccelOut* __restrict__ out) {
	const uint32_t f = threadIdx.x;
	if (f >= 2) return;
	const float inf = __builtin_huge_valf();
	OccAccelOut o;
	const bool any = keys[f * 6] != 0xffffffffu; // the keys start at (0xffffffff, 0): untouched = nothing occupied
	for (int k = 0; k < 3; ++k) {
		o.mn[k] = any ? key_float(keys[f * 6 + k]) : inf;
		o.mx[k] = any ? key_float(keys[f * 6 + 3 + k]) : -inf;
		o.cell[k] = any ? (o.mx[k] - o.mn[k]) / (float)kCoarse : 1.f;
		o.inv_cell[k] = any ? 1.0f / o.cell[k] : 1.f;
	}
	out[f] = o;
}
constexpr uint32_t kAccelMaskBlocks = 160, kAccelWordsPerThread = kCascades * (kGridVol / 64) / (kAccelMaskBlocks * 256);
static_assert(kAccelMaskBlocks * 256 * kAccelWordsPerThread == kCascades * (kGridVol / 64), "the mask pass covers the bitfield exactly");
// A workgroup owns a contiguous (Morton-compact) run of the bitfield, collects its bits in LDS and merges the non-zero words at the end.
__global__ void __launch_bounds__(256) occ_accel_mask_kernel(const uint64_t* __restrict__ bitfield, const OccAccelOut* __restrict__ acc, uint32_t* __restrict__ masks) {
	__shared__ uint32_t lmask[2 * kCoarseWords];
	for (uint32_t j = threadIdx.x; j < 2 * kCoarseWords; j += 256) lmask[j] = 0u;
	__syncthreads();
	const OccAccelOut a0 = acc[0], a1 = acc[1];
	for (uint32_t r = 0; r < kAccelWordsPerThread; ++r) {
		const uint32_t i = (blockIdx.x * kAccelWordsPerThread + r) * 256 + threadIdx.x;
		const uint64_t w = bitfield[i];
		if (!w) continue;
		const uint32_t level = i / (kGridVol / 64), byte0 = (i % (kGridVol / 64)) * 8;
		const float s = ldexpf(1.0f, (int)level), margin = s / (float)kGrid / 16.f;
		for (uint32_t j = 0; j < 8; ++j) {
			if (!((w >> (8 * j)) & 0xffu)) continue;
			const uint32_t m = (byte0 + j) * 8;
			const uint32_t c[3] = {morton3D_invert(m), morton3D_invert(m >> 1), morton3D_invert(m >> 2)};
			const bool exact = accel_block_relevant(level, c, s, margin);
			for (int f = 0; f < (exact ? 2 : 1); ++f) {
				const OccAccelOut& a = f ? a1 : a0;
				int lo[3], hi[3];
				for (int k = 0; k < 3; ++k) {
					const float wmin = ((float)c[k] / (float)kGrid - 0.5f) * s + 0.5f - margin, wmax = ((float)(c[k] + 2u) / (float)kGrid - 0.5f) * s + 0.5f + margin;
					lo[k] = min((int)kCoarse - 1, max(0, (int)floorf((wmin - a.mn[k]) * a.inv_cell[k])));
					hi[k] = min((int)kCoarse - 1, max(0, (int)floorf((wmax - a.mn[k]) * a.inv_cell[k])));
				}
				uint32_t* mask = lmask + f * kCoarseWords;
				static_assert(kCoarse == 32, "one mask word = one row of blocks along x");
				const uint32_t row = (0xffffffffu >> (31 - hi[0])) & (0xffffffffu << lo[0]);
				for (int z = lo[2]; z <= hi[2]; ++z)
					for (int y = lo[1]; y <= hi[1]; ++y) {
						const uint32_t word = (uint32_t)z * kCoarse + (uint32_t)y;
						if ((mask[word] & row) != row) atomicOr(&mask[word], row);
					}
			}
		}
	}
	__syncthreads();
	for (uint32_t j = threadIdx.x; j < 2 * kCoarseWords; j += 256)
		if (lmask[j]) atomicOr(&masks[j], lmask[j]);
}
// d_masks: 2 x kCoarseWords words; d_out: 2 x 12 floats (OccAccelOut of slot 0 / slot 1); d_keys: 12 words of scratch
int launch_occ_accel(const uint8_t* d_bitfield, uint32_t* d_masks, float* d_out, uint32_t* d_keys, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	static const uint32_t init_keys[12] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
	hipError_t e = hipMemcpyAsync(d_keys, init_keys, sizeof(init_keys), hipMemcpyHostToDevice, s);
	if (e == hipSuccess) e = hipMemsetAsync(d_masks, 0, 2 * kCoarseWords * 4, s);
	if (e != hipSuccess) return hip_fail(e, "occ_accel: clear");
	const uint32_t n_words = kCascades * (kGridVol / 64);
	static_assert(kCascades * (kGridVol / 64) % 256 == 0, "one thread per bitfield word, no tail");
	hipLaunchKernelGGL(occ_accel_bounds_kernel, dim3(n_words / 256), dim3(256), 0, s, (const uint64_t*)d_bitfield, d_keys);
	hipLaunchKernelGGL(occ_accel_box_kernel, dim3(1), dim3(64), 0, s, d_keys, (OccAccelOut*)d_out);
	hipLaunchKernelGGL(occ_accel_mask_kernel, dim3(kAccelMaskBlocks), dim3(256), 0, s, (const uint64_t*)d_bitfield, (const OccAccelOut*)d_out, d_masks);
	NRS_LAUNCH_CHECK("occ_accel launch");
	return NRS_OK;
}

// ---- deformed-space occupancy refresh (update_density_grid_nerf_operator, tn:3533-3640) ----------------------------------
// One fused kernel replaces the reference's generate x2 -> map_positions per operator -> density() -> clear_empty_space ->
// activate -> residual -> splat train and its four scratch arrays (positions, indices, mlp_out, empty mask): each lane draws
// its cell sample, walks it through the operators, the wave evaluates hash grid + density MLP on MFMA, and the lane
// max-splats the optical thickness into grid_tmp.  atomicMax on the bit pattern is order-independent => deterministic.
struct GridUpdateArgs {
	const float* grid;        // current density grid (read by the sampler)
	uint32_t* grid_tmp;       // zeroed; float bits
	const DeviceEdit* edits;
	int32_t n_edits;
	uint32_t n_uniform, n_nonuniform, step, n_cascades;
	uint64_t rng_state, rng_inc, rng_state_nonuniform;
	uint32_t cell_order; // walk the cells in Morton order (see grid_refresh_kernel); 0 = sample order (NRS_REFRESH_ORDER=0, for A/B measurements)
};

// Sample order.  The reference draws sample i in cell (i * 56924617 + 96925573) mod 2^21 of a random cascade (common_nerf.cu:189-195): consecutive
// samples land in cells scattered over the whole grid, so every gather of a wave is its own cache line.  The map i -> cell is a bijection of
// [0, 2^21) (the multiplier is odd), and the sample count is a multiple of 2^21 (128^3 per cascade): so the wave walks the CELLS in Morton order --
// 64 neighbouring cells = a 4 x 4 x 4 block of the grid, whose samples share the coarse levels' lines -- and recovers from each cell the sample
// index i (and with it the sample's own random numbers) by inverting the map: i = Kinv * (cell - 96925573) mod 2^21 (+ k * 2^21 for the k-th block
// of 2^21 samples).  Every sample is still evaluated exactly once with exactly its numbers; the max-splat is order-independent: bit-identical.
// pcg32.advance(4 i) per lane, without a 64-step skip loop per lane: i(cell0 + l) = i(cell0) + l * Kinv - w * 2^21 (w = wraps of the sum past 2^21),
// and LCG skips compose, so state = WrapSkip[w] o LaneSkip[l] o Skip(4 i(cell0) + 4 k 2^21): a wave-uniform skip on the scalar unit, a per-lane
// skip whose coefficients are computed once, and a 65-entry table of "minus w * 2^23 steps" in LDS.
constexpr uint32_t kSampleMul = 56924617u, kSampleAdd = 96925573u;
__host__ __device__ constexpr uint32_t inverse_mod_2_32(uint32_t k) { // Newton: x <- x (2 - k x) doubles the number of correct low bits
	uint32_t x = k;
	for (int i = 0; i < 5; ++i) x *= 2u - k * x;
	return x;
}
constexpr uint32_t kSampleMulInv = inverse_mod_2_32(kSampleMul) & (kGridVol - 1u);
static_assert(((kSampleMul * kSampleMulInv) & (kGridVol - 1u)) == 1u, "inverse of the sample multiplier mod 2^21");

// generate_grid_samples_nerf_nonuniform, cn:179-208: cell index + a uniformly random warped position inside that cell
// `rng` arrives already advanced by 4 * i (the kernel splits that skip into a wave-uniform and a per-lane part).
__device__ __forceinline__ uint32_t generate_grid_sample(Pcg32 rng, uint32_t i, uint32_t n_elements, uint32_t step, const Box3& aabb,
                                                         const float* __restrict__ grid_in, uint32_t n_cascades, float thresh, f3& wpos) {
	const uint32_t level = (uint32_t)(rng.next_float() * n_cascades) % n_cascades;
	uint32_t idx = 0;
	#pragma unroll 1
	for (uint32_t j = 0; j < 10; ++j) {
		idx = ((i + step * n_elements) * 56924617u + j * 19349663u + 96925573u) % kGridVol;
		idx += level * kGridVol;
		if (grid_in[idx] > thresh) break;
	}
	const uint32_t pos_idx = idx % kGridVol;
	const float x = (float)morton3D_invert(pos_idx >> 0), y = (float)morton3D_invert(pos_idx >> 1), z = (float)morton3D_invert(pos_idx >> 2);
	const float rx = rng.next_float(), ry = rng.next_float(), rz = rng.next_float();
	const float s = __uint_as_float((127u + level) << 23); // scalbnf(1, level)
	const float inv = 1.0f / (float)kGrid;                  // exact: x / 128 == x * 2^-7
	const f3 pos = {((x + rx) * inv - 0.5f) * s + 0.5f, ((y + ry) * inv - 0.5f) * s + 0.5f, ((z + rz) * inv - 0.5f) * s + 0.5f};
	wpos = warp_position(pos, aabb);
	return idx;
}

template <int NUM>
__global__ __launch_bounds__(256) void grid_refresh_kernel(const DeviceModel m, const GridUpdateArgs a) {
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	__shared__ NetSmem sm;
	__shared__ uint64_t wrap_mult[65], wrap_plus[65];
	if (threadIdx.x < 65) Pcg32::skip_coefficients(a.rng_inc, 0ull - ((uint64_t)threadIdx.x << 23), wrap_mult[threadIdx.x], wrap_plus[threadIdx.x]);
	stage_model_to_lds(m, sm.ml);
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	uint64_t lane_mult, lane_plus, mlane_mult, mlane_plus;
	Pcg32::skip_coefficients(a.rng_inc, (uint64_t)(4 * lane), lane_mult, lane_plus);
	Pcg32::skip_coefficients(a.rng_inc, 4ull * (uint64_t)lane * (uint64_t)kSampleMulInv, mlane_mult, mlane_plus);
	const bool morton = a.cell_order && (a.n_uniform & (kGridVol - 1u)) == 0u; // whole blocks of 2^21 samples: always so for update_density_grid_nerf_render
	const uint32_t n = a.n_uniform + a.n_nonuniform;
	const uint32_t n_tiles = (n + 63) / 64;
	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < n;
		f3 wpos = mk3(0, 0, 0);
		uint32_t cell = 0;
		if (have) {
			const uint32_t t0 = tile * 64, t1 = t0 + 63;
			const bool uni = s < a.n_uniform;
			uint32_t i = uni ? s : s - a.n_uniform;
			Pcg32 rng{uni ? a.rng_state : a.rng_state_nonuniform, a.rng_inc};
			if (morton && t1 < a.n_uniform) {
				// cells c0 .. c0 + 63 of block k; (i + step * n) * K + C = cell (mod 2^21) with step * n = 0 (mod 2^21)
				const uint32_t k = t0 >> 21, c0 = t0 & (kGridVol - 1u);
				const uint32_t i_first = ((c0 - kSampleAdd) * kSampleMulInv) & (kGridVol - 1u);
				const uint32_t sum = i_first + (uint32_t)lane * kSampleMulInv; // < 65 * 2^21
				const uint32_t w = sum >> 21;
				i = (sum & (kGridVol - 1u)) + (k << 21);
				uint64_t mt, pt;
				Pcg32::skip_coefficients(a.rng_inc, 4ull * (uint64_t)i_first + ((uint64_t)k << 23), mt, pt);
				const uint64_t st = mlane_mult * (mt * rng.state + pt) + mlane_plus;
				rng.state = wrap_mult[w] * st + wrap_plus[w];
			} else if ((t0 < a.n_uniform) == (t1 < a.n_uniform)) {
				// rng.advance(4 * i) as a wave-uniform skip to the tile's first sample (scalar unit) and the per-lane skip by 4 * lane
				const uint32_t i0 = (t0 < a.n_uniform) ? t0 : t0 - a.n_uniform;
				uint64_t mt, pt;
				Pcg32::skip_coefficients(a.rng_inc, (uint64_t)(i0 * 4u), mt, pt);
				rng.state = lane_mult * (mt * rng.state + pt) + lane_plus;
			} else {
				rng.advance((uint64_t)(i * 4u));
			}
			cell = generate_grid_sample(rng, i, uni ? a.n_uniform : a.n_nonuniform, a.step, m.aabb, a.grid, a.n_cascades, uni ? -0.01f : 0.01f, wpos);
			f3 unused = mk3(0.5f, 0.5f, 0.5f);
			for (int k = a.n_edits - 1; k >= 0; --k) (void)edit_warp(a.edits[k], false, wpos, unused);
		}
		// (round 6: one sample per occupancy cell shares no line with its neighbours at the fine levels -- the refresh runs on the fabric's request roof like the garden
		// frame, so it takes the same medicine: the L2 phase gate on the trailing hashed level pairs and four record levels per round trip.  aabb 1: 0.81 -> 0.76 ms,
		// aabb 16: 5.10 -> 4.54 ms per refresh; the same loads in another order, bit-identical grids: profiles/r06/ab_refresh_gate.txt)
		encode_num<NUM, true, true, NRS_REFRESH_GATE_PHASES>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		_Float16 raw_b0 = (_Float16)0, raw_b1 = (_Float16)0; // (two scalars, not an array indexed by the rolled loop's counter: that one lived in scratch)
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, x0, x1);
			if (b == 0) raw_b0 = dout[0]; else raw_b1 = dout[0]; // row 0 of sample 32*b + (lane & 31) sits on the g == 0 lanes
		}
		// lane l < 32 owns block 0's sample l; lane 32 + j owns block 1's sample, computed on lane j
		const float from_partner = xchg32((float)raw_b1);
		_Float16 raw = g ? (_Float16)from_partner : raw_b0;
		if (!have) continue;
		// (clear_empty_space, which the reference launches here (tn:3606), has its body commented out (tn:2759-2770): the operators' empty mask changes
		// nothing in the refresh -- a sample that falls into vacated space keeps the density of the place it stands on.  Pinned: tests/test_ref_pin.py.)
		_Float16 act = (_Float16)network_to_density((float)raw, m.density_activation);
		for (int k = a.n_edits - 1; k >= 0; --k) {
			const DeviceEdit& e = a.edits[k];
			float r;
			if (e.apply_poisson && poisson_residual_density(e, wpos, r)) act = act + (_Float16)r;
		}
		const float thickness = (float)act * NRS_MIN_STEP;
		atomicMax(a.grid_tmp + cell, __float_as_uint(thickness));
	}
}

__global__ void grid_ema_kernel(uint32_t n_elements, float decay, float* __restrict__ grid, const uint32_t* __restrict__ grid_tmp) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	const float importance = __uint_as_float(grid_tmp[i]);
	const float prev = grid[i];
	grid[i] = (prev < 0.f) ? prev : fmaxf(prev * decay, importance);
}

int launch_grid_update(const DeviceModel& m, const DeviceEdit* d_edits, int n_edits, const nrs_grid_update& u, uint64_t rng_state_nonuniform,
                       float* d_grid, uint32_t* d_grid_tmp, int n_cus, void* stream) {
	hipStream_t s = (hipStream_t)stream;
	const uint32_t n_elements = kGridVol * kCascades;
	GridUpdateArgs a{};
	a.grid = d_grid;
	a.grid_tmp = d_grid_tmp;
	a.edits = d_edits;
	a.n_edits = n_edits;
	a.n_uniform = u.n_uniform_samples;
	a.n_nonuniform = u.n_nonuniform_samples;
	a.step = u.ema_step;
	a.n_cascades = u.max_cascade + 1;
	a.rng_state = u.rng_state;
	a.rng_inc = u.rng_inc;
	a.rng_state_nonuniform = rng_state_nonuniform;
	static const uint32_t cell_order = []() { const char* e = dev_knob("NRS_REFRESH_ORDER"); return e ? (uint32_t)atoi(e) : 1u; }();
	a.cell_order = cell_order;
	const uint32_t n = a.n_uniform + a.n_nonuniform;
	if (n > 0) {
		const uint32_t n_tiles = (n + 63) / 64;
		uint32_t grid = (n_tiles + 3) / 4;
		const uint32_t cap = (uint32_t)n_cus * 8;
		if (grid > cap) grid = cap;
		if (m.numerics) hipLaunchKernelGGL(grid_refresh_kernel<kNumRuntime>, dim3(grid), dim3(256), 0, s, m, a);
		else hipLaunchKernelGGL(grid_refresh_kernel<0>, dim3(grid), dim3(256), 0, s, m, a);
		NRS_LAUNCH_CHECK("grid_refresh_kernel launch");
	}
	hipLaunchKernelGGL(grid_ema_kernel, dim3((n_elements + 255) / 256), dim3(256), 0, s, n_elements, u.decay, d_grid, d_grid_tmp);
	NRS_LAUNCH_CHECK("grid_ema_kernel launch");
	return NRS_OK;
}

} // namespace nrs
