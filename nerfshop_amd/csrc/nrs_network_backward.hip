// nrs_network_backward.hip -- NerfNetwork::backward: parameter gradients (and dL/dposition) of base.json's network on caller batches (gfx950, wave64).
//
// NerfNetworkFull::backward_impl (nerf_network_full.h:142-221) over tiny-cuda-nn's fully fused backward, as oracle/nrs_oracle.cpp:893-910 restates it, in ONE
// persistent launch that stores no activation in global memory: a wave takes a 64-sample tile, gathers its features and runs the forward pass exactly as
// network_kernel does (same functions, same fragments: the same fp16 activations), keeps the hidden layers in registers and walks back:
//
//   g_o   = rows 0..2 of dL_doutput (extract_rgb; rows 4..15 are never read)
//   g_h2  = fp16(rW3^T g_o) [h2 > 0]     g_h1 = fp16(rW2^T g_h2) [h1 > 0]     g_rin = fp16(rW1^T g_h1)
//   g_d   = g_rin[0:16], row 3 of dL_doutput added onto g_d[0] in fp16 (add_density_gradient)
//   g_h   = fp16(dW2^T g_d) [h > 0]      g_x  = fp16(dW1^T g_h)
//
// Every product is an MFMA with fp32 accumulators; the transposed A operands are fragments TD2 / T1 / T2 / T3 / Bwd of the lowered weights (make_weight_fragments),
// whose k order is the row order of a D tile -- so the packed gradient of one layer is the B operand of the next, as in the forward pass.
//
// Weight gradients dW[out][in] += sum over samples g_out[out] a_in[in]: the samples are the K dimension of an MFMA, so both factors are needed with the lane
// standing for a unit and the elements for samples -- the transpose of how a wave holds them.  They pass through a per-wave LDS slab ([unit][sample], one matrix at
// a time), and the twelve 32 x 32 fp32 tiles of the five matrices stay in the wave's accumulator registers over all its tiles.  At the end the workgroup's waves
// add their tiles into one LDS image in the parameter blob's order and the workgroup issues one float atomic per weight: 64 consecutive floats per instruction.
//
// Grid gradients: per sample, level and corner, two fp32 atomics (w_corner * g_x[2 l + f]) at the entry the forward's index function names: 256 per sample.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_network_backward.h"
#include "nrs_vec.cuh"
#include "nrs_hashgrid.cuh"
#include "nrs_mlp.cuh"

namespace nrs {

constexpr int kBwdWaves = 4;          // one wave per SIMD: 192 accumulator registers per wave
constexpr uint32_t kBwdFrags = 20;    // Bwd[4], then TD2[2] T1[4] T2[8] T3[2] in fragment order
constexpr int kBwdTPitch = 40;        // halfs per row of the transpose slab: 32 samples + 8 (rows stay 16-byte aligned, neighbouring rows start 20 banks apart)
constexpr uint32_t kMlpParams = kDensityW + kRgbW; // 10 240
// first parameter of each matrix in the blob: [density: W1 64x32 | W2 16x64] [rgb: W1 64x32 | W2 64x64 | W3 16x64]
constexpr uint32_t kOffD1 = 0, kOffD2 = 64 * 32, kOffR1 = kDensityW, kOffR2 = kOffR1 + 64 * 32, kOffR3 = kOffR2 + 64 * 64;
// accumulator tiles of a wave: dW1 [mo], dW2 [ni], rW1 [mo], rW2 [mo][ni], rW3 [ni] (mo / ni: 32-row block of the output / input units)
enum { kAccD1 = 0, kAccD2 = 2, kAccR1 = 4, kAccR2 = 6, kAccR3 = 10, kAccTiles = 12 };

struct alignas(16) BwdWaveLds {
	FeatLds fl;                       // the forward's feature slab
	uint32_t gx[kLevels][64];         // dL/dfeatures (2 L, 2 L + 1) packed, [level][sample of the tile]
	_Float16 t[128][kBwdTPitch];      // transpose slab: rows 0..63 g_out, rows 64..127 a_in of the matrix at hand, [unit][sample of the block]
};
struct BwdSmem {
	ModelLds ml;
	half8 bw[kBwdFrags * 64];
	union {
		BwdWaveLds w[kBwdWaves];
		float flush[kMlpParams];      // after the last tile: the workgroup's MLP gradient in the blob's order
	} u;
};
static_assert(sizeof(BwdSmem) <= 160 * 1024, "LDS of a gfx950 CU");

struct BackwardArgs {
	uint32_t n;
	const float* in;        // [n x ld_in]
	uint32_t ld_in;
	const _Float16* dout;   // NRS_PLANES [16 x ld_dout] | NRS_INTERLEAVED [n x 16]
	uint32_t ld_dout;
	int layout;
	float* dparams;         // [kMlpParams + 2 x entries], added to
	float* dinput;          // nullable, [n x ld_in]
};

// a wave's LDS writes before its own later reads of other lanes' slots (no instruction: LDS operations of a wave stay in order)
__device__ __forceinline__ void wave_lds_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// D-tile row of element e of a packed half8 in lane-half g
__device__ __forceinline__ int tile_row(int e, int g) { return (e & 3) + 8 * (e >> 2) + 4 * g; }
// 16 units of sample column j (a packed D half-tile) into the slab's rows base + tile_row
__device__ __forceinline__ void put_rows(BwdWaveLds& wl, int base, int j, int g, half8 p) {
	#pragma unroll
	for (int e = 0; e < 8; ++e) wl.t[base + tile_row(e, g)][j] = p[e];
}
// MFMA operand with k = sample: 8 consecutive samples of unit `row`
__device__ __forceinline__ half8 get_samples(const BwdWaveLds& wl, int row, int ks, int g) {
	return *reinterpret_cast<const half8*>(&wl.t[row][16 * ks + 8 * g]);
}
// acc[mo * NI + ni] += g_out[32 mo ..][samples] a_in[32 ni ..][samples]^T over the block's 32 samples (two k steps).  OUT16: the matrix has 16 output rows.
template <int MO, int NI, bool OUT16>
__device__ __forceinline__ void weight_gradient(const BwdWaveLds& wl, int lane, floatx16* acc) {
	const int u = lane & 31, g = lane >> 5;
	#pragma unroll
	for (int ks = 0; ks < 2; ++ks) {
		half8 b[NI];
		#pragma unroll
		for (int ni = 0; ni < NI; ++ni) b[ni] = get_samples(wl, 64 + 32 * ni + u, ks, g);
		#pragma unroll
		for (int mo = 0; mo < MO; ++mo) {
			half8 a = get_samples(wl, 32 * mo + u, ks, g);
			if (OUT16 && u >= 16) a = half8{};
			#pragma unroll
			for (int ni = 0; ni < NI; ++ni) acc[mo * NI + ni] = NRS_MFMA(a, b[ni], acc[mo * NI + ni]);
		}
	}
}
__device__ __forceinline__ half8 relu_mask(half8 grad, half8 act) {
	half8 r;
	#pragma unroll
	for (int e = 0; e < 8; ++e) r[e] = act[e] > (_Float16)0 ? grad[e] : (_Float16)0;
	return r;
}
// one wave's tile of a matrix into the workgroup's image: register r of lane (column, g) is row tile_row of the 32 x 32 tile
__device__ __forceinline__ void flush_tile(float* img, const floatx16& t, int lane, uint32_t off, int n_in, int n_out, int mo, int ni) {
	const int col = 32 * ni + (lane & 31), g = lane >> 5;
	#pragma unroll
	for (int r = 0; r < 16; ++r) {
		const int row = 32 * mo + (r & 3) + 8 * (r >> 2) + 4 * g;
		if (row < n_out) atomicAdd(&img[off + row * n_in + col], t[r]);
	}
}

__global__ __launch_bounds__(64 * kBwdWaves) void network_backward_kernel(const DeviceModel m, const BackwardArgs a) {
	__shared__ BwdSmem sm;
	{
		constexpr uint32_t per = kFragBytes / 16;
		const uint4* src = reinterpret_cast<const uint4*>(m.wfrag);
		uint4* dst = reinterpret_cast<uint4*>(sm.bw);
		for (uint32_t i = threadIdx.x; i < kBwdFrags * per; i += blockDim.x) {
			const uint32_t f = i / per, from = f < 4u ? NRS_FRAG_BWD(f) : NRS_FRAG_TD2(0) + (f - 4u);
			dst[i] = src[from * per + i % per];
		}
	}
	stage_model_to_lds(m, sm.ml);
	const half8* W = sm.ml.w;
	const half8* BW = sm.bw;
#define NRS_BW(f) ((f) < NRS_FRAG_TD2(0) ? (f) - NRS_FRAG_BWD(0) : (f) - NRS_FRAG_TD2(0) + 4) // slot of device fragment f in sm.bw
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5, j = lane & 31;
	BwdWaveLds& wl = sm.u.w[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	float* dgrid = a.dparams + kMlpParams;
	const uint32_t wave_global = blockIdx.x * kBwdWaves + (threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * kBwdWaves;
	const uint32_t n_tiles = (a.n + 63) / 64;
	floatx16 acc[kAccTiles];
	#pragma unroll
	for (int i = 0; i < kAccTiles; ++i) acc[i] = zero16();

	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < a.n;
		f3 wpos = mk3(0, 0, 0), wdir = mk3(0.5f, 0.5f, 0.5f);
		if (have) {
			const float* c = a.in + (size_t)s * a.ld_in;
			wpos = mk3(c[0], c[1], c[2]);
			wdir = mk3(c[4], c[5], c[6]);
		}
		encode_to_lds<false>(gv, m.levels, sm.ml, wl.fl, lane, g, wpos, have);
		const half8 sh_own = encode_sh4(g, wdir), sh_par = encode_sh4(g, mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z)));

		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			// ---- forward: the layers density_mlp / rgb_mlp are composed of (fp32 accumulators), the hidden ones kept
			const half8 x0 = load_features(wl.fl, lane, sel, 0), x1 = load_features(wl.fl, lane, sel, 1);
			const half8 sh = sel ? sh_par : sh_own;
			half8 h[4], h1[4], h2[4];
			density_hidden<false>(W, lane, x0, x1, h[0], h[1], h[2], h[3]);
			const half8 d = density_output<false>(W, lane, h[0], h[1], h[2], h[3]);
			rgb_hidden0<false, false>(W, lane, d, sh, nullptr, half8{}, h1[0], h1[1], h1[2], h1[3]);
			h2[0] = h1[0]; h2[1] = h1[1]; h2[2] = h1[2]; h2[3] = h1[3];
			hidden_layer_64<false>(W, W + NRS_FRAG_R2(0, 0) * 64, lane, h2[0], h2[1], h2[2], h2[3]);
			// (the output layer's values are not needed: it has no activation)

			// ---- dL_doutput of sample column j: rows 0..2 are D-tile rows of lane-half 0; row 3 is the density's
			const uint32_t sb = tile * 64 + 32 * b + j;
			half8 go = half8{};
			_Float16 g_density = (_Float16)0;
			if (g == 0 && sb < a.n) {
				if (a.layout == NRS_PLANES) {
					go[0] = a.dout[sb]; go[1] = a.dout[(size_t)a.ld_dout + sb]; go[2] = a.dout[2 * (size_t)a.ld_dout + sb];
					g_density = a.dout[3 * (size_t)a.ld_dout + sb];
				} else {
					const _Float16* r = a.dout + (size_t)sb * 16;
					go[0] = r[0]; go[1] = r[1]; go[2] = r[2];
					g_density = r[3];
				}
			}

			// ---- rgb output layer
			half8 gh2[4];
			#pragma unroll
			for (int mb = 0; mb < 2; ++mb) {
				const floatx16 t = mfma_first(BW[NRS_BW(NRS_FRAG_T3(mb)) * 64 + lane], go);
				gh2[2 * mb] = relu_mask(pack(t, 0), h2[2 * mb]); gh2[2 * mb + 1] = relu_mask(pack(t, 8), h2[2 * mb + 1]);
			}
			wave_lds_sync();
			put_rows(wl, 0, j, g, go);
			#pragma unroll
			for (int q = 0; q < 4; ++q) put_rows(wl, 64 + 16 * q, j, g, h2[q]);
			wave_lds_sync();
			weight_gradient<1, 2, true>(wl, lane, acc + kAccR3);
			NRS_STAGE_FENCE();

			// ---- rgb hidden layer 2
			half8 gh1[4];
			#pragma unroll
			for (int mb = 0; mb < 2; ++mb) {
				floatx16 t = mfma_first(BW[NRS_BW(NRS_FRAG_T2(mb, 0)) * 64 + lane], gh2[0]);
				#pragma unroll
				for (int ks = 1; ks < 4; ++ks) t = NRS_MFMA(BW[NRS_BW(NRS_FRAG_T2(mb, ks)) * 64 + lane], gh2[ks], t);
				gh1[2 * mb] = relu_mask(pack(t, 0), h1[2 * mb]); gh1[2 * mb + 1] = relu_mask(pack(t, 8), h1[2 * mb + 1]);
			}
			wave_lds_sync();
			#pragma unroll
			for (int q = 0; q < 4; ++q) { put_rows(wl, 16 * q, j, g, gh2[q]); put_rows(wl, 64 + 16 * q, j, g, h1[q]); }
			wave_lds_sync();
			weight_gradient<2, 2, false>(wl, lane, acc + kAccR2);
			NRS_STAGE_FENCE();

			// ---- rgb layer 0: input [density outputs 16 | SH 16]; the SH half of the input gradient is not propagated (the direction's gradient is out of scope)
			half8 gd;
			{
				floatx16 t = mfma_first(BW[NRS_BW(NRS_FRAG_T1(0)) * 64 + lane], gh1[0]);
				#pragma unroll
				for (int ks = 1; ks < 4; ++ks) t = NRS_MFMA(BW[NRS_BW(NRS_FRAG_T1(ks)) * 64 + lane], gh1[ks], t);
				gd = pack(t, 0);
				if (g == 0) gd[0] = gd[0] + g_density; // add_density_gradient, in fp16
			}
			wave_lds_sync();
			#pragma unroll
			for (int q = 0; q < 4; ++q) put_rows(wl, 16 * q, j, g, gh1[q]);
			put_rows(wl, 64, j, g, d);
			#pragma unroll
			for (int e = 0; e < 8; ++e) wl.t[64 + 16 + 8 * g + e][j] = sh[e];
			wave_lds_sync();
			weight_gradient<2, 1, false>(wl, lane, acc + kAccR1);
			NRS_STAGE_FENCE();

			// ---- density output layer
			half8 gh[4];
			#pragma unroll
			for (int mb = 0; mb < 2; ++mb) {
				const floatx16 t = mfma_first(BW[NRS_BW(NRS_FRAG_TD2(mb)) * 64 + lane], gd);
				gh[2 * mb] = relu_mask(pack(t, 0), h[2 * mb]); gh[2 * mb + 1] = relu_mask(pack(t, 8), h[2 * mb + 1]);
			}
			wave_lds_sync();
			put_rows(wl, 0, j, g, gd);
			#pragma unroll
			for (int q = 0; q < 4; ++q) put_rows(wl, 64 + 16 * q, j, g, h[q]);
			wave_lds_sync();
			weight_gradient<1, 2, true>(wl, lane, acc + kAccD2);
			NRS_STAGE_FENCE();

			// ---- density hidden layer: dL/dfeatures
			{
				floatx16 t = mfma_first(BW[NRS_BW(NRS_FRAG_BWD(0)) * 64 + lane], gh[0]);
				#pragma unroll
				for (int ks = 1; ks < 4; ++ks) t = NRS_MFMA(BW[NRS_BW(NRS_FRAG_BWD(ks)) * 64 + lane], gh[ks], t);
				#pragma unroll
				for (int q = 0; q < 8; ++q) {
					const half2v pr = {(_Float16)t[2 * q], (_Float16)t[2 * q + 1]};
					wl.gx[level_of_pair(q, g)][32 * b + j] = __builtin_bit_cast(uint32_t, pr);
				}
			}
			wave_lds_sync();
			#pragma unroll
			for (int q = 0; q < 4; ++q) put_rows(wl, 16 * q, j, g, gh[q]);
			#pragma unroll
			for (int ks = 0; ks < 2; ++ks) {
				const half8 x = ks ? x1 : x0; // element 2 i + f: feature f of level 2 (4 ks + i) + g
				#pragma unroll
				for (int e = 0; e < 8; ++e) wl.t[64 + 16 * ks + 4 * (e >> 1) + 2 * g + (e & 1)][j] = x[e];
			}
			wave_lds_sync();
			weight_gradient<2, 1, false>(wl, lane, acc + kAccD1);
			NRS_STAGE_FENCE();
		}

		// ---- the hash grid: every lane scatters its own sample, level after level (parameters wave-uniform)
		wave_lds_sync();
		float res[3] = {0.f, 0.f, 0.f};
		#pragma unroll 1
		for (int L = 0; L < (int)kLevels; ++L) {
			const LevelParams& lp = m.levels[L];
			const uint32_t gl = wl.gx[L][lane];
			if (have) {
				const half2v gh16 = __builtin_bit_cast(half2v, gl);
				const float g0 = (float)gh16[0], g1 = (float)gh16[1];
				const CellCoords c = cell_coords(lp, wpos);
				#pragma unroll
				for (int k = 0; k < 8; ++k) { // the forward's index function and weights (the fast paths fetch the same entries with the same weights)
					uint32_t index;
					float weight;
					cell_corner(lp, c.gx, c.gy, c.gz, c.wx, c.wy, c.wz, k, index, weight);
					float* p = dgrid + 2 * (size_t)(lp.offset + index);
					atomicAdd(p, weight * g0);
					atomicAdd(p + 1, weight * g1);
				}
				if (a.dinput) level_input_gradient(gv, lp, wpos, gl, res);
			}
		}
		if (a.dinput && have) {
			float* o = a.dinput + (size_t)s * a.ld_in;
			o[0] = res[0]; o[1] = res[1]; o[2] = res[2];
			for (uint32_t k = 3; k < a.ld_in; ++k) o[k] = 0.f; // dt and the direction are not propagated; whatever else the record carries takes no gradient
		}
	}
#undef NRS_BW

	// ---- the MLP gradients: waves -> one image per workgroup -> one atomic per weight, 64 consecutive floats per instruction
	__syncthreads();
	float* img = sm.u.flush;
	for (uint32_t i = threadIdx.x; i < kMlpParams; i += blockDim.x) img[i] = 0.f;
	__syncthreads();
	#pragma unroll
	for (int mo = 0; mo < 2; ++mo) {
		flush_tile(img, acc[kAccD1 + mo], lane, kOffD1, 32, 64, mo, 0);
		flush_tile(img, acc[kAccR1 + mo], lane, kOffR1, 32, 64, mo, 0);
		#pragma unroll
		for (int ni = 0; ni < 2; ++ni) flush_tile(img, acc[kAccR2 + 2 * mo + ni], lane, kOffR2, 64, 64, mo, ni);
	}
	#pragma unroll
	for (int ni = 0; ni < 2; ++ni) {
		flush_tile(img, acc[kAccD2 + ni], lane, kOffD2, 64, 16, 0, ni);
		flush_tile(img, acc[kAccR3 + ni], lane, kOffR3, 64, 16, 0, ni);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kMlpParams; i += blockDim.x) atomicAdd(&a.dparams[i], img[i]);
}

// d_dparams is added to: the caller zeroes it for EGradientMode::Overwrite.  One workgroup per CU (its LDS and its accumulator registers fill one).
int launch_network_backward(const DeviceModel& m, uint32_t n, const float* d_in, uint32_t ld_in, const void* d_dout, uint32_t ld_dout, int layout,
                            float* d_dparams, float* d_dinput, int n_cus, void* stream) {
	if (n == 0) return NRS_OK;
	BackwardArgs a{};
	a.n = n; a.in = d_in; a.ld_in = ld_in; a.dout = (const _Float16*)d_dout; a.ld_dout = ld_dout; a.layout = layout; a.dparams = d_dparams; a.dinput = d_dinput;
	const uint32_t n_tiles = (n + 63) / 64;
	uint32_t grid = (n_tiles + kBwdWaves - 1) / kBwdWaves;
	if (grid > (uint32_t)n_cus) grid = (uint32_t)n_cus;
	hipLaunchKernelGGL(network_backward_kernel, dim3(grid), dim3(64 * kBwdWaves), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("network_backward_kernel launch");
	return NRS_OK;
}

} // namespace nrs
