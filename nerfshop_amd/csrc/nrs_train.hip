// nrs_train.hip -- the training-ray path (gfx950): rays -> network inputs, and network outputs -> ray loss + dL/doutput, compacted.
//
//   train_count_kernel     generate_training_samples_nerf's first walk (tn:1188-1213): samples per ray.
//   train_tile_*_kernel    exclusive scan of the per-ray counts in input order: tile sums, tile_scan_kernel (nrs_scan.hip) over them, the scan inside each tile.  It stands where the
//                          reference has atomicAdd (tn:1218, :1225, :1834), so the layout does not depend on arrival order.
//   train_write_kernel     the second walk (tn:1232-1246) into the slots the scan fixed; train_fill_kernel zeroes the records behind the last emitted ray.
//   ray_loss_forward_kernel   compute_loss_kernel_train_nerf's first loop, the target and loss_and_gradient (tn:1745-1828, :1847): M, C, g, loss per ray.
//   ray_loss_gradient_kernel  its third loop (tn:1895-1944) at the compact base the scan fixed; ray_loss_tail_kernel zeroes the compact tail.
//
// The generator has one thread per ray, as in the reference (it is bound by the latency of the bitfield walk).  The two loss kernels have one lane per SAMPLE: see
// "one lane per sample" below.  No float atomics: every output is a function of the inputs alone.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_scan.h"
#include "nrs_train.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_shade.cuh"
#include "nrs_loss.cuh"
#include "nrs_scan.cuh"

namespace nrs {

constexpr uint32_t kTrainSteps = 1024;       // NERF_STEPS, common_nerf.h:20
constexpr uint32_t kTrainMaxAdvances = 65536; // empty cells a ray may cross (a ray through the largest box crosses a few thousand): see train_march
constexpr uint32_t kTrainBlock = 128;

// ---- rays -> network inputs -------------------------------------------------------------------------------------------------------------------------------
struct TrainRay { f3 o, d; float startt; bool ok; };
// tn:1188-1195.  A ray the walk cannot end on (non-finite origin, direction of a length outside [0.5, 2]: advance_to_next_voxel steps t by at least MIN_STEP until it
// passes a target that such a ray puts out of reach) has no samples.
__device__ __forceinline__ TrainRay train_ray(const DeviceModel& m, const TrainSamplesArgs& a, uint32_t i) {
	TrainRay r;
	const float* p = a.rays + 6 * (size_t)i;
	r.o = mk3(p[0], p[1], p[2]);
	r.d = mk3(p[3], p[4], p[5]);
	const float sq = dot3(r.d, r.d), os = fabsf(r.o.x) + fabsf(r.o.y) + fabsf(r.o.z);
	r.ok = sq >= 0.25f && sq <= 4.0f && os < 3.0e38f; // false for every NaN
	float tmin;
	ray_intersect(m.aabb.mn, m.aabb.mx, r.o, r.d, tmin);
	tmin = fmaxf(tmin, 0.0f);
	r.startt = tmin + calc_dt(tmin, a.cone) * (a.jitter ? a.jitter[i] : 0.0f);
	return r;
}
// The walk of tn:1203-1213 (WRITE false) and :1235-1246 (true): up to `limit` samples; o + d * t as the render kernel's marcher forms it.
template <bool WRITE>
__device__ __forceinline__ uint32_t train_march(const DeviceModel& m, const TrainRay& r, float cone, uint32_t limit, float* __restrict__ coords, uint32_t ld) {
	const f3 idir = mk3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
	const f3 wdir = warp_direction(r.d);
	float t = r.startt;
	uint32_t j = 0, advances = 0;
	while (j < limit) {
		const f3 pos = r.o + r.d * t;
		if (!box_contains(m.aabb, pos)) break;
		const float dt = calc_dt(t, cone);
		const uint32_t mip = (uint32_t)mip_from_dt(dt, pos);
		if (density_grid_occupied_at(pos, m.bitfield, mip)) {
			if (WRITE) {
				const f3 wpos = warp_position(pos, m.aabb);
				float* c = coords + (size_t)j * ld;
				c[0] = wpos.x; c[1] = wpos.y; c[2] = wpos.z;
				c[3] = warp_dt(dt);
				c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z;
			}
			++j;
			t += dt;
		} else {
			if (++advances > kTrainMaxAdvances) break; // (t no longer moves: an origin so far away that a step is below t's spacing)
			t = advance_to_next_voxel(t, cone, pos, r.d, idir, kGrid >> mip, 1.0f / (float)(kGrid >> mip));
		}
	}
	return j;
}

__global__ __launch_bounds__(kTrainBlock) void train_count_kernel(const DeviceModel m, const TrainSamplesArgs a) {
	const uint32_t i = blockIdx.x * kTrainBlock + threadIdx.x;
	if (i >= a.n_rays) return;
	const TrainRay r = train_ray(m, a, i);
	TrainSamplesWs(a.ws, a.n_rays).count[i] = r.ok ? train_march<false>(m, r, a.cone, kTrainSteps, nullptr, 0) : 0u;
}

// The exclusive scan of the per-ray counts, in three launches as the mesh path does it: sums per tile of kTrainScanTile rays (coalesced, any number of workgroups), the
// one-workgroup scan of the tile sums (launch_tile_scan: 2 x 4 bytes per 1024 rays), and the scan inside each tile on top of its offset.
// Two sums per ray: its count and whether it has one.  count / base / slot: three arrays of n words; rays at or past *live (NULL: all n) count as empty.
// GEN (the generator): slot = the rays with samples before this one -- its place among the emitted rays, because a ray with samples that is dropped puts every later
// one past max_samples too (bases only grow) -- out[0] = emitted rays, out[1] = the sum of all counts, *end = where the last emitted ray ends.
// Otherwise (the loss): out[0] = the sum of all counts.
constexpr uint32_t kScanThreads = 256, kScanPer = kTrainScanTile / kScanThreads;
// a thread's kScanPer consecutive rays of tile blockIdx.x: their counts (0 at or past n) and the two sums over them
struct TileCounts { uint32_t first, c[kScanPer], sum[2]; };
__device__ __forceinline__ TileCounts load_tile_counts(uint32_t n, const uint32_t* __restrict__ live, const uint32_t* __restrict__ count) {
	TileCounts t;
	if (live) n = min(n, *live);
	t.first = blockIdx.x * kTrainScanTile + threadIdx.x * kScanPer;
	t.sum[0] = t.sum[1] = 0u;
	#pragma unroll
	for (uint32_t k = 0; k < kScanPer; ++k) { t.c[k] = t.first + k < n ? count[t.first + k] : 0u; t.sum[0] += t.c[k]; t.sum[1] += t.c[k] ? 1u : 0u; }
	return t;
}
// tiles: [n_tiles][2] sums, then [2] totals
__global__ __launch_bounds__(kScanThreads) void train_tile_sums_kernel(uint32_t n, const uint32_t* __restrict__ live, const uint32_t* __restrict__ count,
                                                                        uint32_t* __restrict__ tiles, uint32_t* __restrict__ zero0, uint32_t* __restrict__ zero1) {
	if (blockIdx.x == 0 && threadIdx.x == 0) { if (zero0) *zero0 = 0u; if (zero1) *zero1 = 0u; } // what train_tile_scan_kernel<true> takes maxima into
	const TileCounts t = load_tile_counts(n, live, count);
	uint32_t before[2], total[2];
	block_exclusive_add<kScanThreads, 2>(t.sum, before, total);
	if (threadIdx.x == 0) { tiles[2 * blockIdx.x] = total[0]; tiles[2 * blockIdx.x + 1] = total[1]; }
}
template <bool GEN>
__global__ __launch_bounds__(kScanThreads) void train_tile_scan_kernel(uint32_t n, const uint32_t* __restrict__ live, const uint32_t* __restrict__ count,
                                                                        const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ totals,
                                                                        uint32_t* __restrict__ base, uint32_t* __restrict__ slot, uint32_t max_samples,
                                                                        uint32_t* __restrict__ out, uint32_t* __restrict__ end) {
	__shared__ uint32_t s_emitted, s_end;
	if (threadIdx.x == 0) { s_emitted = 0; s_end = 0; }
	if (live) n = min(n, *live);
	const TileCounts t = load_tile_counts(n, nullptr, count);
	uint32_t before[2], total[2];
	block_exclusive_add<kScanThreads, 2>(t.sum, before, total); // (its barrier also orders s_emitted = 0 in front of the maxima below)
	uint32_t v_run = tiles[2 * blockIdx.x] + before[0], t_run = tiles[2 * blockIdx.x + 1] + before[1]; // (tiles: exclusive after the one-workgroup scan)
	uint32_t emitted_to = 0, my_end = 0;
	#pragma unroll
	for (uint32_t k = 0; k < kScanPer; ++k) {
		if (t.first + k < n) {
			base[t.first + k] = v_run;
			if (GEN) {
				slot[t.first + k] = t_run;
				if (t.c[k] && v_run <= max_samples && t.c[k] <= max_samples - v_run) { emitted_to = t_run + 1u; my_end = v_run + t.c[k]; }
			}
		}
		v_run += t.c[k];
		t_run += t.c[k] ? 1u : 0u;
	}
	if (GEN) { // the emitted rays are the first of the rays with samples: their number is the last one's slot + 1.  Integer maxima: the result does not depend on the order
		if (emitted_to) { atomicMax(&s_emitted, emitted_to); atomicMax(&s_end, my_end); }
		__syncthreads();
		if (threadIdx.x == 0) {
			if (s_emitted) { atomicMax(&out[0], s_emitted); atomicMax(end, s_end); }
			if (blockIdx.x == 0) out[1] = totals[0];
		}
	} else if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = totals[0];
}
// tiles: train_scan_words(n) words of workspace
template <bool GEN>
static int launch_train_scan(uint32_t n, const uint32_t* live, const uint32_t* count, uint32_t* tiles, uint32_t* base, uint32_t* slot, uint32_t max_samples, uint32_t* out,
                             uint32_t* end, hipStream_t st) {
	const uint32_t n_tiles = train_scan_tiles(n);
	uint32_t* totals = tiles + 2 * (size_t)n_tiles;
	hipLaunchKernelGGL(train_tile_sums_kernel, dim3(n_tiles), dim3(kScanThreads), 0, st, n, live, count, tiles, GEN ? out : nullptr, GEN ? end : nullptr);
	NRS_LAUNCH_CHECK("train_tile_sums_kernel launch");
	const int status = launch_tile_scan(n_tiles, 2, tiles, totals, nullptr, st);
	if (status != NRS_OK) return status;
	hipLaunchKernelGGL(train_tile_scan_kernel<GEN>, dim3(n_tiles), dim3(kScanThreads), 0, st, n, live, count, (const uint32_t*)tiles, (const uint32_t*)totals, base, slot, max_samples,
	                   out, end);
	NRS_LAUNCH_CHECK("train_tile_scan_kernel launch");
	return NRS_OK;
}

__global__ __launch_bounds__(kTrainBlock) void train_write_kernel(const DeviceModel m, const TrainSamplesArgs a) {
	const uint32_t i = blockIdx.x * kTrainBlock + threadIdx.x;
	if (i >= a.n_rays) return;
	const TrainSamplesWs ws(a.ws, a.n_rays);
	const uint32_t j = ws.count[i], base = ws.base[i];
	if (j == 0u || base > a.max_samples || j > a.max_samples - base) return; // tn:1214-1221
	const uint32_t s = ws.slot[i];
	a.ray_indices[s] = i;
	a.numsteps[2 * s] = j;
	a.numsteps[2 * s + 1] = base;
	const TrainRay r = train_ray(m, a, i);
	train_march<true>(m, r, a.cone, j, a.coords + (size_t)base * a.ld, a.ld);
}
// records [*end, max_samples): floats 0..6 zero (end NULL: from 0)
__global__ __launch_bounds__(256) void train_fill_kernel(uint32_t max_samples, const uint32_t* __restrict__ end, float* __restrict__ coords, uint32_t ld) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= max_samples || (end && k < *end)) return;
	float* c = coords + (size_t)k * ld;
	#pragma unroll
	for (int q = 0; q < 7; ++q) c[q] = 0.f;
}

int launch_training_samples(const DeviceModel& m, const TrainSamplesArgs& a, void* stream) {
	hipStream_t st = (hipStream_t)stream;
	uint32_t* end = nullptr;
	if (a.n_rays) {
		const uint32_t blocks = (a.n_rays + kTrainBlock - 1) / kTrainBlock;
		const TrainSamplesWs ws(a.ws, a.n_rays);
		end = ws.end;
		hipLaunchKernelGGL(train_count_kernel, dim3(blocks), dim3(kTrainBlock), 0, st, m, a);
		NRS_LAUNCH_CHECK("train_count_kernel launch");
		const int status = launch_train_scan<true>(a.n_rays, nullptr, ws.count, ws.tiles, ws.base, ws.slot, a.max_samples, a.counters, end, st);
		if (status != NRS_OK) return status;
		hipLaunchKernelGGL(train_write_kernel, dim3(blocks), dim3(kTrainBlock), 0, st, m, a);
		NRS_LAUNCH_CHECK("train_write_kernel launch");
	} else {
		const hipError_t e = hipMemsetAsync(a.counters, 0, 2 * sizeof(uint32_t), st);
		if (e != hipSuccess) return hip_fail(e, "nrs_training_samples: zeroing the counters");
	}
	hipLaunchKernelGGL(train_fill_kernel, dim3((a.max_samples + 255) / 256), dim3(256), 0, st, a.max_samples, (const uint32_t*)end, a.coords, a.ld);
	NRS_LAUNCH_CHECK("train_fill_kernel launch");
	return NRS_OK;
}

// ---- network outputs -> loss and dL/doutput ------------------------------------------------------------------------------------------------------------------
constexpr float kLossEps = 1e-4f; // EPSILON, tn:1747

__device__ __forceinline__ float network_to_rgb_derivative(float v, uint32_t act) { // tn:297-306
	switch (act) {
		case NRS_ACT_RELU: return v > 0.0f ? 1.0f : 0.0f;
		case NRS_ACT_LOGISTIC: { const float density = 1.0f / (1.0f + __expf(-v)); return density * (1 - density); }
		case NRS_ACT_EXPONENTIAL: return __expf(clampf_(v, -10.0f, 10.0f));
		default: return 1.0f;
	}
}
// the four raw outputs of sample s
struct RawOut { float v[4]; };
__device__ __forceinline__ RawOut load_raw(const __half* __restrict__ out, uint32_t ld, int layout, size_t s) {
	RawOut r;
	if (layout == NRS_PLANES) {
		#pragma unroll
		for (int c = 0; c < 4; ++c) r.v[c] = __half2float(out[(size_t)c * ld + s]);
	} else {
		const uint2 w = *reinterpret_cast<const uint2*>(out + 16 * s); // 32-byte records: aligned
		const __half2 a = __builtin_bit_cast(__half2, w.x), b = __builtin_bit_cast(__half2, w.y);
		r.v[0] = __low2float(a); r.v[1] = __high2float(a); r.v[2] = __low2float(b); r.v[3] = __high2float(b);
	}
	return r;
}
__device__ __forceinline__ void store_dl(__half* __restrict__ dl, uint32_t ld, int layout, size_t s, const float v[4]) {
	if (layout == NRS_PLANES) {
		#pragma unroll
		for (int c = 0; c < 4; ++c) dl[(size_t)c * ld + s] = __float2half(v[c]);
	} else {
		const __half2 a = __halves2half2(__float2half(v[0]), __float2half(v[1])), b = __halves2half2(__float2half(v[2]), __float2half(v[3]));
		*reinterpret_cast<uint2*>(dl + 16 * s) = make_uint2(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b));
	}
}

// what one sample adds to the composite (tn:1758-1770 / :1906-1913)
struct Sample { RawOut raw; f3 rgb; float dt, alpha, rest; }; // rest = 1 - alpha
__device__ __forceinline__ Sample load_sample(const DeviceModel& m, const RayLossArgs& a, size_t s) {
	Sample q;
	q.raw = load_raw(reinterpret_cast<const __half*>(a.output), a.ld_out, a.out_layout, s);
	q.rgb = mk3(network_to_rgb(q.raw.v[0], m.rgb_activation), network_to_rgb(q.raw.v[1], m.rgb_activation), network_to_rgb(q.raw.v[2], m.rgb_activation));
	q.dt = unwarp_dt(a.coords[s * a.ld_in + 3]);
	const float density = network_to_density(q.raw.v[3], m.density_activation);
	// 1 - alpha is exp(-density dt) itself: the reference's 1.f - alpha = 1 - (1 - e) loses e's low bits (all of them below 6e-8), which its T then carries
	q.rest = __expf(-density * q.dt);
	q.alpha = 1.f - q.rest;
	return q;
}
__device__ __forceinline__ uint32_t live_rays(const RayLossArgs& a) { return a.ray_counter ? live_slots(a.ray_counter, a.n_rays) : a.n_rays; }

// The ray's target, the background behind a ray that was not stopped, loss_and_gradient, and the ray's row of the workspace (tn:1789-1828, :1847-1858)
__device__ __forceinline__ void finish_ray(const RayLossArgs& a, uint32_t i, uint32_t M, uint32_t n, f3 C, float T) {
	// tn:1789-1828
	const nrs_ray_loss_params& p = a.p;
	const float* bgp = a.background ? a.background + 3 * (size_t)i : p.background;
	f3 bg;
	if (a.background_linear) { // nrs_ray_loss_ex: what the ray sees behind its last sample, already linear (the environment map over the background, nrs_envmap_background)
		const float* bl = a.background_linear + 3 * (size_t)i;
		bg = mk3(bl[0], bl[1], bl[2]);
	} else bg = mk3(train_srgb_to_linear(bgp[0]), train_srgb_to_linear(bgp[1]), train_srgb_to_linear(bgp[2]));
	const float* texp = a.target_rgba + 4 * (size_t)i;
	const float4 tex = make_float4(texp[0], texp[1], texp[2], texp[3]);
	f3 target;
	if (p.train_in_linear_colors || p.color_space == NRS_COLOR_LINEAR) {
		target = mk3(tex.x, tex.y, tex.z) + (1.0f - tex.w) * bg;
		if (!p.train_in_linear_colors) {
			target = mk3(train_linear_to_srgb(target.x), train_linear_to_srgb(target.y), train_linear_to_srgb(target.z));
			bg = mk3(train_linear_to_srgb(bg.x), train_linear_to_srgb(bg.y), train_linear_to_srgb(bg.z));
		}
	} else {
		bg = mk3(train_linear_to_srgb(bg.x), train_linear_to_srgb(bg.y), train_linear_to_srgb(bg.z));
		if (tex.w > 0) {
			target = mk3(train_linear_to_srgb(tex.x / tex.w), train_linear_to_srgb(tex.y / tex.w), train_linear_to_srgb(tex.z / tex.w)) * tex.w + (1.0f - tex.w) * bg;
		} else target = bg;
	}
	if (M == n) C = C + T * bg;
	float lx, ly, lz, gx, gy, gz;
	loss_and_gradient(p.loss_type, target.x, C.x, lx, gx);
	loss_and_gradient(p.loss_type, target.y, C.y, ly, gy);
	loss_and_gradient(p.loss_type, target.z, C.z, lz, gz);
	const RayLossWs ws(a.ws, a.n_rays);
	ws.M[i] = M;
	ws.C[0][i] = C.x; ws.C[1][i] = C.y; ws.C[2][i] = C.z;
	ws.g[0][i] = gx; ws.g[1][i] = gy; ws.g[2][i] = gz;
	ws.loss[i] = sum3(lx, ly, lz) / 3.0f / (float)a.n_rays;
	if (a.ray_aux) { // nrs_ray_loss_ex: the slot's record, kRayAuxWords words (g, T | target, C.x | C.yz, n, M)
		float4* aux = reinterpret_cast<float4*>(a.ray_aux + kRayAuxWords * (size_t)i);
		aux[0] = make_float4(gx, gy, gz, T);
		aux[1] = make_float4(target.x, target.y, target.z, C.x);
		aux[2] = make_float4(C.y, C.z, __uint_as_float(n), __uint_as_float(M));
	}
}

// ---- one lane per sample -------------------------------------------------------------------------------------------------------------------------------------
// A wave owns 64 consecutive rays (lane k holds ray k's count and base) and walks them in packets: consecutive rays whose counts fit into 64 lanes, one lane per
// sample, so that the loads of outputs and records are contiguous over the wave; a ray of more than 64 samples goes alone, in chunks of 64, and carries (T, C) from
// chunk to chunk in wave-uniform registers.  T in front of a sample is a segmented exclusive product scan of 1 - alpha; C three segmented sums.
//
// walk_samples is that walk, for both passes over the samples: the forward pass reads a ray's C out of it, the gradient pass the C in front of every sample, and
// dL/doutput needs their difference -- what lies behind the sample -- to be exact (0 behind the last consumed sample of a stopped ray).  It is, because both values are
// this one function's: the same lanes scanned in the same order.  The passes differ only in the weight they give a sample (the forward pass stops a ray) and in what
// they do with a chunk's scans.  The gradient pass takes that difference only at the ray's last sample of a chunk and sums the samples between from the far end
// (GradientBody::chunk): C - C2 at every sample carries the rounding of C into a difference that is a thousandth of it late in a ray.
constexpr uint32_t kWaveBlock = 256;
__device__ __forceinline__ uint32_t shfl_u(uint32_t v, uint32_t lane) { return (uint32_t)__shfl((int)v, (int)lane); }
__device__ __forceinline__ f3 shfl3(f3 v, uint32_t lane) { return mk3(__shfl(v.x, (int)lane), __shfl(v.y, (int)lane), __shfl(v.z, (int)lane)); }
// inclusive scans over the lanes st..lane of a segment (lane >= st)
__device__ __forceinline__ float seg_scan_mul(float x, uint32_t lane, uint32_t st) { return wave_segmented_scan(x, lane, st, [](float a, float b) { return a * b; }); }
__device__ __forceinline__ float seg_scan_add(float x, uint32_t lane, uint32_t st) { return wave_segmented_scan(x, lane, st, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ unsigned long long lane_range(uint32_t first, uint32_t last) { // bits first..last
	return ((2ull << last) - 1ull) & ~((1ull << first) - 1ull);
}
// the ray of the packet that sample lane `lane` belongs to: the first k in c..e with P_k - Ec > lane (every lane takes the same six steps)
__device__ __forceinline__ uint32_t packet_ray(uint32_t c, uint32_t e, uint32_t lane, uint32_t P, uint32_t Ec) {
	uint32_t lo = c, hi = e;
	#pragma unroll
	for (int k = 0; k < 6; ++k) {
		const uint32_t mid = min((lo + hi) >> 1, e);
		const uint32_t pm = shfl_u(P, mid) - Ec;
		if (pm > lane) hi = mid; else lo = mid + 1u;
	}
	return min(lo, e);
}

// What the walk shows its body.
struct Walk {
	uint32_t lane, n, P, E; // as a ray of the wave: its samples, the inclusive and the exclusive sum of n over the lanes
	// the packet (wave-uniform): rays c..e with tot samples, the first of them sample Ec of the wave; lng: ray c alone, and this is its chunk ch of `lanes` samples
	uint32_t c, e, tot, Ec, ch, lanes;
	bool lng;
	float Tin; f3 Cin;      // (T, C) of the chunks in front of this one
	// as a sample of the chunk: sample j of ray r (a lane of the wave), whose samples start at lane st of the chunk; record si; valid: there is such a sample
	uint32_t r, st, j; bool valid; size_t si;
	Sample q;               // (not valid: one that adds nothing)
	float x, Tb, T, w;      // the product of 1 - alpha over the ray's samples of this chunk up to this one; T in front of the sample and behind it; its weight
	f3 y, C2;               // the sums of w * rgb over the same lanes; C up to and including this sample
};
// the packet that starts at ray k.c: the rays from c on whose counts fit into 64 lanes together, or ray c alone when it is longer
__device__ __forceinline__ void next_packet(Walk& k) {
	// (tot and Ec come out of shuffles: the same in every lane, which the compiler has to be told to keep them in scalar registers)
	k.Ec = (uint32_t)__builtin_amdgcn_readfirstlane((int)shfl_u(k.E, k.c));
	uint32_t tot = shfl_u(k.n, k.c);
	k.lng = tot > 64u;
	k.e = k.c;
	if (!k.lng) {
		const unsigned long long fit = __ballot(k.lane >= k.c && k.P - k.Ec <= 64u); // P grows with the lane: a run that starts at c
		k.e = k.c + (uint32_t)__popcll(fit) - 1u;
		tot = shfl_u(k.P, k.e) - k.Ec;
	}
	k.tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
}
// body.weight(k): the sample's weight, given k.Tb.  body.chunk(k): the chunk's scans are complete; returns how many of the chunk's lanes the ray consumed (fewer than
// k.lanes ends a long ray there).  body.long_ray(k): a long ray is done, (k.Tin, k.Cin) are its T and C.
template <class Body>
__device__ __forceinline__ void walk_samples(const DeviceModel& m, const RayLossArgs& a, uint32_t n, uint32_t base, Body& body) {
	Walk k;
	const uint32_t lane = k.lane = threadIdx.x & 63u;
	k.n = n; k.P = wave_inclusive_add(n, lane); k.E = k.P - n;
	for (k.c = 0; k.c < 64u; k.c = k.e + 1u) {
		next_packet(k);
		k.Tin = 1.f; k.Cin = mk3(0, 0, 0);
		const uint32_t chunks = (k.tot + 63u) / 64u;
		for (k.ch = 0; k.ch < chunks; ++k.ch) {
			k.lanes = min(64u, k.tot - k.ch * 64u);
			k.r = k.c; k.st = 0; k.j = k.ch * 64u + lane;
			if (!k.lng) {
				k.r = packet_ray(k.c, k.e, lane, k.P, k.Ec);
				k.st = shfl_u(k.E, k.r) - k.Ec;
				k.j = lane - k.st;
			}
			k.valid = k.lng ? k.j < k.tot : lane < k.tot;
			k.si = (size_t)shfl_u(base, k.r) + k.j;
			k.q.alpha = 0.f; k.q.rest = 1.f; k.q.dt = 0.f; k.q.rgb = mk3(0, 0, 0); k.q.raw.v[0] = k.q.raw.v[1] = k.q.raw.v[2] = k.q.raw.v[3] = 0.f;
			if (k.valid) k.q = load_sample(m, a, k.si);
			k.x = seg_scan_mul(k.q.rest, lane, k.st);
			const float up = wave_lane_before(k.x);
			k.Tb = (lane == k.st ? 1.f : up) * k.Tin;
			k.T = k.x * k.Tin;
			k.w = body.weight(k);
			k.y = mk3(seg_scan_add(k.w * k.q.rgb.x, lane, k.st), seg_scan_add(k.w * k.q.rgb.y, lane, k.st), seg_scan_add(k.w * k.q.rgb.z, lane, k.st));
			k.C2 = k.Cin + k.y;
			const uint32_t used = body.chunk(k);
			if (k.lng) { // what the next chunk starts from, or the ray ends with
				if (used) { k.Cin = shfl3(k.C2, used - 1u); k.Tin = __shfl(k.T, (int)used - 1); }
				if (used < k.lanes) break;
			}
		}
		if (k.lng) body.long_ray(k);
	}
}

// The forward pass: a ray's M, C and T.  The early stop is a predicate per lane (T in front of it < EPS), balloted: the first set bit of a segment is the ray's M, and
// every lane at or behind it contributes exactly nothing.
struct ForwardBody {
	f3 C; float T; uint32_t M; // of the lane's ray
	unsigned long long bad;    // the chunk's lanes with T in front of them below EPS
	__device__ __forceinline__ float weight(const Walk& k) {
		bad = __ballot(k.valid && k.Tb < kLossEps);
		const bool active = k.valid && !(bad & lane_range(k.st, k.lane));
		return active ? k.q.alpha * k.Tb : 0.f;
	}
	// A ray's sums are read at the lane of its last consumed sample, not at the end of its segment: see walk_samples.
	__device__ __forceinline__ uint32_t chunk(const Walk& k) {
		if (k.lng) {
			const uint32_t used = bad ? (uint32_t)__builtin_ctzll(bad) : k.lanes;
			if (k.lane == k.c) M = k.ch * 64u + used; // (of the last chunk the walk comes to)
			return used;
		}
		const bool mine = k.lane >= k.c && k.lane <= k.e && k.n > 0u;
		const uint32_t first = mine ? k.E - k.Ec : 0u, last = mine ? first + k.n - 1u : 0u;
		const unsigned long long stop = bad & lane_range(first, last);
		const uint32_t Mr = stop ? (uint32_t)__builtin_ctzll(stop) - first : k.n; // >= 1 for a ray with samples: T in front of its first sample is 1
		const f3 p = shfl3(k.y, mine ? first + Mr - 1u : 0u);
		const float px = __shfl(k.x, (int)last);
		if (mine) { M = Mr; C = p; T = px; }
		return k.lanes;
	}
	__device__ __forceinline__ void long_ray(const Walk& k) {
		if (k.lane == k.c) { C = k.Cin; T = k.Tin; }
	}
};

__global__ __launch_bounds__(kWaveBlock) void ray_loss_forward_kernel(const DeviceModel m, const RayLossArgs a) {
	const uint32_t i = blockIdx.x * kWaveBlock + threadIdx.x;
	const uint32_t live = live_rays(a);
	uint32_t n = 0, base = 0;
	if (i < live) {
		n = a.numsteps[2 * i];
		base = a.numsteps[2 * i + 1];
		if (base > a.n_samples || n > a.n_samples - base || n > kTrainSteps) n = 0u; // not inside the buffers, or longer than a ray can be: no samples
	}
	ForwardBody f{mk3(0, 0, 0), 1.f, 0u, 0ull};
	walk_samples(m, a, n, base, f);
	if (i >= a.n_rays) return;
	if (i >= live) {
		RayLossWs(a.ws, a.n_rays).M[i] = 0u;
		if (a.loss) a.loss[i] = 0.f;
		return;
	}
	finish_ray(a, i, f.M, n, f.C, f.T);
}

// The gradient pass: the M' samples of every ray that fit the compact buffer, replayed (tn:1835) -- each sample's record copied to its compact place, its dL/doutput
// from what lies in front of it and behind it.
struct GradientBody {
	const DeviceModel& m;
	const RayLossArgs& a;
	uint32_t i, cbase; // the lane's ray, its compact base
	f3 C, g;           // and what the forward pass left of it
	float s, l2reg, l1reg;
	__device__ __forceinline__ float weight(const Walk& k) { return k.q.alpha * k.Tb; }
	__device__ __forceinline__ uint32_t chunk(const Walk& k) {
		const nrs_ray_loss_params& p = a.p;
		const uint32_t scbase = shfl_u(cbase, k.r);
		const f3 Cr = shfl3(C, k.r), gr = shfl3(g, k.r);
		// What lies behind a sample: the weighted colours of the ray's later samples in this chunk, summed from the ray's end towards the sample, plus what lies behind
		// the chunk's last sample of the ray (C - C2 there: 0 behind the last consumed sample of a stopped ray, both being walk_samples' values).  C - C2 at the sample
		// itself is the same number with the rounding of C on it -- half a float32 step of C, which late in a ray that is about to stop (T rgb and what lies behind it
		// both near 1e-3 of C) is hundreds of float32 steps of the difference the density gradient is made of.
		const uint32_t en = k.lng ? k.lanes - 1u : k.st + shfl_u(k.n, k.r) - 1u; // the last lane of the ray's samples in this chunk
		f3 later = k.w * k.q.rgb; // (a lane without a sample has weight 0)
		#pragma unroll
		for (uint32_t d = 1; d < 64; d <<= 1) {
			const f3 v = mk3(__shfl_down(later.x, d), __shfl_down(later.y, d), __shfl_down(later.z, d));
			if (k.lane + d <= en) later = later + v;
		}
		const f3 next = mk3(__shfl_down(later.x, 1), __shfl_down(later.y, 1), __shfl_down(later.z, 1));
		const f3 C2end = shfl3(k.C2, en & 63u);
		if (k.valid) {
			const Sample& q = k.q;
			const size_t so = (size_t)scbase + k.j;
			const float* cin = a.coords + k.si * a.ld_in;
			float* cout = a.coords_out + so * a.ld_in;
			for (uint32_t f = 0; f < a.ld_in; ++f) cout[f] = cin[f];
			const f3 behind = Cr - C2end;
			const f3 suffix = k.lane < en ? next + behind : behind;
			const f3 dr = k.w * gr;
			float dl[4];
			dl[0] = s * (dr.x * network_to_rgb_derivative(q.raw.v[0], m.rgb_activation) + fmaxf(0.0f, l2reg * q.raw.v[0]));
			dl[1] = s * (dr.y * network_to_rgb_derivative(q.raw.v[1], m.rgb_activation) + fmaxf(0.0f, l2reg * q.raw.v[1]));
			dl[2] = s * (dr.z * network_to_rgb_derivative(q.raw.v[2], m.rgb_activation) + fmaxf(0.0f, l2reg * q.raw.v[2]));
			const float by_mlp = network_to_density_derivative(q.raw.v[3], m.density_activation) * (q.dt * dot3(gr, k.T * q.rgb - suffix));
			float near_term = 0.0f;
			if (p.near_distance > 0.f && q.raw.v[3] > -10.0f) {
				const size_t ray = (size_t)(i - k.lane) + k.r;
				const f3 dv = unwarp_position(mk3(cin[0], cin[1], cin[2]), m.aabb) - mk3(a.origins[3 * ray], a.origins[3 * ray + 1], a.origins[3 * ray + 2]);
				if (sqrtf(dot3(dv, dv)) < p.near_distance) near_term = 1e-4f;
			}
			dl[3] = s * by_mlp + (q.raw.v[3] < 0.0f ? -l1reg : 0.0f) + near_term;
			store_dl(reinterpret_cast<__half*>(a.dl), a.ld_dl, a.dl_layout, so, dl);
		}
		return k.lanes;
	}
	__device__ __forceinline__ void long_ray(const Walk&) {}
};

__global__ __launch_bounds__(kWaveBlock) void ray_loss_gradient_kernel(const DeviceModel m, const RayLossArgs a) {
	const uint32_t i = blockIdx.x * kWaveBlock + threadIdx.x;
	const RayLossWs ws(a.ws, a.n_rays);
	const nrs_ray_loss_params& p = a.p;
	GradientBody b{m, a, i, 0u, mk3(0, 0, 0), mk3(0, 0, 0), p.loss_scale / (float)a.n_rays, m.rgb_activation == NRS_ACT_EXPONENTIAL ? 1e-4f : 0.0f, p.density_l1_reg ? 1e-4f : 0.0f};
	uint32_t n = 0, base = 0; // n: the samples to replay, M' (tn:1835)
	if (i < live_rays(a)) {
		const uint32_t M = ws.M[i], cap = p.max_samples_compacted;
		b.cbase = ws.cbase[i];
		n = min(cap - min(cap, b.cbase), M);
		a.numsteps_out[2 * i] = n;
		a.numsteps_out[2 * i + 1] = b.cbase;
		if (a.loss) a.loss[i] = n ? ws.loss[i] : 0.f;
		if (n) {
			base = a.numsteps[2 * i + 1];
			b.C = mk3(ws.C[0][i], ws.C[1][i], ws.C[2][i]);
			b.g = mk3(ws.g[0][i], ws.g[1][i], ws.g[2][i]);
		}
	}
	walk_samples(m, a, n, base, b);
}

// compact indices [min(*total, cap), cap): a zero record and dL rows 0..3 zero
__global__ __launch_bounds__(256) void ray_loss_tail_kernel(const RayLossArgs a) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= a.p.max_samples_compacted || k < *a.counter_out) return;
	float* c = a.coords_out + (size_t)k * a.ld_in;
	for (uint32_t q = 0; q < a.ld_in; ++q) c[q] = 0.f;
	const float z[4] = {0.f, 0.f, 0.f, 0.f};
	store_dl(reinterpret_cast<__half*>(a.dl), a.ld_dl, a.dl_layout, k, z);
}

int launch_ray_loss(const DeviceModel& m, const RayLossArgs& a, void* stream) {
	hipStream_t st = (hipStream_t)stream;
	if (a.n_rays) {
		const uint32_t blocks = (a.n_rays + kWaveBlock - 1) / kWaveBlock;
		hipLaunchKernelGGL(ray_loss_forward_kernel, dim3(blocks), dim3(kWaveBlock), 0, st, m, a);
		NRS_LAUNCH_CHECK("ray_loss_forward_kernel launch");
		const RayLossWs ws(a.ws, a.n_rays);
		const int status = launch_train_scan<false>(a.n_rays, a.ray_counter, ws.M, ws.tiles, ws.cbase, nullptr, 0u, a.counter_out, nullptr, st);
		if (status != NRS_OK) return status;
		hipLaunchKernelGGL(ray_loss_gradient_kernel, dim3(blocks), dim3(kWaveBlock), 0, st, m, a);
		NRS_LAUNCH_CHECK("ray_loss_gradient_kernel launch");
	} else {
		const hipError_t e = hipMemsetAsync(a.counter_out, 0, sizeof(uint32_t), st);
		if (e != hipSuccess) return hip_fail(e, "nrs_ray_loss: zeroing the counter");
	}
	hipLaunchKernelGGL(ray_loss_tail_kernel, dim3((a.p.max_samples_compacted + 255) / 256), dim3(256), 0, st, a);
	NRS_LAUNCH_CHECK("ray_loss_tail_kernel launch");
	return NRS_OK;
}

} // namespace nrs
