// nrs_kernels.hip -- HIP kernels of the NeRFshop render path for gfx950 (MI355X), wave64.
//
//   render_kernel        one persistent launch per frame: rays are pulled in 8x8-pixel packets from a device-side
//                        queue, marched, warped, encoded, evaluated on MFMA and composited in registers.  It replaces
//                        the reference's per-iteration launch train + host syncs: no NerfPayload / network
//                        input / network output arrays exist in HBM; the only traffic is the hash-table gather, the
//                        occupancy bitfield, the cage tables and one float4 per hit pixel.
//                        Template parameter TEAM: 1 lane per ray, 2 / 4 lanes per ray (lane teams, for launches that cannot
//                        fill the GPU), or 0 = every generation sizes its teams by the rays its wave has pending: the
//                        small-launch schedule (packets of 16 / 32 / 64 pixels by the size of the launch: the automatic choice
//                        since round 3) and the hybrid schedule (one lane per ray for the bulk of a whole image's queue, teams
//                        for its tail).  TEAM == 0 waves re-team when a generation has thinned out, test a team's next positions
//                        in parallel, and hand rays over to waves of their workgroup that have run out of work.
//   network_kernel       NerfNetwork::inference_mixed_precision / density / hash-grid encode on caller batches.
//   cell_records_kernel  the cell-record cache of the coarse hash-grid levels (nrs_model_set_cell_cache).
//   grid_eval_kernel     get_density_on_grid / get_rgba_on_grid; grid_refresh / grid_ema: the occupancy refresh.
//   selection_rays_kernel, poisson_fit_kernel   the selection tool's ray shooting, the membrane boundary fit.
//   map_rays_kernel      EditOperator::map_rays / map_positions on caller batches.
//   trace_samples_kernel test hook: the (t, dt) stream of listed pixels.
//   grid -> bitfield     update_density_grid_mean_and_bitfield.
//   detile_kernel        multi-GPU tile scatter.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <utility>
#include "nrs_internal.h"
#include "nrs_device.cuh"
#include "nrs_mlp.cuh"

namespace nrs {

static thread_local char g_launch_err[512];
const char* launch_last_error() { return g_launch_err; }
static int hip_fail(hipError_t e, const char* what) {
	snprintf(g_launch_err, sizeof(g_launch_err), "%s: %s", what, hipGetErrorString(e));
	return NRS_ERR_HIP;
}
#define NRS_LAUNCH_CHECK(what)                               \
	do {                                                     \
		hipError_t e_ = hipGetLastError();                   \
		if (e_ != hipSuccess) return hip_fail(e_, what);     \
	} while (0)

// The hand-over words in LDS are polled and published with relaxed atomics: a `volatile` access through a generic pointer loses the LDS address space and
// becomes a FLAT load (aperture check, both wait counters) -- one per round at the top of the frame loop.
__device__ __forceinline__ uint32_t lds_peek(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void lds_poke(uint32_t* p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
constexpr int kRing = 128; // pending-ray ring entries per wave (>= 63 + 64)
// A wave takes new rays only when this many of its lanes are idle.  64 = "generations": all lanes are (re)filled at once with the hits
// of the next few neighbouring packets, the rays then advance in step -- similar depth, neighbouring pixels -- and the wave's
// gathers share cache lines; lanes whose ray ends early idle until the generation is over.  Measured (1080p lego, cage edit):
// 1 (refill every idle lane at once, 98 % of lanes busy) 7.41 Gsamples/s, 16/32 7.08, 48 7.60, 56 7.78, 60 7.80, 64 8.09 -- once
// the marcher's VALU diet made the gather's L1/TA path the first limiter, coherence became worth more than occupancy (aabb-16
// scene: 3.49 -> 3.92).
constexpr int kTeamMax = 4; // the widest lane team of the automatic schedule (eight lanes per ray once a wave holds <= 8 rays was measured and loses: profiles/r03_schedules.md)
// Measurement builds (-DNRS_MEASURE=<n>; production: undefined): 1 fill, 2 cage warp, 3 gather, 4 MLPs, 5 march executed twice (results unchanged) -- the frame time's
// difference is that phase's marginal cost; 9 = ISA listing with phase markers (tools/isa_phases.py: comments only, for counting instructions per phase).
#ifndef NRS_MEASURE
#define NRS_MEASURE 0
#endif
constexpr uint32_t kRefillWhenIdle = 64;
// (Round 6 measured the middle ground once more on the automatic schedule: idle lanes refilled in place from 16 / 32 / 48 idle lanes while the queue has packets, instead of
// re-teaming the survivors of a thinned generation: lego + cage 12.5 -> 11.4 / 11.4 / 11.8, varied 11.2 -> 9.7 / 9.1 / 9.8 Gsamples/s; profiles/r06/ab_refill_*.txt.)

template <int WAVES>
struct RenderSmem {
	ModelLds ml;
	FeatLds fl[WAVES];
	uint2 ring[WAVES][kRing]; // {x | y << 16, t bits}; the output index follows from the pixel (pixel_out_idx).  BATCH: {x | y << 13 | sample << 26, t bits} (kBatchXYBits)
	uint32_t coarse[kMarchLdsWords]; // DeviceModel::coarse_mask (marching shortcut 2) | the Morton spread table (stage_march_lds)
	unsigned long long queue;       // the workgroup's chunk of the frame's packet queue: next packet | end << 32 (claim_packet)
	unsigned long long sum_samples; // statistics of the workgroup's waves, flushed by the last one to finish
	uint32_t sum_alive, sum_hit, n_finished;
	// ray hand-over between the waves of a workgroup (render_body, "donate"): waves that wait for rays (bit per wave), waves that still hold some,
	// and per waiting wave the number of rays a sibling has put into its FeatLds (0 = none yet)
	uint32_t idle_mask, n_busy, mail[WAVES];
};

// (XCD-aware order -- one cursor per XCD over stripes of 8 / 16 / 32 / 64 pixel rows, workgroups of an XCD working on neighbouring packets so
// that they share their L2, with stealing at the end -- was built and measured in round 2: 1080p lego 9.58 -> 9.67 / 9.47 / 9.24 / 8.68
// Gsamples/s, aabb-16 4.36 -> 4.35 / 4.34 / 4.35 / 4.24: the L2 misses of this kernel come from the fine levels, whose lines no two
// samples share wherever they run (profiles/r02_gather_probe.md), so there is nothing for a shared L2 to keep.  One queue it stays.)
// The frame's work queue is one device-wide counter.  Device-scope atomics on one address serialise across the 8 XCDs at
// ~18 ns each (an all-miss 1080p frame, 32 400 packets, took 0.57 ms for that reason alone), so the waves of a workgroup
// share a chunk of kQueueChunk packets held in LDS and only the wave that finds the chunk used up goes to the global
// counter.  State word: low half = next packet of the chunk, high half = its end; bit 31 of the low half = queue dry.
// Round 3: kQueueChunk 8 -> 2.  With 64-pixel packets a chunk of 8 is 200 rays that only one workgroup can see, and its 8 waves march through neighbouring
// packets in step; chunks of 16 / 8 / 4 / 2 / 1: 10.0 / 11.2 / 11.8 / 12.0 / 11.7 Gsamples/s on lego + cage, 8.4 / 9.6 / 10.3 / 10.6 / 10.8 on the varied scene, a 1/8 share
// 0.509 (8) / 0.494 / 0.496 / 0.532 ms (chunks of 1 pay the atomics: 16 640 of them in half a millisecond); shrinking chunks towards the end of the queue only
// ("guided") was no better than a constant 4.
constexpr uint32_t kGiveMin = 16u; // ray hand-over: a wave gives half of the rays it holds in lanes when it holds more than this many
constexpr uint32_t kFullGen = 56u; // small-launch schedule with 64-pixel packets: pending rays from which a generation runs one lane per ray
constexpr uint32_t kQueueChunk = 2;
constexpr uint32_t kNoPacket = 0xffffffffu;
__device__ __forceinline__ uint32_t claim_packet(unsigned long long* state, uint32_t* global_next, uint32_t n_packets, int lane) {
	uint32_t result = kNoPacket;
	if (lane == 0) {
		for (;;) {
			const unsigned long long old = atomicAdd(state, 1ull);
			const uint32_t cur = (uint32_t)old, end = (uint32_t)(old >> 32);
			if (cur & 0x80000000u) break; // dry
			if (cur < end) { result = cur; break; }
			if (cur == end) { // the first wave past the end fetches the next chunk (and takes its first packet)
				const uint32_t chunk = kQueueChunk;
				const uint32_t base = atomicAdd(global_next, chunk);
				if (base >= n_packets) {
					atomicExch(state, 0x80000000ull);
				} else {
					const uint32_t e = min(base + chunk, n_packets);
					atomicExch(state, ((unsigned long long)e << 32) | (unsigned long long)(base + 1u));
					result = base;
				}
				break;
			}
			for (;;) { // another wave is fetching: wait for the new chunk (its end differs: the global counter only grows)
				const unsigned long long s = __atomic_load_n(state, __ATOMIC_RELAXED);
				if ((uint32_t)(s >> 32) != end || ((uint32_t)s & 0x80000000u)) break;
				__builtin_amdgcn_s_sleep(2);
			}
		}
	}
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)result);
}

// packet -> pixel of this lane.  Packets are 8x8 pixel blocks; with lane teams (TEAM lanes per ray) a packet is the 64 / TEAM
// pixels of an 8x4 / 4x4 block and the TEAM lanes of a team stand on the same pixel.
template <int TEAM>
__device__ __forceinline__ bool packet_pixel(const RenderArgs& a, uint32_t pk, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	constexpr uint32_t PW = TEAM >= 16 ? 2u : (TEAM >= 4 ? 4u : 8u), PH = 64u / TEAM / PW; // 8x8, 8x4, 4x4, 4x2, 2x2
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	const uint32_t idx = (uint32_t)lane / TEAM;
	const uint32_t lx = idx % PW, ly = idx / PW;
	if (a.p.tile_size == 0) {
		// whole image: packets in row-major order (runs of neighbouring packets per claim were measured and lose: a wave's
		// unstarted packets are invisible to idle waves)
		// (packet rows from the middle of the image outwards -- thick rays first, silhouettes last -- measured in round 6: -4 % lego, -1 % varied, -11 % membrane:
		// neighbouring rows share more than a shorter tail saves; profiles/r06/ab_roworder_*.txt)
		const uint32_t bx = pk % a.tiles_x, by = pk / a.tiles_x;
		x = bx * PW + lx;
		y = by * PH + ly;
		out_idx = x + W * y;
	} else {
		const uint32_t ppt = a.packets_per_tile_x * (a.p.tile_size / PH);
		const uint32_t k = pk / ppt, b = pk % ppt;
		const uint32_t stride = a.p.tile_stride ? a.p.tile_stride : 1;
		const uint32_t T = a.p.tile_first + k * stride;
		const uint32_t Tx = T % a.tiles_x, Ty = T / a.tiles_x;
		const uint32_t tx = (b % a.packets_per_tile_x) * PW + lx, ty = (b / a.packets_per_tile_x) * PH + ly;
		x = Tx * a.p.tile_size + tx;
		y = Ty * a.p.tile_size + ty;
		out_idx = (k * a.p.tile_size + ty) * a.p.tile_size + tx;
	}
	return x < W && y < H;
}

// WAVES = waves per workgroup (they share one LDS copy of the weights); OCC = waves per SIMD the register allocator must
// leave room for (__launch_bounds__' second argument).
// PROF adds s_memtime stamps around the phases of a round (NRS_DEBUG & 4); the production instantiation has none.
#if NRS_MEASURE == 9
#define NRS_MARK(i) asm volatile("; NRS_MARK " #i)
#else
#define NRS_MARK(i)
#endif
// (wave priorities per phase -- s_setprio around the memory phases or the MFMA chain -- and the next sample's occupancy word requested ahead of the MLPs were
// measured and are gone: profiles/r03_schedules.md, profiles/r05/ab_small_knobs.txt)
#define NRS_PHASE(i)                                                         \
	do {                                                                     \
		NRS_MARK(i);                                                         \
		if (PROF) {                                                          \
			const unsigned long long now_ = __builtin_amdgcn_s_memtime();     \
			ph_acc[ph_cur] += now_ - ph_last;                                \
			ph_last = now_;                                                  \
			ph_cur = (i);                                                    \
		}                                                                    \
	} while (0)

// POISSON compiles in the membrane correction (off by default in the reference): a separate instantiation, so
// the common path pays neither its registers nor its code.
// AFFINE compiles in the AffineDuplication operator (edit_warp's second kind): frames whose operators are all cage
// deformations -- the common case and the benchmark -- run the instantiation without it (2 % faster: 122 vs 128 VGPRs).
// where pixel (x, y) of this launch lands in the caller's buffers: packet_pixel's out_idx from the pixel alone
__device__ __forceinline__ uint32_t pixel_out_idx(const RenderArgs& a, uint32_t x, uint32_t y) {
	if (a.p.tile_size == 0) return x + (uint32_t)a.p.resolution[0] * y;
	const uint32_t ts = a.p.tile_size, Tx = x / ts, Ty = y / ts, T = Ty * a.tiles_x + Tx;
	const uint32_t stride = a.p.tile_stride ? a.p.tile_stride : 1;
	const uint32_t k = (T - a.p.tile_first) / stride;
	return (k * ts + (y - Ty * ts)) * ts + (x - Tx * ts);
}

// Hybrid launches (TEAM == 0, whole-image mode): every tail_every-th (3rd) packet row of the image is taken out of the 8x8 packet
// list and appended to the queue as 4x4 packets ("tail" packets, a uniform sample of the picture, so the same share of the rays
// whatever the scene).  Waves that reach them switch to lane teams: the last rays of a frame then take a quarter of a
// ray's life while the waves still on their last 64-ray generation finish (see render_kernel).
__device__ __forceinline__ bool packet_pixel_bulk(const RenderArgs& a, uint32_t pk, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	const uint32_t rb = pk / a.tiles_x, col = pk % a.tiles_x, row = rb + rb / (a.tail_every - 1u); // every tail_every-th row is a tail row
	x = col * 8u + ((uint32_t)lane & 7u);
	y = row * 8u + ((uint32_t)lane >> 3);
	out_idx = x + W * y;
	return x < W && y < H;
}
__device__ __forceinline__ bool packet_pixel_tail(const RenderArgs& a, uint32_t q, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	// a tail row is 8 pixels high; its packets are 4x4 / 8x4 / 8x8 pixels with fill_lanes = 4 / 2 / 1 lanes on a pixel (as in packet_pixel<4 / 2 / 1>)
	const uint32_t L = a.fill_lanes, cols = L == 4u ? a.tiles_x * 2u : a.tiles_x, per_row = cols * (L == 1u ? 1u : 2u);
	const uint32_t trow = q / per_row, s = q % per_row, sy = s / cols, sx = s % cols;
	const uint32_t idx = (uint32_t)lane / L, pw = L == 4u ? 4u : 8u;
	x = sx * pw + (idx % pw);
	y = (trow * a.tail_every + a.tail_every - 1u) * 8u + sy * 4u + (idx / pw);
	out_idx = x + W * y;
	return x < W && y < H;
}

// TEAM = lanes per ray (1, 2, 4) -- *lane teams* for launches with too few rays to fill the GPU (one GPU's tiles of a frame
// sharded over 4-8 GPUs).  A ray needs one round per sample and a round is a latency chain, so such a launch takes one
// ray's life (~30 rounds) however few rays it has.  With TEAM lanes per ray, lane k of a team stands k samples ahead of
// lane 0 (same marching arithmetic, same t values), all evaluate their sample in the same round, then every lane of the
// team composites the TEAM samples in order (identical float operations => identical accumulators in every lane, the
// result of the sequential loop bit for bit) and walks TEAM samples on.  Samples past the one that saturates the ray are
// discarded, as the reference discards the rest of a batch (tn:951-960).  The fill works on 64 / TEAM pixels per packet.
// NUM: 0 = the default roundings compiled in; kNumRuntime = tiny-cuda-nn's other roundings chosen at run time from DeviceModel::numerics (bit 0 grid
//      accumulation in network precision, bit 1 fp16 MLP accumulators; wave-uniform branches, both flavours in the code): every schedule and every
//      operator combination has such a twin, so no entry point refuses a rounding mode.
// EXTRA: the rest of render_nerf's surface -- composite_kernel_nerf's per-sample render modes (AO / Positions / Depth / Distance / Stepsize, tn:905-937),
//      show_accel's opaque samples (tn:788-790), shade's mode handling (tn:2466-2478) and pixel_to_ray's thin-lens branch (common_device.cuh:285-293).
//      A separate instantiation (one lane per ray): the Shade / Cost kernels carry none of it.
// XTRA: 0 = none of it, 1 = EXTRA, 2 = EXTRA + INTRO: render modes Normals and EncodingVis (the network's input gradient / a visualised activation per sample,
//      tn:2923-2927: a second pass over the hash grid and a backward or partial forward pass of the MLPs -- a separate instantiation again);
//      3 / 4 = 1 / 2 with a third hidden layer in the rgb MLP (DeviceModel::rgb_deep, configs/nerf/base_3layer.json), 5 = that layer and nothing else of EXTRA: the
//      automatic schedule's instantiation for such a network (plain Shade / Cost frames; nrs_render_nerf decides); 6 = the plain kernel with the L2 phase gate (GATE).
// BATCH: the queue holds the packets of RenderArgs::spp_count samples of the view (nrs_render_nerf_spp): K times the packet list of one sample -- under the hybrid schedule all
//      samples' 8x8 packets, then all samples' tail packets, so that the launch still has one tail and one drain.  The sample s of a packet is wave-uniform (claim_packet hands
//      one packet to the whole wave): the fill forms the pixel offsets and the Sobol draws of sample spp_index + s and writes to slab s of the buffers (+ s * slab_stride
//      pixels); a ring entry carries s (6 bits beside 13-bit pixel coordinates: nrs_render_nerf_spp refuses what does not fit).  From its first hit on a ray is an ordinary
//      ray.  The instantiations without it are what they were before the flag existed: a single frame pays nothing for it.
constexpr uint32_t kBatchXYBits = 13u, kBatchXYMask = (1u << kBatchXYBits) - 1u;
static_assert((NRS_SPP_BATCH_MAX - 1u) >> (32u - 2u * kBatchXYBits) == 0u, "a ring entry holds the sample index beside the pixel");
template <int WAVES, int OCC, bool PROF, bool POISSON, bool AFFINE, int TEAM, int NUM = 0, int XTRA = 0, bool BATCH = false>
__device__ __forceinline__ void render_body(const DeviceModel& m_arg, const RenderArgs& a_arg) {
	constexpr XtraTraits kX = xtra_traits(XTRA); // (nrs_route.h: the host plans routes with the same decoder)
	constexpr bool EXTRA = kX.extra, INTRO = kX.intro, DEEP = kX.deep; // (3 / 4: 1 / 2 for a network whose rgb MLP has a third hidden layer, base_3layer.json; 5: that layer alone)
	// 7 / 8: a network trained with light directions (DeviceModel::n_extra_dims = 3; rgb_mlp's LIGHT).  7 = the light term and nothing else: the twin of the default kernel
	// (plain frames and cage edits on the automatic schedule); 8 = the catch-all of such a network: EXTRA + INTRO, the third hidden layer where the network has one
	// (DeviceModel::rgb_deep, a wave-uniform run-time branch here), every numerics, AffineDuplication -- whatever 7 does not serve.
	constexpr bool LIGHT = kX.light;
	// four levels per round trip in the gathers (encode_to_lds QUADS): the automatic schedule's instantiations with the default or the fully tiny-cuda-nn roundings -- since
	// round 6 the membrane instantiation too (both of its gathers: 9.68 -> 10.06 Gsamples/s, same registers; profiles/r06/ab_poisson_quads.txt)
	constexpr bool kQuads = TEAM == 0 && !EXTRA && NUM >= 0;
	constexpr int GATE = kX.gate ? (int)kGateMaxPhases : 0; // the plain kernel with the L2 phase gate on the four finest hashed levels (encode_to_lds): cone-stepping scenes
	// The two argument structs (~1.3 KB of wave-uniform values) live in the kernel-argument segment and are read with scalar loads.
	// Left alone, the compiler hoists every such load out of the frame loop and then spills ~150 scalar registers into VGPR lanes
	// (v_writelane / v_readlane: VALU slots in the round loop, 3 VGPRs).  NRS_FRESH_ARGS re-derives the two references from an
	// offset the compiler cannot see through (always 0), so the loads of a phase stay inside that phase: short-lived SGPRs, re-read
	// from the scalar cache on use.
	#define NRS_FRESH_ARGS(m, a)                                                                          \
		uint32_t zofs_##m = 0;                                                                            \
		asm volatile("" : "+s"(zofs_##m));                                                                \
		const DeviceModel& m = *reinterpret_cast<const DeviceModel*>(reinterpret_cast<const char*>(&m_arg) + zofs_##m); \
		const RenderArgs& a = *reinterpret_cast<const RenderArgs*>(reinterpret_cast<const char*>(&a_arg) + zofs_##m);
	const DeviceModel& m = m_arg;
	const RenderArgs& a = a_arg;
	__shared__ RenderSmem<WAVES> sm;
	__shared__ uint32_t poisson_stash[(POISSON && !AFFINE) ? WAVES * 64 : 1]; // per lane: the tet the first operator's warp found (see warp_scan)
	stage_march_lds(sm.coarse, m.occ.mask);
	if (threadIdx.x == 0) { sm.queue = 0ull; sm.sum_samples = 0ull; sm.sum_alive = 0u; sm.sum_hit = 0u; sm.n_finished = 0u; sm.idle_mask = 0u; sm.n_busy = (uint32_t)WAVES; }
	if (threadIdx.x < WAVES) sm.mail[threadIdx.x] = 0u;
	stage_model_to_lds(m, sm.ml, a.dbg); // (ends with the barrier that also publishes sm.coarse and the words above)

	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int g = lane >> 5;
	// lanes per ray of the current generation: TEAM, or chosen per generation in hybrid launches (TEAM == 0)
	uint32_t gen_t = TEAM ? (uint32_t)TEAM : 1u;
	int tk = lane & (int)(gen_t - 1u), team_base = lane & ~(int)(gen_t - 1u); // position in the lane team, its first lane
	bool tail_seen = false; // TEAM == 0: this wave has reached the queue's tail packets
	uint2* ring = sm.ring[wave];
	FeatLds& fl = sm.fl[wave];
	const nrs_render_params& p = a.p;
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	const bool ops = p.apply_operators && a.n_edits > 0;

	float off_x, off_y; // wave-uniform: kept in scalar registers
	ld_random_pixel_offset(p.snap_to_pixel_centers ? 0u : p.spp_index, off_x, off_y);
	off_x = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(off_x)));
	off_y = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(off_y)));

	// ---- per-lane ray state (registers) ----
	bool have = false;
	bool valid = true; // TEAM > 1: this lane's sample exists (the ray has not left the render box before it)
	f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
	float t = 0.f;
	float cr = 0.f, cg = 0.f, cb = 0.f, ca = 0.f; // accumulated premultiplied colour / alpha
	float ray_depth = 0.f, max_weight = 0.f;
	uint32_t out_idx = 0, n_steps = 0;
	// ---- wave-uniform queue state ----
	uint32_t ring_head = 0, ring_count = 0;
	bool more = true;
	// ---- statistics ----
	uint32_t st_samples = 0, st_alive = 0, st_hit = 0;
	unsigned long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ph_last = PROF ? __builtin_amdgcn_s_memtime() : 0ull;
	unsigned long long pf_rounds = 0, pf_packets = 0, pf_tq = 0, pf_rounds_q = 0;
	unsigned long long pf_walk[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // see RenderCounters::walk
	const unsigned long long pf_wall0 = PROF ? wall_clock64() : 0ull; // 100 MHz, identical on every XCD (s_memtime is the per-XCD shader clock)
	int ph_cur = 0;

	for (;;) {
		NRS_FRESH_ARGS(m1, a1);
		const nrs_render_params& p1 = a1.p;
		NRS_PHASE(0); // fill
		// ---- the end of a wave's work (TEAM == 0): nothing left to claim, nothing pending, and at most half of the lanes still hold a ray --
		// the survivors are the long rays, and each of them costs one latency-bound round per sample whatever the wave's occupancy.  Spread them
		// over the idle lanes: 2 or 4 lanes per ray, as in a team generation (lane k of a team stands k samples ahead, all composite the team's
		// samples in order: same bits).  The state of a ray moves with 15 shuffles, once.
		// ---- ray hand-over (TEAM == 0): the queue is dry and this wave still holds more rays than run at four lanes each, while a sibling wave of the
		// workgroup has run out of work and waits.  Half of the rays move to it through its (idle) FeatLds: 15 words per ray, written by the lead lanes;
		// both waves then re-team (the block below here, the pick-up there), so the rays of both halves advance twice as many samples per round.
		// The state of a ray at this point is its lead lane's registers (as for re-teaming): same float operations afterwards, same bits.
		// (A wave in the middle of a generation does not look at the queue; a waiting sibling is how it learns that the queue is dry.)
		// Rays that wait in this wave's ring for its next generation go first (two words per ray, copied into the sibling's ring: it starts them at once).
		if (TEAM == 0 && a1.steal && __builtin_amdgcn_readfirstlane((int)lds_peek(&sm.idle_mask)) != 0) {
			more = false;
			int ln = lane; // (opaque copy: lane predicates of this rare block are then formed here, not hoisted into scalar-register pairs that live through the frame loop)
			asm volatile("" : "+v"(ln));
			auto claim_waiting_wave = [&]() -> uint32_t { // the wave whose bit this wave clears is this wave's to serve: it waits for the mail
				uint32_t target = 0xffffffffu;
				if (ln == 0) {
					uint32_t idle = lds_peek(&sm.idle_mask);
					while (idle) {
						const uint32_t w = (uint32_t)__builtin_ctz(idle), bit = 1u << w;
						const uint32_t old = atomicAnd(&sm.idle_mask, ~bit);
						if (old & bit) { target = w; break; }
						idle = old & ~bit;
					}
					if (target != 0xffffffffu) atomicAdd(&sm.n_busy, 1u); // (on the receiver's behalf, before it can look)
				}
				return (uint32_t)__builtin_amdgcn_readfirstlane((int)target);
			};
			if (ring_count != 0u) {
				if (__any(have)) { // (a wave without running rays starts its pending ones itself, below)
					const uint32_t target = claim_waiting_wave();
					if (target != 0xffffffffu) {
						const uint32_t n = min(ring_count, 64u);
						if ((uint32_t)ln < n) sm.ring[target][ln] = ring[(ring_head + (uint32_t)ln) & (kRing - 1)];
						ring_head += n;
						ring_count -= n;
						__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
						__builtin_amdgcn_wave_barrier();
						if (ln == 0) { lds_poke(&sm.mail[target], n | 0x80000000u); atomicAdd(&a1.counters->walk[7], (unsigned long long)n | (1ull << 32)); }
					}
				}
			} else if (ring_count == 0u) {
				const unsigned long long lead_mask = __ballot(have && tk == 0);
				const uint32_t live = (uint32_t)__popcll(lead_mask);
				const uint32_t target = live > kGiveMin ? claim_waiting_wave() : 0xffffffffu;
				if (target != 0xffffffffu) {
					const uint32_t keep = (live + 1u) / 2u, give = live - keep;
					const bool team_live = ((lead_mask >> team_base) & 1ull) != 0ull;
					const uint32_t lead_rank = (uint32_t)__popcll(lead_mask & ((1ull << team_base) - 1ull));
					const bool moved = team_live && lead_rank >= keep;
					uint32_t* mb = &sm.fl[target].feat[0][0][0];
					if (moved && tk == 0) {
						const uint32_t r = lead_rank - keep;
						mb[0 * 32 + r] = __float_as_uint(o.x); mb[1 * 32 + r] = __float_as_uint(o.y); mb[2 * 32 + r] = __float_as_uint(o.z);
						mb[3 * 32 + r] = __float_as_uint(d.x); mb[4 * 32 + r] = __float_as_uint(d.y); mb[5 * 32 + r] = __float_as_uint(d.z);
						mb[6 * 32 + r] = __float_as_uint(t);
						mb[7 * 32 + r] = __float_as_uint(cr); mb[8 * 32 + r] = __float_as_uint(cg); mb[9 * 32 + r] = __float_as_uint(cb); mb[10 * 32 + r] = __float_as_uint(ca);
						mb[11 * 32 + r] = __float_as_uint(ray_depth); mb[12 * 32 + r] = __float_as_uint(max_weight);
						mb[13 * 32 + r] = out_idx; mb[14 * 32 + r] = n_steps;
					}
					if (moved) have = false;
					__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
					__builtin_amdgcn_wave_barrier();
					if (ln == 0) { lds_poke(&sm.mail[target], give); atomicAdd(&a1.counters->walk[7], (unsigned long long)give | (1ull << 32)); }
				}
			}
		}
		if (TEAM == 0 && a1.reteam && (((a1.reteam & 2u) && tail_seen) || (!more && ring_count == 0u))) { // (bit 1: at any time once the wave runs tail generations, not only at its end) // (bit 1: at any time once the wave runs tail generations, not only at its end)
			const unsigned long long lead_mask = __ballot(have && tk == 0);
			const uint32_t live = (uint32_t)__popcll(lead_mask);
			const uint32_t new_t = live <= 16u ? 4u : (live <= 32u ? 2u : 1u);
			if (live != 0u && new_t > gen_t) {
				if (have && tk == 0) {
					const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(lead_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lead_mask, 0u));
					fl.feat[0][0][rank] = (uint32_t)lane; // (the feature staging area is free between rounds: scratch)
				}
				__builtin_amdgcn_wave_barrier();
				const uint32_t r = (uint32_t)lane / new_t;
				const int src = r < live ? (int)fl.feat[0][0][r] : lane;
				__builtin_amdgcn_wave_barrier();
				o.x = __shfl(o.x, src, 64); o.y = __shfl(o.y, src, 64); o.z = __shfl(o.z, src, 64);
				d.x = __shfl(d.x, src, 64); d.y = __shfl(d.y, src, 64); d.z = __shfl(d.z, src, 64);
				t = __shfl(t, src, 64);
				cr = __shfl(cr, src, 64); cg = __shfl(cg, src, 64); cb = __shfl(cb, src, 64); ca = __shfl(ca, src, 64);
				ray_depth = __shfl(ray_depth, src, 64); max_weight = __shfl(max_weight, src, 64);
				out_idx = (uint32_t)__shfl((int)out_idx, src, 64); n_steps = (uint32_t)__shfl((int)n_steps, src, 64);
				have = r < live;
				valid = true;
				gen_t = new_t;
				tk = lane & (int)(gen_t - 1u);
				team_base = lane & ~(int)(gen_t - 1u);
				if (have) {
					for (int j = 0; j < tk && valid; ++j) {
						t += calc_dt(t, p1.cone_angle_constant);
						f3 npos; float ndt;
						valid = march_to_occupied(p1, m1, sm.coarse, o, d, t, npos, ndt, nullptr);
					}
				}
			}
		}
		const unsigned long long free_mask = __ballot(!have);
		const uint32_t nfree = (uint32_t)__popcll(free_mask);

		// ---- fill the ring with rays that found an occupied cell (init_rays + advance_pos_nerf) ----
		// (Measured: moving this into its own lean kernel does not pay -- the DDA's dependent bitfield loads overlap with
		// other waves' gather/MLP work here for free, while a separate launch adds ~1 ms of serial time at 1080p.)
		while (more && ring_count < (TEAM > 1 ? 64u / gen_t : (TEAM == 0 && tail_seen ? a1.tail_target : nfree)) && nfree >= kRefillWhenIdle) {
			uint32_t pk = claim_packet(&sm.queue, &a1.counters->next_packet, a1.n_packets, lane);
			if (pk == kNoPacket) { more = false; if (PROF) { pf_tq = wall_clock64() - pf_wall0; pf_rounds_q = pf_rounds; } break; }
			if (PROF) ++pf_packets;
			// BATCH: the packet's sample (wave-uniform: scalar registers) and its number in that sample's own list
			uint32_t bs = 0u;
			bool b_small = false;
			float fo_x = off_x, fo_y = off_y;
			if (BATCH && a1.spp_count > 1u) {
				uint32_t per = a1.spp_packets;
				if (TEAM == 0 && !a1.all_tail && a1.p_big) { // hybrid: [0, p_big) the samples' 8x8 packets, behind them the samples' tail packets
					b_small = pk >= a1.p_big;
					per = b_small ? a1.spp_packets - a1.spp_big : a1.spp_big;
					pk = b_small ? pk - a1.p_big : pk;
				}
				bs = pk / per;
				pk -= bs * per;
			}
			const uint32_t spp = p1.spp_index + bs;
			if (BATCH) {
				ld_random_pixel_offset(p1.snap_to_pixel_centers ? 0u : spp, fo_x, fo_y);
				fo_x = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(fo_x)));
				fo_y = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(fo_y)));
			}
			uint32_t x, y, oi;
			bool alive = false;
			float t0 = 0.f;
			bool small = TEAM > 1, inside;
			if (TEAM == 0 && a1.all_tail) { // a launch of 4x4 packets only (few rays for the GPU): every generation sizes its teams
				small = true;
				tail_seen = true;
				// (a1.fill_lanes lanes stand on one pixel during the fill: packets of 16 / 32 / 64 pixels)
				inside = a1.fill_lanes == 4u ? packet_pixel<4>(a1, pk, lane, x, y, oi) : (a1.fill_lanes == 2u ? packet_pixel<2>(a1, pk, lane, x, y, oi) : packet_pixel<1>(a1, pk, lane, x, y, oi));
			} else if (TEAM == 0 && a1.p_big) {
				small = BATCH && a1.spp_count > 1u ? b_small : pk >= a1.p_big;
				tail_seen = tail_seen || small;
				inside = small ? packet_pixel_tail(a1, BATCH && a1.spp_count > 1u ? pk : pk - a1.p_big, lane, x, y, oi) : packet_pixel_bulk(a1, pk, lane, x, y, oi);
			} else {
				inside = packet_pixel<(TEAM ? TEAM : 1)>(a1, pk, lane, x, y, oi);
			}
			const bool first_of_team = TEAM == 0 ? (!small || (lane & (int)(a1.fill_lanes - 1u)) == 0) : tk == 0;
			if (BATCH) oi += bs * a1.slab_stride;
			if (inside) {
				Ray r = BATCH ? init_ray<EXTRA, true>(p1, x, y, fo_x, fo_y, spp) : init_ray<EXTRA>(p1, x, y, off_x, off_y);
				if (first_of_team) {
					a1.depth[oi] = 1e10f; // tn:2586
					if (a1.steps) a1.steps[oi] = 0;
				}
				alive = r.alive;
				if (EXTRA) {
					if (p1.d_envmap) reinterpret_cast<float4*>(a1.frame)[oi] = read_envmap(p1.d_envmap, p1.envmap_resolution, r.d); // tn:2590-2592: replaces the frame value
					if (alive && p1.render_mode == NRS_RENDER_DISTORTION) { // tn:2602-2613: the distortion map as a picture; nothing is traced
						float d0 = 0.f, d1 = 0.f;
						if (p1.d_distortion_map) {
							read_image2(p1.d_distortion_map, p1.distortion_resolution, ((float)x + 0.5f) / (float)p1.resolution[0], ((float)y + 0.5f) / (float)p1.resolution[1], d0, d1);
							d0 = d0 * 50.0f + 0.5f; d1 = d1 * 50.0f + 0.5f;
						} else {
							d0 = 0.5f; d1 = 0.5f;
						}
						reinterpret_cast<float4*>(a1.frame)[oi] = make_float4(d0, d1, 0.5f, 1.0f);
						a1.depth[oi] = 1.0f;
						alive = false;
					}
				}
				uint32_t it_fill = 0;
#if NRS_MEASURE == 1
				if (alive) { Ray r2 = r; const bool a2 = first_hit(p1, m1, sm.coarse, x + (uint32_t)p1.resolution[0] * y, r2, nullptr); asm volatile("" :: "v"(r2.t), "s"((int)__ballot(a2))); }
#endif
				if (alive) alive = BATCH ? first_hit<true>(p1, m1, sm.coarse, x + (uint32_t)p1.resolution[0] * y, r, PROF ? &it_fill : nullptr, spp)
				                         : first_hit(p1, m1, sm.coarse, x + (uint32_t)p1.resolution[0] * y, r, PROF ? &it_fill : nullptr);
				if (PROF) {
					uint32_t mx = it_fill;
					for (int sh = 32; sh > 0; sh >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, sh, 64));
					pf_walk[0] += it_fill; pf_walk[1] += (lane == 0) ? mx : 0u;
				}
				t0 = r.t;
			}
			if (TEAM != 1) alive = alive && first_of_team; // the lanes of a team found the same ray: one ring entry
			const unsigned long long am = __ballot(alive);
			if (alive) {
				const uint32_t slot = ring_head + ring_count + __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
				ring[slot & (kRing - 1)] = make_uint2(BATCH ? x | (y << kBatchXYBits) | (bs << (2u * kBatchXYBits)) : x | (y << 16), __float_as_uint(t0));
				++st_alive;
			}
			ring_count += (uint32_t)__popcll(am);
		}
		__builtin_amdgcn_wave_barrier();
		NRS_PHASE(1); // refill

		// ---- hand pending rays to idle lanes ----
		if (nfree >= kRefillWhenIdle && ring_count) {
			if (TEAM == 0) { // hybrid: full generations until the tail packets, then as many lanes per ray as the pending rays allow
				// (a launch of tail packets only runs one lane per ray only where it is large -- 64-pixel packets -- and the wave can fill its lanes:
				// otherwise more than 32 pending rays = 32 now as teams of two, the rest in the next generation or handed to a waiting sibling)
				gen_t = tail_seen ? (ring_count > 32u && (!a1.all_tail || (a1.fill_lanes == 1u && ring_count >= kFullGen)) ? 1u : (ring_count > 16u ? 2u : 4u)) : 1u;
				tk = lane & (int)(gen_t - 1u);
				team_base = lane & ~(int)(gen_t - 1u);
			}
			const uint32_t take = min(TEAM != 1 ? 64u / gen_t : nfree, ring_count);
			const uint32_t rank = TEAM != 1 ? (uint32_t)lane / gen_t // (all 64 lanes are idle: kRefillWhenIdle)
			                                : __builtin_amdgcn_mbcnt_hi((uint32_t)(free_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)free_mask, 0u));
			if (!have && rank < take) {
				const uint2 e = ring[(ring_head + rank) & (kRing - 1)];
				const uint32_t x = BATCH ? e.x & kBatchXYMask : e.x & 0xffffu, y = BATCH ? (e.x >> kBatchXYBits) & kBatchXYMask : e.x >> 16;
				if (BATCH) { // the pending rays of a wave may belong to different samples: the offsets per lane here
					const uint32_t es = e.x >> (2u * kBatchXYBits), espp = p1.spp_index + es;
					float eo_x, eo_y;
					ld_random_pixel_offset(p1.snap_to_pixel_centers ? 0u : espp, eo_x, eo_y);
					ray_origin_dir<EXTRA, true>(p1, x, y, eo_x, eo_y, o, d, espp);
					out_idx = pixel_out_idx(a1, x, y) + es * a1.slab_stride;
				} else {
				ray_origin_dir<EXTRA>(p1, x, y, off_x, off_y, o, d); // same arithmetic as at enqueue time -> same bits
				out_idx = pixel_out_idx(a1, x, y);
				}
				t = __uint_as_float(e.y);
				cr = cg = cb = ca = 0.f;
				ray_depth = 0.f; max_weight = 0.f; n_steps = 0;
				have = true;
				if (TEAM != 1) { // lane k of the team walks k samples ahead
					valid = true;
					for (int j = 0; j < tk && valid; ++j) {
						t += calc_dt(t, p1.cone_angle_constant);
						f3 npos; float ndt;
						valid = march_to_occupied(p1, m1, sm.coarse, o, d, t, npos, ndt, nullptr);
					}
				}
			}
			ring_head += take;
			ring_count -= take;
		}
		__builtin_amdgcn_wave_barrier();

		if (!__any(have)) {
			if (!more && ring_count == 0) {
				if (!(TEAM == 0 && a1.steal)) break;
				// nothing left for this wave: wait for rays from a sibling that still holds many (see "ray hand-over" above), until no wave holds any
				uint32_t got = 0u;
				int ln = lane; // (opaque copy, as in the hand-over block above)
				asm volatile("" : "+v"(ln));
				if (ln == 0) {
					const uint32_t bit = 1u << wave;
					atomicOr(&sm.idle_mask, bit);
					atomicSub(&sm.n_busy, 1u);
					bool promised = false; // a sibling has cleared this wave's bit: its rays are on their way
					for (;;) {
						got = lds_peek(&sm.mail[wave]);
						if (got) break;
						if (!promised && lds_peek(&sm.n_busy) == 0u) {
							if (atomicAnd(&sm.idle_mask, ~bit) & bit) break; // nobody holds rays any more and nobody has picked this wave: done
							promised = true;
						}
						__builtin_amdgcn_s_sleep(8);
					}
				}
				got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
				if (!got) break;
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
				if (got & 0x80000000u) { // rays that had not started: they stand in this wave's ring now
					ring_head = 0u;
					ring_count = got & 0x7fffffffu;
					tail_seen = true; // (lane teams by the number of rays, as for the queue's tail packets)
					__builtin_amdgcn_wave_barrier();
					if (ln == 0) lds_poke(&sm.mail[wave], 0u);
					continue;
				}
				const uint32_t* mb = &sm.fl[wave].feat[0][0][0];
				gen_t = got <= 16u ? 4u : 2u; // (a sibling hands over at most 32 rays)
				tk = ln & (int)(gen_t - 1u);
				team_base = ln & ~(int)(gen_t - 1u);
				const uint32_t r = (uint32_t)ln / gen_t;
				have = r < got;
				valid = true;
				if (have) {
					o = mk3(__uint_as_float(mb[0 * 32 + r]), __uint_as_float(mb[1 * 32 + r]), __uint_as_float(mb[2 * 32 + r]));
					d = mk3(__uint_as_float(mb[3 * 32 + r]), __uint_as_float(mb[4 * 32 + r]), __uint_as_float(mb[5 * 32 + r]));
					t = __uint_as_float(mb[6 * 32 + r]);
					cr = __uint_as_float(mb[7 * 32 + r]); cg = __uint_as_float(mb[8 * 32 + r]); cb = __uint_as_float(mb[9 * 32 + r]); ca = __uint_as_float(mb[10 * 32 + r]);
					ray_depth = __uint_as_float(mb[11 * 32 + r]); max_weight = __uint_as_float(mb[12 * 32 + r]);
					out_idx = mb[13 * 32 + r]; n_steps = mb[14 * 32 + r];
					for (int j = 0; j < tk && valid; ++j) { // lane k of a team stands k samples ahead
						t += calc_dt(t, p1.cone_angle_constant);
						f3 npos; float ndt;
						valid = march_to_occupied(p1, m1, sm.coarse, o, d, t, npos, ndt, nullptr);
					}
				}
				__builtin_amdgcn_wave_barrier();
				if (ln == 0) lds_poke(&sm.mail[wave], 0u);
			}
			continue;
		}

		NRS_FRESH_ARGS(m2, a2);
		const nrs_render_params& p2 = a2.p;
		const GridView gv = make_grid_view(m2); // (formed per round from fresh scalar loads: ten scalar registers that need not live through the other phases)
		NRS_PHASE(2); // sample set-up + cage warp
		if (PROF) ++pf_rounds;
		// ---- one sample per live ray: generate_next_nerf_network_inputs body (tn:668-692) ----
		const f3 pos = o + d * t;
		const float dt = calc_dt(t, p2.cone_angle_constant);
		f3 wpos = m2.diag_pow2 ? mk3((pos.x - m2.aabb.mn[0]) * m2.inv_diag[0], (pos.y - m2.aabb.mn[1]) * m2.inv_diag[1], (pos.z - m2.aabb.mn[2]) * m2.inv_diag[2])
		                      : warp_position(pos, m2.aabb);
		f3 wdir = warp_direction(d);
		// (constant stepping: dt == MIN_STEP, so warp_dt is exactly 0 and the IEEE division it contains -- by a constant, but the compiler may not turn
		// it into a multiplication -- is skipped with a scalar branch)
		float wdt = p2.cone_angle_constant == 0.f ? 0.f : warp_dt(dt);
		bool empty = false;
		// POISSON: the tet the first operator's search found for this sample (its membrane terms are interpolated in the same tet: poisson_residual_find)
		uint32_t warp_scan = kTetNotSearched;
		const bool act = TEAM != 1 ? (have && valid) : have; // this lane evaluates a sample in this round
		uint32_t pf_scan = 0; // (PROF: bit 16 in a deformed box, bit 17 tet found, low half candidates tested)
		if (ops && act) { // map_rays, last-to-first (tn:2899-2902)
#if NRS_MEASURE == 2
			{ f3 wp2 = wpos, wd2 = wdir; asm volatile("" : "+v"(wp2.x), "+v"(wp2.y), "+v"(wp2.z)); bool e2 = false;
			  for (int ei = a2.n_edits - 1; ei >= 0; --ei) e2 |= AFFINE ? edit_warp(a2.edits[ei], true, wp2, wd2) : tet_warp(a2.edits[ei], true, wp2, wd2);
			  asm volatile("" :: "v"(wp2.x), "v"(wp2.y), "v"(wp2.z), "v"(wd2.x), "v"(wd2.y), "v"(wd2.z), "s"((int)__ballot(e2))); }
#endif
			for (int ei = a2.n_edits - 1; ei >= 0; --ei) {
				if (AFFINE) {
					empty |= edit_warp(a2.edits[ei], true, wpos, wdir);
				} else if (POISSON) {
					uint32_t scan; // (a local of the iteration, selected below: a pointer that is sometimes null made warp_scan a stack object)
					empty |= tet_warp(a2.edits[ei], true, wpos, wdir, sm.coarse, &scan);
					if (ei == a2.n_edits - 1) warp_scan = scan;
				} else {
					empty |= tet_warp(a2.edits[ei], true, wpos, wdir, sm.coarse, nullptr, PROF ? &pf_scan : nullptr);
				}
			}
		}
		if (PROF && !POISSON && !AFFINE) {
			uint32_t mx = pf_scan & 0xffffu;
			for (int sh = 32; sh > 0; sh >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, sh, 64));
			pf_walk[8] += (pf_scan >> 16) & 1u; pf_walk[9] += (lane == 0 && __any((pf_scan >> 16) & 1u)) ? 1u : 0u;
			pf_walk[10] += pf_scan & 0xffffu; pf_walk[11] += (lane == 0) ? mx : 0u; pf_walk[12] += (pf_scan >> 17) & 1u;
		}
		if (POISSON && !AFFINE) poisson_stash[wave * 64 + lane] = warp_scan; // (through LDS, not a register across the gather -- this instantiation's peak)
		NRS_PHASE(3); // gather
		// ---- gather: own sample (block g) and the partner lane's sample (block 1-g), levels 2*it+g ----
#if NRS_MEASURE == 3
		{ f3 wp2 = wpos; asm volatile("" : "+v"(wp2.x), "+v"(wp2.y), "+v"(wp2.z));
		  encode_num<NUM, kQuads>(nm, gv, m2.levels, sm.ml, fl, lane, g, wp2, act); }
#endif
		encode_num<NUM, kQuads, false, GATE>(nm, gv, m2.levels, sm.ml, fl, lane, g, wpos, act); // (four record levels in flight: the hybrid instantiation has the registers; features of idle lanes are never looked at: not zeroed)
		NRS_PHASE(4); // SH + MLP
		const f3 pdir = mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z));
		half8 sh_own, sh_par;
		encode_sh4_2(g, wdir, pdir, sh_own, sh_par);

		// ---- fused MLPs on MFMA, one 32-sample block at a time ----
#if NRS_MEASURE == 4
		{ uint32_t sink = 0;
		  #pragma unroll 1
		  for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			asm volatile("" : "+v"(x0), "+v"(x1));
			const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, x0, x1);
			const half8 rout = rgb_mlp_num<NUM>(nm, sm.ml.w, lane, dout, sel ? sh_par : sh_own);
			sink ^= __builtin_bit_cast(u32x4, dout)[0] ^ __builtin_bit_cast(u32x4, rout)[1];
		  }
		  asm volatile("" :: "v"(sink)); }
#endif
		uint32_t res_d = 0, res_rg = 0, res_b = 0;
		const half8* deep_w = (DEEP && (XTRA != kXtraLightAll || m2.rgb_deep)) ? reinterpret_cast<const half8*>(m2.wfrag) : nullptr; // (the third rgb hidden layer's fragments are read from HBM)
		// LIGHT: the frame's light direction (nrs_model_set_light_dir), the same for every sample: the B operand of layer 0's third k step, its A fragments in HBM
		const half8* light_w = (LIGHT && (XTRA != kXtraLightAll || m2.n_extra_dims)) ? reinterpret_cast<const half8*>(m2.wfrag) : nullptr;
		const half8 lb = LIGHT ? light_operand(g, m2.light01[0], m2.light01[1], m2.light01[2]) : half8{};
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			half8 dout = x0, rout = x1;
			if (!(a2.dbg & 2u)) {
				dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, x0, x1);
				rout = rgb_mlp_num<NUM, DEEP, LIGHT>(nm, sm.ml.w, lane, dout, sel ? sh_par : sh_own, deep_w, light_w, lb);
			}
			const u32x4 dd = __builtin_bit_cast(u32x4, dout), rr = __builtin_bit_cast(u32x4, rout);
			// rows 0..2 of a block sit in its lanes 0..31; block 1's samples belong to the rays of lanes 32..63
			uint32_t vd = dd[0], vrg = rr[0], vb = rr[1];
			if (b == 1) { vd = xchg32u(vd); vrg = xchg32u(vrg); vb = xchg32u(vb); }
			if (g == b) { res_d = vd; res_rg = vrg; res_b = vb; }
		}
		const half2v hd = __builtin_bit_cast(half2v, res_d), hrg = __builtin_bit_cast(half2v, res_rg), hb = __builtin_bit_cast(half2v, res_b);
		const float sigma_raw = (float)hd[0];
		const float raw_r = (float)hrg[0], raw_g = (float)hrg[1], raw_b = (float)hb[0];

		// ---- INTRO: the network's input gradient (Normals) or a visualised activation (EncodingVis) of this round's samples, tn:2923-2927 ----
		f3 intro_v = mk3(0.f, 0.f, 0.f); // Normals: d density_raw / d warped position; EncodingVis: (max(-v, 0), max(v, 0), 0)
		if (INTRO) {
			NRS_FRESH_ARGS(m2i, a2i);
			const nrs_render_params& p2i = a2i.p;
			const bool acc16 = (nm & 2u) != 0u;
			if (p2i.render_mode == NRS_RENDER_ENCODING_VIS) {
				// network.visualize_activation(stream, layer, dim, positions_matrix, positions_matrix): unit `dim` of forward_activations(layer)
				const uint32_t layer = p2i.visualized_layer, dim = p2i.visualized_dimension;
				float v = 0.f;
				if (layer == 0u) { // the hash-grid output: the slab still holds this round's features (level L of the own sample: see encode_to_lds)
					const uint32_t L = dim >> 1;
					const uint32_t w = ((L & 1u) == (uint32_t)g) ? fl.feat[L >> 1][0][lane] : fl.feat[L >> 1][1][lane ^ 32];
					v = (float)__builtin_bit_cast(half2v, w)[dim & 1u];
				} else if (LIGHT && layer == 2u && dim >= 32u) { // the Identity encoding of the light direction: units 32..34, then its padding ones
					v = dim < 35u ? (float)(_Float16)m2i.light01[dim - 32u] : 1.0f;
				} else if (layer == 2u && dim >= 16u) { // an SH coefficient of the own direction: 8 g .. 8 g + 7 are here, the others in the partner lane's sh_par
					const uint32_t cidx = dim - 16u;
					const float mine = (float)pick8(sh_own, (int)(cidx & 7u)), theirs = xchg32((float)pick8(sh_par, (int)(cidx & 7u)));
					v = ((cidx >> 3) == (uint32_t)g) ? mine : theirs;
				} else {
					#pragma unroll 1
					for (int b = 0; b < 2; ++b) {
						const int sel = (b != g) ? 1 : 0;
						const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
						float val;
						int half_of_row;
						if (layer == 2u) { // a density-MLP output (rows 0..15 of the rgb network's input)
							const half8 dout = acc16 ? density_mlp<true>(sm.ml.w, lane, x0, x1) : density_mlp<false>(sm.ml.w, lane, x0, x1);
							const int e = (int)((dim & 3u) + 4u * (dim >> 3)); // element of row dim: row = (e & 3) + 8 (e >> 2) + 4 half
							val = (float)pick8(dout, e);
							half_of_row = (int)((dim >> 2) & 1u);
						} else {
							half8 din = x0;
							if (layer >= 3u) din = acc16 ? density_mlp<true>(sm.ml.w, lane, x0, x1) : density_mlp<false>(sm.ml.w, lane, x0, x1);
							const half8 shb = sel ? sh_par : sh_own;
							val = acc16 ? mlp_hidden_activation<true, LIGHT>(sm.ml.w, lane, x0, x1, din, shb, layer, dim, deep_w, light_w, lb) : mlp_hidden_activation<false, LIGHT>(sm.ml.w, lane, x0, x1, din, shb, layer, dim, deep_w, light_w, lb);
							half_of_row = tile_half(dim);
						}
						// the value of sample (b, j) sits in lane j + 32 * half_of_row; its ray is lane j + 32 * b
						if (half_of_row != b) val = xchg32(val);
						if (g == b) v = val;
					}
				}
				intro_v = mk3(fmaxf(-v, 0.0f), fmaxf(v, 0.0f), 0.0f); // extract_dimension_pos_neg_kernel (tiny-cuda-nn), rows 0..2
				// The reference hands the network INPUT to visualize_activation as its output matrix (tn:2926): the sample's NerfCoordinate is overwritten --
				// position = the three values above, dt = 1, direction = (1, 1, 1) -- and composite_kernel_nerf reads them back as warped_pos (the colour,
				// tn:925; also the position of the depth test), dt (tn:762: every sample composites with the largest step) and the membrane colour's direction.
				wpos = intro_v;
				wdt = 1.0f;
				wdir = mk3(1.0f, 1.0f, 1.0f);
			} else if (p2i.render_mode == NRS_RENDER_NORMALS) {
				// network.input_gradient(stream, 3, positions, gradients): backward of 128 e_3 (see density_backward_features), then the grid's input gradient
				uint32_t dfe[2][8];
				#pragma unroll
				for (int b = 0; b < 2; ++b) { // (unrolled: dfe must stay in registers)
					const int sel = (b != g) ? 1 : 0;
					const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
					if (acc16) density_backward_features<true>(sm.ml.w, reinterpret_cast<const half8*>(m2i.wfrag), lane, x0, x1, dfe[b]);
					else density_backward_features<false>(sm.ml.w, reinterpret_cast<const half8*>(m2i.wfrag), lane, x0, x1, dfe[b]);
				}
				// dL/dfeatures of sample (b, j) -> the slab, G[L][ray lane j + 32 b] (both lane halves of a column hold 8 of its 16 level pairs)
				__builtin_amdgcn_wave_barrier();
				uint32_t* G = &fl.feat[0][0][0];
				#pragma unroll
				for (int b = 0; b < 2; ++b)
					#pragma unroll
					for (int q = 0; q < 8; ++q) G[level_of_pair(q, g) * 64 + (lane & 31) + 32 * b] = dfe[b][q];
				__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
				__builtin_amdgcn_wave_barrier();
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
				float res[3] = {0.f, 0.f, 0.f};
				const GridView gvi = make_grid_view(m2i);
				const f3 q = act ? wpos : mk3(0.f, 0.f, 0.f);
				#pragma unroll 1
				for (int L = 0; L < (int)kLevels; ++L) level_input_gradient(gvi, m2i.levels[L], q, G[L * 64 + lane], res);
				intro_v = mk3(res[0] * (1.0f / 128.0f), res[1] * (1.0f / 128.0f), res[2] * (1.0f / 128.0f));
				__builtin_amdgcn_wave_barrier();
			}
		}
		// ---- membrane correction inputs (compute_poisson_full_residuals, tn:2867-2883) + the un-deformed network pass (tn:2890-2892) ----
		// Behind the main pass, not in front of it as the reference runs them (round 4): the boundary terms (5 values) and the old density then are not
		// live across the gather -- the kernel's register peak -- and the instantiation fits the 8-wave / 128-VGPR launch shape of the default kernel.
		// The un-deformed position is recomputed from the ray (the same arithmetic as at the top of the round: the same bits), the feature slab is free again.
		float p_rgb[3] = {0.f, 0.f, 0.f}, p_out = 0.f, p_res = 0.f, sigma_old_raw = 0.f;
		bool has_res = false;
		if (POISSON) {
			NRS_FRESH_ARGS(m2b, a2b);
			const nrs_render_params& p2b = a2b.p;
			if (p2b.apply_operators && a2b.n_edits > 0) {
				const f3 pos0 = o + d * t;
				const f3 wpos0 = m2b.diag_pow2 ? mk3((pos0.x - m2b.aabb.mn[0]) * m2b.inv_diag[0], (pos0.y - m2b.aabb.mn[1]) * m2b.inv_diag[1], (pos0.z - m2b.aabb.mn[2]) * m2b.inv_diag[2])
				                              : warp_position(pos0, m2b.aabb);
				// step 1: which tet of which membrane edit holds the sample (the last one in the reference's operator order that does), and its two densities
				uint32_t found_tet = 0u;
				int found_edit = -1;
				if (act) {
					const uint32_t searched = !AFFINE ? poisson_stash[wave * 64 + lane] : kTetNotSearched;
					for (int ei = a2b.n_edits - 1; ei >= 0; --ei)
						if (a2b.edits[ei].apply_poisson && poisson_residual_find(a2b.edits[ei], wpos0, found_tet, p_out, p_res, sm.coarse, ei == a2b.n_edits - 1 ? searched : kTetNotSearched)) found_edit = ei;
				}
				has_res = act && p_out > 1e-9f;
				// step 2: the un-deformed network's density.  The reference evaluates it for every sample; its only consumer is the clamp of tn:776-777, i.e.
				// samples with a residual when m_poisson_target is set (the reference's default) -- otherwise the pass is skipped, results unchanged.
				// (round 4, late: and of those only the samples whose residual is POSITIVE -- min(max(target, s), s + res) = s + res whatever the target is when
				// res <= 0, because max(., s) >= s >= s + res: a round whose residuals are all negative or zero skips the pass, the others gather for fewer lanes)
				const bool need_old = has_res && p_res > 0.f;
				if (p2b.poisson_target && __any(need_old)) {
					const GridView gvb = make_grid_view(m2b);
					encode_num<NUM, kQuads>(nm, gvb, m2b.levels, sm.ml, fl, lane, g, wpos0, need_old);
					uint32_t old_d = 0;
					#pragma unroll 1
					for (int b = 0; b < 2; ++b) {
						const int sel = (b != g) ? 1 : 0;
						const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, load_features(fl, lane, sel, 0), load_features(fl, lane, sel, 1));
						uint32_t vd = __builtin_bit_cast(u32x4, dout)[0];
						if (b == 1) vd = xchg32u(vd);
						if (g == b) old_d = vd;
					}
					sigma_old_raw = (float)__builtin_bit_cast(half2v, old_d)[0];
				}
				// step 3: the boundary colour of the samples with a residual (the only ones whose colour is mixed, tn:796-805)
				if (EXTRA ? (found_edit >= 0) : has_res) {
					NRS_FRESH_ARGS(m2d, a2d);
					const f3 pos1 = o + d * t;
					const f3 wpos1 = m2d.diag_pow2 ? mk3((pos1.x - m2d.aabb.mn[0]) * m2d.inv_diag[0], (pos1.y - m2d.aabb.mn[1]) * m2d.inv_diag[1], (pos1.z - m2d.aabb.mn[2]) * m2d.inv_diag[2])
					                              : warp_position(pos1, m2d.aabb);
					const f3 udir = unwarp_direction(wdir);
					for (int ei = a2d.n_edits - 1; ei >= 0; --ei)
						if (a2d.edits[ei].apply_poisson && found_edit == ei) poisson_residual_colour(a2d.edits[ei], found_tet, wpos1, udir, p_rgb);
				}
			}
		}
		// POISSON without EXTRA: the sample reduced HERE to what compositing consumes -- its final alpha and its (mixed) colour -- so that the boundary
		// terms, the old density and the raw outputs end with this phase instead of living through the compositing / marching code (the other register peak).
		// The values are the ones the reference's order of operations gives: weight * (w_N rgb + w_R rgb_residual) is a commutative product of the same two floats.
		float px_alpha = 0.f, px_r = 0.f, px_g = 0.f, px_b = 0.f;
		if (POISSON && !EXTRA) {
			NRS_FRESH_ARGS(m2c, a2c);
			if (act) {
				const float cdt = unwarp_dt(wdt);
				const float sigma = network_to_density(sigma_raw, m2c.density_activation);
				px_alpha = 1.f - __expf(-sigma * cdt);
				px_r = network_to_rgb(raw_r, m2c.rgb_activation); px_g = network_to_rgb(raw_g, m2c.rgb_activation); px_b = network_to_rgb(raw_b, m2c.rgb_activation);
				if (has_res) { // tn:770-780, 796-805, 939-943
					const float targetval = network_to_density(sigma_old_raw, m2c.density_activation);
					const float val = a2c.p.poisson_target ? fminf(fmaxf(targetval, sigma), sigma + p_res) : sigma + p_res;
					const float alpha_N = px_alpha; // 1 - exp(-sigma cdt)
					px_alpha = 1.f - __expf(-(val) * cdt);
					const float alpha_R = 1.f - __expf(-p_out * cdt);
					const float w_N = alpha_N / (alpha_N + alpha_R), w_R = alpha_R / (alpha_N + alpha_R);
					px_r = w_N * px_r + w_R * p_rgb[0]; px_g = w_N * px_g + w_R * p_rgb[1]; px_b = w_N * px_b + w_R * p_rgb[2];
				}
				if (empty) px_alpha = 0.0f;
			}
		}

		NRS_FRESH_ARGS(m3, a3);
		const nrs_render_params& p3 = a3.p;
		NRS_PHASE(5); // composite + march + shade
		// (read here, not in front of the frame loop: six scalar registers that would otherwise live through every phase)
		const f3 cam_fwd = mk3(p3.camera_matrix1[6], p3.camera_matrix1[7], p3.camera_matrix1[8]);
		const f3 cam_o = mk3(p3.camera_matrix1[9], p3.camera_matrix1[10], p3.camera_matrix1[11]);
		// ---- composite_kernel_nerf body (tn:750-955, Shade mode) + next-sample march ----
		uint32_t it_march = 0;
		if (PROF) { pf_walk[4] += (lane == 0) ? 1u : 0u; pf_walk[5] += have ? 1u : 0u; }
		bool team_round = false;
		if constexpr (TEAM != 1) team_round = gen_t > 1u;
		if (TEAM != 1 && team_round) {
			// this lane's sample, reduced to what compositing needs
			float s_alpha = 0.f, s_r = 0.f, s_g = 0.f, s_b = 0.f, s_depth = 0.f;
			if (act) {
				const f3 cpos = unwarp_position(wpos, m3.aabb);
				if (POISSON && !EXTRA) { // (the sample was reduced behind the network pass)
					s_alpha = px_alpha; s_r = px_r; s_g = px_g; s_b = px_b;
				} else {
					const float sigma = network_to_density(sigma_raw, m3.density_activation);
					s_alpha = 1.f - __expf(-sigma * unwarp_dt(wdt));
					if (empty) s_alpha = 0.0f;
					s_r = network_to_rgb(raw_r, m3.rgb_activation); s_g = network_to_rgb(raw_g, m3.rgb_activation); s_b = network_to_rgb(raw_b, m3.rgb_activation);
				}
				s_depth = dot3(cam_fwd, cpos - cam_o);
			}
			// every lane of the team composites the team's samples in marching order (composite_kernel_nerf, tn:750-955)
			bool done = false, shade = true, exited = false; // exited: the ray left the render box un-saturated (Cost mode counts one more step for it, below)
			#pragma unroll
			for (int k = 0; k < (TEAM ? TEAM : kTeamMax); ++k) {
				if (TEAM == 0 && k >= (int)gen_t) break;
				const int src = team_base + k;
				const bool v_k = __shfl((int)act, src, 64) != 0;
				const float al = __shfl(s_alpha, src, 64), kr = __shfl(s_r, src, 64), kg = __shfl(s_g, src, 64), kb = __shfl(s_b, src, 64);
				const float kdepth = __shfl(s_depth, src, 64);
				if (have && !done) {
					if (!v_k) {
						done = true; exited = true; // the walk after the previous sample left the render box
					} else {
						const float weight = al * (1.f - ca);
						cr += kr * weight;
						cg += kg * weight;
						cb += kb * weight;
						ca += weight;
						if (weight > max_weight) {
							max_weight = weight;
							ray_depth = kdepth;
						}
						++n_steps;
						if (tk == 0) ++st_samples;
						if (ca > (1.0f - p3.min_transmittance)) {
							const float inv_a = __builtin_amdgcn_rcpf(ca);
							cr *= inv_a; cg *= inv_a; cb *= inv_a; ca = 1.0f;
							done = true;
						} else if (n_steps >= a3.max_steps) {
							done = true; shade = false;
						}
					}
				}
			}
			// ---- on to this lane's next sample, gen_t samples ahead.  Walked lane by lane that is gen_t dependent marches per round (measured on a 1/8 share
			// of the bench frame: 0.32 of its 0.65 ms).  The team's next positions continue from its LAST lane's position u0, and as long as every
			// position stands in an occupied cell the walk is nothing but `t += dt`: lane k forms its candidate (k + 1 steps from u0, the same additions
			// in the same order) and ALL lanes test theirs at once; the candidates in front of the first one that fails ARE the walk's positions, the
			// lanes from there on walk as before, starting at the last position that held (same arithmetic as lane by lane: same bits).
			const bool need = have && !done;
			if (__any(need)) {
				const int last = team_base + (int)gen_t - 1;
				const float u0 = __shfl(t, last, 64);
				const bool chain = __shfl((int)valid, last, 64) != 0; // the last lane stands on a sample, hence every lane of the team does
				float cand = u0;
				#pragma unroll
				for (int j = 0; j < (TEAM ? TEAM : kTeamMax); ++j)
					if (j <= tk) cand += calc_dt(cand, p3.cone_angle_constant);
				const bool holds = need && chain && stands_in_occupied_cell(p3, m3, sm.coarse, o, d, cand);
				const uint32_t team_bits = (uint32_t)(__ballot(holds) >> team_base) & ((1u << gen_t) - 1u);
				const int first_off = __builtin_ctz(~team_bits); // first lane of the team whose candidate does not hold (gen_t: all hold)
				if (need) {
					if (!chain) {
						valid = false; // (walking on from a sample that does not exist: the ray has left the render box)
					} else if (tk < first_off) {
						t = cand;
						valid = true;
					} else {
						t = u0;
						for (int j = 0; j < first_off; ++j) t += calc_dt(t, p3.cone_angle_constant);
						valid = true;
						for (int j = first_off; j <= tk && valid; ++j) {
							t += calc_dt(t, p3.cone_angle_constant);
							f3 npos; float ndt;
							valid = march_to_occupied(p3, m3, sm.coarse, o, d, t, npos, ndt, nullptr);
						}
					}
				}
			}
			const bool lead_valid = __shfl((int)valid, team_base, 64) != 0;
			if (have && !done && !lead_valid) { done = true; exited = true; } // no further sample: the ray is finished now rather than a round later
			if (have && done) {
				if (tk == 0) {
					if (shade && ca > 0.001f) { // compact_kernel_nerf's hit test (tn:2503) + shade_kernel_nerf (tn:2448-2483)
						float tr = cr, tg = cg, tb = cb, ta = ca;
						if (p3.render_mode == NRS_RENDER_COST) {
							// payload.n_steps = j + current_step (tn:957-960): the samples composited for a ray that saturated (the loop broke AT sample j),
							// one more for a ray that ran out of samples (j is then the count, and current_step starts at 1)
							const float col = (float)(n_steps + (exited ? 1u : 0u)) / 128;
							tr = tg = tb = col; ta = 1.0f;
						} else if (!p3.linear_colors) {
							tr = srgb_to_linear(tr); tg = srgb_to_linear(tg); tb = srgb_to_linear(tb);
						}
						float4* fb = reinterpret_cast<float4*>(a3.frame) + out_idx;
						if (ta == 1.0f) {
							*fb = make_float4(tr, tg, tb, 1.0f); // (see the one-lane path)
						} else {
							const float4 prev = *fb;
							const float om = 1.0f - ta;
							*fb = make_float4(tr + prev.x * om, tg + prev.y * om, tb + prev.z * om, ta + prev.w * om);
						}
						if (ta > 0.2f) a3.depth[out_idx] = ray_depth;
						++st_hit;
					}
					if (a3.steps) a3.steps[out_idx] = n_steps;
				}
				have = false;
			}
		} else
		if (have) { // one lane per ray
			const f3 cpos = unwarp_position(wpos, m3.aabb);
			const float T = 1.f - ca;
			float alpha, weight, sr, sg, sb;
			if (POISSON && !EXTRA) { // the sample was reduced behind the network pass (px_*: final alpha, mixed colour)
				alpha = px_alpha;
				weight = alpha * T;
				sr = px_r; sg = px_g; sb = px_b;
			} else {
			const float cdt = unwarp_dt(wdt);
			const float sigma = network_to_density(sigma_raw, m3.density_activation);
			alpha = 1.f - __expf(-sigma * cdt);
			if (POISSON && has_res) { // tn:770-780
				const float targetval = network_to_density(sigma_old_raw, m3.density_activation);
				const float val = p3.poisson_target ? fminf(fmaxf(targetval, sigma), sigma + p_res) : sigma + p_res;
				alpha = 1.f - __expf(-(val) * cdt);
			}
			if (empty) alpha = 0.0f;
			if (EXTRA && p3.show_accel) alpha = 1.f; // tn:788-790
			weight = alpha * T;
			sr = network_to_rgb(raw_r, m3.rgb_activation); sg = network_to_rgb(raw_g, m3.rgb_activation); sb = network_to_rgb(raw_b, m3.rgb_activation);
			if (EXTRA && p3.glow_mode) glow_overlay(p3, cpos, cam_o, weight, sr, sg, sb); // tn:806-903
			if (EXTRA) render_mode_rgb(p3, cpos, o, cam_fwd, cdt, alpha, sr, sg, sb); // tn:905-937
			if (INTRO) {
				if (p3.render_mode == NRS_RENDER_NORMALS) { // tn:905-910: the direction of decreasing density
					const float k = -network_to_density_derivative(sigma_raw, m3.density_activation);
					const f3 n = mk3(k * intro_v.x, k * intro_v.y, k * intro_v.z);
					const float z = dot3(n, n); // Eigen: squaredNorm, then normalized() (z > 0 ? v / sqrt(z) : v)
					if (z > 0.f) { const float len = sqrtf(z); sr = n.x / len; sg = n.y / len; sb = n.z / len; }
					else { sr = n.x; sg = n.y; sb = n.z; }
				} else if (p3.render_mode == NRS_RENDER_ENCODING_VIS) { // tn:925: rgb = warped_pos (the overwritten input)
					sr = wpos.x; sg = wpos.y; sb = wpos.z;
				} // (every other mode of a network with a third rgb hidden layer runs here too: nothing to add)
			}
			}
			if (POISSON && EXTRA && has_res) { // tn:796-805, 939-943
				const float cdt = unwarp_dt(wdt);
				const float alpha_N = 1.f - __expf(-network_to_density(sigma_raw, m3.density_activation) * cdt);
				const float alpha_R = 1.f - __expf(-p_out * cdt);
				const float w_N = alpha_N / (alpha_N + alpha_R), w_R = alpha_R / (alpha_N + alpha_R);
				cr += weight * (w_N * sr + w_R * p_rgb[0]);
				cg += weight * (w_N * sg + w_R * p_rgb[1]);
				cb += weight * (w_N * sb + w_R * p_rgb[2]);
			} else {
				cr += sr * weight;
				cg += sg * weight;
				cb += sb * weight;
			}
			ca += weight;
			if (weight > max_weight) {
				max_weight = weight;
				ray_depth = dot3(cam_fwd, cpos - cam_o);
			}
			++n_steps;
			++st_samples;
			bool done = false, shade = true, exited = false;
			if (ca > (1.0f - p3.min_transmittance)) {
				// rgba /= alpha (tn:951-953): one v_rcp (1 ulp) + three multiplies instead of four IEEE divisions -- this block runs
				// nearly every round (some lane of the wave saturates), and the colour tolerance (tests) is 5 orders of magnitude wider
				const float inv_a = __builtin_amdgcn_rcpf(ca);
				cr *= inv_a; cg *= inv_a; cb *= inv_a; ca = 1.0f;
				done = true;
			} else if (n_steps >= a3.max_steps) {
				done = true; shade = false; // MARCH_ITER exhausted: the reference never compacts such a ray into the hit list
			} else {
				t += dt;
				f3 npos; float ndt;
#if NRS_MEASURE == 5
				{ float t2 = t; asm volatile("" : "+v"(t2)); f3 np2; float nd2; const bool v2 = march_to_occupied(p3, m3, sm.coarse, o, d, t2, np2, nd2, nullptr); asm volatile("" :: "v"(t2), "s"((int)__ballot(v2))); }
#endif
				done = !march_to_occupied<true>(p3, m3, sm.coarse, o, d, t, npos, ndt, PROF ? &it_march : nullptr);
				exited = done;
			}
			if (done) {
				if (shade && ca > 0.001f) { // compact_kernel_nerf's hit test (tn:2503) + shade_kernel_nerf (tn:2448-2483)
					float tr = cr, tg = cg, tb = cb, ta = ca;
					if (INTRO && p3.render_mode == NRS_RENDER_NORMALS) { // tn:2466-2468
						const f3 v = mk3(tr, tg, tb);
						const float z = dot3(v, v);
						f3 n = v;
						if (z > 0.f) { const float len = sqrtf(z); n = mk3(v.x / len, v.y / len, v.z / len); }
						tr = (0.5f * n.x + 0.5f) * ta; tg = (0.5f * n.y + 0.5f) * ta; tb = (0.5f * n.z + 0.5f) * ta;
					} else if (p3.render_mode == NRS_RENDER_COST) {
						const float col = (float)(n_steps + (exited ? 1u : 0u)) / 128; // payload.n_steps = j + current_step, tn:957-960 (see the team path)
						tr = tg = tb = col; ta = 1.0f;
					} else if (!p3.linear_colors && (!EXTRA || p3.render_mode == NRS_RENDER_SHADE)) { // tn:2474: only Shade (and Slice) accumulate in linear colours
						tr = srgb_to_linear(tr); tg = srgb_to_linear(tg); tb = srgb_to_linear(tb);
					}
					float4* fb = reinterpret_cast<float4*>(a3.frame) + out_idx;
					// A ray that saturated was normalised to alpha = 1 exactly (tn:951-953), so shade_kernel_nerf's `tmp + frame * (1 - tmp.w)` is
					// `tmp + frame * 0` = tmp for every finite frame value: such a ray WRITES its pixel without reading it -- the frame read is an HBM miss on the
					// round's dependency chain, and nearly every round of a wave retires some ray.  (A non-finite value in the caller's frame would have turned into NaN
					// through the multiplication by 0; it is overwritten instead.)
					if (ta == 1.0f) {
						*fb = make_float4(tr, tg, tb, 1.0f);
					} else {
						const float4 prev = *fb;
						const float om = 1.0f - ta;
						*fb = make_float4(tr + prev.x * om, tg + prev.y * om, tb + prev.z * om, ta + prev.w * om);
					}
					if (ta > 0.2f) a3.depth[out_idx] = ray_depth;
					++st_hit;
				}
				if (a3.steps) a3.steps[out_idx] = n_steps;
				have = false;
			}
		}
		if (PROF) {
			uint32_t mx = it_march;
			for (int sh = 32; sh > 0; sh >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, sh, 64));
			pf_walk[2] += it_march; pf_walk[3] += (lane == 0) ? mx : 0u; pf_walk[6] += (lane == 0 && mx > 1) ? 1u : 0u;
		}
	}

	if (PROF) {
		for (int i = 0; i < 13; ++i) if (pf_walk[i]) atomicAdd(&a.counters->walk[i], pf_walk[i]);
		NRS_PHASE(7);
		if (lane == 0) {
			unsigned long long life = 0;
			for (int i = 0; i < 8; ++i) { life += ph_acc[i]; if (i != 6) atomicAdd(&a.counters->phase_cycles[i], ph_acc[i]); }
			atomicMax(&a.counters->phase_cycles[6], life); // longest-lived wave
			if (a.wave_log) {
				unsigned int xcc = 0;
				asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
				unsigned long long* w = a.wave_log + 4 * (size_t)(blockIdx.x * WAVES + wave);
				unsigned int hw = 0;
				asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
				w[0] = life | ((unsigned long long)st_alive << 48);
				w[1] = pf_rounds | (pf_rounds_q << 16) | (pf_tq << 32);
				w[2] = (pf_packets & 0xffffull) | ((unsigned long long)(hw & 0xffffu) << 16) | ((unsigned long long)(ph_acc[0] >> 8) << 32 & 0x00ffffff00000000ull) | ((unsigned long long)(xcc & 0xf) << 56);
				w[3] = (wall_clock64() - pf_wall0) | ((pf_wall0 & 0xffffffffull) << 32);
			}
		}
	}
	// statistics: per workgroup in LDS, one set of device atomics from the last wave to finish (see claim_packet for why)
	atomicAdd(&sm.sum_samples, (unsigned long long)st_samples);
	atomicAdd(&sm.sum_alive, st_alive);
	atomicAdd(&sm.sum_hit, st_hit);
	__builtin_amdgcn_wave_barrier();
	if (lane == 0 && atomicAdd(&sm.n_finished, 1u) == (uint32_t)WAVES - 1u) {
		atomicAdd(&a.counters->n_samples, __atomic_load_n(&sm.sum_samples, __ATOMIC_RELAXED));
		atomicAdd(&a.counters->n_rays_hit, __atomic_load_n(&sm.sum_hit, __ATOMIC_RELAXED));
		// the last workgroup of the launch tells the host which share of the pixels became rays: the next launch sizes its
		// lane teams with it (nrs_render_nerf).  A heuristic input only -- results do not depend on the team size.  The
		// returned value orders this workgroup's count before its "done" mark (no fence: a device-scope fence writes the
		// L2 back, 0.15 ms per launch when 512 workgroups do it over a freshly written frame).
		const uint32_t before = atomicAdd(&a.counters->n_rays_alive, __atomic_load_n(&sm.sum_alive, __ATOMIC_RELAXED));
		uint32_t one = 1u;
		asm volatile("" : "+v"(one) : "v"(before)); // the increment below waits for the count above to have returned
		if (atomicAdd(&a.counters->blocks_done, one) == gridDim.x - 1u) { // the launch's last workgroup
			if (a.feedback) *a.feedback = (unsigned long long)atomicAdd(&a.counters->n_rays_alive, 0u) | ((unsigned long long)a.pixels_owned << 32);
			if (a.counters_next) { // the slot's next launch finds its block zeroed (nrs_render_nerf: no memset between frames)
				unsigned long long* z = reinterpret_cast<unsigned long long*>(a.counters_next);
				#pragma unroll
				for (uint32_t i = 0; i < sizeof(RenderCounters) / 8; ++i) z[i] = 0ull;
			}
		}
	}
}

template <int WAVES, int OCC, bool PROF, bool POISSON, bool AFFINE, int TEAM, int NUM = 0, int EXTRA = 0, bool BATCH = false>
__global__ __launch_bounds__(64 * WAVES, OCC) void render_kernel(const DeviceModel m_arg, const RenderArgs a_arg) {
	render_body<WAVES, OCC, PROF, POISSON, AFFINE, TEAM, NUM, EXTRA, BATCH>(m_arg, a_arg);
}
// The same kernel scheduled for 3 waves per SIMD but held to the 128 VGPRs that still give 4 (512-thread workgroups, 2 per CU): the
// scheduler hides more latency per wave when it does not aim at occupancy 4, and the cap keeps the occupancy it did not aim at.
// (An attribute argument cannot depend on a template parameter, hence a second entry point rather than a template flag.)
// Scheduled for TWO waves per SIMD measured +-0 on the lego scenes and +1 % on the garden frame (profiles/r06/ab_c128_occ2_*.txt): the GATE instantiation takes that.
template <int WAVES, bool PROF, bool POISSON, bool AFFINE, int TEAM, int NUM = 0, int XTRA = 0, bool BATCH = false>
__global__ __launch_bounds__(64 * WAVES, XTRA == kXtraGate ? 2 : 3) __attribute__((amdgpu_num_vgpr(128))) void render_kernel_c128(const DeviceModel m_arg, const RenderArgs a_arg) {
	render_body<WAVES, 3, PROF, POISSON, AFFINE, TEAM, NUM, XTRA, BATCH>(m_arg, a_arg);
}
#ifndef NRS_BODY_ONLY // (tools/one_kernel.sh compiles ONE explicit instantiation of render_kernel for register work: everything below is left out)
// The precondition of every render launch: the packets were sized (a.team, tile_geometry) for the TEAM of the row that is launched.  Both come from one plan
// (nrs_route.h plan_route), so this should never fire -- it stays as the last guard because a mismatch makes packet_pixel lay out pixels with another packet
// shape than the launch was sized for and write past a tiled frame.  A route that fails it is refused (NRS_ERR_STATE) and nothing is launched.
static std::atomic<unsigned long long> g_render_dispatches{0}; // render-kernel dispatches of this process (launch_render_dispatches)
unsigned long long launch_render_dispatches() { return g_render_dispatches.load(); }
static int check_route(const DeviceModel& m, const RenderArgs& a, const RouteTraits& t, bool batch) {
	const bool intro = a.p.render_mode == NRS_RENDER_NORMALS || a.p.render_mode == NRS_RENDER_ENCODING_VIS;
	const XtraTraits x = xtra_traits(t.xtra);
	const char* why = nullptr;
	if ((int)a.team != t.team) why = "lanes per ray of the packet geometry (a.team) differ from TEAM";
	else if (a.any_affine && !t.affine) why = "an AffineDuplication operator needs AFFINE";
	else if (a.any_poisson && !t.poisson) why = "the membrane correction needs POISSON";
	else if (t.num != kNumRuntime && (uint32_t)t.num != m.numerics) why = "NUM does not match the model's numerics";
	else if ((m.n_extra_dims != 0u) != x.light) why = "a network with light directions needs EXTRA 7 or 8 and only they";
	else if ((a.extra != 0u) != x.extra) why = "a.extra needs EXTRA 1..4 (8 with light directions) and only it";
	else if (t.xtra != kXtraLightAll && (m.rgb_deep != 0u) != x.deep) why = "a third rgb hidden layer needs EXTRA 3..5 and only it";
	else if (x.gate && !a.gate) why = "EXTRA 6 (GATE) without a.gate";
	else if (intro && !x.intro) why = "Normals / EncodingVis need EXTRA 2, 4 or 8";
	else if (t.prof && !(a.dbg & 4u)) why = "PROF without NRS_DEBUG bit 2";
	else if (a.spp_count > 1u && !batch) why = "a batch of samples (spp_count > 1) needs BATCH";
	else if (a.spp_count == 0u || a.spp_packets == 0u || a.n_packets != a.spp_count * a.spp_packets) why = "the queue is not spp_count times the packets of one sample";
	if (!why) return NRS_OK;
	char name[160];
	route_name(name, sizeof(name), t, batch);
	snprintf(g_launch_err, sizeof(g_launch_err), "launch_render: route refused: %s for team %u, affine %u, poisson %u, numerics %u, extra %u, deep %u, gate %u, render mode %u: %s",
	         name, a.team, a.any_affine, a.any_poisson, m.numerics, a.extra, m.rgb_deep, a.gate, (uint32_t)a.p.render_mode, why);
	return NRS_ERR_STATE;
}
// The launcher of row ROW of kRoutes (nrs_route.h): the kernel is instantiated from the row's traits.  BATCH: the twin that serves a queue of several samples
// (render_body).  TWIN: the __launch_bounds__(512, 4) build of a row of the 128-register entry point, see below.
template <int ROW, bool TWIN>
constexpr RouteTraits launched_traits() {
	constexpr RouteTraits R = kRoutes[ROW].t;
	return {TWIN ? kEntryCfg : R.entry, R.waves, TWIN ? 4 : R.occ, R.prof, R.poisson, R.affine, R.team, R.num, R.xtra};
}
template <int ROW, bool BATCH, bool TWIN>
constexpr auto route_kernel() {
	constexpr RouteTraits T = launched_traits<ROW, TWIN>();
	if constexpr (T.entry == kEntryC128) return &render_kernel_c128<T.waves, T.prof, T.poisson, T.affine, T.team, T.num, T.xtra, BATCH>;
	else return &render_kernel<T.waves, T.occ, T.prof, T.poisson, T.affine, T.team, T.num, T.xtra, BATCH>;
}
template <int ROW, bool BATCH, bool TWIN = false>
static int launch_row(const DeviceModel& m, const RenderArgs& a, int n_cus, hipStream_t stream) {
	constexpr RouteTraits T = launched_traits<ROW, TWIN>();
	constexpr bool C128 = T.entry == kEntryC128;
	constexpr auto kernel = route_kernel<ROW, BATCH, TWIN>();
	{ const int rc = check_route(m, a, T, BATCH); if (rc != NRS_OK) return rc; }
	int blocks_per_cu = 0;
	hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, 64 * T.waves, 0);
	if (e != hipSuccess) return hip_fail(e, C128 ? "hipOccupancyMaxActiveBlocksPerMultiprocessor(render_kernel_c128)" : "hipOccupancyMaxActiveBlocksPerMultiprocessor(render_kernel)");
	// amdgpu_num_vgpr is a target, not a limit: when the allocator went past 128 registers for this instantiation (3 waves per SIMD: 7.3 instead of 9.8
	// Gsamples/s), the __launch_bounds__(512, 4) build of the same body -- which cannot -- is the one to launch
	// (a batch twin that went past 128 runs where it is, at 3 waves per SIMD: no third build of the body for it)
	// (the LIGHT twin has no third build either)
	if constexpr (C128 && !BATCH && T.xtra != kXtraLight) { if (blocks_per_cu * T.waves < 16) return launch_row<ROW, false, true>(m, a, n_cus, stream); }
	if (blocks_per_cu < 1) blocks_per_cu = 1;
	uint32_t grid = (uint32_t)(n_cus * blocks_per_cu);
	const uint32_t max_useful = (a.n_packets + T.waves - 1) / T.waves; // at least one packet per wave
	if (grid > max_useful) grid = max_useful;
	if (grid == 0) return NRS_OK;
	static const bool log_kernel = dev_knob("NRS_KERNEL_LOG") != nullptr;
	if (log_kernel) {
		char name[160];
		route_name(name, sizeof(name), T, BATCH);
		fprintf(stderr, "[nrs kernel] %s\n", name);
	}
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * T.waves), 0, stream, m, a);
	NRS_LAUNCH_CHECK("render_kernel launch");
	++g_render_dispatches;
	return NRS_OK;
}

// one row per row of kRoutes: its traits, its single-frame launcher, its batch-twin launcher (null where the row has none: the measurement rows)
typedef int (*RouteLauncher)(const DeviceModel&, const RenderArgs&, int, hipStream_t);
struct RouteLaunch { const RouteTraits* traits; RouteLauncher single, batch; };
template <int ROW>
static constexpr RouteLauncher batch_launcher() {
	if constexpr (kRoutes[ROW].batch) return &launch_row<ROW, true>;
	else return nullptr;
}
template <int... ROW>
struct RouteLaunchTable { RouteLaunch row[sizeof...(ROW)] = {{&kRoutes[ROW].t, &launch_row<ROW, false>, batch_launcher<ROW>()}...}; };
template <int... ROW>
static RouteLaunchTable<ROW...> make_launch_table(std::integer_sequence<int, ROW...>) { return {}; }
static const auto kLaunch = make_launch_table(std::make_integer_sequence<int, kRouteCount>{});

int launch_render(RouteId row, const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream) {
	const bool batch = a.spp_count > 1u;
	const RouteLauncher fn = (int)row >= 0 && row < kRouteCount ? (batch ? kLaunch.row[row].batch : kLaunch.row[row].single) : nullptr;
	if (!fn) {
		snprintf(g_launch_err, sizeof(g_launch_err), "launch_render: route refused: row %d has no instantiation for spp_count %u", (int)row, a.spp_count);
		return NRS_ERR_STATE;
	}
	return fn(m, a, n_cus, (hipStream_t)stream);
}

// per-workgroup LDS of the kernels that run the network on caller batches: the weights + one feature slab per wave
template <int WAVES>
struct NetSmemT {
	ModelLds ml;
	FeatLds fl[WAVES];
};
typedef NetSmemT<4> NetSmem;

// ---- render mode Slice ------------------------------------------------------------------------------------------------
// Testbed::render_nerf's Slice branch (tn:3068-3070, 3109-3162): init_rays_with_payload_kernel_nerf with plane_z < 0 leaves every pixel's ray
// standing on the plane at distance |plane_z| along the view axis (tn:2575-2585: t = -plane_z * |d|, depth buffer = -plane_z, no render-box test);
// generate_nerf_network_inputs_at_current_position (tn:616-622) -> NerfNetwork::inference -> compute_nerf_density (tn:624-635: a = 1 - exp(-sigma / 100),
// premultiplied colour) -> shade_kernel_nerf (srgb_to_linear, alpha-over the frame, NO depth write, tn:2474-2482).  One launch: a wave takes an
// 8x8-pixel packet (the render kernel's packet geometry, whole image or owned tiles), a lane a pixel.
template <int NUM>
__global__ __launch_bounds__(256) void slice_kernel(const DeviceModel m, const RenderArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const nrs_render_params& p = a.p;
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	float off_x, off_y;
	ld_random_pixel_offset(p.snap_to_pixel_centers ? 0u : p.spp_index, off_x, off_y);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	uint32_t n_px = 0;
	for (uint32_t pk = wave_global; pk < a.n_packets; pk += n_waves) {
		uint32_t x, y, oi;
		const bool have = packet_pixel<1>(a, pk, lane, x, y, oi);
		f3 wpos = mk3(0, 0, 0), wdir = mk3(0.5f, 0.5f, 0.5f);
		if (have) {
			f3 o, d;
			pixel_ray_raw<true>(p, x, y, off_x, off_y, 1.0f, o, d, false); // lens distortion applies; dof = 0 when plane_z < 0 (tn:2543-2545)
			const float n = sqrtf(dot3(d, d));
			const f3 dir = (1.0f / n) * d;
			const float t = p.slice_plane_z * n; // -plane_z * n, plane_z = -(m_slice_plane_z + m_scale)
			wpos = warp_position(o + dir * t, m.aabb);
			wdir = warp_direction(dir);
			a.depth[oi] = p.slice_plane_z; // tn:2583
			if (a.steps) a.steps[oi] = 0;
			++n_px;
		}
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		const f3 pdir = mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z));
		half8 sh_own, sh_par;
		encode_sh4_2(g, wdir, pdir, sh_own, sh_par);
		uint32_t res_d = 0, res_rg = 0, res_b = 0;
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, x0, x1);
			// (a network trained with light directions: the frame's light direction for every pixel -- a wave-uniform branch, rgb_mlp's LIGHT)
			const half8 rout = rgb_mlp_num<NUM, true, true>(nm, sm.ml.w, lane, dout, sel ? sh_par : sh_own, m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr,
			                                                m.n_extra_dims ? reinterpret_cast<const half8*>(m.wfrag) : nullptr, light_operand(g, m.light01[0], m.light01[1], m.light01[2]));
			const u32x4 dd = __builtin_bit_cast(u32x4, dout), rr = __builtin_bit_cast(u32x4, rout);
			uint32_t vd = dd[0], vrg = rr[0], vb = rr[1];
			if (b == 1) { vd = xchg32u(vd); vrg = xchg32u(vrg); vb = xchg32u(vb); }
			if (g == b) { res_d = vd; res_rg = vrg; res_b = vb; }
		}
		if (!have) continue;
		const half2v hd = __builtin_bit_cast(half2v, res_d), hrg = __builtin_bit_cast(half2v, res_rg), hb = __builtin_bit_cast(half2v, res_b);
		const float alpha = clampf_(1.f - __expf(-network_to_density((float)hd[0], m.density_activation) / 100.0f), 0.0f, 1.0f);
		float tr = network_to_rgb((float)hrg[0], m.rgb_activation) * alpha, tg = network_to_rgb((float)hrg[1], m.rgb_activation) * alpha,
		      tb = network_to_rgb((float)hb[0], m.rgb_activation) * alpha;
		if (!p.linear_colors) { tr = srgb_to_linear(tr); tg = srgb_to_linear(tg); tb = srgb_to_linear(tb); }
		float4* fb = reinterpret_cast<float4*>(a.frame) + oi;
		const float4 prev = *fb;
		const float om = 1.0f - alpha;
		*fb = make_float4(tr + prev.x * om, tg + prev.y * om, tb + prev.z * om, alpha + prev.w * om);
	}
	// statistics: one evaluated sample, one initialised and one shaded ray per pixel (trace() is not run: n_hit = n_rays_initialized, tn:3109)
	for (int sh = 32; sh > 0; sh >>= 1) n_px += (uint32_t)__shfl_xor((int)n_px, sh, 64);
	if (lane == 0 && n_px) {
		atomicAdd(&a.counters->n_samples, (unsigned long long)n_px);
		atomicAdd(&a.counters->n_rays_alive, n_px);
		atomicAdd(&a.counters->n_rays_hit, n_px);
	}
}
int launch_slice(const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream) {
	if (a.n_packets == 0) return NRS_OK;
	uint32_t grid = (a.n_packets + 3) / 4;
	const uint32_t cap = (uint32_t)n_cus * 8;
	if (grid > cap) grid = cap;
	if (m.numerics) hipLaunchKernelGGL(slice_kernel<kNumRuntime>, dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a);
	else hipLaunchKernelGGL(slice_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("slice_kernel launch");
	return NRS_OK;
}

// ---- CudaRenderBuffer::accumulate (render_buffer.cu:540-560, accumulate_kernel :217-254): the running mean over the spp frames of a view ----------------------
// One thread per pixel, 16 B read x 2 + 16 B written: HBM-bound (100 MB per 1080p frame).  Linear / VisPosNeg are plain fp32 in the reference's order (bit-exact);
// SRGB goes through powf (the device library's here, CUDA's in the reference, glibc's in the oracle: tolerance, not bits).
// one sample joins the running mean of a pixel (accumulate_kernel's body, :217-254)
__device__ __forceinline__ void accumulate_one(float4 color, float4& tmp, float sample_count, int color_space) {
	if (color_space == 2) { // VisPosNeg
		const float val = color.x - color.y;
		float tmp_val = tmp.x - tmp.y;
		tmp_val = (tmp_val * sample_count + val) / (sample_count + 1);
		tmp.x = fmaxf(tmp_val, 0.0f);
		tmp.y = fmaxf(-tmp_val, 0.0f);
	} else {
		if (color_space == 1) { // linear_to_srgb, common_device.cuh:55-61
			color.x = color.x < 0.0031308f ? 12.92f * color.x : 1.055f * powf(color.x, 0.41666f) - 0.055f;
			color.y = color.y < 0.0031308f ? 12.92f * color.y : 1.055f * powf(color.y, 0.41666f) - 0.055f;
			color.z = color.z < 0.0031308f ? 12.92f * color.z : 1.055f * powf(color.z, 0.41666f) - 0.055f;
		}
		tmp.x = (tmp.x * sample_count + color.x) / (sample_count + 1);
		tmp.y = (tmp.y * sample_count + color.y) / (sample_count + 1);
		tmp.z = (tmp.z * sample_count + color.z) / (sample_count + 1);
	}
	tmp.w = (tmp.w * sample_count + color.w) / (sample_count + 1);
}
__global__ __launch_bounds__(256) void accumulate_kernel(uint32_t n, const float4* __restrict__ frame, float4* __restrict__ accum, float sample_count, int color_space, int clear) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 color = frame[i];
	float4 tmp = clear ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i]; // (sample_count == 0: the reference clears the buffer first, :545-547)
	accumulate_one(color, tmp, sample_count, color_space);
	accum[i] = tmp;
}
// The K slabs of a batch (nrs_render_nerf_spp) folded into the running mean in sample order: the per-sample update above K times in registers -- the running mean is not
// associative, so no sum-then-divide -- with one read and one write of the accumulate buffer instead of K.  Every intermediate is the fp32 value K launches of
// accumulate_kernel would have stored and read back: bit-equal to them.
__global__ __launch_bounds__(256) void accumulate_spp_kernel(uint32_t n, const float4* __restrict__ frames, size_t slab_stride, uint32_t spp_count, float4* __restrict__ accum,
                                                             uint32_t sample_count, int color_space) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 tmp = sample_count == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i];
	float4 color = frames[i];
	for (uint32_t k = 0; k < spp_count; ++k) {
		const float4 next = k + 1u < spp_count ? frames[(size_t)(k + 1u) * slab_stride + i] : color; // (the next slab's load is in flight during this sample's divisions)
		accumulate_one(color, tmp, (float)(sample_count + k), color_space);
		color = next;
	}
	accum[i] = tmp;
}
int launch_accumulate(uint32_t n_pixels, const float* d_frame, float* d_accum, uint32_t sample_count, int color_space, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	hipLaunchKernelGGL(accumulate_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frame),
	                   reinterpret_cast<float4*>(d_accum), (float)sample_count, color_space, sample_count == 0 ? 1 : 0);
	NRS_LAUNCH_CHECK("accumulate_kernel launch");
	return NRS_OK;
}
int launch_accumulate_spp(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count, int color_space, void* stream) {
	if (n_pixels == 0 || spp_count == 0) return NRS_OK;
	hipLaunchKernelGGL(accumulate_spp_kernel, dim3((n_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
	                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, color_space);
	NRS_LAUNCH_CHECK("accumulate_spp_kernel launch");
	return NRS_OK;
}

// ---- CudaRenderBuffer::tonemap (render_buffer.cu:562-580, tonemap_kernel :471-501, tonemap :254-332): the display step after accumulate ----------------------------
// One thread per pixel, lanes on consecutive pixels: a wave loads 1 KiB contiguous and stores 1 KiB (RGBA32F) or 256 B (RGBA8) contiguous.  HBM-bound like accumulate
// (32 or 20 B per pixel).  Everything is plain fp32 in the reference's operation order (-ffp-contract=off, no fmaf: bit-exact against a float restatement) except the two
// powf of the sRGB curves (the device library's: tolerance, as in accumulate_kernel).  These are the reference's curves (common_device.cuh:31-37, :55-61) with their powf and
// their division -- not nrs_device.cuh's srgb_to_linear, whose exp2/log2 form is good to 1e-5 only, enough for a network's colour but not for this step's 2e-6.
__device__ __forceinline__ float tonemap_srgb_to_linear(float s) { return s <= 0.04045f ? s / 12.92f : powf((s + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float tonemap_linear_to_srgb(float l) { return l < 0.0031308f ? 12.92f * l : 1.055f * powf(l, 0.41666f) - 0.055f; }
// Array3f::cwiseMax(0.f) / cwiseMin(1.f) as Eigen evaluates them: (a < b) ? b : a and (b < a) ? b : a -- a NaN and the sign of a zero pass through
__device__ __forceinline__ float tonemap_max0(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ float tonemap_min1(float x) { return 1.0f < x ? 1.0f : x; }
// tonemap(Array3f x, ETonemapCurve) of one channel for the two rational curves, :304-308
__device__ __forceinline__ float tonemap_rational(float x, float k0, float k1, float k2, float k3, float k4, float k5) {
	const float sq = x * x;
	const float nom = (sq * k0 + k1 * x) + k2;
	const float denom = (k3 * sq + k4 * x) + k5;
	return nom / denom;
}
// What is uniform across the frame: scale = 2^exposure and, for a colour space other than SRGB, the background's srgb_to_linear (tonemap_kernel does both in every
// thread, :483-485, :321), are evaluated once by launch_tonemap on the host.
struct TonemapArgs {
	float scale;        // powf(2.0f, exposure)
	float bg[4];        // background colour in the accumulate buffer's space
	int color_space;    // EColorSpace of the accumulate buffer
	int out_space;      // EColorSpace of the output (Linear | SRGB)
	int curve;          // ETonemapCurve
	int clamp;          // clamp_output_color
};
// tonemap_kernel's per-pixel work (:487-495) on the value of the accumulate buffer; the branches are wave-uniform
__device__ __forceinline__ float4 tonemap_pixel(float4 c, const TonemapArgs& t) {
	const float weight = (1 - c.w) * t.bg[3];
	c.x += t.bg[0] * weight;
	c.y += t.bg[1] * weight;
	c.z += t.bg[2] * weight;
	c.w += weight;
	if (t.color_space == 1) { c.x = tonemap_srgb_to_linear(c.x); c.y = tonemap_srgb_to_linear(c.y); c.z = tonemap_srgb_to_linear(c.z); } // 1. to linear (VisPosNeg is linear red / green)
	c.x *= t.scale; c.y *= t.scale; c.z *= t.scale;                                                                                 // 2. exposure
	if (t.curve != 0) {                                                                                                               // 3. the curve; Identity returns x untouched
		c.x = tonemap_max0(c.x); c.y = tonemap_max0(c.y); c.z = tonemap_max0(c.z);
		if (t.curve == 3) { // Reinhard
			const float Y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
			const float s = 1.f / (Y + 1.0f);
			c.x *= s; c.y *= s; c.z *= s;
		} else {
			float k0, k1, k2, k3, k4, k5; // constants: folded at compile time, in IEEE fp32 and in this order
			if (t.curve == 1) { // ACES, pre-exposure 0.6 inside the coefficients
				k0 = 0.6f * 0.6f * 2.51f; k1 = 0.6f * 0.03f; k2 = 0.0f;
				k3 = 0.6f * 0.6f * 2.43f; k4 = 0.6f * 0.59f; k5 = 0.14f;
			} else { // Hable, white point 11.2 and exposure bias 2 inside the coefficients
				const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f, W = 11.2f;
				k0 = A * F - A * E; k1 = C * B * F - B * E; k2 = 0.0f;
				k3 = A * F; k4 = B * F; k5 = D * F * F;
				const float nom = k0 * (W * W) + k1 * W + k2;
				const float denom = k3 * (W * W) + k4 * W + k5;
				const float white_scale = denom / nom;
				k0 = 4.0f * k0 * white_scale; k1 = 2.0f * k1 * white_scale; k2 = k2 * white_scale;
				k3 = 4.0f * k3; k4 = 2.0f * k4;
			}
			c.x = tonemap_rational(c.x, k0, k1, k2, k3, k4, k5);
			c.y = tonemap_rational(c.y, k0, k1, k2, k3, k4, k5);
			c.z = tonemap_rational(c.z, k0, k1, k2, k3, k4, k5);
		}
	}
	if (t.out_space == 1) { c.x = tonemap_linear_to_srgb(c.x); c.y = tonemap_linear_to_srgb(c.y); c.z = tonemap_linear_to_srgb(c.z); } // 4. to the output's space
	if (t.clamp) {
		c.x = tonemap_min1(tonemap_max0(c.x)); c.y = tonemap_min1(tonemap_max0(c.y));
		c.z = tonemap_min1(tonemap_max0(c.z)); c.w = tonemap_min1(tonemap_max0(c.w));
	}
	return c;
}
// RGBA32F: the float4 the reference writes to its surface and to lopi.  RGBA8: one dword, bytes R, G, B, A in memory; the clamp is implied (fmaxf / fminf: a NaN becomes 0).
template <int FMT>
__device__ __forceinline__ void tonemap_store(void* out, uint32_t i, float4 c) {
	if (FMT == NRS_TONEMAP_RGBA32F) {
		reinterpret_cast<float4*>(out)[i] = c;
	} else {
		const uint32_t r = (uint32_t)(fminf(fmaxf(c.x, 0.0f), 1.0f) * 255.0f + 0.5f), g = (uint32_t)(fminf(fmaxf(c.y, 0.0f), 1.0f) * 255.0f + 0.5f);
		const uint32_t b = (uint32_t)(fminf(fmaxf(c.z, 0.0f), 1.0f) * 255.0f + 0.5f), a = (uint32_t)(fminf(fmaxf(c.w, 0.0f), 1.0f) * 255.0f + 0.5f);
		reinterpret_cast<uint32_t*>(out)[i] = r | (g << 8) | (b << 16) | (a << 24);
	}
}
// `out` may be `accum` itself for RGBA32F (no __restrict__ on either): a lane reads its pixel before it writes it and touches no other.
template <int FMT>
__global__ __launch_bounds__(256) void tonemap_kernel(uint32_t n, const float4* accum, const TonemapArgs t, void* out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	tonemap_store<FMT>(out, i, tonemap_pixel(accum[i], t));
}
// accumulate_spp_kernel's fold, then tonemap_pixel on the value it stores: the last batch of a view and its display step in one pass (K slabs read, the accumulate buffer
// read once and written once, the output written once).  The same device functions as the two kernels it replaces: bit-equal to them.  `out` aliases nothing here.
template <int FMT>
__global__ __launch_bounds__(256) void accumulate_spp_tonemap_kernel(uint32_t n, const float4* __restrict__ frames, size_t slab_stride, uint32_t spp_count, float4* __restrict__ accum,
                                                                     uint32_t sample_count, const TonemapArgs t, void* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float4 tmp = sample_count == 0u ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[i];
	float4 color = frames[i];
	for (uint32_t k = 0; k < spp_count; ++k) {
		const float4 next = k + 1u < spp_count ? frames[(size_t)(k + 1u) * slab_stride + i] : color;
		accumulate_one(color, tmp, (float)(sample_count + k), t.color_space);
		color = next;
	}
	accum[i] = tmp;
	tonemap_store<FMT>(out, i, tonemap_pixel(tmp, t));
}
static TonemapArgs tonemap_args(const nrs_tonemap_params& p) {
	TonemapArgs t;
	t.scale = powf(2.0f, p.exposure);
	for (int c = 0; c < 4; ++c) t.bg[c] = p.background_color[c];
	if (p.color_space != NRS_COLOR_SRGB) // the background is sRGB-encoded: to linear unless that is the space the buffer is in (:483-485)
		for (int c = 0; c < 3; ++c) t.bg[c] = t.bg[c] <= 0.04045f ? t.bg[c] / 12.92f : powf((t.bg[c] + 0.055f) / 1.055f, 2.4f);
	t.color_space = (int)p.color_space; t.out_space = (int)p.output_color_space; t.curve = (int)p.tonemap_curve; t.clamp = (int)p.clamp_output;
	return t;
}
int launch_tonemap(uint32_t n_pixels, const float* d_accum, const nrs_tonemap_params& p, void* d_out, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	const TonemapArgs t = tonemap_args(p);
	const dim3 grid((n_pixels + 255) / 256), block(256);
	if (p.output_format == NRS_TONEMAP_RGBA8) hipLaunchKernelGGL(tonemap_kernel<NRS_TONEMAP_RGBA8>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_accum), t, d_out);
	else hipLaunchKernelGGL(tonemap_kernel<NRS_TONEMAP_RGBA32F>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_accum), t, d_out);
	NRS_LAUNCH_CHECK("tonemap_kernel launch");
	return NRS_OK;
}
int launch_accumulate_spp_tonemap(uint32_t n_pixels, const float* d_frames, size_t slab_stride_pixels, uint32_t spp_count, float* d_accum, uint32_t sample_count,
                                  const nrs_tonemap_params& p, void* d_out, void* stream) {
	if (n_pixels == 0 || spp_count == 0) return NRS_OK;
	const TonemapArgs t = tonemap_args(p);
	const dim3 grid((n_pixels + 255) / 256), block(256);
	if (p.output_format == NRS_TONEMAP_RGBA8)
		hipLaunchKernelGGL(accumulate_spp_tonemap_kernel<NRS_TONEMAP_RGBA8>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
		                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, t, d_out);
	else
		hipLaunchKernelGGL(accumulate_spp_tonemap_kernel<NRS_TONEMAP_RGBA32F>, grid, block, 0, (hipStream_t)stream, n_pixels, reinterpret_cast<const float4*>(d_frames), slab_stride_pixels,
		                   spp_count, reinterpret_cast<float4*>(d_accum), sample_count, t, d_out);
	NRS_LAUNCH_CHECK("accumulate_spp_tonemap_kernel launch");
	return NRS_OK;
}

// ---- trace_samples ------------------------------------------------------------------------------------------------
// LENS: the camera model nrs_render_nerf's EXTRA instantiation marches with (depth of field, lens distortion, the distortion map) -- the hook must
// emit the samples of the rays the renderer really shoots
template <bool LENS>
__global__ void trace_samples_kernel(const DeviceModel m, const nrs_render_params p, uint32_t n_pixels, const uint32_t* __restrict__ pixel_idx,
                                     uint32_t max_samples, float* __restrict__ t_out, float* __restrict__ dt_out, uint32_t* __restrict__ count_out) {
	__shared__ uint32_t coarse[kMarchLdsWords];
	stage_march_lds(coarse, m.occ.mask);
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_pixels) return;
	float off_x, off_y;
	ld_random_pixel_offset(p.snap_to_pixel_centers ? 0u : p.spp_index, off_x, off_y);
	const uint32_t idx = pixel_idx[k], W = (uint32_t)p.resolution[0];
	Ray r = init_ray<LENS>(p, idx % W, idx / W, off_x, off_y);
	uint32_t cnt = 0;
	if (r.alive && first_hit(p, m, coarse, idx, r)) {
		float t = r.t;
		while (cnt < max_samples) {
			f3 pos; float dt;
			if (!march_to_occupied(p, m, coarse, r.o, r.d, t, pos, dt)) break;
			t_out[(size_t)k * max_samples + cnt] = t;
			dt_out[(size_t)k * max_samples + cnt] = dt;
			++cnt;
			t += dt;
		}
	}
	count_out[k] = cnt;
}

int launch_trace_samples(const DeviceModel& m, const nrs_render_params& p, uint32_t n_pixels, const uint32_t* d_pixel_idx, uint32_t max_samples,
                         float* d_t, float* d_dt, uint32_t* d_count, void* stream) {
	if (n_pixels == 0) return NRS_OK;
	const bool lens = p.dof != 0.f || p.distortion_mode != 0u || p.d_distortion_map != nullptr;
	if (lens) hipLaunchKernelGGL(trace_samples_kernel<true>, dim3((n_pixels + 127) / 128), dim3(128), 0, (hipStream_t)stream, m, p, n_pixels, d_pixel_idx, max_samples, d_t, d_dt, d_count);
	else hipLaunchKernelGGL(trace_samples_kernel<false>, dim3((n_pixels + 127) / 128), dim3(128), 0, (hipStream_t)stream, m, p, n_pixels, d_pixel_idx, max_samples, d_t, d_dt, d_count);
	NRS_LAUNCH_CHECK("trace_samples_kernel launch");
	return NRS_OK;
}


// ---- selection rays ------------------------------------------------------------------------------------------------
// GrowingSelection::project_selection_pixels (growing_selection.cu:1832-2035) in one launch: shoot_selection_rays_kernel
// (:1673; the ray of pixel_to_ray with spp 0, direction NOT normalised, start at max(t_enter, 0), up to NERF_STEPS samples
// on occupied cells, no min_mip) -> NerfNetwork::density -> composite_shot_rays (:1768; the first sample REACHED with
// T <= threshold is the answer: its position after the warp / unwarp round trip and its occupancy cell).  The reference
// writes every sample, runs the network on all of them and then composites; here a lane owns a ray, the wave evaluates one
// sample per ray and round, and a ray stops at its answer -- the samples behind it are never needed.
constexpr uint32_t kNerfSteps = 1024; // NERF_STEPS, common_nerf.h:20
struct SelectionArgs {
	nrs_render_params p;
	const int32_t* pixels; // [n][2]
	uint32_t n;
	float threshold;
	float* positions;      // [n][3]
	uint32_t* cells;       // [n]
	uint8_t* found;        // [n]
};
template <int NUM>
__global__ __launch_bounds__(256) void selection_rays_kernel(const DeviceModel m, const SelectionArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const nrs_render_params& p = a.p;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	bool have = i < a.n;
	f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), idir = mk3(0, 0, 0);
	float t = 0.f, T = 1.f;
	uint32_t j = 0;
	if (have) {
		float off_x, off_y;
		ld_random_pixel_offset(0u, off_x, off_y);
		const float W = (float)p.resolution[0], H = (float)p.resolution[1];
		const float uvx = ((float)a.pixels[2 * i] + off_x) / W, uvy = ((float)a.pixels[2 * i + 1] + off_y) / H;
		const f3 dir = {(uvx - p.screen_center[0]) * W / p.focal_length[0], (uvy - p.screen_center[1]) * H / p.focal_length[1], 1.0f};
		const float* cam = p.camera_matrix1;
		d = mat3_mul(cam, dir);
		o = mk3(cam[9], cam[10], cam[11]);
		idir = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
		float tmin;
		ray_intersect(m.aabb.mn, m.aabb.mx, o, d, tmin);
		t = fmaxf(tmin, 0.0f);
		a.found[i] = 0;
		a.cells[i] = 0;
		a.positions[3 * i] = m.aabb.mn[0] - 1.f; a.positions[3 * i + 1] = m.aabb.mn[1] - 1.f; a.positions[3 * i + 2] = m.aabb.mn[2] - 1.f; // :1826
	}
	while (__any(have)) {
		// next sample of the ray (the walk of :1716-1727 / :1754-1765)
		f3 pos = mk3(0, 0, 0);
		float dt = 0.f;
		if (have) {
			bool at_sample = false;
			while (j < kNerfSteps) {
				pos = o + d * t;
				if (!box_contains(m.aabb, pos)) break;
				dt = calc_dt(t, p.cone_angle_constant);
				const uint32_t mip = (uint32_t)mip_from_dt(dt, pos);
				if (density_grid_occupied_at(pos, m.bitfield, mip)) { at_sample = true; break; }
				t = advance_to_next_voxel(t, p.cone_angle_constant, pos, d, idir, kGrid >> mip, 1.0f / (float)(kGrid >> mip));
			}
			if (!at_sample) have = false; // no further sample: transmittance never fell to the threshold (positions stays at the marker)
		}
		const f3 wpos = have ? warp_position(pos, m.aabb) : mk3(0, 0, 0);
		if (have && T <= a.threshold) { // :1802-1809
			const f3 up = unwarp_position(wpos, m.aabb);
			a.positions[3 * i] = up.x; a.positions[3 * i + 1] = up.y; a.positions[3 * i + 2] = up.z;
			const uint32_t level = (uint32_t)mip_from_pos(up);
			a.cells[i] = level * kGridVol + cascaded_grid_idx_at(up, level);
			a.found[i] = 1;
			have = false;
		}
		if (!__any(have)) break;
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		uint32_t res_d = 0;
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, load_features(fl, lane, sel, 0), load_features(fl, lane, sel, 1));
			uint32_t vd = __builtin_bit_cast(u32x4, dout)[0];
			if (b == 1) vd = xchg32u(vd);
			if (g == b) res_d = vd;
		}
		if (have) {
			const float density = network_to_density((float)__builtin_bit_cast(half2v, res_d)[0], m.density_activation);
			const float alpha = 1.f - __expf(-density * unwarp_dt(warp_dt(dt))); // (the reference reads dt back from the NerfCoordinate)
			T *= (1.f - alpha);
			++j;
			t += dt;
		}
	}
}
int launch_selection_rays(const DeviceModel& m, const nrs_render_params& p, const int32_t* d_pixels, uint32_t n, float threshold,
                          float* d_positions, uint32_t* d_cells, uint8_t* d_found, void* stream) {
	if (n == 0) return NRS_OK;
	SelectionArgs a{};
	a.p = p; a.pixels = d_pixels; a.n = n; a.threshold = threshold; a.positions = d_positions; a.cells = d_cells; a.found = d_found;
	if (m.numerics) hipLaunchKernelGGL(selection_rays_kernel<kNumRuntime>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, a);
	else hipLaunchKernelGGL(selection_rays_kernel<0>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, m, a);
	NRS_LAUNCH_CHECK("selection_rays_kernel launch");
	return NRS_OK;
}

// ---- membrane boundary values -------------------------------------------------------------------------------------
// The device half of GrowingSelection::compute_poisson_boundary (growing_selection.cu:2220-2348) after the network has run on
// the n_sh samples of every cage vertex: activate_network_output (:2182), filter_empty (:2200, is_inside only), the vertex's
// density (its first sample) and the SH9 fit (project_sh9 summed in sample order, times 4 pi / n_sh; sh_utils.cu:30-69).
// One 64-thread workgroup per vertex; thread c < 27 owns coefficient (k = c % 9, colour = c / 9) and sums it sequentially.
__global__ __launch_bounds__(64) void poisson_fit_kernel(const DeviceModel m, uint32_t n_sh, const float* __restrict__ coords /* [n][7] */,
                                                         const _Float16* __restrict__ net /* [n][16] */, int is_inside, float scale,
                                                         float* __restrict__ density_out, float* __restrict__ sh_out /* [n_verts][27] */) {
	const uint32_t v = blockIdx.x, c = threadIdx.x;
	const size_t base = (size_t)v * n_sh;
	if (c == 0) {
		float density = network_to_density((float)net[base * 16 + 3], m.density_activation);
		if (is_inside) {
			const f3 pos = unwarp_position(mk3(coords[base * 7], coords[base * 7 + 1], coords[base * 7 + 2]), m.aabb);
			if (!density_grid_occupied_at(pos, m.bitfield, (uint32_t)mip_from_pos(pos))) density = 0.0f;
		}
		density_out[v] = density;
	}
	if (c >= 27) return;
	const uint32_t kk = c % 9, col = c / 9;
	float acc = 0.f;
	for (uint32_t i = 0; i < n_sh; ++i) {
		const float* co = coords + (base + i) * 7;
		const f3 d = unwarp_direction(mk3(co[4], co[5], co[6]));
		const float rgb = network_to_rgb((float)net[(base + i) * 16 + col], m.rgb_activation);
		const float x = d.x, y = d.y, z = d.z;
		float term;
		switch (kk) { // prefilter.c's constants, rounded to float as the reference's `float c = 0.282095;` does
			case 0: term = rgb * 0.282095f; break;
			case 1: term = rgb * (0.488603f * y); break;
			case 2: term = rgb * (0.488603f * z); break;
			case 3: term = rgb * (0.488603f * x); break;
			case 4: term = rgb * (1.092548f * x * y); break;
			case 5: term = rgb * (1.092548f * y * z); break;
			case 7: term = rgb * (1.092548f * x * z); break;
			case 6: term = rgb * (0.315392f * (3 * z * z - 1)); break;
			default: term = rgb * (0.546274f * (x * x - y * y)); break;
		}
		acc += term; // (times domega = 1.0f: exact)
	}
	sh_out[(size_t)v * 27 + c] = acc * scale;
}
int launch_poisson_fit(const DeviceModel& m, uint32_t n_verts, uint32_t n_sh, const float* d_coords, const void* d_net, int is_inside, float scale,
                       float* d_density, float* d_sh, void* stream) {
	if (n_verts == 0) return NRS_OK;
	hipLaunchKernelGGL(poisson_fit_kernel, dim3(n_verts), dim3(64), 0, (hipStream_t)stream, m, n_sh, d_coords, (const _Float16*)d_net, is_inside, scale, d_density, d_sh);
	NRS_LAUNCH_CHECK("poisson_fit_kernel launch");
	return NRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Cell records (nrs_model_set_cell_cache): for every cell of a level, its 8 corner entries in corner order (x fastest),
// fetched with the level's own index function (grid.h:76-95 as restated in level_eval_slow) -- so a record gather returns
// exactly what the eight hashed / dense gathers would.  One thread per cell, 32 B written per thread, coalesced.
__global__ __launch_bounds__(256) void cell_records_kernel(const uint32_t* __restrict__ grid, const LevelParams lp, uint4* __restrict__ out) {
	const uint32_t n = lp.rec_res * lp.rec_res2;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const uint32_t gx = i % lp.rec_res, gy = (i / lp.rec_res) % lp.rec_res, gz = i / lp.rec_res2;
		uint32_t v[8];
		#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const uint32_t cx = gx + (c & 1), cy = gy + ((c >> 1) & 1), cz = gz + ((c >> 2) & 1);
			uint32_t index = lp.hashed ? ((cx * 1u) ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * lp.resolution + cz * lp.res2);
			index %= lp.count;
			v[c] = grid[lp.offset + index];
		}
		uint4* o = out + 2 * ((size_t)lp.rec_first + i);
		o[0] = make_uint4(v[0], v[1], v[2], v[3]);
		o[1] = make_uint4(v[4], v[5], v[6], v[7]);
	}
}
int launch_cell_records(const DeviceModel& m, uint32_t n_levels, void* d_records, void* stream) {
	for (uint32_t l = 0; l < n_levels; ++l) {
		const LevelParams& lp = m.levels[l];
		const uint64_t n = (uint64_t)lp.rec_res * lp.rec_res2;
		const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 20);
		hipLaunchKernelGGL(cell_records_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m.grid, lp, (uint4*)d_records);
	}
	return hipGetLastError() == hipSuccess ? NRS_OK : NRS_ERR_HIP;
}

// MFMA weight fragments from a parameter blob that lives on the device (nrs_model_set_params_device): frag[i] = params[src[i] - 1], or 0 where
// src[i] == 0 (padding rows).  src is make_weight_fragments' permutation, computed once per model on the host.
__global__ __launch_bounds__(256) void weight_fragments_kernel(const uint16_t* __restrict__ params, const uint16_t* __restrict__ src, uint16_t* __restrict__ frag, uint32_t n) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = src[i];
	// (kFragOne / kFragMinusOne: the constants of the selection fragments and of lowered networks; bit 15: a negated weight -- lower_weights, nrs_api.cpp)
	const uint32_t idx = k & (uint32_t)(kFragNegate - 1u);
	frag[i] = k == kFragOne ? (uint16_t)0x3C00 : (k == kFragMinusOne ? (uint16_t)0xBC00 : (idx ? (uint16_t)(params[idx - 1u] ^ (k & kFragNegate)) : (uint16_t)0));
}
int launch_weight_fragments(const uint16_t* d_params, const uint16_t* d_src, uint16_t* d_frag, uint32_t n, void* stream) {
	hipLaunchKernelGGL(weight_fragments_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_params, d_src, d_frag, n);
	NRS_LAUNCH_CHECK("weight_fragments_kernel launch");
	return NRS_OK;
}

// ---- sparse cell records (nrs_model_set_sparse_cell_cache) -------------------------------------------------------------------------
// brick_mark_kernel: one thread per cell of the 5-cascade mask (density-bitfield layout).  A marked cell allocates every 8^3-cell
// brick of the level that its box touches (one cell of margin: samples sit anywhere inside the density cell, borders included).
// Slots are handed out in arrival order; the records do not depend on it.
__global__ __launch_bounds__(256) void brick_mark_kernel(const LevelParams lp, const Box3 aabb, const uint8_t* __restrict__ mask, uint32_t* __restrict__ table,
                                                         uint32_t* __restrict__ counter, uint32_t* __restrict__ slots, uint32_t capacity) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= kGridVol * kCascades) return;
	if (!((mask[i >> 3] >> (i & 7u)) & 1u)) return;
	const uint32_t level = i / kGridVol, idx = i % kGridVol;
	const float s = ldexpf(1.0f, (int)level);
	const uint32_t cx = morton3D_invert(idx), cy = morton3D_invert(idx >> 1), cz = morton3D_invert(idx >> 2);
	const float c[3] = {(float)cx, (float)cy, (float)cz};
	int lo[3], hi[3];
	for (int k = 0; k < 3; ++k) {
		const float w0 = ((c[k] / (float)kGrid - 0.5f) * s + 0.5f - aabb.mn[k]) / (aabb.mx[k] - aabb.mn[k]);
		const float w1 = (((c[k] + 1.0f) / (float)kGrid - 0.5f) * s + 0.5f - aabb.mn[k]) / (aabb.mx[k] - aabb.mn[k]);
		if (w1 < 0.f || w0 > 1.f) return; // outside the scene box: no lookups there (records cover [0,1]^3)
		const int g0 = (int)floorf(fmaf(lp.scale, fmaxf(w0, 0.f), 0.5f)) - 1, g1 = (int)floorf(fmaf(lp.scale, fminf(w1, 1.f), 0.5f)) + 1;
		lo[k] = max(g0, 0) >> 3;
		hi[k] = min(g1, (int)lp.resolution - 1) >> 3;
	}
	for (int bz = lo[2]; bz <= hi[2]; ++bz)
		for (int by = lo[1]; by <= hi[1]; ++by)
			for (int bx = lo[0]; bx <= hi[0]; ++bx) {
				const uint32_t b = (uint32_t)bz * lp.rec_res2 + (uint32_t)by * lp.rec_res + (uint32_t)bx;
				if (table[b] != 0u) continue;
				if (atomicCAS(&table[b], 0u, 0xffffffffu) == 0u) {
					const uint32_t slot = atomicAdd(counter, 1u);
					if (slot < capacity) slots[slot] = b;
					__atomic_store_n(&table[b], slot + 1u, __ATOMIC_RELAXED);
				}
			}
}
// brick_fill_kernel: one thread per record of an allocated brick: the cell's 8 corner entries, fetched with the level's own index
// function exactly as cell_records_kernel does.
__global__ __launch_bounds__(256) void brick_fill_kernel(const uint32_t* __restrict__ grid, const LevelParams lp, const uint32_t* __restrict__ slots, uint32_t n_bricks,
                                                         uint4* __restrict__ out) {
	const uint64_t n = (uint64_t)n_bricks * kBrickCells;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t b = slots[i >> 9], within = (uint32_t)i & 511u; // (the thread's cell in x-fastest order; its record sits at brick_slot)
		const uint32_t bx = b % lp.rec_res, by = (b / lp.rec_res) % lp.rec_res, bz = b / lp.rec_res2;
		const uint32_t gx = bx * 8u + (within & 7u), gy = by * 8u + ((within >> 3) & 7u), gz = bz * 8u + (within >> 6);
		uint32_t v[8];
		#pragma unroll
		for (int c = 0; c < 8; ++c) {
			const uint32_t cx = gx + (c & 1), cy = gy + ((c >> 1) & 1), cz = gz + ((c >> 2) & 1);
			uint32_t index = lp.hashed ? ((cx * 1u) ^ (cy * 2654435761u) ^ (cz * 805459861u)) : (cx + cy * lp.resolution + cz * lp.res2);
			index %= lp.count;
			v[c] = grid[lp.offset + index];
		}
		uint4* o = out + 2 * ((size_t)lp.rec_first + (i & ~(uint64_t)511u) + brick_slot(within & 7u, (within >> 3) & 7u, within >> 6));
		o[0] = make_uint4(v[0], v[1], v[2], v[3]);
		o[1] = make_uint4(v[4], v[5], v[6], v[7]);
	}
}
int launch_brick_mark(const DeviceModel& m, const LevelParams& lp, const uint8_t* d_mask, uint32_t* d_table, uint32_t* d_counter, uint32_t* d_slots, uint32_t capacity, void* stream) {
	hipLaunchKernelGGL(brick_mark_kernel, dim3((kGridVol * kCascades + 255) / 256), dim3(256), 0, (hipStream_t)stream, lp, m.aabb, d_mask, d_table, d_counter, d_slots, capacity);
	NRS_LAUNCH_CHECK("brick_mark_kernel launch");
	return NRS_OK;
}
int launch_brick_fill(const DeviceModel& m, const LevelParams& lp, const uint32_t* d_slots, uint32_t n_bricks, void* d_records2, void* stream) {
	if (!n_bricks) return NRS_OK;
	const uint64_t n = (uint64_t)n_bricks * kBrickCells;
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 20);
	hipLaunchKernelGGL(brick_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m.grid, lp, d_slots, n_bricks, (uint4*)d_records2);
	NRS_LAUNCH_CHECK("brick_fill_kernel launch");
	return NRS_OK;
}

// MODE 0: inference_mixed_precision (16 channels, c3 = density raw; MODE 5: the same for a network with a third rgb hidden layer), 1: density(), 2: hash-grid features [n x 32]
// 768-thread workgroups: 12 waves share one LDS copy of the weights (24 KB) next to their 12 feature slabs (48 KB), two workgroups per CU
// = 6 waves/SIMD at <= 80 VGPRs.  (256-thread workgroups, the first shape, put 3 workgroups = 3 waves/SIMD on a CU: the weights' copy
// per workgroup was what filled the LDS.)
constexpr int kNetWaves = 12;
// MODE 3: NerfNetwork::input_gradient(stream, 3, ...) -> d density_raw / d position, f32 [n x 3]; MODE 4: visualize_activation(layer, dim) -> f32 [n]
// (layout = layer | dim << 8); both as restated in oracle/nrs_oracle.cpp -- the callers of the render path's Normals / EncodingVis modes and of
// compute_mesh_vertex_normals (tn:4491).
// LIGHT (modes 0 and 4): a network trained with light directions (DeviceModel::n_extra_dims = 3; rgb_mlp's LIGHT) -- every sample gets DeviceModel::light01, or, with
// ld_light != 0, floats 7..9 of its own record (already warped: the reference's PitchedPtr<NerfCoordinate> with extra_stride).  Its MODE 0 serves the third hidden layer
// too (a wave-uniform branch on DeviceModel::rgb_deep).  The instantiations without the flag are what they were before it existed.
template <int MODE, int NUM = 0, bool LIGHT = false>
__global__ __launch_bounds__(64 * kNetWaves, (MODE == 3 || MODE == 4 || LIGHT) ? 3 : 6) void network_kernel(const DeviceModel m, uint32_t n, const float* __restrict__ in, uint32_t ld_in,
                                                      _Float16* __restrict__ out, uint32_t ld_out, int layout, uint32_t ld_light = 0u) {
	constexpr bool FULL = MODE == 0 || MODE == 5; // (5: the full network with a third rgb hidden layer, DeviceModel::rgb_deep -- base_3layer.json)
	const half8* light_w = LIGHT ? reinterpret_cast<const half8*>(m.wfrag) : nullptr;
	const half8* deep_w = (MODE == 5 || (LIGHT && m.rgb_deep)) ? reinterpret_cast<const half8*>(m.wfrag) : nullptr;
	__shared__ NetSmemT<kNetWaves> sm;
	stage_model_to_lds(m, sm.ml);
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5, j = lane & 31;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	const uint32_t n_tiles = (n + 63) / 64;
	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < n;
		f3 wpos = mk3(0, 0, 0), wdir = mk3(0.5f, 0.5f, 0.5f), wlight = mk3(m.light01[0], m.light01[1], m.light01[2]);
		if (have) {
			const float* c = in + (size_t)s * ld_in;
			wpos = mk3(c[0], c[1], c[2]);
			// (NerfNetworkNoDir never looks at the direction rows: a caller may leave them unset, and 0-weights do not stop a NaN)
			if ((FULL || MODE == 4) && !m.no_dir) wdir = mk3(c[4], c[5], c[6]);
			if (LIGHT && ld_light) wlight = mk3(c[7], c[8], c[9]);
		}
		// the light operands of the lane's own sample and of its partner's (lane ^ 32): block b's comes from the lanes 0..31, as for the SH coefficients
		half8 lb_own = half8{}, lb_par = half8{};
		if (LIGHT) {
			lb_own = light_operand(g, wlight.x, wlight.y, wlight.z);
			lb_par = light_operand(g, xchg32(wlight.x), xchg32(wlight.y), xchg32(wlight.z));
		}
		encode_to_lds<(NUM & 1) != 0>(gv, m.levels, sm.ml, fl, lane, g, wpos, have); // (four levels per round trip measured here: ray-ordered batches +-0, random ones -3.5 %: profiles/r06/ab_net_quads.txt; six waves per SIMD hide the trips)

		if (MODE == 3) {
			uint32_t dfe[2][8];
			#pragma unroll
			for (int b = 0; b < 2; ++b) {
				const int sel = (b != g) ? 1 : 0;
				density_backward_features<(NUM & 2) != 0>(sm.ml.w, reinterpret_cast<const half8*>(m.wfrag), lane, load_features(fl, lane, sel, 0), load_features(fl, lane, sel, 1), dfe[b]);
			}
			__builtin_amdgcn_wave_barrier();
			uint32_t* G = &fl.feat[0][0][0];
			#pragma unroll
			for (int b = 0; b < 2; ++b)
				#pragma unroll
				for (int q = 0; q < 8; ++q) G[level_of_pair(q, g) * 64 + (lane & 31) + 32 * b] = dfe[b][q];
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			float res[3] = {0.f, 0.f, 0.f};
			#pragma unroll 1
			for (int L = 0; L < (int)kLevels; ++L) level_input_gradient(gv, m.levels[L], wpos, G[L * 64 + lane], res);
			__builtin_amdgcn_wave_barrier();
			if (have) {
				float* o = reinterpret_cast<float*>(out) + 3 * (size_t)s;
				o[0] = res[0] * (1.0f / 128.0f); o[1] = res[1] * (1.0f / 128.0f); o[2] = res[2] * (1.0f / 128.0f);
			}
			continue;
		}
		if (MODE == 4) {
			const uint32_t layer = (uint32_t)layout & 0xffu, dim = (uint32_t)layout >> 8;
			float v = 0.f;
			if (layer == 0u) {
				const uint32_t L = dim >> 1;
				const uint32_t w = ((L & 1u) == (uint32_t)g) ? fl.feat[L >> 1][0][lane] : fl.feat[L >> 1][1][lane ^ 32];
				v = (float)__builtin_bit_cast(half2v, w)[dim & 1u];
			} else if (LIGHT && layer == 2u && dim >= 32u) { // the Identity encoding of the light direction (units 32..34) and its padding ones
				const float l = dim == 32u ? wlight.x : (dim == 33u ? wlight.y : wlight.z);
				v = dim < 35u ? (float)(_Float16)l : 1.0f;
			} else if (layer == 2u && dim >= 16u) {
				const half8 sh_own = encode_sh4(g, wdir), sh_par = encode_sh4(g, mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z)));
				const uint32_t cidx = dim - 16u;
				const float mine = (float)pick8(sh_own, (int)(cidx & 7u)), theirs = xchg32((float)pick8(sh_par, (int)(cidx & 7u)));
				v = ((cidx >> 3) == (uint32_t)g) ? mine : theirs;
			} else {
				const half8 sh_own = encode_sh4(g, wdir), sh_par = encode_sh4(g, mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z)));
				#pragma unroll 1
				for (int b = 0; b < 2; ++b) {
					const int sel = (b != g) ? 1 : 0;
					const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
					float val;
					int half_of_row;
					if (layer == 2u) {
						const half8 dout = density_mlp<(NUM & 2) != 0>(sm.ml.w, lane, x0, x1);
						val = (float)pick8(dout, (int)((dim & 3u) + 4u * (dim >> 3)));
						half_of_row = (int)((dim >> 2) & 1u);
					} else {
						half8 din = x0;
						if (layer >= 3u) din = density_mlp<(NUM & 2) != 0>(sm.ml.w, lane, x0, x1);
						val = mlp_hidden_activation<(NUM & 2) != 0, LIGHT>(sm.ml.w, lane, x0, x1, din, sel ? sh_par : sh_own, layer, dim, m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr,
						                                                   light_w, sel ? lb_par : lb_own);
						half_of_row = tile_half(dim);
					}
					if (half_of_row != b) val = xchg32(val);
					if (g == b) v = val;
				}
			}
			if (have) reinterpret_cast<float*>(out)[s] = v;
			continue;
		}

		if (MODE == 2) {
			#pragma unroll 1
			for (int b = 0; b < 2; ++b) {
				const uint32_t sb = tile * 64 + 32 * b + j;
				const int sel = (b != g) ? 1 : 0;
				if (sb < n) {
					#pragma unroll
					for (int it = 0; it < 8; ++it) // level 2*it+g, two features per dword
						reinterpret_cast<uint32_t*>(out)[(size_t)sb * 16 + 2 * it + g] = fl.feat[it][sel][lane];
				}
			}
			continue;
		}

		half8 sh_own, sh_par;
		if (FULL) {
			const f3 pdir = mk3(xchg32(wdir.x), xchg32(wdir.y), xchg32(wdir.z));
			sh_own = encode_sh4(g, wdir);
			sh_par = encode_sh4(g, pdir);
		}
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			const half8 dout = density_mlp<(NUM & 2) != 0>(sm.ml.w, lane, x0, x1);
			half8 rout = dout;
			if (FULL) rout = rgb_mlp<(NUM & 2) != 0, MODE == 5 || LIGHT, LIGHT>(sm.ml.w, lane, dout, sel ? sh_par : sh_own, deep_w, light_w, sel ? lb_par : lb_own);
			const uint32_t sb = tile * 64 + 32 * b + j;
			if (sb < n) {
				uint32_t ldo = ld_out; // (opaque per tile: the eight 64-bit row offsets were hoisted out of the tile loop and, in the fp16-accumulator twins, spilled)
				asm volatile("" : "+s"(ldo));
				#pragma unroll
				for (int e = 0; e < 8; ++e) {
					const int row = (e & 3) + 8 * (e >> 2) + 4 * g;
					_Float16 v = rout[e];
					if (FULL && e == 3) v = g ? v : dout[0]; // extract_density (nerf_network_full.h:89-95): row 3 <- density row 0, both on g == 0
					if (layout == NRS_PLANES) out[(size_t)row * ldo + sb] = v;
					else out[(size_t)sb * 16 + row] = v;
				}
			}
		}
	}
}

int launch_network(const DeviceModel& m, int mode, uint32_t n, const float* d_in, uint32_t ld_in, void* d_out, uint32_t ld_out, int layout,
                   int n_cus, void* stream, bool per_sample_light) {
	if (n == 0) return NRS_OK;
	if (per_sample_light && (!m.n_extra_dims || ld_in < 10u)) { snprintf(g_launch_err, sizeof(g_launch_err), "launch_network: per-sample light directions need n_extra_dims = 3 and ld_in >= 10"); return NRS_ERR_STATE; }
	const uint32_t ld_light = per_sample_light ? 1u : 0u;
	const uint32_t n_tiles = (n + 63) / 64;
	uint32_t grid = (n_tiles + kNetWaves - 1) / kNetWaves;
	const uint32_t cap = (uint32_t)n_cus * 2; // resident workgroups: the tiles are strided over them
	if (grid > cap) grid = cap;
	hipStream_t s = (hipStream_t)stream;
	_Float16* out = (_Float16*)d_out;
#define NRS_NET_LAUNCH(MODE, NUM) hipLaunchKernelGGL((network_kernel<MODE, NUM>), dim3(grid), dim3(64 * kNetWaves), 0, s, m, n, d_in, ld_in, out, ld_out, layout)
#define NRS_NET_MODE(MODE)                                      \
	switch (m.numerics & 3u) {                                  \
		case 0: NRS_NET_LAUNCH(MODE, 0); break;                 \
		case 1: NRS_NET_LAUNCH(MODE, 1); break;                 \
		case 2: NRS_NET_LAUNCH(MODE, 2); break;                 \
		default: NRS_NET_LAUNCH(MODE, 3); break;                \
	}
#define NRS_NET_LIGHT(MODE, NUM) hipLaunchKernelGGL((network_kernel<MODE, NUM, true>), dim3(grid), dim3(64 * kNetWaves), 0, s, m, n, d_in, ld_in, out, ld_out, layout, ld_light)
#define NRS_NET_MODE_LIGHT(MODE)                                \
	switch (m.numerics & 3u) {                                  \
		case 0: NRS_NET_LIGHT(MODE, 0); break;                  \
		case 1: NRS_NET_LIGHT(MODE, 1); break;                  \
		case 2: NRS_NET_LIGHT(MODE, 2); break;                  \
		default: NRS_NET_LIGHT(MODE, 3); break;                 \
	}
	if (mode == 0 && m.n_extra_dims) { NRS_NET_MODE_LIGHT(0) }
	else if (mode == 4 && m.n_extra_dims) { NRS_NET_MODE_LIGHT(4) }
	else if (mode == 0 && m.rgb_deep) { NRS_NET_MODE(5) }
	else if (mode == 0) { NRS_NET_MODE(0) }
	else if (mode == 1) { NRS_NET_MODE(1) }
	else if (mode == 3) { NRS_NET_MODE(3) }
	else if (mode == 4) { NRS_NET_MODE(4) }
	else { NRS_NET_MODE(2) }
#undef NRS_NET_MODE_LIGHT
#undef NRS_NET_LIGHT
#undef NRS_NET_MODE
#undef NRS_NET_LAUNCH
	NRS_LAUNCH_CHECK("network_kernel launch");
	return NRS_OK;
}

// ---- the network on a regular grid: Testbed::get_density_on_grid (tn:4538) / get_rgba_on_grid (tn:4588) ------------------------
// MODE 0: raw density (row 0 of the density MLP) per grid point, -10000 where the density grid says "empty" (grid_samples_half_to_float,
//         tn:464-481); MODE 1: premultiplied rgba for a fixed view direction (compute_nerf_density, tn:624-635).  The reference
//         materialises the position array and runs the network in 2^20-point batches; here a lane generates its own point.
struct GridEvalArgs {
	uint32_t res[3];
	float box_mn[3], box_mx[3];  // the box the grid spans (world units)
	float dir01[3];              // MODE 1: warp_direction(ray_dir)
	const float* density_grid;   // MODE 0: nullable
	float* out;                  // MODE 0: float [n]; MODE 1: float4 [n]
};
template <int MODE, int NUM>
__global__ __launch_bounds__(256) void grid_eval_kernel(const DeviceModel m, const GridEvalArgs a) {
	__shared__ NetSmem sm;
	stage_model_to_lds(m, sm.ml);
	const uint32_t nm = NUM == kNumRuntime ? (uint32_t)__builtin_amdgcn_readfirstlane((int)m.numerics) : (uint32_t)NUM;
	const int lane = threadIdx.x & 63;
	const int g = lane >> 5, j = lane & 31;
	FeatLds& fl = sm.fl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
	const GridView gv = make_grid_view(m);
	const uint32_t wave_global = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
	const uint32_t n = a.res[0] * a.res[1] * a.res[2];
	const uint32_t n_tiles = (n + 63) / 64;
	const f3 wdir = mk3(a.dir01[0], a.dir01[1], a.dir01[2]);
	for (uint32_t tile = wave_global; tile < n_tiles; tile += n_waves) {
		const uint32_t s = tile * 64 + lane;
		const bool have = s < n;
		f3 pos = mk3(0, 0, 0), wpos = mk3(0, 0, 0);
		if (have) { // generate_grid_samples_nerf_uniform(_dir), tn:406-431
			const uint32_t x = s % a.res[0], y = (s / a.res[0]) % a.res[1], z = s / (a.res[0] * a.res[1]);
			pos = mk3((float)x * (1.f / (float)a.res[0]), (float)y * (1.f / (float)a.res[1]), (float)z * (1.f / (float)a.res[2]));
			pos = mk3(pos.x * (a.box_mx[0] - a.box_mn[0]) + a.box_mn[0], pos.y * (a.box_mx[1] - a.box_mn[1]) + a.box_mn[1],
			          pos.z * (a.box_mx[2] - a.box_mn[2]) + a.box_mn[2]);
			wpos = warp_position(pos, m.aabb);
		}
		encode_num<NUM>(nm, gv, m.levels, sm.ml, fl, lane, g, wpos, have);
		half8 sh;
		if (MODE == 1) sh = encode_sh4(g, wdir);
		uint32_t res_d = 0, res_rg = 0, res_b = 0;
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			const half8 dout = density_mlp_num<NUM>(nm, sm.ml.w, lane, x0, x1);
			half8 rout = dout;
			if (MODE == 1) rout = rgb_mlp_num<NUM, true, true>(nm, sm.ml.w, lane, dout, sh, m.rgb_deep ? reinterpret_cast<const half8*>(m.wfrag) : nullptr,
			                                                  m.n_extra_dims ? reinterpret_cast<const half8*>(m.wfrag) : nullptr, light_operand(g, m.light01[0], m.light01[1], m.light01[2]));
			const u32x4 dd = __builtin_bit_cast(u32x4, dout), rr = __builtin_bit_cast(u32x4, rout);
			uint32_t vd = dd[0], vrg = rr[0], vb = rr[1]; // rows 0..2 of a block sit in lanes 0..31
			if (b == 1) { vd = xchg32u(vd); vrg = xchg32u(vrg); vb = xchg32u(vb); }
			if (g == b) { res_d = vd; res_rg = vrg; res_b = vb; }
		}
		if (!have) continue;
		const float sigma_raw = (float)__builtin_bit_cast(half2v, res_d)[0];
		if (MODE == 0) {
			float v = sigma_raw;
			if (a.density_grid) {
				const f3 upos = unwarp_position(wpos, m.aabb);
				const uint32_t mip = (uint32_t)mip_from_pos(upos);
				if (a.density_grid[cascaded_grid_idx_at(upos, mip) + mip * kGridVol] < 0.01f) v = -10000.f; // NERF_MIN_OPTICAL_THICKNESS
			}
			a.out[s] = v;
		} else {
			const half2v hrg = __builtin_bit_cast(half2v, res_rg), hb = __builtin_bit_cast(half2v, res_b);
			const float alpha = clampf_(1.f - __expf(-network_to_density(sigma_raw, m.density_activation) / 100.0f), 0.0f, 1.0f);
			reinterpret_cast<float4*>(a.out)[s] = make_float4(network_to_rgb((float)hrg[0], m.rgb_activation) * alpha, network_to_rgb((float)hrg[1], m.rgb_activation) * alpha,
			                                                   network_to_rgb((float)hb[0], m.rgb_activation) * alpha, alpha);
		}
	}
	(void)j;
}

int launch_grid_eval(const DeviceModel& m, int mode, const uint32_t res[3], const float box_mn[3], const float box_mx[3], const float dir01[3],
                     const float* d_density_grid, float* d_out, int n_cus, void* stream) {
	GridEvalArgs a{};
	for (int k = 0; k < 3; ++k) { a.res[k] = res[k]; a.box_mn[k] = box_mn[k]; a.box_mx[k] = box_mx[k]; a.dir01[k] = dir01 ? dir01[k] : 0.5f; }
	a.density_grid = d_density_grid;
	a.out = d_out;
	const uint32_t n = res[0] * res[1] * res[2];
	if (n == 0) return NRS_OK;
	const uint32_t n_tiles = (n + 63) / 64;
	uint32_t grid = (n_tiles + 3) / 4; // 256-thread workgroups: 4 waves, a tile each per trip
	const uint32_t cap = (uint32_t)n_cus * 8; // resident workgroups: the tiles are strided over them
	if (grid > cap) grid = cap;
	constexpr int R = kNumRuntime;
	if (mode == 0) { if (m.numerics) hipLaunchKernelGGL((grid_eval_kernel<0, R>), dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a); else hipLaunchKernelGGL((grid_eval_kernel<0, 0>), dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a); }
	else { if (m.numerics) hipLaunchKernelGGL((grid_eval_kernel<1, R>), dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a); else hipLaunchKernelGGL((grid_eval_kernel<1, 0>), dim3(grid), dim3(256), 0, (hipStream_t)stream, m, a); }
	NRS_LAUNCH_CHECK("grid_eval_kernel launch");
	return NRS_OK;
}

// ---- EditOperator::map_rays / map_positions on caller batches --------------------------------------------------------------
__global__ void map_rays_kernel(const DeviceEdit e, uint32_t n, float* __restrict__ coords, uint32_t ld, int with_dir, uint8_t* __restrict__ empty_mask) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float* c = coords + (size_t)i * ld;
	f3 wpos = mk3(c[0], c[1], c[2]);
	f3 wdir = with_dir ? mk3(c[4], c[5], c[6]) : mk3(0.5f, 0.5f, 0.5f);
	const f3 p0 = wpos, d0 = wdir;
	const bool empty = edit_warp(e, with_dir != 0, wpos, wdir);
	if (wpos.x != p0.x || wpos.y != p0.y || wpos.z != p0.z) { c[0] = wpos.x; c[1] = wpos.y; c[2] = wpos.z; }
	if (with_dir && (wdir.x != d0.x || wdir.y != d0.y || wdir.z != d0.z)) { c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z; }
	if (empty) empty_mask[i] = 1;
}

int launch_map_rays(const DeviceEdit& e, uint32_t n, float* d_coords, uint32_t ld, int with_dir, uint8_t* d_empty, void* stream) {
	if (n == 0) return NRS_OK;
	hipLaunchKernelGGL(map_rays_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e, n, d_coords, ld, with_dir, d_empty);
	NRS_LAUNCH_CHECK("map_rays_kernel launch");
	return NRS_OK;
}

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

// ---- multi-GPU de-tiling ---------------------------------------------------------------------------------------------------
__global__ void detile_kernel(int W, int H, uint32_t tile, uint32_t tiles_x, uint32_t n_ranks, size_t rank_stride, const float* __restrict__ tiles,
                              uint32_t channels, float* __restrict__ image) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (uint32_t)(W * H)) return;
	const uint32_t x = i % (uint32_t)W, y = i / (uint32_t)W;
	const uint32_t T = (y / tile) * tiles_x + (x / tile);
	const uint32_t r = T % n_ranks, k = T / n_ranks;
	const size_t src = (size_t)r * rank_stride + ((((size_t)k * tile + (y % tile)) * tile + (x % tile))) * channels;
	for (uint32_t c = 0; c < channels; ++c) image[(size_t)i * channels + c] = tiles[src + c];
}

int launch_detile(const nrs_render_params& p, uint32_t n_ranks, size_t rank_stride_floats, const float* d_tiles, uint32_t channels,
                  float* d_image, void* stream) {
	const int W = p.resolution[0], H = p.resolution[1];
	const uint32_t tiles_x = tile_pitch((uint32_t)W, p.tile_size);
	const uint32_t n = (uint32_t)(W * H);
	hipLaunchKernelGGL(detile_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, W, H, p.tile_size, tiles_x, n_ranks, rank_stride_floats,
	                   d_tiles, channels, d_image);
	NRS_LAUNCH_CHECK("detile_kernel launch");
	return NRS_OK;
}

#endif // NRS_BODY_ONLY
} // namespace nrs
