// nrs_render.cuh -- the render kernel of the NeRFshop render path for gfx950 (MI355X), wave64: device code only.
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
// nrs_render_rows.hip instantiates it, one instantiation per row of kRoutes (nrs_route.h); slice_kernel (nrs_network.hip) shares the packet geometry
// (nrs_packets.cuh); tools/one_kernel.sh compiles ONE explicit instantiation from this header for register work.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_render.h"
#include "nrs_vec.cuh"
#include "nrs_grid_math.cuh"
#include "nrs_random.cuh"
#include "nrs_camera.cuh"
#include "nrs_march.cuh"
#include "nrs_edit_warp.cuh"
#include "nrs_shade.cuh"
#include "nrs_hashgrid.cuh"
#include "nrs_mlp.cuh"
#include "nrs_packets.cuh"

namespace nrs {

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
#ifndef NRS_ROLL_PROF
#define NRS_ROLL_PROF 0 // (measurement builds: the rolling gather in the wave log's PROF instantiations too, see render_body's kRoll)
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
//      RenderArgs::views (nrs_render_nerf_spp_views; a wave-uniform branch of the same twins -- VIEWS: all but the lean EXTRA row's, see route_carries_views): sample s has its own cameras, focal length and aperture, record s of a
//      device table.  The fill reads the packet's record (wave-uniform), the refill the record of each pending ray's sample, and the round re-reads the six floats of
//      camera_matrix1 that the depth of a sample is measured against (cam_fwd / cam_o) for the lane's sample -- which is out_idx / slab_stride (a slab is at least as long as
//      the pixels a call owns), so a ray carries no word more through re-teaming and the hand-over than it did.
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
	constexpr bool VIEWS = route_carries_views(POISSON, AFFINE, XTRA, BATCH); // (nrs_route.h: every BATCH twin but the lean EXTRA row's, which has XTRA 9 for it)
	// four levels per round trip in the gathers (encode_to_lds QUADS): the automatic schedule's instantiations with the default or the fully tiny-cuda-nn roundings -- since
	// round 6 the membrane instantiation too (both of its gathers: 9.68 -> 10.06 Gsamples/s, same registers; profiles/r06/ab_poisson_quads.txt)
	constexpr bool kQuads = TEAM == 0 && !EXTRA && NUM >= 0;
	// the rolling gather of the default level plan (encode_to_lds ROLL) on the rows that gather four levels per trip and hold it in the parent's registers: not the gated kernel
	// (it keeps the loop), not the membrane rows (scratch 40 -> 1120 bytes at 128 VGPRs, 147 -> 168 VGPRs + 960 bytes in the 12-wave build) and not the wave log's PROF twins
	// (scratch 208 -> 224 bytes; -DNRS_ROLL_PROF=1 builds them with it to measure the gather's share of the new path: profiles/gather_rolling.md)
	constexpr bool kRoll = kQuads && !kX.gate && !POISSON && (!PROF || NRS_ROLL_PROF);
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
				Ray r = BATCH ? init_ray<EXTRA, true>(p1, x, y, fo_x, fo_y, spp, (VIEWS && a1.views) ? a1.views + bs : nullptr) : init_ray<EXTRA>(p1, x, y, off_x, off_y);
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
					ray_origin_dir<EXTRA, true>(p1, x, y, eo_x, eo_y, o, d, espp, (VIEWS && a1.views) ? a1.views + es : nullptr);
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
			  for (int ei = a2.n_edits - 1; ei >= 0; --ei) e2 |= AFFINE ? edit_warp<!POISSON>(a2.edits[ei], true, wp2, wd2) : tet_warp<!POISSON && GATE == 0, GATE == 0>(a2.edits[ei], true, wp2, wd2);
			  asm volatile("" :: "v"(wp2.x), "v"(wp2.y), "v"(wp2.z), "v"(wd2.x), "v"(wd2.y), "v"(wd2.z), "s"((int)__ballot(e2))); }
#endif
			for (int ei = a2.n_edits - 1; ei >= 0; --ei) {
				if (AFFINE) {
					empty |= edit_warp<!POISSON>(a2.edits[ei], true, wpos, wdir); // (the membrane catch-all rows stand at their register limit like the membrane kernel)
				} else if (POISSON) {
					uint32_t scan; // (a local of the iteration, selected below: a pointer that is sometimes null made warp_scan a stack object)
					empty |= tet_warp<false>(a2.edits[ei], true, wpos, wdir, sm.coarse, &scan); // (the parent's map-back: no register to spare, nrs_edit_warp.cuh)
					if (ei == a2.n_edits - 1) warp_scan = scan;
				} else {
					empty |= tet_warp<GATE == 0, GATE == 0>(a2.edits[ei], true, wpos, wdir, sm.coarse, nullptr, PROF ? &pf_scan : nullptr); // (the gated kernel keeps the long chain: nrs_edit_warp.cuh find_tet)
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
		  encode_num<NUM, kQuads, true, 0, kRoll>(nm, gv, m2.levels, sm.ml, fl, lane, g, wp2, act); }
#endif
		encode_num<NUM, kQuads, false, GATE, kRoll>(nm, gv, m2.levels, sm.ml, fl, lane, g, wpos, act); // (four record levels in flight: the hybrid instantiation has the registers; features of idle lanes are never looked at: not zeroed)
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
			if (p2i.render_mode == NRS_RENDER_ENCODING_VIS) {
				// network.visualize_activation(stream, layer, dim, positions_matrix, positions_matrix): unit `dim` of forward_activations(layer)
				const uint32_t layer = p2i.visualized_layer, dim = p2i.visualized_dimension;
				// (the slab still holds this round's features; the frame's light direction for every sample)
				const f3 light = mk3(m2i.light01[0], m2i.light01[1], m2i.light01[2]);
				const float v = wave_visualize_activation<NUM, LIGHT>(nm, fl, sm.ml.w, lane, layer, dim, sh_own, sh_par, deep_w, light_w, lb, lb, light);
				intro_v = mk3(fmaxf(-v, 0.0f), fmaxf(v, 0.0f), 0.0f); // extract_dimension_pos_neg_kernel (tiny-cuda-nn), rows 0..2
				// The reference hands the network INPUT to visualize_activation as its output matrix (tn:2926): the sample's NerfCoordinate is overwritten --
				// position = the three values above, dt = 1, direction = (1, 1, 1) -- and composite_kernel_nerf reads them back as warped_pos (the colour,
				// tn:925; also the position of the depth test), dt (tn:762: every sample composites with the largest step) and the membrane colour's direction.
				wpos = intro_v;
				wdt = 1.0f;
				wdir = mk3(1.0f, 1.0f, 1.0f);
			} else if (p2i.render_mode == NRS_RENDER_NORMALS) {
				// network.input_gradient(stream, 3, positions, gradients): backward of 128 e_3 (see density_backward_features), then the grid's input gradient
				const GridView gvi = make_grid_view(m2i);
				intro_v = wave_density_input_gradient<NUM>(nm, fl, sm.ml.w, reinterpret_cast<const half8*>(m2i.wfrag), gvi, m2i.levels, lane, act ? wpos : mk3(0.f, 0.f, 0.f));
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
					const uint32_t old_d = wave_density<NUM>(nm, fl, sm.ml.w, lane);
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
		f3 cam_fwd = mk3(p3.camera_matrix1[6], p3.camera_matrix1[7], p3.camera_matrix1[8]);
		f3 cam_o = mk3(p3.camera_matrix1[9], p3.camera_matrix1[10], p3.camera_matrix1[11]);
		if (VIEWS && a3.views) { // the lane's sample has its own camera: re-read here, where it is used, not kept through the round (out_idx < spp_count * slab_stride)
			const NRS_GLOBAL float* c1 = (const NRS_GLOBAL float*)(a3.views + (have ? out_idx / a3.slab_stride : 0u)) + 12; // camera_matrix1
			cam_fwd = mk3(c1[6], c1[7], c1[8]);
			cam_o = mk3(c1[9], c1[10], c1[11]);
		}
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

} // namespace nrs
