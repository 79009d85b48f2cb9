// nrs_api_render.cpp -- the render call: tile geometry, argument checks, the operator table, the route request, the launch on its slot, statistics; the route probes.
#include "nrs_host.h"
#include "nrs_route.h"
#include "nrs_render.h"

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace nrs;

extern "C" {

// ---- renderer --------------------------------------------------------------------------------------------------------
static int tile_geometry(const nrs_render_params& p, uint32_t team, uint32_t& tiles_x, uint32_t& owned, uint32_t& n_packets, uint32_t& ppt_x) {
	const uint32_t W = (uint32_t)p.resolution[0], H = (uint32_t)p.resolution[1];
	const uint32_t pw = team >= 16 ? 2u : (team >= 4 ? 4u : 8u), ph = 64u / team / pw; // packet_pixel<TEAM>()
	if (p.tile_size == 0) {
		tiles_x = (W + pw - 1) / pw; // packets per image row
		owned = 1;
		ppt_x = 0;
		n_packets = tiles_x * ((H + ph - 1) / ph);
		return NRS_OK;
	}
	if (p.tile_size % 8) return fail(NRS_ERR_INVALID_ARG, "tile_size must be a multiple of 8");
	tiles_x = tile_pitch(W, p.tile_size); // (odd row pitch: indices beyond the image's last tile column are virtual)
	const uint32_t tiles_y = (H + p.tile_size - 1) / p.tile_size, total = tiles_x * tiles_y;
	const uint32_t stride = p.tile_stride ? p.tile_stride : 1;
	owned = p.tile_first < total ? (total - p.tile_first + stride - 1) / stride : 0;
	ppt_x = p.tile_size / pw;
	n_packets = owned * ppt_x * (p.tile_size / ph);
	return NRS_OK;
}
uint32_t nrs_render_tile_pitch(const nrs_render_params* p) {
	if (!p || p->struct_size != (uint32_t)sizeof(nrs_render_params) || p->resolution[0] <= 0 || p->tile_size == 0) return 0;
	return tile_pitch((uint32_t)p->resolution[0], p->tile_size);
}
uint32_t nrs_render_owned_tiles(const nrs_render_params* p) {
	if (!p || p->struct_size != (uint32_t)sizeof(nrs_render_params) || p->resolution[0] <= 0 || p->resolution[1] <= 0) return 0;
	uint32_t tx, owned, np, ppt;
	if (tile_geometry(*p, 1, tx, owned, np, ppt) != NRS_OK) return 0;
	return owned;
}

// ---- nrs_render_nerf and nrs_render_nerf_spp: spp_count samples of the view into slabs slab_stride pixels apart (a single frame: 1, 0) -----------------
// the aperture of a view: the params' own, or each record of a views batch
static int check_lens(float dof, float slice_plane_z, const std::string& who) {
	if (dof != 0.f && slice_plane_z == 0.f) return fail(NRS_ERR_INVALID_ARG, who + ": dof != 0 needs a focus distance (slice_plane_z = m_slice_plane_z + m_scale != 0)");
	return NRS_OK;
}
static int check_render_args(const nrs_model* m, const nrs_render_params* p, nrs_edit* const* edits, int n_edits, uint32_t spp_count, const float* d_frame,
                             const float* d_depth, size_t slab_stride) {
	if (!m || !p || !d_frame || !d_depth) return fail(NRS_ERR_INVALID_ARG, spp_count > 1u ? "nrs_render_nerf_spp: NULL argument (model, params, d_frames, d_depths)" : "nrs_render_nerf: NULL argument");
	if (!m->have_params) return fail(NRS_ERR_STATE, "nrs_render_nerf: parameters not set (nrs_model_set_params)");
	if (!m->have_bitfield) return fail(NRS_ERR_STATE, "nrs_render_nerf: occupancy not set (nrs_model_set_density_bitfield/_grid)");
	NRS_TRY(check_march_params(*p, "nrs_render_nerf"));
	if (p->render_mode == NRS_RENDER_ENCODING_VIS && p->visualized_dimension >= network_layer_width(m->desc, p->visualized_layer, m->n_extra_dims))
		return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: EncodingVis: visualized_layer is hash grid 32 | density hidden 64 | rgb input 32 | one of 64 per rgb hidden layer (base.json: 0..4) and visualized_dimension a unit of it");
	if (!std::isfinite(p->glow_y_cutoff) || p->glow_mode > 31u) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: glow_mode is a 5-bit mask and glow_y_cutoff must be finite");
	if (p->distortion_mode > 2u) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: distortion_mode must be 0 (None), 1 (Iterative) or 2 (FTheta)");
	for (int i = 0; i < 7; ++i)
		if (!std::isfinite(p->distortion_params[i])) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: distortion parameters must be finite");
	if (p->d_envmap && (p->envmap_resolution[0] < 1 || p->envmap_resolution[1] < 1)) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: envmap without a resolution");
	if (p->d_distortion_map && (p->distortion_resolution[0] < 1 || p->distortion_resolution[1] < 1)) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: distortion map without a resolution");
	if (p->render_mode > NRS_RENDER_SLICE && p->render_mode != NRS_RENDER_ENCODING_VIS) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: unknown render mode");
	if (!std::isfinite(p->dof) || !std::isfinite(p->slice_plane_z) || !std::isfinite(p->depth_scale)) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: dof / slice_plane_z / depth_scale must be finite");
	NRS_TRY(check_lens(p->dof, p->slice_plane_z, "nrs_render_nerf"));
	if (n_edits < 0 || n_edits > nrs_ctx::kMaxEdits) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: too many edit operators");
	if (n_edits > 0 && !edits) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: edits is NULL");
	if (spp_count > 1u) { // what only a batch can get wrong; everything above is the single frame's check
		if (p->render_mode == NRS_RENDER_SLICE)
			return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: render_mode Slice with spp_count > 1: a slice has no persistent launch to share -- call nrs_render_nerf per sample");
		if (p->resolution[0] > NRS_SPP_BATCH_MAX_RESOLUTION || p->resolution[1] > NRS_SPP_BATCH_MAX_RESOLUTION)
			return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: resolution above NRS_SPP_BATCH_MAX_RESOLUTION (8192) in one axis with spp_count > 1");
	}
	if (spp_count > 1u) {
		uint32_t tx = 0, owned = 0, np = 0, ppt = 0;
		NRS_TRY(tile_geometry(*p, 1, tx, owned, np, ppt));
		const uint64_t own_pixels = p->tile_size ? (uint64_t)owned * p->tile_size * p->tile_size : (uint64_t)p->resolution[0] * (uint64_t)p->resolution[1];
		if ((uint64_t)slab_stride < own_pixels)
			return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: slab_stride_pixels is smaller than the pixels one call owns (W * H, or owned tiles * tile_size^2)");
		if ((uint64_t)slab_stride * spp_count >= (1ull << 32))
			return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: spp_count * slab_stride_pixels does not fit the 32-bit pixel index");
		// (16-pixel packets are the smallest any schedule cuts: 4 per 8x8 block; the queue's state word keeps bit 31 for "dry" and workgroups overshoot the counter by a chunk each)
		if ((uint64_t)np * 4ull * spp_count > (1ull << 30) || (uint64_t)np * 64ull * spp_count > (1ull << 30))
			return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: spp_count times the packets / pixels of one sample overflows the 32-bit packet counter (limit 2^30)");
	}
	return NRS_OK;
}

// The development knobs of a render call, read once (dev_knob: a production process ignores them).
struct RenderKnobs {
	RouteKnobs route;
	uint32_t dbg;      // RenderArgs::dbg: NRS_DEBUG | NRS_SKIP_PAIRS << 8 (bit it: level pair (2 it, 2 it + 1) is not gathered -- nrs_hashgrid.cuh: KIND_SKIP; measurement only)
	uint32_t reteam;   // NRS_RETEAM bit 0: at the end of a wave's work, bit 1: whenever a tail generation has thinned out
	uint32_t steal;    // NRS_STEAL
	bool log_teams;    // NRS_TEAM_LOG
};
static const RenderKnobs& render_knobs() {
	static const RenderKnobs knobs = []() {
		RenderKnobs k{};
		auto num = [](const char* name, int unset) { const char* e = dev_knob(name); return e ? atoi(e) : unset; };
		const char* sk = dev_knob("NRS_SKIP_PAIRS");
		k.dbg = ((uint32_t)num("NRS_DEBUG", 0) & 0xffu) | (sk ? ((uint32_t)strtoul(sk, nullptr, 0) & 0xffu) << 8 : 0u);
		k.reteam = (uint32_t)num("NRS_RETEAM", 3);
		k.steal = (uint32_t)num("NRS_STEAL", 1);
		k.log_teams = dev_knob("NRS_TEAM_LOG") != nullptr;
		k.route.team = num("NRS_TEAM", 0);
		k.route.hybrid_on = num("NRS_HYBRID", 1) != 0;
		k.route.render_cfg = num("NRS_RENDER_CFG", 0);
		k.route.render_cfg_set = dev_knob("NRS_RENDER_CFG") != nullptr;
		k.route.debug = k.dbg & 0xffu;
		k.route.l2_gate = num("NRS_L2_GATE", 1) != 0;
		// (<= kRing - 64: the fill adds up to 64 rays per packet to a 128-entry ring) 8 / 16 / 24 / 32 / 48: 8.92 / 8.91 / 9.11 / 9.01 / 8.47 Gsamples/s
		k.route.tail_target = num("NRS_TAIL_TARGET", 0) >= 1 ? (uint32_t)std::min(num("NRS_TAIL_TARGET", 0), 64) : 24u;
		k.route.alltail_target = num("NRS_ALLTAIL_TARGET", 0) >= 1 ? (uint32_t)std::min(num("NRS_ALLTAIL_TARGET", 0), 64) : 16u; // (<= kRing - 64, as above)
		k.route.tail_every = num("NRS_TAIL_EVERY", 0) >= 2 ? (uint32_t)num("NRS_TAIL_EVERY", 0) : 3u;
		const int tf = num("NRS_TAIL_FILL", 0);
		k.route.tail_fill = (tf == 1 || tf == 2 || tf == 4) ? (uint32_t)tf : 4u;
		return k;
	}();
	return knobs;
}

// The operator table of a launch: the operators' device structs and what the route needs to know of them.  The cage that has come to rest gets its fine
// look-up table here (nrs_edit::fine_stale).
struct EditTable { DeviceEdit host[nrs_ctx::kMaxEdits]; int n; uint32_t any_poisson, any_affine; };
static int collect_edits(nrs_edit* const* edits, int n_edits, hipStream_t s, EditTable& t) {
	t.n = n_edits;
	t.any_poisson = t.any_affine = 0u;
	for (int i = 0; i < n_edits; ++i) {
		if (!edits[i]) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf: NULL edit operator");
		if (edits[i]->fine_stale && ++edits[i]->renders_since_move >= 2u) {
			edits[i]->fine_stale = false;
			NRS_TRY(build_fine_lut(edits[i], s));
		}
		t.host[i] = edits[i]->de;
		t.any_poisson |= edits[i]->de.apply_poisson;
		t.any_affine |= (edits[i]->de.kind == kEditAffine) ? 1u : 0u;
	}
	return NRS_OK;
}

// what plan_route is asked: the model, the operators, the parameters, and the context's state (slot: this launch's, not counted as busy)
static RouteRequest route_request(const nrs_model* m, const nrs_render_params& p, const EditTable& t, uint32_t spp_count, const nrs_sample_view* h_views, uint32_t pixels_owned, uint32_t slot, hipStream_t s) {
	const nrs_ctx* ctx = m->ctx;
	RouteRequest q{};
	q.n_extra_dims = m->n_extra_dims; q.rgb_deep = m->dm.rgb_deep; q.numerics = m->dm.numerics;
	const LevelParams* lv = m->dm.levels;
	for (int it = 7; it >= 0 && lv[2 * it].hashed && lv[2 * it + 1].hashed && !lv[2 * it].cached && !lv[2 * it + 1].cached; --it) ++q.hashed_pairs;
	q.any_poisson = t.any_poisson; q.any_affine = t.any_affine; q.apply_operators = p.apply_operators;
	q.render_mode = p.render_mode; q.show_accel = p.show_accel; q.dof_on = p.dof != 0.f; q.distortion_mode = p.distortion_mode; q.distortion_map = p.d_distortion_map != nullptr;
	q.envmap = p.d_envmap != nullptr; q.glow_mode = p.glow_mode;
	q.cone_angle_constant = p.cone_angle_constant;
	q.tile_size = p.tile_size; q.height = (uint32_t)p.resolution[1]; q.spp_count = (uint16_t)spp_count;
	if (h_views) { // a view per sample: the aperture of ANY of them asks for the thin-lens branch
		q.views = 1;
		q.dof_on = 0u;
		for (uint32_t k = 0; k < spp_count; ++k) q.dof_on |= h_views[k].dof != 0.f ? 1u : 0u;
	}
	q.lane_teams = ctx->lane_teams; q.n_cus = ctx->n_cus; q.pixels_owned = pixels_owned;
	const unsigned long long fb = ctx->h_feedback ? __atomic_load_n(ctx->h_feedback, __ATOMIC_RELAXED) : 0ull;
	q.hit_share = (fb >> 32) ? (double)(uint32_t)fb / (double)(fb >> 32) : 0.25;
	// busy = number of OTHER streams with an unfinished launch (launches queued behind one another on a stream do not overlap); a slice has no schedule to choose
	hipStream_t seen[nrs_ctx::kInFlight];
	for (int k = 0; k < nrs_ctx::kInFlight && p.render_mode != NRS_RENDER_SLICE; ++k) {
		if ((uint32_t)k == slot || !ctx->slot_used[k] || ctx->slot_stream[k] == s) continue;
		bool dup = false;
		for (uint32_t i = 0; i < q.busy; ++i) dup = dup || seen[i] == ctx->slot_stream[k];
		if (!dup && hipEventQuery(ctx->slot_done[k]) == hipErrorNotReady) seen[q.busy++] = ctx->slot_stream[k];
	}
	(void)hipGetLastError(); // hipErrorNotReady is an answer, not an error
	q.knobs = render_knobs().route;
	return q;
}

// Enqueues one launch on its slot of the context's rings: `launch` is the render kernel of plan->row, or the slice kernel (plan == nullptr).  -> the launch's statistics block.
// A slot is reused every kInFlight launches, possibly from another stream: the stream waits for the slot's last launch first.
// The statistics / queue block of a launch: a slot owns two, and the render kernel's last workgroup zeroes the one it did NOT use, which the slot's next
// launch takes (launches of a slot are ordered: same stream, or the event wait) -- so a frame costs no memset (two 5-us fill kernels per frame in
// the round-3 timeline: 2 % of a 1/8 share-frame).  The Slice path and a launch after a failed one still clear their block the plain way.
static int enqueue(nrs_model* m, const nrs_render_params& p, hipStream_t s, uint32_t slot, const EditTable& t, const nrs_sample_view* h_views, RenderArgs& a, const RoutePlan* plan, RenderCounters** d_counters) {
	nrs_ctx* ctx = m->ctx;
	if (ctx->slot_used[slot] && ctx->slot_stream[slot] != s) HIP_TRY(hipStreamWaitEvent(s, ctx->slot_done[slot], 0));
	// the operator table of a slot is re-sent only when it changed (a viewer renders many frames per gizmo move)
	DeviceEdit* d_edits_slot = ctx->d_edits.get() + (size_t)slot * nrs_ctx::kMaxEdits;
	DeviceEdit* shadow = ctx->edits_shadow.data() + (size_t)slot * nrs_ctx::kMaxEdits;
	if (t.n > 0 && (ctx->shadow_n[slot] != t.n || memcmp(shadow, t.host, sizeof(DeviceEdit) * t.n) != 0)) {
		HIP_TRY(hipMemcpyAsync(d_edits_slot, t.host, sizeof(DeviceEdit) * t.n, hipMemcpyHostToDevice, s));
		memcpy(shadow, t.host, sizeof(DeviceEdit) * t.n);
		ctx->shadow_n[slot] = t.n;
	}
	a.edits = d_edits_slot;
	// the view table of a views batch: into the slot's own records, ordered on the stream like the launch that reads them.  The records travel as kernel arguments
	// (launch_views_upload), which the runtime copies before the call returns: the caller's array is free on return and no pinned staging area is shared between launches.
	a.views = nullptr;
	if (h_views && plan && a.n_packets != 0) {
		nrs_sample_view* d_views_slot = ctx->d_views.get() + (size_t)slot * NRS_SPP_BATCH_MAX;
		NRS_LAUNCH(launch_views_upload(h_views, a.spp_count, d_views_slot, s));
		a.views = d_views_slot;
	}
	a.counters = *d_counters = ctx->d_counters.get() + 2 * slot + ctx->counter_parity[slot];
	const bool clean = plan && ctx->counters_clean[slot];
	ctx->counters_clean[slot] = false; // (until a render launch is known to be enqueued: its last workgroup cleans the other block; slice_kernel cleans nothing)
	if (!clean) HIP_TRY(hipMemsetAsync(a.counters, 0, sizeof(RenderCounters), s));
	if (!plan) { // tn:3109-3162: no marching at all; one network evaluation per owned pixel
		NRS_LAUNCH(launch_slice(m->dm, a, ctx->n_cus, s));
	} else {
		a.counters_next = ctx->d_counters.get() + 2 * slot + (ctx->counter_parity[slot] ^ 1u);
		a.wave_log = (a.dbg & 4u) ? ctx->d_wave_log.get() : nullptr;
		if (a.wave_log) HIP_TRY(hipMemsetAsync(ctx->d_wave_log.get(), 0, 8192 * 4 * 8, s));
		if (a.n_packets != 0) { // (else nothing to launch, no owned tiles: the block stays as it is -- zero)
			const unsigned long long dispatches0 = launch_render_dispatches();
			NRS_LAUNCH(launch_render((RouteId)plan->row, model_for_launch(m, p), a, ctx->n_cus, s));
			ctx->render_dispatches += launch_render_dispatches() - dispatches0;
			ctx->last_schedule = a.team | (a.fill_lanes << 8) | (a.all_tail << 16) | ((a.p_big ? 1u : 0u) << 17) | ((a.spp_count > 1u ? 1u : 0u) << 18) | ((a.views ? 1u : 0u) << 19);
			ctx->counter_parity[slot] ^= 1u;
		}
		ctx->counters_clean[slot] = true;
	}
	HIP_TRY(hipEventRecord(ctx->slot_done[slot], s));
	ctx->slot_stream[slot] = s;
	ctx->slot_used[slot] = true;
	return NRS_OK;
}

// the NRS_DEBUG bit-2 print-out of a launch: phase shares, walk statistics and the per-wave log
static int report_wave_log(nrs_ctx* ctx, const RenderCounters& c) {
	static const char* names[8] = {"fill", "refill", "setup+warp", "gather", "sh+mlp", "composite+march+shade", "-", "exit"};
	unsigned long long tot = 0;
	for (int i = 0; i < 8; ++i) if (i != 6) tot += c.phase_cycles[i];
	fprintf(stderr, "[nrs phases] samples=%llu", (unsigned long long)c.n_samples);
	for (int i = 0; i < 8; ++i)
		if (c.phase_cycles[i] && i != 6) fprintf(stderr, " %s=%.1f%%", names[i], 100.0 * (double)c.phase_cycles[i] / (double)tot);
	fprintf(stderr, " | mean wave lifetime = %.1f%% of the longest (%.2f Mcycles)", 100.0 * ((double)tot / 4096.0) / (double)c.phase_cycles[6], (double)c.phase_cycles[6] / 1e6);
	fprintf(stderr, "\n");
	fprintf(stderr, "[nrs walk] fill: %llu lane iterations in %llu wave trips (%.1f lanes busy per trip); march: %llu lane iterations in %llu wave trips "
	        "(%.1f lanes/trip), %llu of %llu rounds needed > 1 trip; live lanes per round %.1f\n",
	        c.walk[0], c.walk[1], c.walk[1] ? (double)c.walk[0] / (double)c.walk[1] : 0.0, c.walk[2], c.walk[3],
	        c.walk[3] ? (double)c.walk[2] / (double)c.walk[3] : 0.0, c.walk[6], c.walk[4], c.walk[4] ? (double)c.walk[5] / (double)c.walk[4] : 0.0);
	if (c.walk[8])
		fprintf(stderr, "[nrs cage scan] %llu samples inside a deformed box (%.1f %% of the samples), %llu of them found a tet; rounds with such a sample: %llu of %llu (%.1f %%); "
		        "candidates tested %llu (%.2f per sample in the box), scan wave trips %llu (%.2f per round that scans)\n",
		        c.walk[8], 100.0 * (double)c.walk[8] / (double)std::max<unsigned long long>(c.n_samples, 1), c.walk[12], c.walk[9], c.walk[4], 100.0 * (double)c.walk[9] / (double)std::max<unsigned long long>(c.walk[4], 1),
		        c.walk[10], (double)c.walk[10] / (double)c.walk[8], c.walk[11], (double)c.walk[11] / (double)std::max<unsigned long long>(c.walk[9], 1));
	// per-wave log: when did each wave finish (wall clock), when did it first find the frame's queue empty
	std::vector<unsigned long long> wl(8192 * 4);
	HIP_TRY(hipMemcpy(wl.data(), ctx->d_wave_log.get(), wl.size() * 8, hipMemcpyDeviceToHost));
	if (const char* dump = dev_knob("NRS_WAVE_LOG_FILE")) { // raw log of the LAST launch with statistics, for tools/wave_log_report.py
		if (FILE* f = fopen(dump, "wb")) { fwrite(wl.data(), 8, wl.size(), f); fclose(f); }
	}
	std::vector<std::array<unsigned long long, 4>> rec; // {end tick (10 ns), rounds | rounds before queue-empty << 16 | t_queue_empty << 32, packets, xcc}
	unsigned long long t0min = ~0ull;
	for (size_t i = 0; i < 8192; ++i) if (wl[4 * i]) t0min = std::min(t0min, wl[4 * i + 3] >> 32);
	for (size_t i = 0; i < 8192; ++i)
		if (wl[4 * i]) {
			const unsigned long long wall = wl[4 * i + 3] & 0xffffffffull, start = (wl[4 * i + 3] >> 32) - t0min;
			const unsigned long long rq = (wl[4 * i + 1] >> 16) & 0xffff, tq = (wl[4 * i + 1] >> 32) + start;
			rec.push_back({wall + start, (wl[4 * i + 1] & 0xffffull) | (rq << 16) | (tq << 32), wl[4 * i + 2] & 0xffffull, wl[4 * i + 2] >> 56});
		}
	std::sort(rec.begin(), rec.end());
	if (!rec.empty()) {
		auto pr = [&](const char* tag, size_t i) {
			fprintf(stderr, "   %s: end=%.1f us, queue found empty at %.1f us, rounds=%llu (%llu after that), packets=%llu, xcc=%llu\n", tag, rec[i][0] / 100.0,
			        (rec[i][1] >> 32) / 100.0, rec[i][1] & 0xffff, (rec[i][1] & 0xffff) - ((rec[i][1] >> 16) & 0xffff), rec[i][2], rec[i][3]);
		};
		double mean = 0;
		for (auto& r : rec) mean += (double)r[0];
		mean /= rec.size();
		fprintf(stderr, "[nrs waves] n=%zu, mean end = %.1f%% of the last end\n", rec.size(), 100.0 * mean / (double)rec.back()[0]);
		pr("min", 0); pr("p25", rec.size() / 4); pr("p50", rec.size() / 2); pr("p75", rec.size() * 3 / 4); pr("p95", rec.size() * 95 / 100);
		pr("p99", rec.size() * 99 / 100); pr("max", rec.size() - 1);
	}
	return NRS_OK;
}

// the statistics of the launch on stream s (synchronises it); march: the launch ran a render kernel (hand-over counts, the wave log)
static int read_stats(nrs_ctx* ctx, hipStream_t s, const RenderCounters* d_counters, bool march, uint32_t dbg, nrs_render_stats* h_stats) {
	RenderCounters c;
	HIP_TRY(hipMemcpyAsync(&c, d_counters, sizeof(c), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	h_stats->n_samples = c.n_samples;
	h_stats->n_rays_alive = c.n_rays_alive;
	h_stats->n_rays_hit = c.n_rays_hit;
	if (!march) return NRS_OK;
	ctx->last_handover = c.walk[7];
	if (dbg & 12u) fprintf(stderr, "[nrs hand-over] %llu rays in %llu hand-overs\n", c.walk[7] & 0xffffffffull, c.walk[7] >> 32);
	return (dbg & 4u) ? report_wave_log(ctx, c) : NRS_OK;
}

// h_views: spp_count > 1 records, validated by the caller (nrs_render_nerf_spp_views), or NULL: every sample renders the params' own view
static int render_samples(nrs_model* m, const nrs_render_params* p, nrs_edit* const* edits, int n_edits, uint32_t spp_count, float* d_frame, float* d_depth,
                          uint32_t* d_steps, size_t slab_stride, void* stream, nrs_render_stats* h_stats, const nrs_sample_view* h_views = nullptr) {
	NRS_TRY(check_render_args(m, p, edits, n_edits, spp_count, d_frame, d_depth, slab_stride));
	nrs_ctx* ctx = m->ctx;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = (hipStream_t)stream;
	const RenderKnobs& knobs = render_knobs();
	const bool slice = p->render_mode == NRS_RENDER_SLICE;
	std::unique_lock<std::mutex> launch_lock(ctx->launch_mutex); // held until the launch is enqueued and the slot's book-keeping is written (released before the statistics' sync)
	const uint32_t slot = ctx->launch_serial.fetch_add(1u) % (uint32_t)nrs_ctx::kInFlight;

	RenderArgs a{};
	a.p = *p;
	if (p->render_mode == NRS_RENDER_ENCODING_VIS) a.p.visualized_layer = kernel_layer(m->desc, p->visualized_layer); // (the kernels number base.json's layers)
	uint32_t owned_tiles = 0;
	NRS_TRY(tile_geometry(*p, 1, a.tiles_x, owned_tiles, a.n_packets, a.packets_per_tile_x)); // (8x8 packets: the launch's pixels)
	const uint32_t pixels_owned = (uint32_t)std::min<uint64_t>((uint64_t)a.n_packets * 64ull * spp_count, 0xffffffffull); // (a batch: the rays of all its samples decide the schedule)
	EditTable table;
	NRS_TRY(collect_edits(edits, n_edits, s, table));
	const RouteRequest request = route_request(m, *p, table, spp_count, h_views, pixels_owned, slot, s);
	const RoutePlan plan = plan_route(request);
	if (plan.status != NRS_OK) return fail(plan.status, plan.message);
	a.n_edits = n_edits;
	a.any_poisson = plan.any_poisson;
	a.any_affine = table.any_affine;
	a.dbg = knobs.dbg;
	a.extra = plan.extra;
	a.gate = plan.gate;
	a.team = 1;
	a.fill_lanes = 4;
	a.frame = d_frame;
	a.depth = d_depth;
	a.steps = d_steps;
	if (!slice) { // (a slice marches nothing: no schedule, no queue)
		if (knobs.log_teams) fprintf(stderr, "[nrs team] pixels=%u hit_share=%.3f busy=%u rays/lane=%.3f small-launch=%d fill lanes=%u forced=%d\n", pixels_owned, request.hit_share, request.busy, plan.rays_per_lane, 1, plan.fill_lanes_auto, plan.forced);
		a.pixels_owned = pixels_owned;
		a.team = plan.team;
		a.all_tail = plan.all_tail;
		a.fill_lanes = plan.fill_lanes;
		a.tail_every = plan.tail_every;
		a.tail_target = plan.tail_target;
		a.reteam = knobs.reteam;
		a.steal = ctx->handover >= 0 ? (uint32_t)ctx->handover : knobs.steal;
		// the packets of one sample, cut for the plan's lanes per pixel; hybrid: the tail rows leave the 8x8 list and follow it as tail packets
		if (plan.packet_lanes() != 1u) NRS_TRY(tile_geometry(*p, plan.packet_lanes(), a.tiles_x, owned_tiles, a.n_packets, a.packets_per_tile_x));
		if (plan.hybrid) {
			const uint32_t rows = ((uint32_t)p->resolution[1] + 7u) / 8u, tail_rows = rows / plan.tail_every;
			a.p_big = (rows - tail_rows) * a.tiles_x;
			a.n_packets = a.p_big + tail_rows * a.tiles_x * plan.fill_lanes;
		}
		// a batch does not report: the feedback word sizes the caller's next single-frame launch, whose pixels_owned this launch's is not
		a.feedback = spp_count > 1u ? nullptr : ctx->d_feedback;
		// the queue of a batch: spp_count times the packets of one sample (hybrid: all samples' 8x8 packets, then all samples' tail packets -- one tail, one drain)
		a.spp_count = spp_count;
		a.spp_packets = a.n_packets;
		a.spp_big = a.p_big;
		a.slab_stride = spp_count > 1u ? (uint32_t)slab_stride : 0u;
		a.n_packets *= spp_count;
		a.p_big *= spp_count;
		a.max_steps = p->max_march_steps ? p->max_march_steps : 10000u; // MARCH_ITER, testbed_nerf.cu:56
	}
	RenderCounters* d_counters = nullptr;
	NRS_TRY(enqueue(m, *p, s, slot, table, plan.views ? h_views : nullptr, a, slice ? nullptr : &plan, &d_counters));
	launch_lock.unlock();
	return h_stats ? read_stats(ctx, s, d_counters, !slice, a.dbg, h_stats) : NRS_OK;
}

int nrs_render_nerf(nrs_model* m, const nrs_render_params* p, nrs_edit* const* edits, int n_edits, float* d_frame, float* d_depth,
                    uint32_t* d_steps, void* stream, nrs_render_stats* h_stats) {
	return render_samples(m, p, edits, n_edits, 1u, d_frame, d_depth, d_steps, 0, stream, h_stats);
}
// what both batch entry points refuse before anything else
static int check_batch_args(uint32_t spp_count, const float* d_frames, const float* d_depths) {
	if (!d_frames || !d_depths) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: d_frames / d_depths is NULL");
	if (spp_count == 0u) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: spp_count is 0");
	if (spp_count > NRS_SPP_BATCH_MAX) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp: spp_count above NRS_SPP_BATCH_MAX (64)");
	return NRS_OK;
}
int nrs_render_nerf_spp(nrs_model* m, const nrs_render_params* p, nrs_edit* const* edits, int n_edits, uint32_t spp_count, float* d_frames, float* d_depths,
                        uint32_t* d_steps, size_t slab_stride_pixels, void* stream, nrs_render_stats* h_stats) {
	NRS_TRY(check_batch_args(spp_count, d_frames, d_depths));
	return render_samples(m, p, edits, n_edits, spp_count, d_frames, d_depths, d_steps, slab_stride_pixels, stream, h_stats);
}
int nrs_render_nerf_spp_views(nrs_model* m, const nrs_render_params* p, nrs_edit* const* edits, int n_edits, uint32_t spp_count, const nrs_sample_view* h_views,
                              float* d_frames, float* d_depths, uint32_t* d_steps, size_t slab_stride_pixels, void* stream, nrs_render_stats* h_stats) {
	if (!h_views) return nrs_render_nerf_spp(m, p, edits, n_edits, spp_count, d_frames, d_depths, d_steps, slab_stride_pixels, stream, h_stats);
	NRS_TRY(check_batch_args(spp_count, d_frames, d_depths));
	if (!p) return fail(NRS_ERR_INVALID_ARG, "nrs_render_nerf_spp_views: params is NULL");
	NRS_TRY(check_params_abi(p, "nrs_render_nerf_spp_views"));
	for (uint32_t k = 0; k < spp_count; ++k) {
		const nrs_sample_view& v = h_views[k];
		const std::string who = "nrs_render_nerf_spp_views: h_views[" + std::to_string(k) + "]";
		for (int i = 0; i < 12; ++i) {
			if (!std::isfinite(v.camera_matrix0[i])) return fail(NRS_ERR_INVALID_ARG, who + ".camera_matrix0 is not finite");
			if (!std::isfinite(v.camera_matrix1[i])) return fail(NRS_ERR_INVALID_ARG, who + ".camera_matrix1 is not finite");
		}
		for (int i = 0; i < 2; ++i)
			if (!std::isfinite(v.focal_length[i]) || !(v.focal_length[i] > 0.f)) return fail(NRS_ERR_INVALID_ARG, who + ".focal_length must be finite and > 0");
		if (!std::isfinite(v.dof)) return fail(NRS_ERR_INVALID_ARG, who + ".dof is not finite");
		if (!std::isfinite(v.slice_plane_z)) return fail(NRS_ERR_INVALID_ARG, who + ".slice_plane_z is not finite");
		NRS_TRY(check_lens(v.dof, v.slice_plane_z, who));
	}
	// the params as the first sample sees them: what the shared checks look at, what a batch of one renders, and (Slice) what the refusal of a batch is decided on
	nrs_render_params q = *p;
	memcpy(q.camera_matrix0, h_views[0].camera_matrix0, sizeof(q.camera_matrix0));
	memcpy(q.camera_matrix1, h_views[0].camera_matrix1, sizeof(q.camera_matrix1));
	q.focal_length[0] = h_views[0].focal_length[0]; q.focal_length[1] = h_views[0].focal_length[1];
	q.dof = h_views[0].dof;
	q.slice_plane_z = h_views[0].slice_plane_z;
	return render_samples(m, &q, edits, n_edits, spp_count, d_frames, d_depths, d_steps, slab_stride_pixels, stream, h_stats, spp_count > 1u ? h_views : nullptr);
}
int nrs_route_probe(const RouteRequest* requests, uint32_t request_size, uint32_t n, RouteProbe* out, uint32_t probe_size) {
	if (!requests || !out || request_size != sizeof(RouteRequest) || probe_size != sizeof(RouteProbe)) return fail(NRS_ERR_INVALID_ARG, "nrs_route_probe: NULL argument, or the caller's structs are not this library's");
	for (uint32_t i = 0; i < n; ++i) {
		const RoutePlan plan = plan_route(requests[i]);
		RouteProbe& o = out[i];
		memset(&o, 0, sizeof(o));
		o.status = plan.status;
		o.row = plan.row;
		memcpy(o.message, plan.message, sizeof(o.message));
		if (plan.status != NRS_OK) continue;
		o.team = plan.team; o.all_tail = plan.all_tail; o.fill_lanes = plan.fill_lanes; o.tail_every = plan.tail_every; o.tail_target = plan.tail_target; o.hybrid = plan.hybrid;
		o.row_has_batch = kRoutes[plan.row].batch;
		route_name(o.name, sizeof(o.name), kRoutes[plan.row].t, requests[i].spp_count > 1u);
	}
	return NRS_OK;
}
int nrs_route_probe_views(const RouteRequest* requests, uint32_t request_size, uint32_t n, uint32_t* views_out) {
	if (!requests || !views_out || request_size != sizeof(RouteRequest)) return fail(NRS_ERR_INVALID_ARG, "nrs_route_probe_views: NULL argument, or the caller's struct is not this library's");
	for (uint32_t i = 0; i < n; ++i) {
		const RoutePlan plan = plan_route(requests[i]);
		views_out[i] = plan.status == NRS_OK ? plan.views : 0u;
	}
	return NRS_OK;
}

} // extern "C"
