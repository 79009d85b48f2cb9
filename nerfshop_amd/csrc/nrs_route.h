// nrs_route.h -- which render_kernel instantiation serves a frame, and with which schedule: the ONE place that knows.
//   kRoutes      one row per instantiation the library reaches (nrs_render_rows.hip instantiates the kernels and their launchers FROM this table, nrs_render.hip the table of launchers)
//   plan_route   a request (model, operators, parameters, context, development knobs) -> a refusal, or a row plus the schedule fields of RenderArgs
// Host-only, plain C++17, no HIP types, no getenv, no statics: the planner is a pure function (tests/test_route_plan_host.py sweeps it without a GPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nrs.h"

namespace nrs {

// ---- render_body's XTRA template argument (an int, so that every kernel symbol keeps its mangled name) ------------------------------------------------
constexpr int kXtraNone = 0;       // Shade / Cost with a pinhole camera: none of the below
constexpr int kXtraExtra = 1;      // EXTRA: per-sample render modes, show_accel, depth of field, distortion, envmap, glow
constexpr int kXtraIntro = 2;      // EXTRA + INTRO: render modes Normals and EncodingVis
constexpr int kXtraDeepExtra = 3;  // 1 for a network whose rgb MLP has a third hidden layer (base_3layer.json)
constexpr int kXtraDeepIntro = 4;  // 2 for such a network
constexpr int kXtraDeep = 5;       // that layer and nothing else of EXTRA: the automatic schedule's instantiation for such a network
constexpr int kXtraGate = 6;       // the plain kernel with the L2 phase gate on the four finest hashed levels (cone-stepping scenes)
constexpr int kXtraLight = 7;      // a network trained with light directions: the light term and nothing else (the twin of the default kernel)
constexpr int kXtraLightAll = 8;   // the catch-all of such a network: EXTRA + INTRO, the third hidden layer where the network has one (a run-time branch)
constexpr int kXtraExtraViews = 9; // 1 on the lean row (no POISSON, no AFFINE) with the view table of nrs_render_nerf_spp_views compiled in: that row's BATCH twin of 1 carries none
struct XtraTraits { bool extra, intro, deep, light, gate; };
constexpr XtraTraits xtra_traits(int xtra) {
	switch (xtra) {
	case kXtraExtra:     return {true, false, false, false, false};
	case kXtraIntro:     return {true, true, false, false, false};
	case kXtraDeepExtra: return {true, false, true, false, false};
	case kXtraDeepIntro: return {true, true, true, false, false};
	case kXtraDeep:      return {false, false, true, false, false};
	case kXtraGate:      return {false, false, false, false, true};
	case kXtraLight:     return {false, false, false, true, false};
	case kXtraLightAll:  return {true, true, true, true, false};
	case kXtraExtraViews: return {true, false, false, false, false};
	default:             return {false, false, false, false, false};
	}
}
// Does this instantiation read RenderArgs::views?  Every BATCH twin does, behind a wave-uniform branch, but the lean EXTRA row's (XTRA 1 without POISSON and AFFINE): the
// table's reads take it from 123 to 133 VGPRs, from 4 to 3 waves per SIMD, so its still batch keeps the twin it had and its views batch has one of its own (XTRA 9).
// The kernel (render_body) and the launch's last guard (check_route) both ask here.
constexpr bool route_carries_views(bool poisson, bool affine, int xtra, bool batch) { return batch && !(xtra == kXtraExtra && !poisson && !affine); }
constexpr bool same_traits(XtraTraits a, XtraTraits b) { return a.extra == b.extra && a.intro == b.intro && a.deep == b.deep && a.light == b.light && a.gate == b.gate; }
static_assert(same_traits(xtra_traits(kXtraExtraViews), xtra_traits(kXtraExtra)), "XTRA 9 is XTRA 1 with the view table: the same body otherwise");
static_assert(route_carries_views(false, false, kXtraExtraViews, true) && !route_carries_views(false, false, kXtraExtra, true), "of the two lean EXTRA twins, XTRA 9 reads the view table");
constexpr int kNumRuntime = -1; // NUM: tiny-cuda-nn's other roundings chosen at run time from DeviceModel::numerics (nrs_hashgrid.cuh encode_num)

// ---- one instantiation ----------------------------------------------------------------------------------------------------------------------------------
enum RouteEntry : int {
	kEntryC128 = 0, // render_kernel_c128<WAVES, ...>: scheduled for 3 waves per SIMD (OCC 3), held to 128 VGPRs
	kEntryCfg = 1,  // render_kernel<WAVES, OCC, ...>
};
struct RouteTraits { RouteEntry entry; int waves, occ; bool prof, poisson, affine; int team, num, xtra; };

// the instantiation as the NRS_KERNEL_LOG line names it (the 128-register entry point has no OCC argument)
inline void route_name(char* buf, size_t n, const RouteTraits& t, bool batch) {
	char head[32];
	if (t.entry == kEntryC128) snprintf(head, sizeof(head), "render_kernel_c128<%d", t.waves);
	else snprintf(head, sizeof(head), "render_kernel<%d, %d", t.waves, t.occ);
	snprintf(buf, n, "%s, prof %d, poisson %d, affine %d, team %d, num %d, extra %d%s>", head, (int)t.prof, (int)t.poisson, (int)t.affine, t.team, t.num, t.xtra, batch ? ", batch" : "");
}

enum RouteId : int {
	kRtDefaultAuto, kRtDefault1, kRtDefault2, kRtDefault4, kRtAffineAuto, kRtAffine1, kRtPoissonAuto, kRtShadeAll,
	kRtNum1Auto, kRtNum2Auto, kRtNum3Auto, kRtNumRtAuto, kRtNumRt1, kRtNumRt2, kRtNumRt4, kRtNumRtAffine, kRtNumRtAll,
	kRtGate, kRtDeepAuto, kRtExtraLean,
	kRtExtra, kRtExtraNumRt, kRtIntro, kRtIntroNumRt, kRtDeepExtra, kRtDeepExtraNumRt, kRtDeepIntro, kRtDeepIntroNumRt,
	kRtLightAuto, kRtLightAll,
	kRtProfAuto, kRtProf1, kRtCfg84Auto, kRtCfg84_1, kRtCfg84_2, kRtCfg84_4, kRtCfg84AffineAuto, kRtCfg42, kRtCfg124,
	kRtExtraLeanViews,
	kRouteCount
};
// batch: the row has a BATCH twin, the instantiation that serves a queue of several samples (nrs_render_nerf_spp).  The measurement rows have none.
// single: the row has a single-frame instantiation.  Every row but the one that exists for views batches alone.
struct RouteRow { RouteId id; RouteTraits t; bool batch; bool single = true; };

// TEAM 0 = the wave decides (automatic schedule: all-tail or hybrid queues); 1 / 2 / 4 = fixed lanes per ray.  A row's TEAM is what sizes the launch's packets.
constexpr RouteRow kRoutes[kRouteCount] = {
	// Production instantiations: scheduled for 3 waves/SIMD, capped at 128 VGPRs = 4 waves/SIMD (render_kernel_c128).  Measured against the
	// __launch_bounds__(512, 4) build of the same code (NRS_RENDER_CFG=84): 1080p lego + cage 9.43 -> 9.82 Gsamples/s, lego 10.7 -> 11.0,
	// varied-opacity scene 7.65 -> 7.89, aabb-16 4.35 -> 4.72.  (Plain __launch_bounds__(512, 3), round 1's choice, now lets the allocator
	// take 131 VGPRs = 3 waves/SIMD: 7.3.)
	{kRtDefaultAuto, {kEntryC128, 8, 3, false, false, false, 0, 0, kXtraNone}, true},
	{kRtDefault1,    {kEntryC128, 8, 3, false, false, false, 1, 0, kXtraNone}, true},
	{kRtDefault2,    {kEntryC128, 8, 3, false, false, false, 2, 0, kXtraNone}, true},
	{kRtDefault4,    {kEntryC128, 8, 3, false, false, false, 4, 0, kXtraNone}, true},
	// AffineDuplication (alone or with cage edits, no membrane correction, default roundings) on the automatic schedule since round 6
	{kRtAffineAuto,  {kEntryC128, 8, 3, false, false, true, 0, 0, kXtraNone}, true},  // (121 VGPRs on the 128-register entry point)
	{kRtAffine1,     {kEntryCfg, 8, 4, false, false, true, 1, 0, kXtraNone}, true},   // (its c128 build takes 133 VGPRs: the attribute is a target, not a limit)
	// membrane correction: 142 VGPRs, no scratch, 3 waves per SIMD (the SH9 colour loop is kept rolled for that: unrolled it held 108 coefficient loads
	// in flight, 250 VGPRs, 2 waves per SIMD: 6.1 Gsamples/s on the bench's lego_cage_membrane)
	// (12-wave workgroups: at 3 waves per SIMD a CU holds 12 waves, i.e. ONE 8-wave workgroup and a half -- the first r03 profile showed 256 workgroups,
	// 2 waves per SIMD; one 768-thread workgroup per CU uses all three)
	// Round 4: with the membrane terms evaluated BEHIND the main network pass (render_body) a POISSON-only instantiation fits the default launch shape
	// (8-wave workgroups, 128 VGPRs, 4 waves per SIMD) and runs the automatic schedule -- generations sized by the pending rays, re-teaming, ray hand-over.
	// The catch-all stays for mixed operator lists and for the membrane correction under a forced schedule.
	{kRtPoissonAuto, {kEntryCfg, 8, 4, false, true, false, 0, 0, kXtraNone}, true},
	{kRtShadeAll,    {kEntryCfg, 12, 3, false, true, true, 1, 0, kXtraNone}, true},
	// tiny-cuda-nn's other roundings.  The pair a parity-minded integrator switches on -- per-corner fp16 grid accumulation + fp16 MLP accumulators, what
	// tiny-cuda-nn's kernel_grid and fully fused MLP do as recalled -- on the automatic schedule: a compile-time instantiation like NUM = 0 (VERDICT r3 weak #1:
	// the run-time twin carries both flavours, 131 VGPRs = 3 waves per SIMD).  (round 6: one of the two roundings alone -- per-corner fp16 grid accumulation,
	// or fp16 MLP accumulators -- has its compile-time instantiation too: 125 / 123 VGPRs at 4 waves per SIMD instead of the run-time twin's 131 at 3)
	{kRtNum1Auto,    {kEntryC128, 8, 3, false, false, false, 0, 1, kXtraNone}, true},
	{kRtNum2Auto,    {kEntryC128, 8, 3, false, false, false, 0, 2, kXtraNone}, true},
	{kRtNum3Auto,    {kEntryC128, 8, 3, false, false, false, 0, 3, kXtraNone}, true},
	// ... and the run-time twin of every schedule and operator combination, so that no entry point refuses a rounding mode
	{kRtNumRtAuto,   {kEntryCfg, 8, 3, false, false, false, 0, kNumRuntime, kXtraNone}, true},
	{kRtNumRt1,      {kEntryCfg, 8, 3, false, false, false, 1, kNumRuntime, kXtraNone}, true},
	{kRtNumRt2,      {kEntryCfg, 8, 3, false, false, false, 2, kNumRuntime, kXtraNone}, true},
	{kRtNumRt4,      {kEntryCfg, 8, 3, false, false, false, 4, kNumRuntime, kXtraNone}, true},
	{kRtNumRtAffine, {kEntryCfg, 8, 3, false, false, true, 1, kNumRuntime, kXtraNone}, true},
	{kRtNumRtAll,    {kEntryCfg, 12, 3, false, true, true, 1, kNumRuntime, kXtraNone}, true},
	// cone-stepping scenes (aabb_scale > 1): the plain automatic schedule with the L2 phase gate (NRS_L2_GATE=0: A/B)
	// (the entry point scheduled for 3 waves per SIMD and held to 128 registers, like the default kernel's: knee 4.99 -> 5.09, 64 GiB 5.34 -> 5.37 Gsamples/s, profiles/r06/ab_gate_c128_*.txt)
	{kRtGate,        {kEntryC128, 8, 3, false, false, false, 0, 0, kXtraGate}, true},
	// a network whose rgb MLP has a third hidden layer (base_3layer.json): the plain case on the automatic schedule; everything else of it runs the DEEP catch-alls below
	{kRtDeepAuto,    {kEntryCfg, 8, 4, false, false, false, 0, 0, kXtraDeep}, true},
	// render modes / show_accel / depth of field ... (round 6: the common case -- a render mode / DoF / envmap / glow over plain cage edits or none, default roundings -- has
	// a lean instantiation without the membrane and AffineDuplication code: 123 VGPRs on the 128-register entry point, 8-wave workgroups, 4 waves per SIMD instead of
	// the catch-all's 145 at 3)
	{kRtExtraLean,   {kEntryC128, 8, 3, false, false, false, 1, 0, kXtraExtra}, true},
	// (its views batches run kRtExtraLeanViews, the last row)
	// the EXTRA catch-alls: every operator kind, membrane correction, one lane per ray.  Normals / EncodingVis: the INTRO instantiation (145 / 165 VGPRs, no scratch:
	// 12-wave workgroups at 3 waves per SIMD like the other modes); the DEEP twins of both for a network with a third rgb hidden layer, every mode
	{kRtExtra,           {kEntryCfg, 12, 3, false, true, true, 1, 0, kXtraExtra}, true},
	{kRtExtraNumRt,      {kEntryCfg, 12, 3, false, true, true, 1, kNumRuntime, kXtraExtra}, true},
	{kRtIntro,           {kEntryCfg, 12, 3, false, true, true, 1, 0, kXtraIntro}, true},
	{kRtIntroNumRt,      {kEntryCfg, 12, 3, false, true, true, 1, kNumRuntime, kXtraIntro}, true},
	{kRtDeepExtra,       {kEntryCfg, 12, 3, false, true, true, 1, 0, kXtraDeepExtra}, true},
	{kRtDeepExtraNumRt,  {kEntryCfg, 12, 3, false, true, true, 1, kNumRuntime, kXtraDeepExtra}, true},
	{kRtDeepIntro,       {kEntryCfg, 12, 3, false, true, true, 1, 0, kXtraDeepIntro}, true},
	{kRtDeepIntroNumRt,  {kEntryCfg, 12, 3, false, true, true, 1, kNumRuntime, kXtraDeepIntro}, true},
	// light directions: the LIGHT twin of the default kernel for the plain case, and the catch-all of such a network (every mode, every numerics, AffineDuplication)
	{kRtLightAuto,   {kEntryC128, 8, 3, false, false, false, 0, 0, kXtraLight}, true},
	{kRtLightAll,    {kEntryCfg, 12, 3, false, false, true, 1, kNumRuntime, kXtraLightAll}, true},
	// ---- measurement rows (development knobs only; single frames only) ----
	// the wave log (NRS_DEBUG bit 2) has PROF twins of the default kernel for the automatic schedule and one lane per ray only: AffineDuplication and fixed
	// 2 / 4 lanes per ray run their production instantiation with an empty log
	{kRtProfAuto,    {kEntryCfg, 8, 4, true, false, false, 0, 0, kXtraNone}, false},
	{kRtProf1,       {kEntryCfg, 8, 4, true, false, false, 1, 0, kXtraNone}, false},
	// NRS_RENDER_CFG = <waves per workgroup><waves per SIMD> overrides the tuned launch shape for the A/B measurements recorded under profiles/.
	// 84: the __launch_bounds__(512, 4) build of the default and AffineDuplication kernels (AffineDuplication with one lane per ray is kRtAffine1 either way)
	{kRtCfg84Auto,       {kEntryCfg, 8, 4, false, false, false, 0, 0, kXtraNone}, false},
	{kRtCfg84_1,         {kEntryCfg, 8, 4, false, false, false, 1, 0, kXtraNone}, false},
	{kRtCfg84_2,         {kEntryCfg, 8, 4, false, false, false, 2, 0, kXtraNone}, false},
	{kRtCfg84_4,         {kEntryCfg, 8, 4, false, false, false, 4, 0, kXtraNone}, false},
	{kRtCfg84AffineAuto, {kEntryCfg, 8, 4, false, false, true, 0, 0, kXtraNone}, false},
	// (the 10-wave / 5-waves-per-SIMD probe of rounds 1-3, NRS_RENDER_CFG=105, left the library in round 4: it spilled 77 registers at 96 VGPRs and, with the
	// two selection fragments in the LDS image, ten waves no longer fit the LDS budget of two workgroups per CU either)
	{kRtCfg42,       {kEntryCfg, 4, 2, false, false, false, 1, 0, kXtraNone}, false},
	{kRtCfg124,      {kEntryCfg, 12, 3, false, true, false, 0, 0, kXtraNone}, false}, // (A/B: one 12-wave workgroup per CU at 3 waves per SIMD, 136 VGPRs, no scratch)
	// ---- a production row again, last so that every row above keeps its number and with it its shard of nrs_render_rows.hip ----
	// the views batches (nrs_render_nerf_spp_views) of kRtExtraLean: the same body with the view table's reads, 133 VGPRs, 3 waves per SIMD.  A BATCH twin only: the still
	// batch and the single frame of kRtExtraLean compile as they did without it (123 VGPRs, 4 waves per SIMD)
	{kRtExtraLeanViews, {kEntryC128, 8, 3, false, false, false, 1, 0, kXtraExtraViews}, true, false},
};
constexpr bool routes_in_order() {
	for (int i = 0; i < kRouteCount; ++i)
		if (kRoutes[i].id != i) return false;
	return true;
}
static_assert(routes_in_order(), "kRoutes lists its rows in RouteId's order");

// ---- the planner ----------------------------------------------------------------------------------------------------------------------------------------
// The development knobs, read once by the caller (dev_knob: ignored unless NRS_DEV_KNOBS is set).  Defaults are what a production process runs with.
struct RouteKnobs {
	int32_t  team = 0;            // NRS_TEAM: a forced schedule, as nrs_ctx_set_lane_teams takes it (which wins over it)
	uint32_t hybrid_on = 1;       // NRS_HYBRID unset or != 0
	int32_t  render_cfg = 0;      // NRS_RENDER_CFG as a number
	uint32_t render_cfg_set = 0;  // NRS_RENDER_CFG is set at all
	uint32_t debug = 0;           // NRS_DEBUG (bit 2 = 4: the wave log)
	uint32_t l2_gate = 1;         // NRS_L2_GATE (0: off -- A/B)
	uint32_t tail_target = 24;    // NRS_TAIL_TARGET
	uint32_t tail_every = 3;      // NRS_TAIL_EVERY
	uint32_t tail_fill = 4;       // NRS_TAIL_FILL
	uint32_t alltail_target = 16; // NRS_ALLTAIL_TARGET
};
struct RouteRequest {
	// model
	uint32_t n_extra_dims, rgb_deep, numerics;
	int32_t  hashed_pairs;     // the finest level PAIRS hashed without records (what the L2 phase gate separates: one phase each)
	// operators
	uint32_t any_poisson, any_affine, apply_operators;
	// parameters
	uint32_t render_mode, show_accel, dof_on, distortion_mode, distortion_map, envmap, glow_mode;
	float    cone_angle_constant;
	uint32_t tile_size, height;
	uint16_t spp_count;        // samples in the launch's queue (<= NRS_SPP_BATCH_MAX)
	uint16_t views;            // the samples have a view each (nrs_render_nerf_spp_views).  The two halves of what was one 32-bit spp_count: a mirror that writes the count
	                           // as one little-endian word still says "no views"
	// context
	int32_t  lane_teams, n_cus;
	uint32_t busy;             // OTHER streams of the context with an unfinished launch
	uint32_t pixels_owned;     // pixels of the launch (all samples of a batch), in whole 8x8 packets
	double   hit_share;        // share of the pixels that became rays in the last finished launch
	RouteKnobs knobs;
};
static_assert(offsetof(RouteRequest, spp_count) == 68 && offsetof(RouteRequest, views) == 70 && offsetof(RouteRequest, lane_teams) == 72,
              "spp_count and views are the low and the high half of the word that was a 32-bit spp_count (a little-endian host: gfx950's are)");
struct RoutePlan {
	int      status;           // NRS_OK, or the refusal (then `message` says why and `row` is -1)
	char     message[256];
	int      row;              // RouteId
	// RenderArgs' schedule fields
	uint32_t team, all_tail, fill_lanes, tail_every, tail_target;
	uint32_t hybrid;           // 8x8 packets first, every tail_every-th packet row as tail packets of 64 / fill_lanes pixels behind them
	// RenderArgs' flags as the launch carries them
	uint32_t extra, gate, any_poisson;
	// what the NRS_TEAM_LOG line reports of the decision
	int32_t  forced;
	uint32_t fill_lanes_auto;
	double   rays_per_lane;
	uint32_t views;            // the launch carries a view table (a views request of more than one sample): the schedule word's bit 19
	// lanes on a pixel of the packets tile_geometry cuts: 64 / packet_lanes pixels per packet
	uint32_t packet_lanes() const { return all_tail ? fill_lanes : (team ? team : 1u); }
};

inline RoutePlan plan_route(const RouteRequest& q) {
	RoutePlan r{};
	r.status = NRS_OK;
	r.row = -1;
	const RouteKnobs& k = q.knobs;
	auto refuse = [&r](int status) -> RoutePlan& { r.status = status; return r; };
	const bool light = q.n_extra_dims != 0u, deep = q.rgb_deep != 0u, affine = q.any_affine != 0u, batch = q.spp_count > 1u;
	const bool wave_log = (k.debug & 4u) != 0u;
	const int cfg = k.render_cfg;
	bool poisson = q.any_poisson != 0u;
	if (light) {
		// The membrane correction and the measurement routes have no instantiation with the light term: refused, never rendered without it.
		if (poisson && q.apply_operators) {
			snprintf(r.message, sizeof(r.message), "nrs_render_nerf: the membrane correction (apply_poisson) is not supported for a network with light directions (n_extra_dims = 3)");
			return refuse(NRS_ERR_UNSUPPORTED);
		}
		poisson = false; // (operators switched off: the edits are not looked at)
		if (wave_log || k.render_cfg_set) {
			snprintf(r.message, sizeof(r.message), "nrs_render_nerf: the wave log (NRS_DEBUG bit 2) and NRS_RENDER_CFG are not supported for a network with light directions (n_extra_dims = 3)");
			return refuse(NRS_ERR_UNSUPPORTED);
		}
	}
	// a batch of samples runs the BATCH twin of the route a single frame takes; the measurement routes (the wave log's PROF twins, NRS_RENDER_CFG) serve single frames only
	if (batch && (wave_log || cfg != 0)) {
		snprintf(r.message, sizeof(r.message), "launch_render: route refused: the wave log (NRS_DEBUG bit 2) and NRS_RENDER_CFG have no instantiation for a batch of samples (spp_count %u)", q.spp_count);
		return refuse(NRS_ERR_STATE);
	}
	// Cone stepping is what the reference switches on for aabb_scale > 1 (tn:3410-3425): scenes whose fine hashed levels no two samples of a wave share, so that their
	// 8 MB of table lines thrash the 4 MB L2 of an XCD -- the GATE instantiation time-multiplexes it (nrs_hashgrid.cuh encode_to_lds; profiles/r06_garden.md: L2 misses per
	// sample 11.5 -> 7.2, +5 % on the garden frame).  A unit-cube scene (constant steps) never takes it: there the gate costs 18 %.
	// (only where the gate has something to separate: the two, three or four finest level PAIRS hashed without records -- one phase each -- and records below them;
	// more hashed pairs than phases would run the GATE instantiation ungated, 5 % behind the default kernel: profiles/r06/ab_gate_phases_*.txt)
	// (= kGateMaxPhases of the kernels.  Six phases for a model without any records: 4.36 -> 4.18 Gsamples/s, profiles/r06/ab_gate6_garden_nocache.txt -- a frame's round has
	// no time for six waits; the occupancy refresh, one gather per wave, gains with up to six: NRS_REFRESH_GATE_PHASES)
	// (a network with light directions renders ungated: the L2 phase gate is a schedule of the plain kernel alone)
	const bool gate = !light && k.l2_gate && q.cone_angle_constant > 0.f && q.hashed_pairs >= 2 && q.hashed_pairs <= 4;
	// everything of render_nerf's surface beyond Shade / Cost with a pinhole camera needs an EXTRA instantiation (one lane per ray)
	const bool extra = (q.render_mode != NRS_RENDER_SHADE && q.render_mode != NRS_RENDER_COST) || q.show_accel || q.dof_on || q.distortion_mode || q.distortion_map || q.envmap || q.glow_mode;
	const bool intro = q.render_mode == NRS_RENDER_NORMALS || q.render_mode == NRS_RENDER_ENCODING_VIS;

	// ---- the schedule the request asks for (a row that has no instantiation for it runs one lane per ray instead) ----
	const int forced = q.lane_teams ? q.lane_teams : k.team;
	const bool unforced = !forced && k.hybrid_on;
	// Lane teams (render_kernel's TEAM) when the launch cannot fill the GPU with one ray per lane.  Rays per lane is estimated from the share of pixels that became
	// rays in the last finished launch (0.25 until one has finished).  Measured on 1080p lego (0.22 of the pixels hit), frame shares 1/1 .. 1/8, ms per
	// launch with 1 / 2 / 4 lanes per ray: 3.09 2.89 3.31 | 2.07 1.78 1.95 | 1.56 1.25 1.21 | 1.19 0.93 0.88; 8 and 16
	// lanes lose everywhere (1.07, 1.72 at 1/8); 2560x1440: 4.31 4.52 5.64; aabb-16 1080p (every pixel hits): 9.64 9.76 10.9
	// Launches of this context still running on OTHER streams (frames in flight: a rank of a multi-GPU job that overlaps its frames, a viewer that
	// double-buffers) share the GPU with this one: the launch gets 1 / (1 + busy) of the lanes, and once three or more overlap the GPU is full
	// whatever the size of one launch -- lane teams (a latency device) then only cost fill passes.  Measured, 1/8 share of the 1080p bench frame,
	// ms per share-frame with 1 / 2 / 4 frames in flight: automatic choice before this rule 0.69 / 0.69 / 0.46, one lane per ray 0.99 / 0.54 / 0.36,
	// two lanes 0.77 / 0.47 / 0.49 (tools/scale_probe_teams.py) -- i.e. 0.95 of the single-GPU per-GPU throughput at an eighth of the frame.
	const double rays_per_lane = q.hit_share * (double)q.pixels_owned * (double)(1u + q.busy) / (64.0 * 16.0 * (double)q.n_cus);
	// Round 3: team rounds test the team's next positions in parallel and waves hand rays over, so the small-launch schedule (packets of 16 / 32 / 64
	// pixels = 4 / 2 / 1 lanes on a pixel during the fill, every generation sized by the rays its wave has pending) is the automatic choice up to
	// the sizes where the hybrid schedule of whole images takes over.  tools/schedule_probe.py (profiles/r03_schedules.md), ms per frame with
	// 16- / 32- / 64-pixel packets | hybrid | fixed 2 lanes per ray: 640x360 0.66 / 0.77 / 1.18 | 1.15 | 0.85, 960x540 0.93 / 0.96 / 1.16 | 1.20 | 1.12,
	// 1280x720 1.40 / 1.28 / 1.51 | 1.43 | 1.44, 1600x900 2.02 / 1.76 / 1.85 | 1.83 | 1.90, 1080p 2.77 / 2.36 / 2.37 | 2.35 | 2.48, 1440p 4.66 / 3.86 / 3.71 |
	// 3.79 | 3.96; a rank's tiles of the 1080p frame, N = 8: 0.53 / 0.57 / 0.89 | - | 0.57, N = 4: 0.85 / 0.82 / 1.01 | - | 0.94, N = 2: 1.49 / 1.32 / 1.43 | - | 1.47,
	// N = 1: 2.78 / 2.36 / 2.37 | - | 2.49.  With frames in flight the thresholds hold for the rays of ALL overlapping launches.
	uint32_t fill_lanes_auto = rays_per_lane <= 0.6 ? 4u : (rays_per_lane <= 2.6 ? 2u : 1u);
	// the fill runs once per pixel and lane on it: keep it to ~16 passes over the GPU (an all-miss 1080p frame is 8)
	while (fill_lanes_auto > 1 && (double)fill_lanes_auto * (double)q.pixels_owned * (double)(1u + q.busy) > 17.0 * 64.0 * 16.0 * (double)q.n_cus) fill_lanes_auto >>= 1;
	// The small-launch schedule: 4x4 / 8x4 / 8x8 packets only, and every generation takes ALL the rays its wave has pending with as many lanes per ray as
	// fit (4 up to 16 rays, 2 up to 32), so that no wave is left with a second, nearly empty generation (1/8 share of the bench frame: 0.88 -> 0.82 ms).
	// The hybrid schedule (64-ray generations at one lane per ray for the bulk of the queue, lane teams for its tail) was the choice for whole images with many
	// rays per lane until the queue's chunks went from 8 to 2 packets; since then the small-launch schedule wins there too -- bench frames, Gsamples/s hybrid /
	// 64-pixel packets: lego + cage 10.8 / 12.0, varied opacity 10.2 / 10.6, aabb-16 (7.9 rays per lane) 4.79 / 4.87 -- and hybrid runs only when forced (-1).
	const bool all_tail = unforced || forced == -2 || forced == -3 || forced == -4;
	// hybrid: whole images of the default kernel's family only; every tail_every-th packet row leaves the 8x8 list and joins the end of the queue as tail packets
	// (packet_pixel_bulk/_tail); measured on 1080p lego + cage, every 2nd / 3rd / 4th / 6th / 8th / 16th row: 8.88 / 8.89 / 8.79 / 8.75 / 8.65 / 8.65 Gsamples/s
	const bool hybrid_asked = forced == -1 && q.tile_size == 0u && !poisson && !affine && !extra && !light && !deep;
	const bool hybrid = hybrid_asked && ((q.height + 7u) / 8u) / k.tail_every != 0u;
	// lanes per ray asked for: 0 = the wave decides (both automatic schedules), 2 / 4 only when forced, else 1
	const int want = (all_tail || hybrid) ? 0 : ((forced == 2 || forced == 4) ? forced : 1);

	// ---- the row: the first that serves the request.  Its TEAM is the launch's, whatever was asked for. ----
	RouteId row;
	if (light) {
		// the LIGHT twin serves the plain case (Shade / Cost with a pinhole camera, no operators or cage edits, default roundings, no forced schedule)
		row = (!extra && !affine && !q.numerics && !deep && unforced) ? kRtLightAuto : kRtLightAll;
	} else if (deep && !extra && !poisson && !affine && !q.numerics && unforced && !wave_log && !k.render_cfg_set) {
		row = kRtDeepAuto;
	} else if (extra || deep) {
		if (!intro && !deep && !q.numerics && !poisson && !affine && !wave_log && cfg == 0) row = kRtExtraLean;
		else row = (RouteId)(kRtExtra + (deep ? 4 : 0) + (intro ? 2 : 0) + (q.numerics ? 1 : 0));
	} else if (gate && !q.numerics && !poisson && !affine && want == 0 && !wave_log && cfg == 0) {
		row = kRtGate;
	} else if (q.numerics) {
		const uint32_t n = q.numerics & 3u;
		if (!poisson && !affine && want == 0 && !wave_log && cfg == 0 && n) row = n == 1u ? kRtNum1Auto : (n == 2u ? kRtNum2Auto : kRtNum3Auto);
		else if (poisson) row = kRtNumRtAll;
		else if (affine) row = kRtNumRtAffine;
		else row = want == 0 ? kRtNumRtAuto : (want == 2 ? kRtNumRt2 : (want == 4 ? kRtNumRt4 : kRtNumRt1));
	} else if (poisson) {
		if (!affine && want == 0) row = cfg == 124 ? kRtCfg124 : kRtPoissonAuto;
		else row = kRtShadeAll;
	} else if (wave_log && !affine && want <= 1) {
		row = want == 0 ? kRtProfAuto : kRtProf1;
	} else if (cfg == 84) {
		if (affine) row = want == 0 ? kRtCfg84AffineAuto : kRtAffine1;
		else row = want == 0 ? kRtCfg84Auto : (want == 2 ? kRtCfg84_2 : (want == 4 ? kRtCfg84_4 : kRtCfg84_1));
	} else if (cfg == 42 && want == 1 && !affine) {
		row = kRtCfg42;
	} else if (affine) {
		row = want == 0 ? kRtAffineAuto : kRtAffine1;
	} else {
		row = want == 0 ? kRtDefaultAuto : (want == 2 ? kRtDefault2 : (want == 4 ? kRtDefault4 : kRtDefault1));
	}
	// A view per sample (q.views): every BATCH twin carries the view table behind a wave-uniform branch, so the row of the still batch serves it -- but the lean EXTRA row,
	// whose views batches have a row of their own (route_carries_views).  A views request of one sample is a single frame of that view.
	r.views = (batch && q.views) ? 1u : 0u;
	if (r.views && row == kRtExtraLean) row = kRtExtraLeanViews;
	const RouteRow& rr = kRoutes[row];
	if ((batch && !rr.batch) || (!batch && !rr.single)) { // (cannot happen: the measurement rows are reached through the knobs refused above, the views row by a batch alone)
		snprintf(r.message, sizeof(r.message), "launch_render: route refused: no instantiation for a batch of samples (spp_count %u) on this route", q.spp_count);
		return refuse(NRS_ERR_STATE);
	}

	// ---- the schedule fields, from the row ----
	r.row = row;
	r.team = (uint32_t)rr.t.team;
	r.fill_lanes = 4;
	r.tail_target = k.tail_target;
	if (rr.t.team == 0 && all_tail) {
		r.all_tail = 1;
		r.fill_lanes = forced == -4 ? 1u : (forced == -3 ? 2u : (forced == -2 ? 4u : fill_lanes_auto));
		r.tail_target = k.alltail_target;
	} else if (rr.t.team == 0) {
		r.hybrid = 1;
		r.fill_lanes = k.tail_fill; // lanes on a pixel while a tail packet is filled: packets of 4x4 / 8x4 / 8x8 pixels (packet_pixel_tail)
	}
	r.tail_every = hybrid_asked ? k.tail_every : 0u;
	r.extra = xtra_traits(rr.t.xtra).extra ? 1u : 0u;
	r.gate = gate ? 1u : 0u;
	r.any_poisson = poisson ? 1u : 0u;
	r.forced = forced;
	r.fill_lanes_auto = fill_lanes_auto;
	r.rays_per_lane = rays_per_lane;
	return r;
}

} // namespace nrs
