// nrs_render.h -- the render launch as the host units see it: its argument and counter blocks, the launchers of nrs_render.hip (and the slice
// launch of nrs_network.hip, which takes the same arguments), and the planner's test-only C symbols.
#pragma once
#include <stdint.h>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"

namespace nrs {

struct RenderCounters {    // zeroed before every launch
	unsigned long long n_samples;
	uint32_t next_packet;
	uint32_t n_rays_alive;
	uint32_t n_rays_hit;
	uint32_t blocks_done; // workgroups that have flushed their statistics (the last one reports to RenderArgs::feedback)
	unsigned long long phase_cycles[8]; // NRS_DEBUG & 4: per-phase wave cycles (profiling build of the kernel only)
	// NRS_DEBUG & 4: voxel-walk statistics. [0]/[1] fill: lane iterations / wave trips (= max over lanes per call);
	// [2]/[3] the same for the per-sample march; [4] sample rounds, [5] live lanes summed over rounds, [6] march calls with > 1 trip
	// [8] samples inside a cage's deformed box (they scan a LUT cell), [9] rounds with such a sample, [10] candidates tested (lane iterations of the scan),
	// [11] the scan's wave trips (max over the lanes of a round), [12] samples that found their tet
	unsigned long long walk[13];
};

struct RenderArgs {
	nrs_render_params p;
	const DeviceEdit* edits;   // device array, applied last-to-first
	int32_t  n_edits;
	uint32_t any_poisson;      // some edit has apply_poisson set
	uint32_t any_affine;       // some edit is an AffineDuplication
	uint32_t extra;            // a render mode other than Shade / Cost, show_accel or dof != 0: render_kernel's EXTRA instantiation
	uint32_t gate;             // cone stepping (aabb_scale > 1 scenes): the plain kernel's GATE instantiation (L2 phase gate on the four finest hashed levels)
	uint32_t n_packets;        // pixel packets owned by this call (8x8 pixels; 8x4 / 4x4 with lane teams of 2 / 4)
	uint32_t tiles_x;          // image width in tiles (tiled mode) or in packets (whole-image mode)
	uint32_t packets_per_tile_x;
	uint32_t pixels_owned;     // pixels this launch covers (for the feedback word)
	unsigned long long* feedback; // host-mapped: rays that found an occupied cell | pixels_owned << 32, written by the last workgroup
	uint32_t tail_every;       // hybrid launches: every tail_every-th packet row is a tail row (3)
	uint32_t reteam;           // hybrid launches: spread a wave's last rays over its idle lanes (render_kernel)
	uint32_t tail_target;      // hybrid launches: rays a wave collects per generation once it works on tail packets (24)
	uint32_t all_tail;         // hybrid launches: every packet is a 4x4 tail packet (packet_pixel<4>'s geometry, whole-image or tiles)
	uint32_t steal;            // hybrid launches: waves that run out of work take half the rays of a sibling of their workgroup (render_body, "ray hand-over")
	uint32_t fill_lanes;       // small-launch schedule (all_tail): lanes that stand on one pixel during the fill (4, 2 or 1: packets of 16 / 32 / 64 pixels)
	uint32_t p_big;            // hybrid launches (team == 0): packets [0, p_big) are 8x8, the rest 4x4 tail packets; else 0
	uint32_t team;             // 0 = hybrid (full generations, lane teams for the queue's tail); lanes per ray: 1, or 2 / 4 for launches with too few rays to fill the GPU (render_kernel's TEAM)
	uint32_t spp_count;        // samples of the view in this launch's queue (nrs_render_nerf_spp; 1: a single frame): n_packets = spp_count * spp_packets and, hybrid, p_big = spp_count * spp_big
	uint32_t spp_packets;      // packets of ONE sample (what n_packets is for a single frame)
	uint32_t spp_big;          // hybrid launches: 8x8 packets of one sample (what p_big is for a single frame)
	uint32_t slab_stride;      // pixels from one sample's slab of frame / depth / steps to the next (0 for a single frame)
	uint32_t max_steps;
	uint32_t dbg;              // NRS_DEBUG ablation bits (profiling only; 0 in production): 1 = all gathers hit entry 0, 2 = skip the MLPs
	float*    frame;           // f32x4
	float*    depth;
	uint32_t* steps;           // nullable
	RenderCounters* counters;
	RenderCounters* counters_next; // the block the slot's NEXT launch will use: zeroed by this launch's last workgroup (nullable)
	unsigned long long* wave_log; // NRS_DEBUG & 4: 4 words per wave (see nrs_render_nerf)
	const nrs_sample_view* views; // nrs_render_nerf_spp_views: spp_count records in the launch slot's device table, sample s renders with record s (null: every sample with p's camera)
};

// launches row `row` of kRoutes (nrs_route.h; the caller planned it: plan_route), or its batch twin when a.spp_count > 1
int launch_render(RouteId row, const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream);
// n records of a views batch into the launch slot's table, ordered on the stream; h_views is free when the call returns (the records travel as kernel arguments)
int launch_views_upload(const nrs_sample_view* h_views, uint32_t n, nrs_sample_view* d_views, void* stream);
unsigned long long launch_render_dispatches(); // render-kernel dispatches of this process so far (nrs_ctx_render_launches counts with it)
// render mode Slice (Testbed::render_nerf's branch, testbed_nerf.cu:3111-3175): one network evaluation per owned pixel on the slice plane
int launch_slice(const DeviceModel& m, const RenderArgs& a, int n_cus, void* stream);

// The planner behind one C symbol (exported from libnrs.so, declared here only: not part of include/nrs.h): tests sweep it without a GPU.
struct RouteProbe {
	int32_t  status;
	int32_t  row;              // RouteId, -1 when refused
	uint32_t team, all_tail, fill_lanes, tail_every, tail_target, hybrid;
	uint32_t row_has_batch;
	char     name[96];         // the row as route_name prints it for this request (", batch" for spp_count > 1)
	char     message[256];
};

} // namespace nrs

// plans n requests; request_size / probe_size are the caller's sizeof of the two structs (a mirror that has drifted is refused: NRS_ERR_INVALID_ARG)
extern "C" int nrs_route_probe(const nrs::RouteRequest* requests, uint32_t request_size, uint32_t n, nrs::RouteProbe* out, uint32_t probe_size);
// RoutePlan::views of each request (0 for a refused one): what nrs_route_probe's answer has no field for
// (a second test-only export that plans every request again for one field: RouteProbe gets a `views` member, and this goes, when RouteProbe's mirrors next change)
extern "C" int nrs_route_probe_views(const nrs::RouteRequest* requests, uint32_t request_size, uint32_t n, uint32_t* views_out);
