// nrs_render.hip -- the host side of the render launch: the last guard, the table of launchers (one per row of kRoutes), launch_render.
// The launchers themselves, and with them every instantiation of the render kernel, are compiled in shards from nrs_render_rows.hip.
#include <hip/hip_runtime.h>
#include <utility>
#include "nrs_internal.h"
#include "nrs_launch.h"
#include "nrs_render.h"

namespace nrs {

std::atomic<unsigned long long> g_render_dispatches{0};
unsigned long long launch_render_dispatches() { return g_render_dispatches.load(); }

// The precondition of every render launch: the packets were sized (a.team, tile_geometry) for the TEAM of the row that is launched.  Both come from one plan
// (nrs_route.h plan_route), so this should never fire -- it stays as the last guard because a mismatch makes packet_pixel lay out pixels with another packet
// shape than the launch was sized for and write past a tiled frame.  A route that fails it is refused (NRS_ERR_STATE) and nothing is launched.
int check_route(const DeviceModel& m, const RenderArgs& a, const RouteTraits& t, bool batch) {
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

// one row per row of kRoutes: its traits, its single-frame launcher, its batch-twin launcher (null where the row has none: the measurement rows)
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

} // namespace nrs
