// nrs_render.hip -- the host side of the render launch: the last guard, the table of launchers (one per row of kRoutes), launch_render.
// The launchers themselves, and with them every instantiation of the render kernel, are compiled in shards from nrs_render_rows.hip.
#include <hip/hip_runtime.h>
#include <string.h>
#include <utility>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_launch.h"
#include "nrs_render.h"
#include "nrs_render_rows.h"

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
	else if (a.views && (!route_carries_views(t.poisson, t.affine, t.xtra, batch) || a.slab_stride == 0u)) why = "a table of views needs a BATCH twin that reads it (EXTRA 9 on the lean row) and slabs";
	else if (a.spp_count == 0u || a.spp_packets == 0u || a.n_packets != a.spp_count * a.spp_packets) why = "the queue is not spp_count times the packets of one sample";
	if (!why) return NRS_OK;
	char name[160];
	route_name(name, sizeof(name), t, batch);
	snprintf(g_launch_err, sizeof(g_launch_err), "launch_render: route refused: %s for team %u, affine %u, poisson %u, numerics %u, extra %u, deep %u, gate %u, render mode %u: %s",
	         name, a.team, a.any_affine, a.any_poisson, m.numerics, a.extra, m.rgb_deep, a.gate, (uint32_t)a.p.render_mode, why);
	return NRS_ERR_STATE;
}

// The view table of nrs_render_nerf_spp_views reaches the device as kernel arguments, 32 records (3.5 KB of the 4 KB segment) per launch: the runtime copies the
// arguments of a launch before it returns, so the caller's host array is free at once, the write is ordered on the stream in front of the render launch, and nothing
// waits on the host -- which a copy from pageable memory does not promise and a shared pinned staging area would need an event wait for.
constexpr uint32_t kViewsPerUpload = 32u, kViewFloats = sizeof(nrs_sample_view) / 4u;
struct ViewChunk { float w[kViewsPerUpload * kViewFloats]; };
static_assert(sizeof(nrs_sample_view) == 112 && sizeof(ViewChunk) + 16 <= 4096, "a chunk of views fits the kernel-argument segment");
__global__ __launch_bounds__(256) void views_upload_kernel(const ViewChunk c, float* __restrict__ dst, uint32_t n_floats) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_floats) dst[i] = c.w[i];
}
int launch_views_upload(const nrs_sample_view* h_views, uint32_t n, nrs_sample_view* d_views, void* stream) {
	for (uint32_t first = 0; first < n; first += kViewsPerUpload) {
		const uint32_t count = n - first < kViewsPerUpload ? n - first : kViewsPerUpload, n_floats = count * kViewFloats;
		ViewChunk c;
		memcpy(c.w, h_views + first, (size_t)n_floats * 4u);
		memset(c.w + n_floats, 0, sizeof(c.w) - (size_t)n_floats * 4u);
		hipLaunchKernelGGL(views_upload_kernel, dim3((n_floats + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, c, reinterpret_cast<float*>(d_views + first), n_floats);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) { snprintf(g_launch_err, sizeof(g_launch_err), "launch_views_upload: %s", hipGetErrorString(e)); return NRS_ERR_HIP; }
	}
	return NRS_OK;
}

// one row per row of kRoutes: its traits, its single-frame launcher (null on the row of views batches alone), its batch-twin launcher (null where the row has none: the measurement rows)
struct RouteLaunch { const RouteTraits* traits; RouteLauncher single, batch; };
template <int ROW>
static constexpr RouteLauncher single_launcher() {
	if constexpr (kRoutes[ROW].single) return &launch_row<ROW, false>;
	else return nullptr;
}
template <int ROW>
static constexpr RouteLauncher batch_launcher() {
	if constexpr (kRoutes[ROW].batch) return &launch_row<ROW, true>;
	else return nullptr;
}
template <int... ROW>
struct RouteLaunchTable { RouteLaunch row[sizeof...(ROW)] = {{&kRoutes[ROW].t, single_launcher<ROW>(), batch_launcher<ROW>()}...}; };
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
