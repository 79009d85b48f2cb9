// nrs_render_rows.hip -- the launchers of the rows of kRoutes, and through them every instantiation of the render kernel (nrs_render.cuh).
// Compiled NRS_ROW_SHARDS times, with -DNRS_ROW_SHARD=0 .. NRS_ROW_SHARDS - 1 (Makefile): each build instantiates the rows of its shard, so the instantiations
// compile in parallel.  Row ROW belongs to shard ROW % NRS_ROW_SHARDS: every row is in exactly one shard, and a new row of kRoutes needs no edit here.
#include <hip/hip_runtime.h>
#include <utility>
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_launch.h"
#include "nrs_render.h"
#include "nrs_render_rows.h"
#include "nrs_render.cuh"

#if !defined(NRS_ROW_SHARD) || !defined(NRS_ROW_SHARDS) || NRS_ROW_SHARD < 0 || NRS_ROW_SHARD >= NRS_ROW_SHARDS
#error "compile with -DNRS_ROW_SHARDS=<n> -DNRS_ROW_SHARD=<0 .. n - 1>"
#endif

namespace nrs {

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
template <int ROW, bool BATCH, bool TWIN>
int launch_row(const DeviceModel& m, const RenderArgs& a, int n_cus, hipStream_t stream) {
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

// This shard's rows: of each, the single-frame launcher and the batch twin that the row has.  Naming them in a class that is instantiated explicitly is what
// instantiates them here (a __launch_bounds__(512, 4) twin is instantiated from inside its row's launch_row: the same shard).
template <int SHARD, typename Rows>
struct RowShard;
template <int SHARD, int... ROW>
struct RowShard<SHARD, std::integer_sequence<int, ROW...>> {
	template <int R>
	static constexpr RouteLauncher single() {
		if constexpr (R % NRS_ROW_SHARDS == SHARD && kRoutes[R].single) return &launch_row<R, false>;
		else return nullptr;
	}
	template <int R>
	static constexpr RouteLauncher batch() {
		if constexpr (R % NRS_ROW_SHARDS == SHARD && kRoutes[R].batch) return &launch_row<R, true>;
		else return nullptr;
	}
	static inline const RouteLauncher launchers[2 * sizeof...(ROW)] = {single<ROW>()..., batch<ROW>()...};
};
template struct RowShard<NRS_ROW_SHARD, std::make_integer_sequence<int, kRouteCount>>;

} // namespace nrs
