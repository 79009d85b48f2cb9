// nrs_render_rows.h -- what the host side of the render launch (nrs_render.hip) and the launchers of the rows (nrs_render_rows.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_render.h"

namespace nrs {

extern std::atomic<unsigned long long> g_render_dispatches; // render-kernel dispatches of this process (launch_render_dispatches)
int check_route(const DeviceModel& m, const RenderArgs& a, const RouteTraits& t, bool batch);
// The launcher of row ROW of kRoutes: declared here, defined in nrs_render_rows.hip, which is compiled once per shard and instantiates the rows of
// that shard -- and through them the kernels.  No other translation unit sees the definition, so none can instantiate a kernel by accident.
typedef int (*RouteLauncher)(const DeviceModel&, const RenderArgs&, int, hipStream_t);
template <int ROW, bool BATCH, bool TWIN = false>
int launch_row(const DeviceModel& m, const RenderArgs& a, int n_cus, hipStream_t stream);

} // namespace nrs
