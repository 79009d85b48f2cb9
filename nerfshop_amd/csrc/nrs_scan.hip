// nrs_scan.hip -- the middle step of every three-launch exclusive scan of the library: one workgroup over the tiles' sums.
//
// The callers (cage look-up tables: nrs_cage.hip, 1 value per tile of 4096 cells; marching cubes: nrs_mesh.hip, 2 values per block of 256 points; training rays:
// nrs_train.hip, 2 values per tile of 1024 rays) sum their tiles into `sums`, launch this, and scan inside each tile on top of its now exclusive prefix.
#include <hip/hip_runtime.h>
#include "../../include/nrs.h"
#include "nrs_launch.h"
#include "nrs_scan.h"
#include "nrs_scan.cuh"

namespace nrs {

// Thread t owns a contiguous run of tiles, sums it, the 1024 sums are scanned across the workgroup, and the run is rewritten as running prefixes: any number of tiles.
// (A few bytes per tile -- 1 MiB for a 512^3 lattice -- L2-resident between the two passes over the run.)
constexpr uint32_t kTileScanThreads = 1024;
template <uint32_t N>
__global__ __launch_bounds__(kTileScanThreads) void tile_scan_kernel(uint32_t n_tiles, uint32_t* __restrict__ sums, uint32_t* __restrict__ totals, uint32_t* __restrict__ total_copy) {
	const uint32_t per = (n_tiles + kTileScanThreads - 1) / kTileScanThreads;
	const uint32_t first = min(threadIdx.x * per, n_tiles), last = min(first + per, n_tiles);
	uint32_t v[N], run[N], all[N];
	#pragma unroll
	for (uint32_t k = 0; k < N; ++k) v[k] = 0u;
	for (uint32_t b = first; b < last; ++b) {
		#pragma unroll
		for (uint32_t k = 0; k < N; ++k) v[k] += sums[N * b + k];
	}
	block_exclusive_add<kTileScanThreads, N>(v, run, all);
	for (uint32_t b = first; b < last; ++b) {
		#pragma unroll
		for (uint32_t k = 0; k < N; ++k) {
			const uint32_t s = sums[N * b + k];
			sums[N * b + k] = run[k];
			run[k] += s;
		}
	}
	if (threadIdx.x == 0) {
		#pragma unroll
		for (uint32_t k = 0; k < N; ++k) totals[k] = all[k];
		if (total_copy) *total_copy = all[0];
	}
}

int launch_tile_scan(uint32_t n_tiles, uint32_t n_values, uint32_t* d_sums, uint32_t* d_totals, uint32_t* d_total_copy, void* stream) {
	if (n_values == 1u) hipLaunchKernelGGL(tile_scan_kernel<1>, dim3(1), dim3(kTileScanThreads), 0, (hipStream_t)stream, n_tiles, d_sums, d_totals, d_total_copy);
	else if (n_values == 2u) hipLaunchKernelGGL(tile_scan_kernel<2>, dim3(1), dim3(kTileScanThreads), 0, (hipStream_t)stream, n_tiles, d_sums, d_totals, d_total_copy);
	else { snprintf(g_launch_err, sizeof(g_launch_err), "tile_scan_kernel: %u values per tile", n_values); return NRS_ERR_INVALID_ARG; }
	NRS_LAUNCH_CHECK("tile_scan_kernel launch");
	return NRS_OK;
}

} // namespace nrs
