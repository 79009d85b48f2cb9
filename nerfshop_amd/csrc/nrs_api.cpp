// nrs_api.cpp -- C++ host code behind the C-ABI of include/nrs.h: the error message, the ABI version, the context.  (Model, operators, render call, display: nrs_api_*.cpp.)
// Plain C++17 + the HIP runtime API; no torch, no third-party dependencies.
#include "nrs_host.h"
#include "nrs_render.h"

#include <cmath>
#include <cstdio>
#include <new>

using namespace nrs;

static thread_local std::string g_err;
namespace nrs { void set_last_error(const char* msg) { g_err = msg ? msg : ""; } }
int nrs::fail(int code, const std::string& msg) {
	g_err = msg;
	return code;
}
int nrs::fail_hip(hipError_t e, const char* what) {
	g_err = std::string(what) + ": " + hipGetErrorString(e);
	return NRS_ERR_HIP;
}

// Marching parameters every ray-marching entry point hands to the kernels: min_mip indexes the 5-cascade bitfield (min_mip > 4 reads past
// it and makes kGrid >> mip zero, i.e. a voxel walk without progress), a negative / non-finite cone angle breaks calc_dt's clamp, a
// non-positive resolution divides by zero on the device.
int nrs::check_params_abi(const nrs_render_params* p, const char* who) {
	// (nothing zero-extends a struct built against another header -- the size is the contract)
	if (p->struct_size != (uint32_t)sizeof(nrs_render_params))
		return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": nrs_render_params.struct_size is " + std::to_string(p->struct_size) + ", this library's is " +
		            std::to_string(sizeof(nrs_render_params)) + " (ABI " + std::to_string(NRS_ABI_VERSION) + "): initialise with NRS_RENDER_PARAMS_INIT from the same nrs.h");
	return NRS_OK;
}
int nrs::check_march_params(const nrs_render_params& p, const char* who) {
	NRS_TRY(check_params_abi(&p, who));
	if (p.resolution[0] <= 0 || p.resolution[1] <= 0 || p.resolution[0] > 65535 || p.resolution[1] > 65535)
		return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": resolution out of range (1..65535)");
	if (p.min_mip > kCascades - 1) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": min_mip > 4 (the occupancy grid has 5 cascades)");
	if (!(p.cone_angle_constant >= 0.f) || !std::isfinite(p.cone_angle_constant)) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": cone_angle_constant must be finite and >= 0");
	if (!(p.min_transmittance >= 0.f && p.min_transmittance <= 1.f)) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": min_transmittance outside [0, 1]");
	for (int i = 0; i < 3; ++i)
		if (!std::isfinite(p.render_aabb_min[i]) || !std::isfinite(p.render_aabb_max[i])) return fail(NRS_ERR_INVALID_ARG, std::string(who) + ": render box is not finite");
	return NRS_OK;
}
// ---------------------------------------------------------------------------------------------------------------
extern "C" {

const char* nrs_last_error(void) { return g_err.c_str(); }
int nrs_abi_version(void) { return NRS_ABI_VERSION; }

int nrs_ctx_create(int device, nrs_ctx** out) {
	if (!out) return fail(NRS_ERR_INVALID_ARG, "nrs_ctx_create: out is NULL");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) return fail(NRS_ERR_NO_DEVICE, "nrs_ctx_create: no HIP device visible (this library has no CPU fallback)");
	if (device < 0 || device >= n) return fail(NRS_ERR_INVALID_ARG, "nrs_ctx_create: device index out of range");
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	nrs_ctx* c = new (std::nothrow) nrs_ctx();
	if (!c) return fail(NRS_ERR_STATE, "out of host memory");
	c->device = device;
	c->n_cus = prop.multiProcessorCount;
	c->hbm_bytes = prop.totalGlobalMem;
	snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
	hipError_t he = c->d_counters.alloc(nrs_ctx::kInFlight * 2);
	if (he == hipSuccess) he = hipMemset(c->d_counters.get(), 0, sizeof(RenderCounters) * nrs_ctx::kInFlight * 2);
	for (int i = 0; i < nrs_ctx::kInFlight; ++i) c->counters_clean[i] = he == hipSuccess;
	if (he == hipSuccess) he = c->d_edits.alloc((size_t)nrs_ctx::kMaxEdits * (nrs_ctx::kInFlight + 1));
	if (he == hipSuccess) he = c->d_views.alloc((size_t)NRS_SPP_BATCH_MAX * nrs_ctx::kInFlight);
	for (int i = 0; i < nrs_ctx::kInFlight && he == hipSuccess; ++i) he = hipEventCreateWithFlags(&c->slot_done[i], hipEventDisableTiming);
	if (he == hipSuccess) he = c->d_mean.alloc((8 + 256 * 8) / sizeof(float)); // mean + partial sums (launch_grid_to_bitfield)
	if (he == hipSuccess) he = c->d_wave_log.alloc(8192 * 4);
	if (he != hipSuccess) {
		nrs_ctx_destroy(c);
		return fail_hip(he, "nrs_ctx_create: hipMalloc");
	}
	// one device-visible host word for the launch feedback (lane-team sizing); optional: without it the estimate stays at its default
	if (hipHostMalloc((void**)&c->h_feedback, 8, hipHostMallocMapped) == hipSuccess) {
		*c->h_feedback = 0ull;
		if (hipHostGetDevicePointer((void**)&c->d_feedback, c->h_feedback, 0) != hipSuccess) c->d_feedback = nullptr;
	} else {
		(void)hipGetLastError();
		c->h_feedback = nullptr;
	}
	*out = c;
	return NRS_OK;
}
void nrs_ctx_destroy(nrs_ctx* c) {
	if (!c) return;
	for (int i = 0; i < nrs_ctx::kInFlight; ++i)
		if (c->slot_done[i]) (void)hipEventDestroy(c->slot_done[i]);
	if (c->h_feedback) (void)hipHostFree(c->h_feedback);
	delete c; // (its buffers go with it)
}
int nrs_ctx_set_lane_teams(nrs_ctx* ctx, int lanes_per_ray) {
	if (!ctx || !(lanes_per_ray == -4 || lanes_per_ray == -3 || lanes_per_ray == -2 || lanes_per_ray == -1 || lanes_per_ray == 0 || lanes_per_ray == 1 || lanes_per_ray == 2 || lanes_per_ray == 4))
		return fail(NRS_ERR_INVALID_ARG, "nrs_ctx_set_lane_teams: lanes_per_ray must be 0 (automatic), 1, 2, 4, -1 (hybrid), -2, -3 or -4 (small-launch schedule: teams sized per generation, 4x4- / 8x4- / 8x8-pixel packets)");
	ctx->lane_teams = lanes_per_ray;
	return NRS_OK;
}
int nrs_ctx_set_ray_handover(nrs_ctx* ctx, int enabled) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "ctx is NULL");
	ctx->handover = enabled ? 1 : 0;
	return NRS_OK;
}
int nrs_ctx_ray_handovers(const nrs_ctx* ctx, uint64_t* n_rays, uint64_t* n_handovers) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "ctx is NULL");
	if (n_rays) *n_rays = ctx->last_handover & 0xffffffffull;
	if (n_handovers) *n_handovers = ctx->last_handover >> 32;
	return NRS_OK;
}
int nrs_ctx_device_info(const nrs_ctx* c, char* name_out, size_t name_len, int* n_cus, size_t* hbm_bytes) {
	if (!c) return fail(NRS_ERR_INVALID_ARG, "ctx is NULL");
	if (name_out && name_len) snprintf(name_out, name_len, "%s", c->name);
	if (n_cus) *n_cus = c->n_cus;
	if (hbm_bytes) *hbm_bytes = c->hbm_bytes;
	return NRS_OK;
}
int nrs_ctx_render_launches(const nrs_ctx* ctx, uint64_t* n_dispatches, uint32_t* last_schedule) {
	if (!ctx) return fail(NRS_ERR_INVALID_ARG, "nrs_ctx_render_launches: NULL context");
	std::lock_guard<std::mutex> lock(const_cast<nrs_ctx*>(ctx)->launch_mutex);
	if (n_dispatches) *n_dispatches = ctx->render_dispatches;
	if (last_schedule) *last_schedule = ctx->last_schedule;
	return NRS_OK;
}

} // extern "C"
