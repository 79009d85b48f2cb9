// nrs_launch.cpp -- the one definition of the launchers' error message (nrs_launch.h).
#include "../../include/nrs.h"
#include "nrs_internal.h"
#include "nrs_launch.h"

namespace nrs {

thread_local char g_launch_err[512];
const char* launch_last_error() { return g_launch_err; }
int hip_fail(hipError_t e, const char* what) {
	snprintf(g_launch_err, sizeof(g_launch_err), "%s: %s", what, hipGetErrorString(e));
	return NRS_ERR_HIP;
}

} // namespace nrs
