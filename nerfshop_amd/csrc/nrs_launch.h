// nrs_launch.h -- the launch-error plumbing of the device translation units: ONE thread-local message (nrs_launch.cpp), which the host units read
// through launch_last_error() (NRS_LAUNCH, nrs_host.h) after a launcher has returned anything but NRS_OK.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

namespace nrs {

extern thread_local char g_launch_err[512];
int hip_fail(hipError_t e, const char* what); // writes "<what>: <HIP's error string>", returns NRS_ERR_HIP
#define NRS_LAUNCH_CHECK(what)                               \
	do {                                                     \
		hipError_t e_ = hipGetLastError();                   \
		if (e_ != hipSuccess) return hip_fail(e_, what);     \
	} while (0)

} // namespace nrs
