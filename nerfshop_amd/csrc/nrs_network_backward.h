// nrs_network_backward.h -- the launcher of nrs_network_backward.hip.
#pragma once
#include <stdint.h>
#include "nrs_internal.h"

namespace nrs {

// NerfNetwork::backward for base.json's architecture at the default numerics (nrs_network_backward.hip): parameter gradients ADDED to d_dparams (fp32, the blob's order),
// optionally dL/dposition into floats 0..2 of d_dinput's records
int launch_network_backward(const DeviceModel& m, uint32_t n, const float* d_in, uint32_t ld_in, const void* d_dout, uint32_t ld_dout, int layout,
                            float* d_dparams, float* d_dinput, int n_cus, void* stream);

} // namespace nrs
