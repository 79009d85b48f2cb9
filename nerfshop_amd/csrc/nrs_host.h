// nrs_host.h -- what the host units behind the C-ABI (nrs_api.cpp, nrs_api_*.cpp) share: the three opaque structs of include/nrs.h, the error
// helpers, the owner of a device allocation (all three in nrs_handles.h), and the few helpers that cross unit borders.  Host-only C++17: no .hip / .cuh includes it.
#pragma once
#include "nrs_handles.h"
#include "../../include/nrs.h"
#include "nrs_internal.h"

namespace nrs {

// nrs_api.cpp
int check_params_abi(const nrs_render_params* p, const char* who);
int check_march_params(const nrs_render_params& p, const char* who);
// nrs_api_lowering.cpp
uint32_t kernel_layer(const nrs_model_desc& d, uint32_t layer);
uint32_t network_layer_width(const nrs_model_desc& d, uint32_t layer, uint32_t n_extra_dims = 0);
bool desc_supported(const nrs_model_desc& d);
uint32_t n_mlp_weights(const nrs_model_desc& d, uint32_t n_extra_dims = 0);
const char* extra_dims_refusal(const nrs_model_desc& d, uint32_t n_extra_dims);
struct LowerOps { uint16_t one, minus_one; uint16_t (*negate)(uint16_t); };
extern const LowerOps kLowerValues, kLowerIndices;
void lower_weights(const nrs_model_desc& d, const uint16_t* w, uint16_t* canon, const LowerOps& ops, uint32_t n_extra_dims = 0);
uint32_t make_levels(const nrs_model_desc& d, LevelParams* lv);
void make_weight_fragments(const uint16_t* w, uint16_t* frag, uint16_t one = 0x3C00);
// nrs_api_model.cpp
DeviceModel model_for_launch(const nrs_model* m, const nrs_render_params& p);
// nrs_api_edit.cpp
int build_fine_lut(nrs_edit* e, hipStream_t s);

} // namespace nrs
