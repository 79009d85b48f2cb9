// nrs_api_lowering.cpp -- the network family of configs/nerf/: which descriptions are supported, their sizes and level tables, and the lowering of their weights onto the kernels' one network shape.
#include "nrs_host.h"

#include <cmath>
#include <cstring>

using namespace nrs;

// ---------------------------------------------------------------------------------------------------------------
// NerfNetworkFull::width(layer) / num_forward_activations (nerf_network_full.h:507-521): the hash-grid output, the density network's hidden layer, the rgb
// network's input, then one layer per rgb hidden layer.  NerfNetworkNoDir (nerf_network_nodir.h:419-438): the first two (its num_forward_activations counts two
// more, which its own forward_activations cannot serve).  0 = no such layer.
// The kernels number the layers of base.json's shape: 0 grid, 1 density hidden, 2 rgb input, 3.. rgb hidden.  A density network WITHOUT hidden layer
// (configs/nerf/linear.json) has no layer 1 in the reference's numbering: its layer k >= 1 is the kernels' layer k + 1.
// (A layer number beyond every network of the family -- e.g. 0xFFFFFFFF, which `layer + 1` would wrap to the hash grid -- maps to a layer nobody has: width 0.)
uint32_t nrs::kernel_layer(const nrs_model_desc& d, uint32_t layer) {
	if (layer >= 8u) return 0xFFu;
	return (d.density_hidden_layers == 0u && layer >= 1u) ? layer + 1u : layer;
}
uint32_t nrs::network_layer_width(const nrs_model_desc& d, uint32_t layer, uint32_t n_extra_dims) {
	const uint32_t k = kernel_layer(d, layer);
	if (k == 0u) return 32u;
	if (k == 1u) return 64u;
	if (d.sh_degree == 0u) return 0u;
	if (k == 2u) return n_extra_dims ? 48u : 32u; // (light directions: 16 density outputs | 16 SH coefficients | Identity(light 3) padded with ones to 16)
	return k - 3u < d.rgb_hidden_layers ? 64u : 0u;
}
// configs/nerf/base.json's family: hash grid of 16 x 2 features (any table size: base_14 / small / base / big.json), the 64-wide density network with one hidden
// layer -- or none: one [16 x 32] matrix (CutlassMLP, linear.json) --, and an rgb network of 0 (CutlassMLP, base_0layer.json), 1, 2 (base.json) or 3 hidden layers (base_{1,2,3}layer.json) on SH degree 4 -- or none at all
// (base_nodir.json -> NerfNetworkNoDir, testbed.cu:2314-2353: sh_degree == 0).
bool nrs::desc_supported(const nrs_model_desc& d) {
	const bool trunk = d.n_levels == 16 && d.n_features_per_level == 2 && d.n_neurons == 64 && d.density_hidden_layers <= 1 && d.density_output_dims == 16 &&
	                   d.log2_hashmap_size >= 8 && d.log2_hashmap_size <= 24 && d.base_resolution >= 1;
	if (!trunk) return false;
	if (d.sh_degree == 0) return d.rgb_hidden_layers == 0;
	return d.sh_degree == 4 && d.rgb_hidden_layers <= 3;
}
// rgb network parameters in the caller's blob (tiny-cuda-nn's layouts as recalled: the submodule is absent): FullyFusedMLP with L >= 1 hidden layers =
// [64 x 32] + (L - 1) [64 x 64] + [16 x 64] (3 outputs padded to 16 rows); CutlassMLP without hidden layer = one [8 x 32] matrix (outputs padded to 8).
static uint32_t n_rgb_weights(const nrs_model_desc& d) {
	if (d.sh_degree == 0) return 0u;
	if (d.rgb_hidden_layers == 0) return 8u * 32u;
	return 64u * 32u + (d.rgb_hidden_layers - 1u) * 64u * 64u + 16u * 64u;
}
static uint32_t n_density_weights(const nrs_model_desc& d) { return d.density_hidden_layers == 0 ? 16u * 32u : kDensityW; }
// n_extra_dims = 3 (light directions): the direction encoding is Composite[SH(3 dims, degree 4) | Identity(3 dims)] = 19 outputs padded to the rgb network's
// alignment, 32, so the first rgb matrix is [64 x 48] instead of [64 x 32] (nerf_network_full.h:43; tiny-cuda-nn as recalled)
uint32_t nrs::n_mlp_weights(const nrs_model_desc& d, uint32_t n_extra_dims) { return n_density_weights(d) + n_rgb_weights(d) + (n_extra_dims ? 64u * 16u : 0u); }
// nrs_model_create_ex / nrs_model_n_params_ex: which networks may carry extra dims.  nullptr = fine.
const char* nrs::extra_dims_refusal(const nrs_model_desc& d, uint32_t n_extra_dims) {
	if (n_extra_dims == 0u) return nullptr;
	if (d.sh_degree == 0u) return "NerfNetworkNoDir (no direction encoding, base_nodir.json) with extra input dimensions is not supported";
	if (d.rgb_hidden_layers == 0u) return "the 0-layer CutlassMLP rgb network (base_0layer.json) with extra input dimensions is not supported";
	return nullptr;
}

// ---- lowering of the family onto the kernels' network (kCanonW entries, nrs_internal.h) -------------------------------------------------------------
// Entries are opaque 16-bit words: fp16 bit patterns (nrs_model_set_params) or weight indices (nrs_model_set_params_device's permutation); `ops` says what
// zero, +1, -1 and a negated entry look like.  Every lowered network computes the values of the network it stands for EXACTLY, in both rounding models:
//   one hidden layer:  Wr2 = I.  The second hidden layer is relu(round(1 x h)) = h (h >= 0, an fp16 value; the other addends are zeros).
//   no hidden layer:   y = W x is formed by the FIRST layer with its own k blocks ([density outputs | SH coefficients]: the roundings of the one-matrix network),
//                      once as W and once as -W (rounding is symmetric): hidden = (relu(y), relu(-y)); Wr2 = I; the output layer subtracts the two, one of which is 0.
//   no rgb network:    the same with unit rows in place of W: (r, g, b) = density-network outputs 1..3 (NerfNetworkNoDir::inference_mixed_precision_impl,
//                      nerf_network_nodir.h:47-91).
//   three hidden layers: Wr2b, the kernels' optional layer (DeviceModel::rgb_deep).
// (A value of -0 comes out as +0: equal, not bit-identical.)
void nrs::lower_weights(const nrs_model_desc& d, const uint16_t* w, uint16_t* canon, const LowerOps& ops, uint32_t n_extra_dims) {
	memset(canon, 0, kCanonW * sizeof(uint16_t));
	if (d.density_hidden_layers == 0) {
		// no hidden layer in the density network (linear.json): y = W f by the first layer as (W, -W), the output layer subtracts relu(y) and relu(-y) -- as for the
		// rgb network below.  (The density's input gradient goes through the same two layers: (y > 0) W^T 128 - (y < 0) (-W)^T 128 = W^T 128, the linear layer's
		// own backward pass, for every y but an exact 0.)
		uint16_t* Wd1 = canon;           // [64 x 32]
		uint16_t* Wd2 = canon + 64 * 32; // [16 x 64]
		for (int row = 0; row < 16; ++row) {
			for (int k = 0; k < 32; ++k) { Wd1[row * 32 + k] = w[row * 32 + k]; Wd1[(16 + row) * 32 + k] = ops.negate(w[row * 32 + k]); }
			Wd2[row * 64 + row] = ops.one;
			Wd2[row * 64 + 16 + row] = ops.minus_one;
		}
	} else {
		memcpy(canon, w, kDensityW * sizeof(uint16_t));
	}
	const uint16_t* r = w + n_density_weights(d);
	uint16_t* Wr1 = canon + kDensityW;   // [64 x 32]
	uint16_t* Wr2 = Wr1 + 64 * 32;       // [64 x 64]
	uint16_t* Wr3 = Wr2 + 64 * 64;       // [16 x 64]
	uint16_t* Wr2b = Wr3 + 16 * 64;      // [64 x 64]
	auto identity = [&](uint16_t* M) { for (int i = 0; i < 64; ++i) M[i * 64 + i] = ops.one; };
	const uint32_t L = d.rgb_hidden_layers;
	std::vector<uint16_t> narrow;
	if (n_extra_dims && d.sh_degree != 0 && L >= 1) {
		// light directions: the first rgb matrix is [64 x 48].  Columns 0..31 take Wr1's place, columns 32..47 (light 3 | padding 13) go to Wr1x; the rest of the
		// rgb part follows as in the plain network
		uint16_t* Wr1x = Wr2b + 64 * 64; // [64 x 16]
		const uint32_t n_rest = n_rgb_weights(d) - 64u * 32u;
		narrow.resize(n_rgb_weights(d));
		for (int row = 0; row < 64; ++row) {
			memcpy(narrow.data() + row * 32, r + row * 48, 32 * 2);
			memcpy(Wr1x + row * 16, r + row * 48 + 32, 16 * 2);
		}
		memcpy(narrow.data() + 64 * 32, r + 64 * 48, (size_t)n_rest * 2);
		r = narrow.data();
	}
	if (d.sh_degree == 0 || L == 0) {
		for (int row = 0; row < 8; ++row) {
			if (d.sh_degree == 0) {
				if (row < 3) { Wr1[row * 32 + 1 + row] = ops.one; Wr1[(8 + row) * 32 + 1 + row] = ops.minus_one; }
			} else {
				for (int k = 0; k < 32; ++k) { Wr1[row * 32 + k] = r[row * 32 + k]; Wr1[(8 + row) * 32 + k] = ops.negate(r[row * 32 + k]); }
			}
			Wr3[row * 64 + row] = ops.one;
			Wr3[row * 64 + 8 + row] = ops.minus_one;
		}
		identity(Wr2);
	} else if (L == 1) {
		memcpy(Wr1, r, 64 * 32 * 2);
		identity(Wr2);
		memcpy(Wr3, r + 64 * 32, 16 * 64 * 2);
	} else if (L == 2) {
		memcpy(Wr1, r, kRgbW * 2);
	} else {
		memcpy(Wr1, r, (64 * 32 + 64 * 64) * 2);
		memcpy(Wr2b, r + 64 * 32 + 64 * 64, 64 * 64 * 2);
		memcpy(Wr3, r + 64 * 32 + 2 * 64 * 64, 16 * 64 * 2);
	}
}
const LowerOps nrs::kLowerValues{0x3C00, 0xBC00, [](uint16_t h) -> uint16_t { return (uint16_t)(h ^ 0x8000u); }};
const LowerOps nrs::kLowerIndices{kFragOne, kFragMinusOne, [](uint16_t i) -> uint16_t { return (uint16_t)(i | kFragNegate); }};

// tcnn GridEncoding level geometry: scale = exp2(l*log2(b))*Nmin - 1, res = ceil(scale)+1,
// entries = min(align8(res^3), 2^log2_T).  tiny-cuda-nn evaluates the scale in FLOAT -- exp2f(level * log2f(per_level_scale)) *
// base_resolution - 1.0f, in the encoding's constructor and again in kernel_grid -- so it is float here too: evaluated in double it can
// land one ulp away, and next to an integer that changes ceil(scale) + 1 and every later level offset (a real checkpoint would be
// mis-addressed).  Host libm stands in for the device's exp2f (<= 2 ulp on NVIDIA hardware: that last bit is outside anyone's control).
uint32_t nrs::make_levels(const nrs_model_desc& d, LevelParams* lv) {
	uint32_t off = 0;
	const float l2 = log2f(d.per_level_scale);
	for (uint32_t l = 0; l < d.n_levels; ++l) {
		LevelParams& p = lv[l];
		p.scale = exp2f((float)l * l2) * (float)d.base_resolution - 1.0f;
		p.resolution = (uint32_t)ceilf(p.scale) + 1u;
		p.res2 = p.resolution * p.resolution;
		uint64_t n = (uint64_t)p.resolution * p.resolution * p.resolution;
		n = (n + 7ull) / 8ull * 8ull;
		p.count = (uint32_t)std::min<uint64_t>(n, 1ull << d.log2_hashmap_size);
		uint64_t stride = 1;
		for (int dim = 0; dim < 3 && stride <= p.count; ++dim) stride *= p.resolution;
		p.hashed = p.count < stride ? 1u : 0u;
		p.mask = p.hashed ? p.count - 1u : 0u;
		p.offset = off;
		p.tab_first = 0;
		p.cached = p.rec_first = p.rec_res = p.rec_res2 = 0;
		off += p.count;
	}
	return off;
}

// Arrange the five row-major fp16 weight matrices (tcnn FullyFusedMLP: [out x in], no biases) as MFMA A operands
// in the order nrs_mlp.cuh consumes them.  For fragment F, lane l = (i = l & 31, g = l >> 5), element e: the weight
// of output unit (32*mb + i) for the input that the B operand's element e of lane-half g carries.
// `one` = what the constant 1.0 is written as: 0x3C00 for real weights, kFragOne when the routine runs on the identity permutation (set_params_device).
void nrs::make_weight_fragments(const uint16_t* w, uint16_t* frag, uint16_t one) {
	const uint16_t* Wd1 = w;                 // [64 x 32]
	const uint16_t* Wd2 = Wd1 + 64 * 32;     // [16 x 64]
	const uint16_t* Wr1 = Wd2 + 16 * 64;     // [64 x 32]
	const uint16_t* Wr2 = Wr1 + 64 * 32;     // [64 x 64]
	const uint16_t* Wr3 = Wr2 + 64 * 64;     // [16 x 64]
	const uint16_t* Wr2b = Wr3 + 16 * 64;    // [64 x 64] (kCanonW: lower_weights' layout)
	const uint16_t* Wr1x = Wr2b + 64 * 64;   // [64 x 16] columns 32..47 of a [64 x 48] first rgb matrix (light directions), else zeros
	auto hidden_row = [](int mb, int g, int r) { return 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * g; }; // D-tile row of reg r
	auto at = [&](int f, int lane, int e) -> uint16_t& { return frag[((size_t)f * 64 + lane) * 8 + e]; };
	memset(frag, 0, kWfragDeviceBytes);
	for (int lane = 0; lane < 64; ++lane) {
		const int i = lane & 31, g = lane >> 5;
		for (int e = 0; e < 8; ++e) {
			// Sel0 / Sel1: row i of the product picks the packed accumulator that came out of D register e (Sel0) / 8 + e (Sel1) of lane-half g
			at(24, lane, e) = i == hidden_row(0, g, e) ? one : (uint16_t)0;
			at(25, lane, e) = i == hidden_row(0, g, 8 + e) ? one : (uint16_t)0;
			// Bwd[ks]: dL/dfeatures[i] = sum_k W1[k][i] dL/dhidden[k] (density MLP, input gradient): output row i = feature i, the B operand of k step ks is
			// the packed dL/dhidden in the layout the hidden layer's D tiles come out in (as for D2)
			for (int ks = 0; ks < 4; ++ks) at(26 + ks, lane, e) = Wd1[hidden_row(ks >> 1, g, 8 * (ks & 1) + e) * 32 + i];
			for (int mb = 0; mb < 2; ++mb)
				for (int ks = 0; ks < 2; ++ks) {
					const int feat = 2 * (2 * (4 * ks + (e >> 1)) + g) + (e & 1); // level 2*it+g, it = 4ks + e/2
					at(mb * 2 + ks, lane, e) = Wd1[(32 * mb + i) * 32 + feat];
				}
			for (int ks = 0; ks < 4; ++ks) {
				const int k = hidden_row(ks >> 1, g, 8 * (ks & 1) + e);
				if (i < 16) at(4 + ks, lane, e) = Wd2[i * 64 + k];
				if (i < 16) at(20 + ks, lane, e) = Wr3[i * 64 + k];
				for (int mb = 0; mb < 2; ++mb) at(12 + mb * 4 + ks, lane, e) = Wr2[(32 * mb + i) * 64 + k];
				for (int mb = 0; mb < 2; ++mb) at(30 + mb * 4 + ks, lane, e) = Wr2b[(32 * mb + i) * 64 + k];
			}
			for (int mb = 0; mb < 2; ++mb) {
				const int kd = (e & 3) + 8 * (e >> 2) + 4 * g; // density-output row in element e
				at(8 + mb * 2 + 0, lane, e) = Wr1[(32 * mb + i) * 32 + kd];
				at(8 + mb * 2 + 1, lane, e) = Wr1[(32 * mb + i) * 32 + 16 + 8 * g + e]; // SH coefficient 8g+e
				at(38 + mb, lane, e) = Wr1x[(32 * mb + i) * 16 + 8 * g + e];            // R1L: light component / padding one 8g+e (rows as in R1)
			}
			// The transposed operands of the backward pass (nrs_network_backward.hip), built as Bwd is: dL/din[32 mb + i] = sum_k W[k][32 mb + i] dL/dout[k], the B operand
			// of k step ks being the packed dL/dout in the layout the D tiles come out in, k = 16 ks + hidden_row(0, g, e).  TD2[mb] (density output layer, 16 outputs: one k
			// step), T1[ks] (rgb layer 0; rows = its 32 inputs), T2[mb][ks], T3[mb] (rgb output layer: rows 0..2 only -- extract_rgb copies three rows, the padding rows' weights
			// must not meet anything).
			const int k0 = hidden_row(0, g, e);
			for (int mb = 0; mb < 2; ++mb) {
				at(40 + mb, lane, e) = Wd2[k0 * 64 + 32 * mb + i];
				at(54 + mb, lane, e) = k0 < 3 ? Wr3[k0 * 64 + 32 * mb + i] : (uint16_t)0;
				for (int ks = 0; ks < 4; ++ks) at(46 + mb * 4 + ks, lane, e) = Wr2[(16 * ks + k0) * 64 + 32 * mb + i];
			}
			for (int ks = 0; ks < 4; ++ks) at(42 + ks, lane, e) = Wr1[(16 * ks + k0) * 32 + i];
		}
	}
}

extern "C" {

size_t nrs_model_n_params(const nrs_model_desc* d) {
	if (!d || !desc_supported(*d)) return 0;
	LevelParams lv[kLevels];
	return (size_t)n_mlp_weights(*d) + (size_t)make_levels(*d, lv) * 2;
}
int nrs_model_level_table(const nrs_model_desc* d, float* scale, uint32_t* resolution, uint32_t* entry_offset, uint32_t* entry_count,
                          uint32_t* hashed) {
	if (!d || !desc_supported(*d)) return fail(NRS_ERR_UNSUPPORTED, "model description outside configs/nerf/base.json's family (hash grid 16 x 2, 64-wide density network of 0..1 hidden layers, rgb network of 0..3 hidden layers or none)");
	LevelParams lv[kLevels];
	make_levels(*d, lv);
	for (uint32_t l = 0; l < d->n_levels; ++l) {
		if (scale) scale[l] = lv[l].scale;
		if (resolution) resolution[l] = lv[l].resolution;
		if (entry_offset) entry_offset[l] = lv[l].offset;
		if (entry_count) entry_count[l] = lv[l].count;
		if (hashed) hashed[l] = lv[l].hashed;
	}
	return NRS_OK;
}

size_t nrs_model_n_params_ex(const nrs_model_desc* d, uint32_t n_extra_dims) {
	if (!d || !desc_supported(*d) || (n_extra_dims != 0u && n_extra_dims != 3u) || extra_dims_refusal(*d, n_extra_dims)) return 0;
	return nrs_model_n_params(d) + (n_extra_dims ? 64u * 16u : 0u);
}

} // extern "C"
