// nrs_mlp.cuh -- fused MLPs on MFMA for one wavefront (gfx950), fed by the hash-grid gather of nrs_hashgrid.cuh.
//
// Replaces tiny-cuda-nn's kernel_grid + 2x kernel_mlp_fused + SH encoding + extract_density with one
// on-chip pipeline.  A wave owns 64 samples, processed as two 32-sample MFMA column blocks:
//
//   block b holds the samples of lanes 32b..32b+31.  Every lane gathers the 16 hash-grid levels of its OWN sample, two levels per
//   iteration (level parameters wave-uniform, in scalar registers), and writes them into the per-wave LDS slab in the order the
//   MFMA B operands want: lane l = (j = l & 31, g = l >> 5) supplies, for sample j of each block, the levels 2*it + g (it = 0..7)
//   and the SH coefficients 8g..8g+7.
//
// Every layer is computed transposed, H^T[unit][sample] = W[unit][k] * X^T[k][sample], with
// v_mfma_f32_32x32x16_f16: A = a 32x16 weight tile (LDS, pre-arranged on the host), B = 16 x 32 samples.  The D tile of
// one layer (lane = sample column, 16 rows per lane) is, after ReLU + fp16 rounding, directly the B operand of the next
// layer: the k index of an MFMA is free as long as A and B agree, so the host arranges the weight tiles in the order the
// D registers come out (make_weight_fragments in nrs_api_lowering.cpp).  No cross-lane shuffles between layers, no global
// intermediates.  The gathered features pass through a 4 KiB per-wave LDS slab only because the level loop is kept
// rolled (small code, few live registers, which buys occupancy for the gather latency).
//
// Numerics (stated; parity at the tcnn boundary is unpinned): grid entries fp16, trilinear sum in fp32 via
// fmaf in corner order 0..7, rounded to fp16; MLP products fp16 x fp16 accumulated in fp32 by the MFMA, ReLU, rounded to
// fp16 between layers; outputs rounded to fp16.
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_internal.h"
#include "nrs_route.h"
#include "nrs_vec.cuh"
#include "nrs_hashgrid.cuh"

namespace nrs {

// fragment indices inside the LDS weight image
#define NRS_FRAG_D1(mb, ks) ((mb) * 2 + (ks))
#define NRS_FRAG_D2(ks) (4 + (ks))
#define NRS_FRAG_R1(mb, ks) (8 + (mb) * 2 + (ks))
#define NRS_FRAG_R2(mb, ks) (12 + (mb) * 4 + (ks))
#define NRS_FRAG_R3(ks) (20 + (ks))
#define NRS_FRAG_R2B(mb, ks) (30 + (mb) * 4 + (ks)) // (HBM only, like NRS_FRAG_BWD: the third rgb hidden layer of base_3layer.json)
#define NRS_FRAG_R1L(mb) (38 + (mb)) // (HBM only: the third k block of rgb layer 0 of a network trained with light directions, n_extra_dims = 3)
// (HBM only, staged by the backward kernel: the transposed matrices, k = the D-tile row order -- make_weight_fragments)
#define NRS_FRAG_TD2(mb) (40 + (mb))
#define NRS_FRAG_T1(ks) (42 + (ks))
#define NRS_FRAG_T2(mb, ks) (46 + (mb) * 4 + (ks))
#define NRS_FRAG_T3(mb) (54 + (mb))

// B operand of block b for k-step ks: levels it = 4ks..4ks+3 of sample (b, j) as this lane gathered them
__device__ __forceinline__ half8 load_features(const FeatLds& fl, int lane, int sel, int ks) {
	u32x4 v;
	v[0] = fl.feat[4 * ks + 0][sel][lane];
	v[1] = fl.feat[4 * ks + 1][sel][lane];
	v[2] = fl.feat[4 * ks + 2][sel][lane];
	v[3] = fl.feat[4 * ks + 3][sel][lane];
	return __builtin_bit_cast(half8, v);
}

// SH degree 4 (tcnn SphericalHarmonics) of a direction given as (d+1)/2: the 8 coefficients 8g..8g+7 this lane owns.
__device__ __forceinline__ half8 encode_sh4(int g, f3 dir01) {
	float x = dir01.x * 2.f - 1.f, y = dir01.y * 2.f - 1.f, z = dir01.z * 2.f - 1.f;
	float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
	float o[8];
	if (g == 0) {
		o[0] = 0.28209479177387814f;
		o[1] = -0.48860251190291987f * y;
		o[2] = 0.48860251190291987f * z;
		o[3] = -0.48860251190291987f * x;
		o[4] = 1.0925484305920792f * xy;
		o[5] = -1.0925484305920792f * yz;
		o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
		o[7] = -1.0925484305920792f * xz;
	} else {
		o[0] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
		o[1] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
		o[2] = 2.8906114426405538f * xy * z;
		o[3] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
		o[4] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
		o[5] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
		o[6] = 1.4453057213202769f * z * (x2 - y2);
		o[7] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
	}
	half8 r;
	#pragma unroll
	for (int e = 0; e < 8; ++e) r[e] = (_Float16)o[e];
	return r;
}

// The same for two directions (the lane's own sample and its partner's) in packed fp32: every product and sum is the scalar
// one (+1.7 % on the bench).  The same treatment of the trilinear weights measured -11 %, of the cell coordinates 0.
__device__ __forceinline__ void encode_sh4_2(int g, f3 dirA, f3 dirB, half8& outA, half8& outB) {
	const f2 two = {2.f, 2.f}, one = {1.f, 1.f};
	const f2 x = (f2){dirA.x, dirB.x} * two - one, y = (f2){dirA.y, dirB.y} * two - one, z = (f2){dirA.z, dirB.z} * two - one;
	const f2 xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
	f2 o[8];
	if (g == 0) {
		o[0] = (f2){0.28209479177387814f, 0.28209479177387814f};
		o[1] = -0.48860251190291987f * y;
		o[2] = 0.48860251190291987f * z;
		o[3] = -0.48860251190291987f * x;
		o[4] = 1.0925484305920792f * xy;
		o[5] = -1.0925484305920792f * yz;
		o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
		o[7] = -1.0925484305920792f * xz;
	} else {
		o[0] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
		o[1] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
		o[2] = 2.8906114426405538f * xy * z;
		o[3] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
		o[4] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
		o[5] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
		o[6] = 1.4453057213202769f * z * (x2 - y2);
		o[7] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
	}
	#pragma unroll
	for (int e = 0; e < 8; ++e) { outA[e] = (_Float16)o[e].x; outB[e] = (_Float16)o[e].y; }
}

// ReLU + fp16 rounding of 8 accumulator rows.  max(round(x), 0) == round(max(x, 0)); done on packed halfs.
__device__ __forceinline__ half8 relu_pack(const floatx16& d, int base) {
	half8 r;
	#pragma unroll
	for (int e = 0; e < 8; ++e) r[e] = (_Float16)d[base + e];
	const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
	return __builtin_elementwise_max(r, zero);
}
__device__ __forceinline__ half8 pack(const floatx16& d, int base) {
	half8 r;
	#pragma unroll
	for (int e = 0; e < 8; ++e) r[e] = (_Float16)d[base + e];
	return r;
}
__device__ __forceinline__ floatx16 zero16() {
	floatx16 z;
	#pragma unroll
	for (int i = 0; i < 16; ++i) z[i] = 0.f;
	return z;
}

#define NRS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#define NRS_FRAG_SEL(h) (24 + (h))
#define NRS_FRAG_BWD(ks) (26 + (ks)) // (HBM only: DeviceModel::wfrag + ...; see nrs_internal.h)
// ACC16 (nrs_mlp_acc FP16): the running sums are rounded to fp16 after every 16-wide k step, the model of tiny-cuda-nn's fp16 accumulator fragments.
// (round 4) the rounded sums go back into the accumulator registers THROUGH THE MATRIX CORE -- pack to fp16 (8 v_cvt_pk_f16_f32: the
// rounding), then MFMA(Sel0, lo, 0) and MFMA(Sel1, hi, .) with the two constant 0 / 1 fragments, which reproduce the packed values exactly in fp32
// (1.0 x h summed with zeros) in the D layout -- and the k step's own MFMA accumulates on top as before.  8 VALU slots per rounding instead of 24-32 on a
// kernel that is VALU-bound (the packed-conversion round trip on the vector pipe: profiles/r04/ab_numerics_variants.txt), paid with two issues on a pipe
// that is 10 % busy; same values (tests/test_gpu_numerics.py).
template <bool ACC16>
__device__ __forceinline__ floatx16 mfma_step(const half8* lds_w, int lane, half8 a, half8 b, floatx16 c) {
	if (ACC16) {
		half8 lo, hi;
		#pragma unroll
		for (int e = 0; e < 8; ++e) { lo[e] = (_Float16)c[e]; hi[e] = (_Float16)c[8 + e]; }
		floatx16 z;
		#pragma unroll
		for (int i = 0; i < 16; ++i) z[i] = 0.f;
		__builtin_amdgcn_sched_barrier(0); // (keeps the selection fragments' LDS reads of later steps from being hoisted over this one: registers)
		c = NRS_MFMA(lds_w[NRS_FRAG_SEL(0) * 64 + lane], lo, z);
		c = NRS_MFMA(lds_w[NRS_FRAG_SEL(1) * 64 + lane], hi, c);
	}
	return NRS_MFMA(a, b, c);
}
// the first k step of a layer: nothing to round yet
__device__ __forceinline__ floatx16 mfma_first(half8 a, half8 b) {
	floatx16 z;
	#pragma unroll
	for (int i = 0; i < 16; ++i) z[i] = 0.f;
	return NRS_MFMA(a, b, z);
}
// Scheduling fence between MLP stages: without it hipcc hoists all 24 weight-fragment LDS reads (96 VGPRs) to the top of
// the MLP, which costs a wave of occupancy.  The gather, not the MLP, is the phase that needs the latency hiding.
#define NRS_STAGE_FENCE() __builtin_amdgcn_sched_barrier(0)

// The layers of the two MLPs for one 32-sample block, each stated once: the inference kernels, the introspection operators and the backward kernel's forward
// pass all run these.  A layer's packed outputs are the B operands of the next: element e of lane (j, g) = output row (e&3) + 8*(e>>2) + 4g of its 32-row tile.
// Density hidden layer 32 -> 64 (ReLU).  x0/x1: features (k-steps 0/1); p0..p3: hidden rows 0..31 then 32..63, each tile reduced to its two packed operands
// before the next accumulator is started.
// (ACC16: mfma_step rounds the sum it is handed before it adds its own k step; the last sum of a layer is rounded by relu_pack / pack themselves)
template <bool ACC16>
__device__ __forceinline__ void density_hidden(const half8* lds_w, int lane, half8 x0, half8 x1, half8& p0, half8& p1, half8& p2, half8& p3) {
	floatx16 h = mfma_first(lds_w[NRS_FRAG_D1(0, 0) * 64 + lane], x0);
	h = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D1(0, 1) * 64 + lane], x1, h);
	p0 = relu_pack(h, 0); p1 = relu_pack(h, 8);
	NRS_STAGE_FENCE();
	h = mfma_first(lds_w[NRS_FRAG_D1(1, 0) * 64 + lane], x0);
	h = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D1(1, 1) * 64 + lane], x1, h);
	p2 = relu_pack(h, 0); p3 = relu_pack(h, 8);
	NRS_STAGE_FENCE();
}
// Density output layer 64 -> 16 (no activation).
template <bool ACC16>
__device__ __forceinline__ half8 density_output(const half8* lds_w, int lane, half8 p0, half8 p1, half8 p2, half8 p3) {
	floatx16 o = mfma_first(lds_w[NRS_FRAG_D2(0) * 64 + lane], p0);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D2(1) * 64 + lane], p1, o);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D2(2) * 64 + lane], p2, o);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D2(3) * 64 + lane], p3, o);
	NRS_STAGE_FENCE();
	return pack(o, 0);
}
// Density MLP 32 -> 64 (ReLU) -> 16: the fp16-rounded outputs, the rgb MLP's first B operand.
template <bool ACC16 = false>
__device__ __forceinline__ half8 density_mlp(const half8* lds_w, int lane, half8 x0, half8 x1) {
	half8 p0, p1, p2, p3;
	density_hidden<ACC16>(lds_w, lane, x0, x1, p0, p1, p2, p3);
	return density_output<ACC16>(lds_w, lane, p0, p1, p2, p3);
}

// One 64 -> 64 ReLU layer of the rgb MLP whose fragments `w` (8: [mb][ks]) may live in LDS or in HBM: b0..b3 in, the packed B operands of the next layer out.
template <bool ACC16>
__device__ __forceinline__ void hidden_layer_64(const half8* lds_w, const half8* w, int lane, half8& b0, half8& b1, half8& b2, half8& b3) {
	floatx16 c = mfma_first(w[0 * 64 + lane], b0);
	c = mfma_step<ACC16>(lds_w, lane, w[1 * 64 + lane], b1, c);
	c = mfma_step<ACC16>(lds_w, lane, w[2 * 64 + lane], b2, c);
	c = mfma_step<ACC16>(lds_w, lane, w[3 * 64 + lane], b3, c);
	const half8 q0 = relu_pack(c, 0), q1 = relu_pack(c, 8);
	NRS_STAGE_FENCE();
	c = mfma_first(w[4 * 64 + lane], b0);
	c = mfma_step<ACC16>(lds_w, lane, w[5 * 64 + lane], b1, c);
	c = mfma_step<ACC16>(lds_w, lane, w[6 * 64 + lane], b2, c);
	c = mfma_step<ACC16>(lds_w, lane, w[7 * 64 + lane], b3, c);
	const half8 q2 = relu_pack(c, 0), q3 = relu_pack(c, 8);
	NRS_STAGE_FENCE();
	b0 = q0; b1 = q1; b2 = q2; b3 = q3;
}
// RGB MLP [density out 16 | SH 16] -> 64 -> 64 -> 16 (3 used) for one block.  Same output row map.
// DEEP instantiations take `deep_w` (wave-uniform; DeviceModel::wfrag when DeviceModel::rgb_deep, else null): a third hidden layer between the second and the
// output layer, its fragments read from HBM (base_3layer.json; the other members of the family are lowered onto the two-layer shape, nrs_api_lowering.cpp lower_weights).
// LIGHT instantiations take `light_w` (wave-uniform; DeviceModel::wfrag when DeviceModel::n_extra_dims, else null) and `lb`: a network trained with light
// directions has a 48-wide input -- [density out 16 | SH 16 | Identity(light 3) padded with ones to 16] -- i.e. one more k step in layer 0 (25 MFMA issues per
// block instead of 24), k order density, SH, light; its two A fragments R1L are read from HBM like the DEEP ones.  The instantiations without the flag are what
// they were before it existed.
// B operand of that k step (k = 8 (lane >> 5) + e): lanes 0..31 hold the warped light direction of sample column j, rounded to fp16 by the Identity encoding
// (scale 1, offset 0), and five of the thirteen padding ones; lanes 32..63 the other eight.
__device__ __forceinline__ half8 light_operand(int g, float l0, float l1, float l2) {
	const _Float16 one = (_Float16)1.0f;
	half8 r = {one, one, one, one, one, one, one, one};
	if (g == 0) { r[0] = (_Float16)l0; r[1] = (_Float16)l1; r[2] = (_Float16)l2; }
	return r;
}
template <bool ACC16, bool LIGHT>
__device__ __forceinline__ floatx16 rgb_layer0_tile(const half8* lds_w, int lane, int mb, half8 din, half8 sh, const half8* light_w, half8 lb) {
	floatx16 a = mfma_first(lds_w[NRS_FRAG_R1(mb, 0) * 64 + lane], din);
	a = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_R1(mb, 1) * 64 + lane], sh, a);
	if (LIGHT && light_w) a = mfma_step<ACC16>(lds_w, lane, light_w[NRS_FRAG_R1L(mb) * 64 + lane], lb, a);
	return a;
}
// rgb layer 0 (32 or 48 -> 64, ReLU): b0..b3 as density_hidden's p0..p3
template <bool ACC16, bool LIGHT>
__device__ __forceinline__ void rgb_hidden0(const half8* lds_w, int lane, half8 din, half8 sh, const half8* light_w, half8 lb, half8& b0, half8& b1, half8& b2, half8& b3) {
	floatx16 a = rgb_layer0_tile<ACC16, LIGHT>(lds_w, lane, 0, din, sh, light_w, lb);
	b0 = relu_pack(a, 0); b1 = relu_pack(a, 8);
	NRS_STAGE_FENCE();
	a = rgb_layer0_tile<ACC16, LIGHT>(lds_w, lane, 1, din, sh, light_w, lb);
	b2 = relu_pack(a, 0); b3 = relu_pack(a, 8);
	NRS_STAGE_FENCE();
}
template <bool ACC16 = false, bool DEEP = false, bool LIGHT = false>
__device__ __forceinline__ half8 rgb_mlp(const half8* lds_w, int lane, half8 din, half8 sh, const half8* deep_w = nullptr, const half8* light_w = nullptr, half8 lb = half8{}) {
	half8 b0, b1, b2, b3;
	rgb_hidden0<ACC16, LIGHT>(lds_w, lane, din, sh, light_w, lb, b0, b1, b2, b3);
	hidden_layer_64<ACC16>(lds_w, lds_w + NRS_FRAG_R2(0, 0) * 64, lane, b0, b1, b2, b3);
	if (DEEP && deep_w) hidden_layer_64<ACC16>(lds_w, deep_w + NRS_FRAG_R2B(0, 0) * 64, lane, b0, b1, b2, b3);
	floatx16 o = mfma_first(lds_w[NRS_FRAG_R3(0) * 64 + lane], b0);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_R3(1) * 64 + lane], b1, o);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_R3(2) * 64 + lane], b2, o);
	o = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_R3(3) * 64 + lane], b3, o);
	NRS_STAGE_FENCE();
	return pack(o, 0);
}

// ---- network introspection: the pieces of wave_visualize_activation / wave_density_input_gradient below ------------------------------------------
// tiny-cuda-nn's visualize_activation / input_gradient as restated in oracle/nrs_oracle.cpp (network_activation_one, density_input_gradient_one).
// register r (wave-uniform) of a D tile
__device__ __forceinline__ float pick16(const floatx16& d, int r) {
	float v = d[0];
	#pragma unroll
	for (int i = 1; i < 16; ++i) v = (r == i) ? d[i] : v;
	return v;
}
__device__ __forceinline__ _Float16 pick8(const half8& h, int e) {
	_Float16 v = h[0];
	#pragma unroll
	for (int i = 1; i < 8; ++i) v = (e == i) ? h[i] : v;
	return v;
}
// Activation `unit` of hidden layer `layer` (1: density MLP hidden, 3 / 4 / 5: rgb MLP hidden 1 / 2 / 3 -- 5 with deep_w only) for one 32-sample block: the value of sample column j sits,
// after the call, in the lanes whose half (lane >> 5) equals tile_half(unit); the other half returns another row.  din = density_mlp's output (layers 3, 4).
__device__ __forceinline__ int tile_half(uint32_t unit) { return (int)((unit >> 2) & 1u); }
// (LIGHT, light_w, lb: as for rgb_mlp)
template <bool ACC16, bool LIGHT = false>
__device__ __forceinline__ float mlp_hidden_activation(const half8* lds_w, int lane, half8 x0, half8 x1, half8 din, half8 sh, uint32_t layer, uint32_t unit, const half8* deep_w = nullptr,
                                                       const half8* light_w = nullptr, half8 lb = half8{}) {
	const int mb = (int)((unit >> 5) & 1u), R = (int)(unit & 31u), r = (R & 3) + 4 * (R >> 3); // D register of row R in its lane half
	floatx16 t;
	if (layer == 1u) {
		t = mfma_first(lds_w[NRS_FRAG_D1(mb, 0) * 64 + lane], x0);
		t = mfma_step<ACC16>(lds_w, lane, lds_w[NRS_FRAG_D1(mb, 1) * 64 + lane], x1, t);
	} else if (layer == 3u) {
		t = rgb_layer0_tile<ACC16, LIGHT>(lds_w, lane, mb, din, sh, light_w, lb);
	} else {
		half8 b0, b1, b2, b3;
		rgb_hidden0<ACC16, LIGHT>(lds_w, lane, din, sh, light_w, lb, b0, b1, b2, b3);
		const half8* w = lds_w + NRS_FRAG_R2(mb, 0) * 64;
		if (layer == 5u && deep_w) { // the third hidden layer: behind the whole second one
			hidden_layer_64<ACC16>(lds_w, lds_w + NRS_FRAG_R2(0, 0) * 64, lane, b0, b1, b2, b3);
			w = deep_w + NRS_FRAG_R2B(mb, 0) * 64;
		}
		t = mfma_first(w[0 * 64 + lane], b0);
		t = mfma_step<ACC16>(lds_w, lane, w[1 * 64 + lane], b1, t);
		t = mfma_step<ACC16>(lds_w, lane, w[2 * 64 + lane], b2, t);
		t = mfma_step<ACC16>(lds_w, lane, w[3 * 64 + lane], b3, t);
	}
	NRS_STAGE_FENCE();
	const _Float16 h = (_Float16)pick16(t, r);
	return (float)(h > (_Float16)0 ? h : (_Float16)0); // the stored activation: ReLU, fp16
}
// Backward of 128 * e_0 through the density MLP for one 32-sample block (input_gradient(stream, 3, ...): the one-hot lands on the density network's output
// row 0, nerf_network_full.h:188-195): dL/dhidden[k] = (hidden[k] > 0) * fp16(W2[0][k] * 128) in the layout of the hidden tiles, then
// dL/dfeatures = W1^T dL/dhidden on MFMA (A operands Bwd[ks] from HBM: DeviceModel::wfrag), accumulated as the forward pass is (ACC16).
// out[q] = features (2 L, 2 L + 1) packed, L = level_of_pair(q, lane >> 5), of sample column j.
__device__ __forceinline__ int level_of_pair(int q, int gg) { const int r = 2 * q; return ((r & 3) + 8 * (r >> 2) + 4 * gg) >> 1; }
template <bool ACC16>
__device__ __forceinline__ void density_backward_features(const half8* lds_w, const half8* __restrict__ gfrag, int lane, half8 x0, half8 x1, uint32_t out[8]) {
	half8 p0, p1, p2, p3;
	density_hidden<ACC16>(lds_w, lane, x0, x1, p0, p1, p2, p3);
	// W2[0][k] for the k's this lane's hidden registers stand for: what lane (0, lane >> 5) of the D2 fragments holds (output row 0)
	const int row0 = lane & 32;
	auto dhidden = [&](const half8& p, int ks) {
		const half8 w = lds_w[NRS_FRAG_D2(ks) * 64 + row0];
		half8 q;
		#pragma unroll
		for (int e = 0; e < 8; ++e) q[e] = p[e] > (_Float16)0 ? (_Float16)(w[e] * (_Float16)128) : (_Float16)0; // x 128 in fp16: the same value as fp16(float(w) * 128)
		return q;
	};
	const half8 q0 = dhidden(p0, 0), q1 = dhidden(p1, 1), q2 = dhidden(p2, 2), q3 = dhidden(p3, 3);
	NRS_STAGE_FENCE();
	floatx16 d = mfma_first(gfrag[NRS_FRAG_BWD(0) * 64 + lane], q0);
	d = mfma_step<ACC16>(lds_w, lane, gfrag[NRS_FRAG_BWD(1) * 64 + lane], q1, d);
	d = mfma_step<ACC16>(lds_w, lane, gfrag[NRS_FRAG_BWD(2) * 64 + lane], q2, d);
	d = mfma_step<ACC16>(lds_w, lane, gfrag[NRS_FRAG_BWD(3) * 64 + lane], q3, d);
	NRS_STAGE_FENCE();
	#pragma unroll
	for (int q = 0; q < 8; ++q) {
		half2v pr = {(_Float16)d[2 * q], (_Float16)d[2 * q + 1]};
		out[q] = __builtin_bit_cast(uint32_t, pr);
	}
}

// tiny-cuda-nn's roundings as a template value: NUM >= 0 fixes them at compile time (bit 0 grid accumulation in network precision, bit 1 fp16 MLP
// accumulators), kNumRuntime reads them from `nm` (DeviceModel::numerics, wave-uniform) -- both flavours compiled in, one scalar branch.
template <int NUM>
__device__ __forceinline__ half8 density_mlp_num(uint32_t nm, const half8* lds_w, int lane, half8 x0, half8 x1) {
	if (NUM == kNumRuntime ? (nm & 2u) != 0u : (NUM & 2) != 0) return density_mlp<true>(lds_w, lane, x0, x1);
	return density_mlp<false>(lds_w, lane, x0, x1);
}
template <int NUM, bool DEEP = false, bool LIGHT = false>
__device__ __forceinline__ half8 rgb_mlp_num(uint32_t nm, const half8* lds_w, int lane, half8 din, half8 sh, const half8* deep_w = nullptr, const half8* light_w = nullptr, half8 lb = half8{}) {
	if (NUM == kNumRuntime ? (nm & 2u) != 0u : (NUM & 2) != 0) return rgb_mlp<true, DEEP, LIGHT>(lds_w, lane, din, sh, deep_w, light_w, lb);
	return rgb_mlp<false, DEEP, LIGHT>(lds_w, lane, din, sh, deep_w, light_w, lb);
}
template <int NUM, bool LIGHT>
__device__ __forceinline__ float mlp_hidden_activation_num(uint32_t nm, const half8* lds_w, int lane, half8 x0, half8 x1, half8 din, half8 sh, uint32_t layer, uint32_t unit, const half8* deep_w,
                                                           const half8* light_w, half8 lb) {
	if (NUM == kNumRuntime ? (nm & 2u) != 0u : (NUM & 2) != 0) return mlp_hidden_activation<true, LIGHT>(lds_w, lane, x0, x1, din, sh, layer, unit, deep_w, light_w, lb);
	return mlp_hidden_activation<false, LIGHT>(lds_w, lane, x0, x1, din, sh, layer, unit, deep_w, light_w, lb);
}
template <int NUM>
__device__ __forceinline__ void density_backward_features_num(uint32_t nm, const half8* lds_w, const half8* __restrict__ gfrag, int lane, half8 x0, half8 x1, uint32_t out[8]) {
	if (NUM == kNumRuntime ? (nm & 2u) != 0u : (NUM & 2) != 0) density_backward_features<true>(lds_w, gfrag, lane, x0, x1, out);
	else density_backward_features<false>(lds_w, gfrag, lane, x0, x1, out);
}

// Exchange a value with the partner lane (l ^ 32): one ds_bpermute.
__device__ __forceinline__ float xchg32(float v) { return __shfl_xor(v, 32, 64); }
__device__ __forceinline__ uint32_t xchg32u(uint32_t v) { return (uint32_t)__shfl_xor((int)v, 32, 64); }

// ---- the two introspection operators for a wave's 64 samples whose features encode_to_lds has left in `fl`: network_kernel's kNetVisualizeActivation /
// kNetInputGradient and render_body's INTRO block (EncodingVis / Normals).  The callers differ in where the operands come from, never in what is done with them.
// network.visualize_activation(stream, layer, dim, ...): unit `dim` of forward_activations(layer) of the lane's own sample.  sh_own / sh_par, lb_own / lb_par: the SH
// coefficients and the light operand (rgb_mlp) of the lane's own sample and of its partner's (lane ^ 32); light: the own sample's warped light direction;
// NUM, nm: as for density_mlp_num.
template <int NUM, bool LIGHT>
__device__ __forceinline__ float wave_visualize_activation(uint32_t nm, const FeatLds& fl, const half8* lds_w, int lane, uint32_t layer, uint32_t dim, half8 sh_own, half8 sh_par, const half8* deep_w,
                                                           const half8* light_w, half8 lb_own, half8 lb_par, f3 light) {
	const int g = lane >> 5;
	float v = 0.f;
	if (layer == 0u) { // the hash-grid output: the slab holds level L of the own sample (see encode_to_lds)
		const uint32_t L = dim >> 1;
		const uint32_t w = ((L & 1u) == (uint32_t)g) ? fl.feat[L >> 1][0][lane] : fl.feat[L >> 1][1][lane ^ 32];
		v = (float)__builtin_bit_cast(half2v, w)[dim & 1u];
	} else if (LIGHT && layer == 2u && dim >= 32u) { // the Identity encoding of the light direction (units 32..34) and its padding ones
		const float l = dim == 32u ? light.x : (dim == 33u ? light.y : light.z);
		v = dim < 35u ? (float)(_Float16)l : 1.0f;
	} else if (layer == 2u && dim >= 16u) { // an SH coefficient of the own direction: 8 g .. 8 g + 7 are here, the others in the partner lane's sh_par
		const uint32_t cidx = dim - 16u;
		const float mine = (float)pick8(sh_own, (int)(cidx & 7u)), theirs = xchg32((float)pick8(sh_par, (int)(cidx & 7u)));
		v = ((cidx >> 3) == (uint32_t)g) ? mine : theirs;
	} else {
		#pragma unroll 1
		for (int b = 0; b < 2; ++b) {
			const int sel = (b != g) ? 1 : 0;
			const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
			float val;
			int half_of_row;
			if (layer == 2u) { // a density-MLP output (rows 0..15 of the rgb network's input)
				const half8 dout = density_mlp_num<NUM>(nm, lds_w, lane, x0, x1);
				val = (float)pick8(dout, (int)((dim & 3u) + 4u * (dim >> 3))); // element of row dim: row = (e & 3) + 8 (e >> 2) + 4 half
				half_of_row = (int)((dim >> 2) & 1u);
			} else {
				half8 din = x0;
				if (layer >= 3u) din = density_mlp_num<NUM>(nm, lds_w, lane, x0, x1);
				val = mlp_hidden_activation_num<NUM, LIGHT>(nm, lds_w, lane, x0, x1, din, sel ? sh_par : sh_own, layer, dim, deep_w, light_w, sel ? lb_par : lb_own);
				half_of_row = tile_half(dim);
			}
			// the value of sample (b, j) sits in lane j + 32 * half_of_row; its sample's lane is j + 32 * b
			if (half_of_row != b) val = xchg32(val);
			if (g == b) v = val;
		}
	}
	return v;
}
// network.input_gradient(stream, 3, positions, gradients): d density_raw / d warped position of the lane's own sample at `pos` -- backward of 128 e_0 through the
// density MLP (density_backward_features), the hash grid's input gradient level by level, then the 1 / 128.  Overwrites the feature slab with dL/dfeatures.
template <int NUM>
__device__ __forceinline__ f3 wave_density_input_gradient(uint32_t nm, FeatLds& fl, const half8* lds_w, const half8* __restrict__ gfrag, const GridView& gv, const LevelParams* levels, int lane, f3 pos) {
	const int g = lane >> 5;
	uint32_t dfe[2][8];
	#pragma unroll
	for (int b = 0; b < 2; ++b) { // (unrolled: dfe must stay in registers)
		const int sel = (b != g) ? 1 : 0;
		density_backward_features_num<NUM>(nm, lds_w, gfrag, lane, load_features(fl, lane, sel, 0), load_features(fl, lane, sel, 1), dfe[b]);
	}
	// dL/dfeatures of sample (b, j) -> the slab, G[L][lane j + 32 b] (both lane halves of a column hold 8 of its 16 level pairs)
	__builtin_amdgcn_wave_barrier();
	uint32_t* G = &fl.feat[0][0][0];
	#pragma unroll
	for (int b = 0; b < 2; ++b)
		#pragma unroll
		for (int q = 0; q < 8; ++q) G[level_of_pair(q, g) * 64 + (lane & 31) + 32 * b] = dfe[b][q];
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	float res[3] = {0.f, 0.f, 0.f};
	#pragma unroll 1
	for (int L = 0; L < (int)kLevels; ++L) level_input_gradient(gv, levels[L], pos, G[L * 64 + lane], res);
	__builtin_amdgcn_wave_barrier();
	return mk3(res[0] * (1.0f / 128.0f), res[1] * (1.0f / 128.0f), res[2] * (1.0f / 128.0f));
}

// The two-block evaluation: the wave's 64 samples (features in `fl`) go through the MLPs as two 32-sample blocks; block b's samples belong to the lanes of half b,
// its rows 0..2 sit in its lanes 0..31.  Returns the lane's own sample as packed raw fp16 pairs.
struct NetRaw { uint32_t d, rg, b; }; // (density row 0, .), (r, g), (b, .)
// the density MLP alone: NetRaw::d
template <int NUM>
__device__ __forceinline__ uint32_t wave_density(uint32_t nm, const FeatLds& fl, const half8* lds_w, int lane) {
	const int g = lane >> 5;
	uint32_t res_d = 0;
	#pragma unroll 1
	for (int b = 0; b < 2; ++b) {
		const int sel = (b != g) ? 1 : 0;
		const half8 dout = density_mlp_num<NUM>(nm, lds_w, lane, load_features(fl, lane, sel, 0), load_features(fl, lane, sel, 1));
		uint32_t vd = __builtin_bit_cast(u32x4, dout)[0];
		if (b == 1) vd = xchg32u(vd);
		if (g == b) res_d = vd;
	}
	return res_d;
}
// (sh_own / sh_par: the SH coefficients of the lane's own sample and of its partner's; deep_w, light_w, lb: as for rgb_mlp -- both wave-uniform branches compiled
// in -- the same for every sample)
template <int NUM>
__device__ __forceinline__ NetRaw wave_network(uint32_t nm, const FeatLds& fl, const half8* lds_w, int lane, half8 sh_own, half8 sh_par, const half8* deep_w, const half8* light_w, half8 lb) {
	const int g = lane >> 5;
	NetRaw r = {0, 0, 0};
	#pragma unroll 1
	for (int b = 0; b < 2; ++b) {
		const int sel = (b != g) ? 1 : 0;
		const half8 x0 = load_features(fl, lane, sel, 0), x1 = load_features(fl, lane, sel, 1);
		const half8 dout = density_mlp_num<NUM>(nm, lds_w, lane, x0, x1);
		const half8 rout = rgb_mlp_num<NUM, true, true>(nm, lds_w, lane, dout, sel ? sh_par : sh_own, deep_w, light_w, lb);
		const u32x4 dd = __builtin_bit_cast(u32x4, dout), rr = __builtin_bit_cast(u32x4, rout);
		uint32_t vd = dd[0], vrg = rr[0], vb = rr[1];
		if (b == 1) { vd = xchg32u(vd); vrg = xchg32u(vrg); vb = xchg32u(vb); }
		if (g == b) { r.d = vd; r.rg = vrg; r.b = vb; }
	}
	return r;
}

// per-workgroup LDS of the kernels that run the network on caller batches: the weights + one feature slab per wave
template <int WAVES>
struct NetSmemT {
	ModelLds ml;
	FeatLds fl[WAVES];
};
typedef NetSmemT<4> NetSmem;

} // namespace nrs
