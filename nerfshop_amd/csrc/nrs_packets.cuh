// nrs_packets.cuh -- packet geometry of a render launch: which pixel a lane of a packet stands on and where that pixel lands in the
// caller's buffers.  Shared by render_body (nrs_render.cuh) and slice_kernel (nrs_network.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "nrs_render.h"

namespace nrs {

// packet -> pixel of this lane.  Packets are 8x8 pixel blocks; with lane teams (TEAM lanes per ray) a packet is the 64 / TEAM
// pixels of an 8x4 / 4x4 block and the TEAM lanes of a team stand on the same pixel.
template <int TEAM>
__device__ __forceinline__ bool packet_pixel(const RenderArgs& a, uint32_t pk, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	constexpr uint32_t PW = TEAM >= 16 ? 2u : (TEAM >= 4 ? 4u : 8u), PH = 64u / TEAM / PW; // 8x8, 8x4, 4x4, 4x2, 2x2
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	const uint32_t idx = (uint32_t)lane / TEAM;
	const uint32_t lx = idx % PW, ly = idx / PW;
	if (a.p.tile_size == 0) {
		// whole image: packets in row-major order (runs of neighbouring packets per claim were measured and lose: a wave's
		// unstarted packets are invisible to idle waves)
		// (packet rows from the middle of the image outwards -- thick rays first, silhouettes last -- measured in round 6: -4 % lego, -1 % varied, -11 % membrane:
		// neighbouring rows share more than a shorter tail saves; profiles/r06/ab_roworder_*.txt)
		const uint32_t bx = pk % a.tiles_x, by = pk / a.tiles_x;
		x = bx * PW + lx;
		y = by * PH + ly;
		out_idx = x + W * y;
	} else {
		const uint32_t ppt = a.packets_per_tile_x * (a.p.tile_size / PH);
		const uint32_t k = pk / ppt, b = pk % ppt;
		const uint32_t stride = a.p.tile_stride ? a.p.tile_stride : 1;
		const uint32_t T = a.p.tile_first + k * stride;
		const uint32_t Tx = T % a.tiles_x, Ty = T / a.tiles_x;
		const uint32_t tx = (b % a.packets_per_tile_x) * PW + lx, ty = (b / a.packets_per_tile_x) * PH + ly;
		x = Tx * a.p.tile_size + tx;
		y = Ty * a.p.tile_size + ty;
		out_idx = (k * a.p.tile_size + ty) * a.p.tile_size + tx;
	}
	return x < W && y < H;
}

// where pixel (x, y) of this launch lands in the caller's buffers: packet_pixel's out_idx from the pixel alone
__device__ __forceinline__ uint32_t pixel_out_idx(const RenderArgs& a, uint32_t x, uint32_t y) {
	if (a.p.tile_size == 0) return x + (uint32_t)a.p.resolution[0] * y;
	const uint32_t ts = a.p.tile_size, Tx = x / ts, Ty = y / ts, T = Ty * a.tiles_x + Tx;
	const uint32_t stride = a.p.tile_stride ? a.p.tile_stride : 1;
	const uint32_t k = (T - a.p.tile_first) / stride;
	return (k * ts + (y - Ty * ts)) * ts + (x - Tx * ts);
}

// Hybrid launches (TEAM == 0, whole-image mode): every tail_every-th (3rd) packet row of the image is taken out of the 8x8 packet
// list and appended to the queue as 4x4 packets ("tail" packets, a uniform sample of the picture, so the same share of the rays
// whatever the scene).  Waves that reach them switch to lane teams: the last rays of a frame then take a quarter of a
// ray's life while the waves still on their last 64-ray generation finish (see render_kernel).
__device__ __forceinline__ bool packet_pixel_bulk(const RenderArgs& a, uint32_t pk, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	const uint32_t rb = pk / a.tiles_x, col = pk % a.tiles_x, row = rb + rb / (a.tail_every - 1u); // every tail_every-th row is a tail row
	x = col * 8u + ((uint32_t)lane & 7u);
	y = row * 8u + ((uint32_t)lane >> 3);
	out_idx = x + W * y;
	return x < W && y < H;
}
__device__ __forceinline__ bool packet_pixel_tail(const RenderArgs& a, uint32_t q, int lane, uint32_t& x, uint32_t& y, uint32_t& out_idx) {
	const uint32_t W = (uint32_t)a.p.resolution[0], H = (uint32_t)a.p.resolution[1];
	// a tail row is 8 pixels high; its packets are 4x4 / 8x4 / 8x8 pixels with fill_lanes = 4 / 2 / 1 lanes on a pixel (as in packet_pixel<4 / 2 / 1>)
	const uint32_t L = a.fill_lanes, cols = L == 4u ? a.tiles_x * 2u : a.tiles_x, per_row = cols * (L == 1u ? 1u : 2u);
	const uint32_t trow = q / per_row, s = q % per_row, sy = s / cols, sx = s % cols;
	const uint32_t idx = (uint32_t)lane / L, pw = L == 4u ? 4u : 8u;
	x = sx * pw + (idx % pw);
	y = (trow * a.tail_every + a.tail_every - 1u) * 8u + sy * 4u + (idx / pw);
	out_idx = x + W * y;
	return x < W && y < H;
}

} // namespace nrs
