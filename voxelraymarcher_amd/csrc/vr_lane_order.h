// vr_lane_order.h -- the shapes the tile pass (vr_march.hip: lane_pixel) and the lane order's
// kernel (vr_order.hip: perm_kernel) must agree on: the tile workgroup, the lane block, the
// perm entry type and the seat rule.  One set of -D switches, so an A/B build with another
// shape (the Makefile's EXTRA reaches every unit) stays consistent.
#pragma once
#include <stdint.h>

#include <type_traits>

namespace vr {
namespace {

// Tile pass workgroup: kTilesX x kTilesY waves, one 8x8 pixel tile each.  Two
// tiles side by side (128 threads) measured faster than 2 x 2 (256): a
// workgroup's slot is held until its slowest wave ends, so smaller ones pack the
// CUs more tightly (per frame in flight: C2 0.151 -> 0.1415 ms, C3 0.420 -> 0.385,
// C4 0.101 -> 0.096; one tile per workgroup: C2 0.1423, C3 0.377, C4 0.0955).
#ifndef VR_TILES_X
#define VR_TILES_X 2
#endif
#ifndef VR_TILES_Y
#define VR_TILES_Y 1
#endif
constexpr uint32_t kTilesX = VR_TILES_X, kTilesY = VR_TILES_Y;

// The lane block (see lane_pixel, vr_march.hip): the pixels the tile groups of one block share.
// The block is kLaneBlockX x kLaneBlockY pixels, 16 wide and 32 high by default (8 wave
// slots, 2-byte perm entries): VR_LANE_BLOCK=16|32 sets both sides, VR_LANE_BLOCK_X /
// VR_LANE_BLOCK_Y one each.  Measured per frame in flight, either seat rule
// (profiles/lane_seat/): C2 16x16 0.0975 ms, 32x16 0.104, 32x32 0.0957, 16x32 0.0950; 16x32 is
// also the fastest on C3 (0.1843 -> 0.1798), C4 (0.0473 -> 0.0458; 32x32: 0.0490) and C5.  A
// launch alone with both orders learned is slower with it (C2 0.1096 -> 0.1220 ms; 32x32
// 0.127): larger blocks make fewer, fuller waves, which pays when frames overlap.
#ifdef VR_LANE_BLOCK
#define VR_LANE_BLOCK_DEFAULT_X VR_LANE_BLOCK
#define VR_LANE_BLOCK_DEFAULT_Y VR_LANE_BLOCK
#else
#define VR_LANE_BLOCK_DEFAULT_X 16
#define VR_LANE_BLOCK_DEFAULT_Y 32
#endif
#ifndef VR_LANE_BLOCK_X
#define VR_LANE_BLOCK_X VR_LANE_BLOCK_DEFAULT_X
#endif
#ifndef VR_LANE_BLOCK_Y
#define VR_LANE_BLOCK_Y VR_LANE_BLOCK_DEFAULT_Y
#endif
constexpr uint32_t kLaneBlockX = VR_LANE_BLOCK_X, kLaneBlockY = VR_LANE_BLOCK_Y;
static_assert((kLaneBlockX == 16 || kLaneBlockX == 32) && (kLaneBlockY == 16 || kLaneBlockY == 32),
              "lane block: 16 or 32 pixels a side");
constexpr uint32_t kLanePixels = kLaneBlockX * kLaneBlockY;
constexpr uint32_t kLbX = kLaneBlockX / (8u * kTilesX), kLbY = kLaneBlockY / (8u * kTilesY);
using PermT = std::conditional<kLanePixels == 256, uint8_t, uint16_t>::type;
// The seat of a pixel within its wave slot (which lane renders it; the slot's 64 pixels are
// the same either way): 0 = by cost rank, as perm_kernel's sort leaves them, 1 = in ascending
// Morton order of (column, row) in the block, so that neighbouring lanes, lane quads and
// 16-lane groups cover compact patches of the block.  Morton seats measured no faster and
// moved no vector-L1 counter (C2 per frame in flight 0.0976 -> 0.0974 ms, inside the run-to-run
// spread; TCP tag accesses per launch 1.570e7 -> 1.580e7, profiles/lane_seat/), so 0 stays.
#ifndef VR_LANE_SEAT
#define VR_LANE_SEAT 0
#endif
constexpr uint32_t kLaneSeat = VR_LANE_SEAT;
static_assert(kLaneSeat <= 1u, "lane seat: 0 (cost order) or 1 (Morton order)");
constexpr bool kLaneOrder = kTilesX == 2 && kTilesY == 1;   // (other tile shapes ignore perm)
// perm_kernel's sort keys: (walk length << kLaneShift | pixel of the block)
constexpr uint32_t kLaneShift = kLanePixels == 256 ? 8u : kLanePixels == 512 ? 9u : 10u;

}  // namespace
}  // namespace vr
