// vr_lights_state.h -- the per-ray hit state that lights_primary_kernel (vr_lights.hip) leaves for
// the passes after it: light_term_kernel there, bounce_compact_kernel in vr_reflect.hip.  What
// light_and_shadow (vr_walk.h) reads of a Hit, 32 bytes as two 16-byte words --
//   a = {col, nc | flags, so.x, so.y}     b = {so.z, region.x, region.y, region.z}
// Hit::nc is bits(+-1.0f) | axis: its bits 2-22 are 0, and the flags sit there: kStLongest
// (Hit::longest), kStHit (a primary VOXEL hit: the light passes run) and kStNever (the primary
// walk never ends; kept apart from a miss for a reader of the buffer, the light passes skip
// both).  A ray without a hit writes {0, flags, 0, 0} and a zero `b`, which is never read.
#pragma once

#include <stdint.h>

namespace vr {

constexpr uint32_t kStLongest = 4u, kStHit = 8u, kStNever = 16u, kStFlags = kStLongest | kStHit | kStNever;

}  // namespace vr
