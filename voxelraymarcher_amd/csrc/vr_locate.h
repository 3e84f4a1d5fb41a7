// vr_locate.h -- a world voxel's place in the live image of either store, for the kernels that
// address voxels by coordinate and not along a walk: vr_access.hip (vr_scene_lookup,
// vr_scene_paint) and vr_occlusion.hip (vr_occlusion).
//   locate()                     the value word of a voxel, or null: every read dependent on the one before
//   cell_of() / presence_word()  the same answer to "is it stored?" in two stages, each a single
//                                load, so that a lane with several voxels to ask about can have
//                                all of a stage's loads in flight at once
#pragma once

#include "vr_device.h"

namespace vr {

using LocF = Ctx<STORE_VCS, false, kTileBudget>;   // (for its static arithmetic: word_index, word_bit5)

// The word that holds the colour of world voxel (x, y, z) -- an entry of vcs_vals, or the value
// half of a cuckoo slot -- or null when the voxel is not stored: its 64^3 region outside the
// frame, a null region, an absent cluster, an absent key.  Set membership in the voxel set
// vr_scene_voxels returns: a world coordinate always has local coordinates in [0, 64), so none
// of the walks' out-of-region lookups (vr_device.h lookup_aliased, wrapped keys) exists here.
template <int STORE>
__device__ __forceinline__ const uint32_t* locate(const KScene& s, int32_t x, int32_t y, int32_t z) {
    // region = floor(c / 64), tested against the frame as Ctx::in_scene does (unsigned wrap:
    // any int32 coordinate gives a region in [-2^25, 2^25), far from wrapping back into D <= 1024)
    const uint32_t mc = (uint32_t)s.min_coord;
    const uint32_t ux = (uint32_t)(x >> 6) - mc, uy = (uint32_t)(y >> 6) - mc, uz = (uint32_t)(z >> 6) - mc;
    if (ux >= s.D || uy >= s.D || uz >= s.D) return nullptr;
    const uint32_t r = s.region_slot[ux + uy * s.D + uz * s.D * s.D];
    if (r == kNone) return nullptr;
    const uint32_t lx = (uint32_t)x & 63u, ly = (uint32_t)y & 63u, lz = (uint32_t)z & 63u;
    const uint32_t w = LocF::word_index(lx, ly, lz), bit = LocF::word_bit5(ly, lz) & 31u;
    if (STORE == STORE_VCS) {
        const uint2 m = s.vcs_mask[(size_t)r * 8192u + w];      // an absent cluster's words are {0, kNone}
        if (!((m.x >> bit) & 1u)) return nullptr;
        return s.vcs_vals + (m.y + __popc(m.x & ((1u << bit) - 1u)));
    }
    if (!((s.ht_filter[(size_t)r * kHashFilterWords + w] >> bit) & 1u)) return nullptr;
    const uint32_t key = (lx << 20) | (ly << 10) | lz;          // generate3DPoint
    const uint4 m = s.ht_meta[r];                                // {base, M, prime, offset}
    const uint2* e = s.ht_slots + m.x + hash1(key, m.w) % m.y;
    if (e->x != key) e = s.ht_slots + m.x + m.y + hash2(key, m.z) % m.y;
    if (e->x != key) return nullptr;                             // (a filter bit without its key: never, by construction)
    return &e->y;
}

// locate()'s question "is the voxel stored?" in two stages.  Stage 1, cell_of: the voxel's region
// entry (index into region_slot, or kNone outside the frame: locate()'s frame test), its word
// within the region's 8192 presence words and its bit there -- arithmetic only.  Stage 2,
// presence_word: the 32 presence bits around the voxel in region slot r (!= kNone) -- a VCS mask
// record's bits, or the cuckoo filter's word, which holds exactly the keys in the tables (it is
// what vr_scene_voxels exports from): one 4-byte load, where locate() goes on to the value.
struct VoxelCell {
    uint32_t entry, word, bit;
};
__device__ __forceinline__ VoxelCell cell_of(const KScene& s, int32_t x, int32_t y, int32_t z) {
    const uint32_t mc = (uint32_t)s.min_coord;
    const uint32_t ux = (uint32_t)(x >> 6) - mc, uy = (uint32_t)(y >> 6) - mc, uz = (uint32_t)(z >> 6) - mc;
    const uint32_t lx = (uint32_t)x & 63u, ly = (uint32_t)y & 63u, lz = (uint32_t)z & 63u;
    const bool in = ux < s.D && uy < s.D && uz < s.D;
    return VoxelCell{in ? ux + uy * s.D + uz * s.D * s.D : kNone, LocF::word_index(lx, ly, lz),
                     LocF::word_bit5(ly, lz) & 31u};
}
template <int STORE>
__device__ __forceinline__ uint32_t presence_word(const KScene& s, uint32_t r, uint32_t word) {
    if (STORE == STORE_VCS) return s.vcs_mask[(size_t)r * 8192u + word].x;   // an absent cluster's bits are 0
    return s.ht_filter[(size_t)r * kHashFilterWords + word];
}

}  // namespace vr
