// vr_internal.h -- layouts shared by the host builder (vr_scene.cpp) and the
// HIP kernels (vr_march.hip, vr_order.hip, vr_query.hip, vr_shade.hip, vr_util.hip, vr_access.hip; the walker: vr_walk.h).  See DESIGN.md "Data layout in HBM".
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace vr {

// Sets the thread's vr_last_error() message and returns `code` (vr_host.cpp).
int set_error(int code, const std::string& msg);

constexpr uint32_t kEmpty = 1u << 30;        // EMPTY_KEY == EMPTY_VAL (VoxelFunctions.cuh:20-21)
constexpr uint32_t kNone = 0xFFFFFFFFu;      // null region / null cluster in the tables
constexpr int32_t kBlock = 64;               // BLOCK_SIZE (VoxelFunctions.cuh:24)
// Iteration limits ("Walks that never finish").  The walks
// themselves have no budget: the reference runs every finite walk to its end.
//  kTileBudget : a tile-pass pixel whose walks exceed this many loop
//                iterations is handed to the crawl pass and walked there from
//                its start (normal pixels of every config take < 300; only
//                cluster-skip crawls run longer).
//  kCrawlBudget: the crawl pass's hang guard.  Walks that never finish are
//                detected exactly there (a loop iteration that leaves the
//                loop's state unchanged); the longest finite walk of any
//                config takes 1.4e6 iterations, ~770x below this.
constexpr uint32_t kTileBudget = 4096u;
constexpr uint32_t kCrawlBudget = 1u << 30;
// A tile-pass pixel that could not be deferred (the list was full) is written
// as kDeferMarker (no colour is >= 2^24) and counted in slot word 2; the crawl
// pass then finds it in the frame.
constexpr uint32_t kDeferMarker = 0xFFFFFFFFu;
// VCS walks address a region's cluster masks as a 32-bit byte offset from the
// scene's mask array (64 KB per occupied 64^3 region): at most 65536 occupied
// regions (4 GB of masks) per VCS scene; the builders reject larger scenes.  Cuckoo
// scenes have no such bound (as the reference's): their key-presence filter (32 KB per
// occupied region) is addressed with 64-bit offsets.
constexpr uint32_t kVcsMaxRegions = 65536u;
// words of a cuckoo region's key-presence filter (64^3 bits)
constexpr uint32_t kHashFilterWords = 8192u;

// Device view of one scene (vr_scene_edit replaces its buffers as a set; vr_scene_paint stores colours into them).  Offsets are 32-bit word indices.
//  region_slot[D^3]          : region index r, or kNone (null StorageStructure*)
//  VCS   : vcs_mask[r*8192 + slot*16 + w]  (one 128-B record per cluster of an
//                              occupied region; VoxelClusterStore::deviceBlockMemAddress
//                              + the cluster's sorted keys, VoxelClusterStore.cuh:37-85)
//                              {bits, index}: bit b set <=> the voxel with in-cluster index
//                              q = 32w+b ((x&7)<<6|(y&7)<<3|z&7, the keys' order) is stored;
//                              index = vcs_vals position of the word's first stored voxel.
//                              Absent cluster: {0, kNone} in all 16 words.  slot =
//                              z-cluster<<6 | y-cluster<<3 | x-cluster (a permutation of the
//                              reference's cluster id x<<6|y<<3|z, so that the word of an
//                              in-region voxel is y2 | x<<1 | (y>>3)<<7 | (z>>3)<<10).
//          vcs_vals[]        : colours, cluster by cluster in key order.
//  Cuckoo: ht_meta[r]        : {base, M, prime, offset}
//          ht_slots[base+i]  : table 1 slot i {key, value};
//          ht_slots[base+M+i]: table 2 slot i {key, value}; empty key = kEmpty
//  VCS   : vcs_cbits[r*16 + w]: bit b set <=> cluster slot 32w+b of region r is present
//                              (derived from vcs_mask after either build; the crawl
//                              pass caches a region's 64 B in LDS)
//  Cuckoo: ht_filter[r*8192 + w]: key-presence bits of region r's tables, one bit per voxel
//                              of the 64^3 region in the VCS mask-word order: voxel (x,y,z)
//                              is word vcs_word_index(x,y,z), bit (y&3)<<3 | z&7 (derived
//                              from ht_slots after either build).  A probe whose key is not
//                              in the tables -- most of them -- is answered here; the
//                              tables are probed for the keys they hold.
struct KScene {
    const uint32_t* region_slot;
    const uint2* vcs_mask;
    const uint32_t* vcs_vals;
    const uint32_t* vcs_cbits;
    const uint4* ht_meta;
    const uint2* ht_slots;
    const uint32_t* ht_filter;
    uint32_t D;
    int32_t min_coord;
    uint32_t n_regions;
};

// Per-launch view: camera, lighting, scene transform and the row mapping.
// Local row l of the output maps to frame row
//   y = row0 + ((l / band_rows) * nranks + rank) * band_rows + (l % band_rows);
// rows with y >= row_limit (<= H) are written as 0.  The output's rows are LW words
// (= W, or the 2-D tile deal's local width).  2-D tile deal (tile_cols > 0; the row
// deal then has nranks = 1, rank = 0): local column x of band b = l / band_rows maps to
// frame column
//   X = ((x / tile_cols) * col_R + (col_rank - col_stride * b) mod col_R) * tile_cols + x % tile_cols;
// columns with X >= W are written as 0.
struct KView {
    float llc[3], hor[3], ver[3], org[3];
    float L[3], LC[3], LP[3];
    // the light direction's reciprocals RN(1 / L_i) (host division, correctly
    // rounded: exact in div_fast) and whether all three are in div_fast's divisor
    // domain -- kernel arguments, so the shadow walks keep them in SGPRs
    float Lr[3];
    uint32_t L_fast;
    // the light as a longest-axis walk sees it (Ray::convertRayToLongestAxisDirection,
    // Ray.cuh:19-71): axis order 0..5 (L,M,S = xyz, xzy, yxz, yzx, zxy, zyx), direction
    // k * L with k = 1 / |L_L| (xyz), its sign classes (bit 2a: > 0, bit 2a+1: < 0),
    // L_unit = that direction is (+-1, +-1, +-1) exactly and the order is zyx (equal
    // magnitudes), L_eq = L's three components are equal
    float Lw[3];
    uint32_t L_order, L_cls, L_unit, L_eq;
    float translation[3];
    float scale_f;
    int32_t use_point_light, use_shadows;
    uint32_t W, H;
    uint32_t row0, band_rows, rank, nranks, local_rows, row_limit;
    uint32_t band_minv;       // floor(2^32 / band_rows) (2^32 - 1 for 1): l / band_rows by a multiply-high
    uint32_t LW;              // output row stride in words (local columns)
    uint32_t tile_cols;       // 0: whole rows (no column deal)
    uint32_t tile_minv;       // floor(2^32 / tile_cols) (2^32 - 1 for 1)
    uint32_t col_R, col_rank, col_stride;   // 2-D deal: ranks, this rank, stride (< col_R)
    // ---- end of the view's identity.  Everything above `out` is hashed, with the scene and
    // the algorithm, into the view key (vr_launch.cpp view_key) under which the learned orders
    // and the crawl-pass skip are kept: a field that changes any pixel, or which pixels the
    // tile pass defers to the crawl pass, MUST sit above this line.  Everything below is a
    // per-launch buffer or a launch knob that changes neither (checked by the static_assert
    // after the struct: adding a field below fails the build until it is reviewed here).
    // (The deferral's other inputs are compile-time: kTileBudget, and the walk itself.)
    uint32_t* out;
    unsigned long long* bytes;
    // (COUNT launches, optional) [0] crawl iterations the crawl pass fast-forwarded in
    // closed form, [1] the existence-read bytes credited for them (part of *bytes, never loaded)
    unsigned long long* stats;
    uint32_t* defer;         // crawl deferral slot: [count, done, overflow, 0, records (kDeferRecWords each)...]
    uint32_t defer_cap;
    uint32_t crawl_rewalk;    // 1: deferred crawls are walked from the pixel's start (VR_KERNEL_TILE_REWALK)
    uint32_t crawl_rpw;       // crawl records per wave (0 = 4): 2 for a lone frame, 32 with frames in flight
    uint32_t* defer_stat;     // host-mapped word: the crawl pass writes its record count there (grid sizing)
    // Tile-pass work order ("Heaviest tiles first"): workgroup i of the grid
    // renders tile order[i] = (tile row << 16 | tile column) -- a permutation of the grid
    // made from an earlier launch's costs -- or, when null, tile i in grid order.  cost
    // (or null): each wave writes its walk length (the max over its lanes of the pixel's
    // loop iterations) to cost[tile * kWavesPerTileGroup + wave], tile = row * columns + column.
    const uint32_t* order;
    uint32_t* cost;
    // Lane order (round 5, vr_march.hip lane_pixel): per pixel block (16x32 by default) the slot
    // of each pixel, dealing them to the block's waves heaviest first (or null: 8x8 tiles;
    // vr::perm_bytes(gx, gy) bytes); pcost (or null): each lane
    // writes its pixel's walk lengths at [l * LW + x] (primary << 16 | shadow, each saturated at
    // 0xFFFF; loop iterations), for the next lane order.
    const uint8_t* perm;
    uint32_t* pcost;
    // (or null) the launch slot's host-mapped crawl report: the crawl pass writes
    // {launch_id, records deferred} there in one 8-B store (the host's crawl-pass skip);
    // a tile pass that defers a pixel writes {launch_id, 1} there first (deferral_report:
    // on a launch whose crawl pass the host skipped, the report ends the skipping)
    uint32_t* slot_stat;
    uint32_t launch_id;
};
// The per-launch tail of KView (see "end of the view's identity" above): out, bytes, stats,
// defer, defer_cap, crawl_rewalk, crawl_rpw, defer_stat, order, cost, perm, pcost, slot_stat,
// launch_id.  defer_cap and crawl_rewalk change only how deferred pixels are resumed, never
// which ones defer; the crawl-pass skip keys them anyway (vr_launch.cpp crawl_key).
// (10 pointers, 4 words, padding: 104 bytes)
static_assert(sizeof(KView) - offsetof(KView, out) == 104,
              "a KView field was added after `out`: review whether it belongs to the view identity");

// Rays that start a cluster-skip crawl (see vr_crawl.h crawl_steps) in the
// tile pass, and pixels that exceed kTileBudget, are deferred to a second pass
// over a per-launch list.
// A slot is [count, done, overflow, 0] and kDeferCap records of kDeferRecWords
// words: the crawling walk's state at the crawl (vr_walk.h, grid_original_rt),
// from which the crawl pass resumes it, or just the pixel (flag 4: walk it from
// its start).  Record words:
//   0 pixel (row << 16 | x)   1 flags (1 shadow walk, 2 longest-axis shadow, 4 walk from the start)
//   2-4 stepped position      5-7 region         8 unused (0)
//   9 iterations so far       10 counted bytes so far
//   11-13 tX, tY, tZ of the last voxel step (hit normal; 0 for shadow walks)
//   14 reserved (0)           15-17 the crawl iteration's voxel (filled in by the crawl pass)
//   18 lit colour             19 unused
// A slot is used by one launch at a time (vr_launch.cpp SlotRing).
constexpr uint32_t kDeferCap = 16384;
constexpr uint32_t kDeferRecWords = 20;
constexpr uint32_t kDeferWords = 4 + kDeferCap * kDeferRecWords;

// Launch one render (defined in vr_march.hip): the tile pass and the crawl pass on
// `stream`, the crawl pass with `crawl_wgs` workgroups (any number is correct).
// in_flight: another stream's launch is still running on the device (the tile pass then
// takes its higher-occupancy variant where one exists, vr_march.hip TileWaves)
hipError_t launch_march(int store, int algo, bool count, const KScene& s, const KView& v,
                        hipStream_t stream, uint32_t crawl_wgs, bool in_flight, bool crawl = true);
// Crawl-pass grid for a launch that expects about `records` deferred pixels.
uint32_t crawl_grid(uint32_t records, uint32_t rpw);
// vr_pick's kernel (vr_query.hip, as the two below): the primary hit behind each of n pixels (px[i], py[i]) of the view's frame
// as 64-byte vr_hit records (hits: 16-byte aligned device memory), one lane per query with the
// exact walker.  The view is make_view's with one band over the frame; nothing below `out` is read.
constexpr uint32_t kPickMiss = 0, kPickVoxel = 1, kPickNever = 2, kPickOutside = 3;   // = VR_HIT_*
hipError_t launch_pick(int store, int algo, const KScene& s, const KView& v, const uint32_t* px, const uint32_t* py,
                       uint32_t n, void* hits, hipStream_t stream);
// vr_trace's kernel: the primary hit of each of n rays (32-byte vr_ray records, 16-byte aligned
// device memory) as vr_hit records, one lane per ray with the pick's walker.  idx (or null):
// lane i walks ray idx[i] and writes record idx[i]; it must be a permutation of 0..n-1.  Of the
// view only translation and scale_f are read.
hipError_t launch_trace(int store, int algo, const KScene& s, const KView& v, const void* rays, const uint32_t* idx,
                        uint32_t n, void* hits, hipStream_t stream);
// vr_shade's kernel (vr_shade.hip): the render's colour for each of n rays (vr_ray records and idx
// as for launch_trace), one 4-byte word per ray in colors; hits (or null): launch_trace's records
// too, from the same walk.  Of the view the lighting block, translation and scale_f are read.
hipError_t launch_shade(int store, int algo, const KScene& s, const KView& v, const void* rays, const uint32_t* idx,
                        uint32_t n, uint32_t* colors, void* hits, hipStream_t stream);
// vr_shade_lights' kernels (vr_lights.hip).  launch_lights_primary: the primary walk of each of n
// rays (vr_ray records and idx as for launch_trace); state (32 bytes per ray, 16-byte aligned)
// receives what a light pass needs of the hit, colors[r] the ambient term (ambient: three host
// floats, or null: 0), hits (or null) launch_trace's records.  Of the view translation and
// scale_f are read.  launch_light_term: one light's term for every ray with a hit -- the word
// launch_shade writes under the view's lighting block -- summed into colors byte-wise with a
// clamp at 255 per channel; after launch_lights_primary on the same stream, once per light.
hipError_t launch_lights_primary(int store, int algo, const KScene& s, const KView& v, const void* rays,
                                 const uint32_t* idx, uint32_t n, const float* ambient, void* state, uint32_t* colors,
                                 void* hits, hipStream_t stream);
hipError_t launch_light_term(int store, int algo, const KScene& s, const KView& v, const uint32_t* idx, uint32_t n,
                             const void* state, uint32_t* colors, hipStream_t stream);
// vr_camera_rays' kernel: the rays of pixels (px[i], py[i]) of the view's frame (one band over it).
hipError_t launch_camera_rays(const KView& v, const uint32_t* px, const uint32_t* py, uint32_t n, void* rays,
                              hipStream_t stream);
// The coherent order of n rays (vr_trace.hip): a key per ray -- direction signs, the Morton code
// of the origin's 8-voxel cell clamped to the scene's frame, the direction's cube-map cell -- and
// a stable radix sort of (key, index).  *scratch is one hipMalloc on the current device that
// holds the keys, the indices and the sort's temporary; *idx points into it at the sorted
// indices.  The caller frees *scratch once the work queued on `stream` is done (on failure it is
// already freed and null).
hipError_t trace_order(const KScene& s, const KView& v, const void* rays, uint32_t n, hipStream_t stream,
                       void** scratch, const uint32_t** idx);
// (vr_access.hip: voxel access by coordinate)
// vr_scene_lookup's kernel: rgb[i] = the stored colour of world voxel xyz[3i..3i+2], or 0xFFFFFFFF
// (VR_VOXEL_ABSENT) when it is not stored; one lane per query.
hipError_t launch_lookup(int store, const KScene& s, const int32_t* xyz, uint32_t n, uint32_t* rgb, hipStream_t stream);
// vr_scene_paint, before any write: sets stat[0] to the first index whose colour is >= 2^24
// (0xFFFFFFFF: none) and stat[1] to 0xFFFFFFFF - the number of edits whose voxel is not stored.
hipError_t launch_paint_check(int store, const KScene& s, const int32_t* xyz, const uint32_t* rgb, uint32_t n,
                              uint32_t* stat, hipStream_t stream);
// vr_scene_paint's writes into vcs_vals / the value halves of ht_slots: the tag kernel and the
// resolve kernel (the last edit of a voxel wins).  n < 2^31, every colour < 2^24, and nothing else
// may run on the scene between the two.
hipError_t launch_paint_apply(int store, const KScene& s, const int32_t* xyz, const uint32_t* rgb, uint32_t n,
                              hipStream_t stream);
// (vr_occlusion.hip: voxel ambient occlusion)
// vr_occlusion's kernel: ao[i] = the occlusion (0..255, 255 open) of the n vr_hit records at hits
// (16-byte aligned device memory), one lane per record.  launch_occlusion_apply: the same value
// per record, written to ao_out[i] when ao_out is not null, and colors[i] scaled per channel by
// the factor `strength` (0..255) makes of it.
hipError_t launch_occlusion(int store, const KScene& s, const void* hits, uint32_t n, uint32_t* ao, hipStream_t stream);
hipError_t launch_occlusion_apply(int store, const KScene& s, const void* hits, uint32_t n, uint32_t strength,
                                  uint32_t* colors, uint32_t* ao_out, hipStream_t stream);
// (vr_reflect.hip: mirror reflections)
// vr_bounce_rays' kernel: out[i] = the bounce of rays[i] at hits[i] (vr_reflect_math.h) for n
// records, one lane per record; rays, hits and out are 16-byte aligned device memory, scale_f is
// (float)scale.
hipError_t launch_bounce_rays(const void* rays, const void* hits, uint32_t n, const float translation[3], float scale_f,
                              void* out, hipStream_t stream);
// One depth's descent of vr_shade_lights_reflect, after launch_lights_primary on the same stream:
// for each of the n_prev rays r = prev[i] (prev null: r = i) whose hit state says VOXEL and whose
// stored colour has (col & mask) == value, rays_out[r] = the bounce of rays_in[r] at that hit, and
// r is appended to list (n_prev words) with *count (zeroed by the caller) counting the entries.
// rays_in and rays_out are different buffers of vr_ray records indexed by ray number.
hipError_t launch_bounce_compact(const void* state, const void* rays_in, const uint32_t* prev, uint32_t n_prev,
                                 uint32_t mask, uint32_t value, const float translation[3], float scale_f, void* rays_out,
                                 uint32_t* list, uint32_t* count, hipStream_t stream);
// shallow[r] = mix_rgb(shallow[r], deep[r], k) for the n rays r of list (k in 0..255).
hipError_t launch_fold(const uint32_t* list, uint32_t n, uint32_t* shallow, const uint32_t* deep, uint32_t k,
                       hipStream_t stream);
// (vr_atmos.hip: sky and distance fog; AtmosParams: vr_atmos_math.h)
struct AtmosParams;
// vr_shade_lights_atmosphere's pass for one depth, after that depth's last colour pass on the same
// stream: colors[r] = atmos(colors[r], rays[r], the hit state of r) for the n rays r = list[i]
// (list null: r = i).  state and rays are 16-byte aligned device memory indexed by ray number.
hipError_t launch_atmos_state(const void* state, const void* rays, const uint32_t* list, uint32_t n, const AtmosParams& p,
                              const float translation[3], float scale_f, uint32_t* colors, hipStream_t stream);
// vr_atmosphere_apply's kernel: out[i] = atmos(in[i], rays[i], hits[i]) for n records, one lane per
// record; rays and hits are 16-byte aligned device memory; out may be in.
hipError_t launch_atmos_records(const void* rays, const void* hits, const uint32_t* in, uint32_t n, const AtmosParams& p,
                                const float translation[3], float scale_f, uint32_t* out, hipStream_t stream);
// (vr_util.hip, to launch_assemble_tiles)
// vcs_cbits of a VCS scene from its mask records (one thread per 32 cluster slots).
hipError_t launch_cluster_bits(const uint2* vcs_mask, uint32_t n_regions, uint32_t* cbits, hipStream_t stream);
// ht_filter of a cuckoo scene from its tables (one workgroup per region).
hipError_t launch_hash_filter(const uint4* ht_meta, const uint2* ht_slots, uint32_t n_regions, uint32_t* filter,
                              hipStream_t stream);
hipError_t launch_pack_rgb8(const uint32_t* words, uint8_t* rgb, uint64_t n, hipStream_t stream);
// The 2-D tile deal's layout (vr_render_opts.tile_cols) for rank 0's reassembly: the frame
// W x H, bands of band_rows rows, column blocks of tile_cols, R ranks dealt with `stride`;
// LW = local row width (words), rank_words = one rank's buffer (pixels).
struct TileLayout {
    uint32_t W, H, band_rows, tile_cols, R, stride, LW;
    uint64_t rank_words;
};
// frame[y][x] <- parts[rank][local pixel] for every frame pixel, elem_bytes (1..4) per pixel.
hipError_t launch_assemble_tiles(const void* parts, void* frame, uint32_t elem_bytes, const TileLayout& t,
                                 hipStream_t stream);
// The tile pass's grid for a view (columns, rows of workgroups) and its waves per workgroup.
void march_grid(const KView& v, uint32_t& columns, uint32_t& rows);
constexpr uint32_t kWavesPerTileGroup = 2;
// (vr_order.hip, to launch_perm)
// Heaviest-first work order of a grid of `columns` x `n / columns` workgroups from the
// costs a launch wrote (KView::cost): one workgroup, a counting sort by cost.
hipError_t launch_order(const uint32_t* cost, uint32_t n, uint32_t columns, uint32_t* order, hipStream_t stream);
// The lane orders of a grid of gx x gy tile groups (gx x ceil(gy / 4) 16x32 blocks by default) from the
// per-pixel walk lengths a launch wrote (KView::pcost, rows x LW words); with cost non-null
// also the waves' walk lengths under the new lane order (KView::cost's layout).
size_t perm_bytes(uint32_t gx, uint32_t gy);   // the lane order of a gx x gy grid
// How the build lays a lane order out: the block's sides in pixels, the bytes of one perm
// entry and the seat rule (vr_lane_order.h VR_LANE_SEAT) -- for vr_debug_lane_order's readers.
struct LaneShape {
    uint32_t block_x, block_y, entry_bytes, seat;
};
LaneShape lane_shape();
hipError_t launch_perm(const uint32_t* pcost, uint32_t LW, uint32_t rows, uint32_t gx, uint32_t gy, uint8_t* perm,
                       uint32_t* cost, hipStream_t stream);
// (vr_resolve.hip: supersampled frames)
// vr_resolve's kernel: the (S * W) x (S * rows) words at `fine` box-filtered to W x rows pixels,
// S in {1, 2, 4, 8}, as packed words in out and/or RGB8 in rgb (either may be null, not both), from
// one read of the fine frame.  resolve_vector_path: whether the launch takes its 16-byte loads (a
// 16-byte aligned base and S = 4, S = 8 or S = 2 with an even W) or one-word loads.
bool resolve_vector_path(const void* fine, uint32_t W, uint32_t S);
hipError_t launch_resolve(const uint32_t* fine, uint32_t W, uint32_t rows, uint32_t S, uint32_t* out, uint8_t* rgb,
                          hipStream_t stream);

}  // namespace vr
