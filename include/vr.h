/*
 * vr.h -- C ABI of the MI355X-native voxel ray-march renderer (libvr.so).
 *
 * Drop-in boundary for the hot path of lukeduball/VoxelRaymarcher.  Every
 * entry point names the reference interface it replaces (paths relative to
 * /root/reference/VoxelRaymarcher/src).  No HIP or torch types appear in the
 * signatures: device buffers are plain pointers, streams are `void*`
 * (a hipStream_t, NULL = the null stream).
 *
 * Return codes: VR_OK (0) or a negative VR_E_*; vr_last_error() gives a
 * thread-local message for the last failure on the calling thread.
 */
#ifndef VR_H
#define VR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_OK 0
#define VR_E_INVALID (-1)   /* bad argument */
#define VR_E_HIP (-2)       /* HIP runtime error / no device */
#define VR_E_NOMEM (-3)     /* host or device allocation failed */
#define VR_E_IO (-4)        /* file could not be read or written */
#define VR_E_BUILD (-5)     /* storage structure could not be built */
#define VR_E_PARSE (-6)     /* malformed .vox line (std::stoi would throw) */

/* = enum class StorageType {VOXEL_CLUSTER_STORE, HASH_TABLE}
 *   (geometry/VoxelFunctions.cuh:37; selected in main/Main.cu:45-55) */
typedef enum { VR_STORE_VCS = 0, VR_STORE_HASHTABLE = 1 } vr_store;

/* = rayMarchFunctionID (main/Main.cu:58-68,119-128):
 *   0 -> rayMarchSceneJumpAxis, 1 -> rayMarchSceneOriginal */
typedef enum { VR_ALGO_LONGESTAXIS = 0, VR_ALGO_ORIGINAL = 1 } vr_algo;

/* = class Camera field order (renderer/camera/Camera.cuh:34-39) */
typedef struct {
    float origin[3];
    float lower_left[3];
    float horizontal[3];
    float vertical[3];
    float forward[3];
} vr_camera;

/* = the __constant__ block LIGHT_DIRECTION / LIGHT_COLOR / LIGHT_POSITION /
 *   USE_POINT_LIGHT / USE_SHADOWS (geometry/VoxelFunctions.cuh:27-35) as
 *   uploaded by setupConstantValues (main/Main.cu:26-42). */
typedef struct {
    float light_dir[3];
    float light_color[3];
    float light_pos[3];
    int32_t use_point_light;
    int32_t use_shadows;
} vr_lighting;

/* Per-device scene (changed only by vr_scene_edit and vr_scene_paint): region table + VCS or cuckoo storage images.
 * Replaces VoxelSceneCPU::generateVoxelScene's device pointer table
 * (geometry/VoxelSceneCPU.cuh:49-93) plus the device-side virtual adapters
 * built by the generateVoxelScene kernel (renderer/Renderer.cuh:1066-1086). */
typedef struct vr_scene vr_scene;

typedef struct {
    uint32_t diameter;       /* = VoxelSceneCPU::getArrayDiameter (VoxelSceneCPU.cuh:107-110) */
    int32_t min_coord;       /* = VoxelSceneCPU::getMinCoord (:118-121) */
    uint32_t region_count;   /* non-empty 64^3 regions */
    uint32_t store;          /* vr_store */
    uint64_t voxel_count;    /* distinct voxels after duplicate resolution */
    uint64_t device_bytes;   /* HBM footprint of the scene */
    int32_t device;
} vr_scene_info;

/* Synthetic grid generator; counter-hash occupancy. */
typedef struct {
    uint32_t n;              /* grid side, multiple of 64, <= 1024 */
    double p_region, p_cluster, p_voxel;
    uint64_t seed;
} vr_synth_params;

/* Camera::Camera(o, lookAt, globalUp, fov, aspect) (Camera.cuh:11-23), host. */
int vr_camera_make(const float eye[3], const float look_at[3], const float up[3],
                   float fov_deg, float aspect, vr_camera* out);

/* setupConstantValues defaults (Main.cu:26-42): directional light
 * normalize(1,1,1), white, point light at (10,10,-10) disabled, shadows on. */
int vr_lighting_default(vr_lighting* out);

/* Light direction as the reference uploads it: makeUnitVector(dir)
 * (Main.cu:28, Vector3.cuh:162-165: v / sqrtf(x*x+y*y+z*z), three divides).
 * VR_E_INVALID for a zero, NaN or infinite vector. Other lighting fields are
 * plain data (light_color, light_pos, use_point_light, use_shadows). */
int vr_lighting_set_direction(vr_lighting* lit, const float dir[3]);

/* VoxelSceneCPU::insertVoxel for every voxel (VoxelSceneCPU.cuh:16-46), then
 * generateVoxelScene(storageType) (:49-93) -- VoxelClusterStore ctor
 * (storage/VoxelClusterStore.cuh:37-85) or CuckooHashTable ctor
 * (storage/CuckooHashTable.cuh:20-49,97-178) per region -- and the upload to
 * `device`.  xyz: 3n int32 world voxel coordinates; rgb: n colours
 * 0x00RRGGBB (must be < 2^24).  Later duplicates overwrite earlier ones. */
int vr_scene_create(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb,
                    size_t n, vr_scene** out);

/* Where the scene image is built.  DEVICE: region
 * bucketing, a stable radix sort by (region, cluster, key), last-insertion
 * dedupe, mask records and cuckoo tables on the GPU; HOST: the same on the
 * CPU.  Both produce byte-identical device images (vr_scene_digest).  AUTO =
 * DEVICE (what vr_scene_create uses). */
typedef enum { VR_BUILD_AUTO = 0, VR_BUILD_DEVICE = 1, VR_BUILD_HOST = 2 } vr_build;

/* vr_scene_create with the voxel arrays optionally already on `device`
 * (inputs_on_device != 0) and an explicit builder; `stream` orders the device
 * build (NULL = default stream).  Returns when the scene is ready. */
int vr_scene_create_ex(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n,
                       int inputs_on_device, vr_build build, void* stream, vr_scene** out);

/* FNV-1a digest of each device buffer (region table, VCS masks, VCS colours,
 * cuckoo meta, cuckoo slots) -- to compare builds. */
int vr_scene_digest(const vr_scene* s, uint64_t out[5]);

/* VoxelFile::readVoxelFile (geometry/VoxelFile.cuh:9-35) + vr_scene_create.
 * Unlike the reference the path is used as given (no "resources/" prefix).
 * Accepts the .vox CSV (parsed in parallel, same rules and first-error line)
 * or the .vxb binary sidecar (detected by its magic). */
int vr_scene_load_vox(int device, vr_store store, const char* path, vr_scene** out);

int vr_scene_get_info(const vr_scene* s, vr_scene_info* out);
void vr_scene_destroy(vr_scene* s);

/* As an edit's colour: delete the voxel. */
#define VR_VOXEL_REMOVE 0xFFFFFFFFu

/* Edit a scene in place: VoxelSceneCPU::insertVoxel (VoxelSceneCPU.cuh:16-46) for a batch,
 * plus removal, without building the scene again.  Applies n edits in order: edit i sets
 * voxel xyz[3i..3i+2] (world voxel coordinates) to colour rgb[i] (< 2^24: inserts or
 * overwrites) or, with rgb[i] == VR_VOXEL_REMOVE, deletes it (absent: no-op).  Later edits
 * of a coordinate win over earlier ones.  inputs_on_device != 0: xyz/rgb are buffers on the
 * scene's device.
 *
 * The scene keeps its grid frame (diameter, min_coord).  Afterwards the five buffers of
 * vr_scene_digest are byte for byte what vr_scene_create over the edited voxel set
 * produces whenever that build has the same frame (regions born or emptied, clusters that
 * appear or vanish, value indices, table sizes, bases and the cuckoo placement included);
 * vr_scene_get_info reports the new voxel_count, region_count and device_bytes.
 *
 * All or nothing -- the scene is left exactly as it was when the call fails:
 *   VR_E_INVALID  s NULL; xyz or rgb NULL with n > 0; a colour >= 2^24 other than
 *                 VR_VOXEL_REMOVE, or a voxel whose 64^3 region lies outside the frame (the
 *                 message names the first such index; growing the frame needs
 *                 vr_scene_create); a VCS scene that would pass 65536 occupied regions; a
 *                 stream that is capturing a HIP graph
 *   VR_E_BUILD    a cuckoo region that cannot be built
 * n == 0 returns VR_OK and does nothing.
 *
 * Ordering: the work runs on `stream` (NULL = the null stream) and the call returns when
 * the edited scene is ready, as vr_scene_create_ex does.  Renders of this scene queued
 * earlier on `stream` see the old scene; the old buffers are released only after they
 * have finished.  The caller must have NO render of this scene in flight on another
 * stream, and must not call vr_scene_edit, vr_scene_voxels or vr_render* on this scene
 * from another thread meanwhile. */
int vr_scene_edit(vr_scene* s, const int32_t* xyz, const uint32_t* rgb, size_t n,
                  int inputs_on_device, void* stream);

/* The scene's voxels (after duplicate resolution): the inverse of vr_scene_create, e.g. to
 * save an edited scene with vr_vxb_write.  Each stored voxel once, ordered by ascending
 * region index (x + y * diameter + z * diameter^2 of its region in the frame), then in the
 * store's key order inside a region: the hash table's by x<<20 | y<<10 | z of the local
 * coordinates, the cluster store's by cluster id (x>>3)<<6 | (y>>3)<<3 | z>>3, then by
 * (x&7)<<6 | (y&7)<<3 | z&7.  Two-call protocol like vr_vox_read: with xyz == NULL only
 * counts (*n_out); otherwise writes voxel_count voxels (3 int32 world coordinates + 1
 * colour each) and sets *n_out; a capacity below the count returns VR_E_INVALID with
 * *n_out set.  outputs_on_device != 0: xyz/rgb are buffers on the scene's device.  Runs on
 * `stream` and returns when the arrays are written. */
int vr_scene_voxels(const vr_scene* s, int32_t* xyz, uint32_t* rgb, size_t capacity,
                    int outputs_on_device, void* stream, size_t* n_out);

/* vr_scene_lookup's answer for a voxel that is not stored.  Equal to VR_VOXEL_REMOVE on purpose:
 * vr_scene_edit(xyz, vr_scene_lookup(xyz)) changes nothing. */
#define VR_VOXEL_ABSENT 0xFFFFFFFFu

/* What is stored at (x, y, z): rgb[i] is the stored colour (< 2^24) of world voxel xyz[3i..3i+2]
 * (the coordinates vr_scene_edit, vr_scene_voxels and vr_hit.voxel use), or VR_VOXEL_ABSENT.
 * Set membership in the voxel set vr_scene_voxels returns -- e.g. whether a pick's
 * voxel + normal really is empty, a collision probe, occupancy sampling -- and not the
 * reference lookups' behaviour for coordinates outside a region: a world coordinate always has
 * local coordinates in [0, 64).
 *
 * No voxel is rejected.  Any int32 coordinates, INT32_MIN and INT32_MAX included, whose 64^3
 * region (floor(c / 64) per axis) lies outside the scene's frame give ABSENT, as do a null
 * region, an absent cluster and an absent key.
 *
 * xyz: 3n int32, on the scene's device when inputs_on_device != 0; rgb: n words, on the device
 * when outputs_on_device != 0.  Host arrays are staged through device buffers the call allocates
 * and frees; with everything on the device it allocates nothing.  The work (one small kernel,
 * one lane per query) runs on `stream` and the call returns when rgb[0..n) are written.
 * n == 0 returns VR_OK and does nothing.  As a pick, a lookup is not a render launch: no ring
 * slot, nothing learned or forgotten.
 *
 * VR_E_INVALID: s NULL; xyz or rgb NULL with n > 0; n >= 2^31; a stream that is capturing a HIP
 * graph. */
int vr_scene_lookup(const vr_scene* s, const int32_t* xyz, size_t n, int inputs_on_device,
                    uint32_t* rgb, int outputs_on_device, void* stream);

/* Recolour stored voxels in place, without the rebuild vr_scene_edit makes: edit i sets the
 * colour of voxel xyz[3i..3i+2] to rgb[i] (< 2^24) if that voxel is stored; otherwise it does
 * nothing and the voxel is counted in *n_absent (may be NULL).  A paint never inserts and never
 * removes.  Later edits of a coordinate win over earlier ones, whatever the batch's size or
 * order otherwise.  inputs_on_device != 0: xyz/rgb are buffers on the scene's device.
 *
 * Afterwards the five buffers of vr_scene_digest are byte for byte what vr_scene_edit gives for
 * the same batch restricted to stored voxels, and what vr_scene_create gives for the recoloured
 * voxel set; vr_scene_get_info is unchanged.  The cost is O(n) -- three small kernels and one
 * 8-byte readback -- and nothing is sized by the scene; with the arrays on the device the call
 * allocates nothing (the scene's first paint allocates 8 bytes that the scene keeps).
 *
 * Every check comes before any write.  VR_E_INVALID, with the scene untouched: s NULL; xyz or
 * rgb NULL with n > 0; n >= 2^31; a colour >= 2^24 (the message names the first such index;
 * VR_VOXEL_REMOVE is such a colour: to remove, use vr_scene_edit); a stream that is capturing a
 * HIP graph.  n == 0 returns VR_OK and does nothing (*n_absent = 0).
 * A HIP error after the writes have begun returns VR_E_HIP: the colours of the batch's voxels
 * are then unspecified (every other voxel, and the scene's structure, are as they were).
 *
 * Ordering is vr_scene_edit's: the work runs on `stream` and the call returns when the colours
 * are written.  Renders of this scene queued earlier on `stream` see the old colours.  The caller
 * must have NO render of this scene in flight on another stream, and must not call
 * vr_scene_edit, vr_scene_paint, vr_scene_voxels or vr_render* on this scene from another thread
 * meanwhile.
 *
 * Unlike vr_scene_edit, a paint does not make the next render a first render: the scene's
 * buffers are not replaced and its views keep their learned orders and crawl skips (vr_forget_orders
 * is not implied).  That is sound because no walk reads a colour except to compare it with the
 * empty marker, and the shadow walk starts whatever the lit colour is: a recolour changes
 * neither which pixels defer to the crawl pass nor any walk's length. */
int vr_scene_paint(vr_scene* s, const int32_t* xyz, const uint32_t* rgb, size_t n,
                   int inputs_on_device, void* stream, size_t* n_absent /* may be NULL */);

/* vr_hit.status */
#define VR_HIT_MISS    0u  /* the walk left the scene: the pixel is background */
#define VR_HIT_VOXEL   1u  /* the walk read a stored voxel */
#define VR_HIT_NEVER   2u  /* the reference's primary walk would never finish (the render writes 0) */
#define VR_HIT_OUTSIDE 3u  /* px >= width or py >= height: no ray */

/* The primary hit behind one pixel: what the rendered pixel was shaded from. */
typedef struct {            /* 64 bytes, 16-byte aligned records */
    uint32_t status;        /* VR_HIT_* ; every other field is 0 unless VOXEL */
    uint32_t color;         /* the stored colour the walk read (0x00RRGGBB, unlit) */
    int32_t  voxel[3];      /* world voxel coordinates: what vr_scene_edit / vr_scene_voxels use */
    int32_t  normal[3];     /* the normal the lighting used: one component +-1, others 0 */
    int32_t  region[3];     /* currentRegion at the hit */
    float    point[3];      /* region-local hit location: applyLighting's point, the shadow ray's origin */
    uint32_t reserved[2];   /* 0 */
} vr_hit;

/* Which voxel, face and hit point lie behind pixels of a frame: for each of n queries the hit
 * that vr_render's pixel (px[i], py[i]) -- the word at py * width + px, y = 0 the top row --
 * is shaded from, for the same scene, algorithm, camera, translation, scale and frame size.
 * The ray and the primary walk are the render's, bit for bit (walks of any length run to
 * their end; one the reference would never finish gives VR_HIT_NEVER).  No lighting is taken:
 * only the primary walk runs, no shadow walk.
 *
 *   voxel   the stored voxel whose colour the walk read, in world voxel coordinates
 *           (region * 64 + the matched key's local x, y, z): vr_scene_voxels contains
 *           (voxel, color), and vr_scene_edit takes it as it is.
 *   normal  the REFERENCE's normal, the one the lighting used (getNormalFromTValues,
 *           Renderer.cuh:237-247, or the axis step's): not always the geometric face the ray
 *           crossed.  voxel + normal is usually the empty neighbour to build on, but that
 *           is not guaranteed (vr_scene_lookup tells).
 *   point   region-local.  The scene-space position is region * 64 + point; the lighting's
 *           world point is translation + region * 64 + point (unscaled, as the reference's).
 *
 * px, py: n uint32 each, on the scene's device when inputs_on_device != 0; hits: n records,
 * on the device (16-byte aligned) when outputs_on_device != 0.  Host arrays are staged
 * through device buffers the call allocates and frees; with everything on the device it
 * allocates nothing.  The work runs on `stream` and the call returns when hits[0..n) are
 * written, as vr_scene_voxels does.  n == 0 returns VR_OK and does nothing.
 *
 * A pick is not a render launch: it takes no slot of the per-device ring, learns and forgets
 * no order, and renders before and after it behave as if it had not happened.
 *
 * VR_E_INVALID: s, cam or translation NULL; px, py or hits NULL with n > 0; width or height
 * outside 1..65536; n >= 2^31; an unknown algorithm; a stream that is capturing a HIP graph. */
int vr_pick(const vr_scene* s, vr_algo algo, const vr_camera* cam,
            const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
            const uint32_t* px, const uint32_t* py, size_t n, int inputs_on_device,
            vr_hit* hits, int outputs_on_device, void* stream);

/* One ray of vr_trace. */
typedef struct {            /* 32 bytes, 16-byte aligned records: two 16-byte loads */
    float    origin[3];     /* world space, as a camera's ray origin */
    uint32_t reserved0;     /* write 0; not read */
    float    direction[3];  /* world space, any length: the walk uses makeUnitVector(direction) */
    uint32_t reserved1;     /* write 0; not read */
} vr_ray;

/* Which lane walks which ray of a vr_trace call.  The records never depend on it.
 * AUTO is GIVEN for every n: measured on C2 and C4 at 1920x1080 with 4096 to 2 073 600 rays
 * (tile-order, shuffled and bounce rays; key kernel and sort included; this change on top of
 * fb3c0b6, profiles/trace/README.md), COHERENT won at no size -- the sort costs more than the
 * incoherence it removes (2 073 600 shuffled C2 rays: 0.457 ms GIVEN, 0.697 ms COHERENT).  The
 * mode stays: it is exact and tested, and a caller whose rays are worse than a shuffle can
 * ask for it. */
typedef enum {
    VR_TRACE_ORDER_AUTO = 0,      /* the library's measured choice: GIVEN */
    VR_TRACE_ORDER_GIVEN = 1,     /* lane i of the launch walks ray i */
    VR_TRACE_ORDER_COHERENT = 2   /* rays sorted on the device by direction signs, origin cell and direction */
} vr_trace_order;

/* Closest-hit queries for arbitrary rays: hits[i] is the primary hit of rays[i], the record
 * vr_pick writes (status VR_HIT_MISS, VR_HIT_VOXEL or VR_HIT_NEVER, never VR_HIT_OUTSIDE; every
 * other field 0 unless VOXEL; voxel, color, normal, region and point as for vr_pick).  The walk
 * is rayMarchVoxelScene / rayMarchVoxelSceneLongestAxis from world origin rays[i].origin in
 * direction d / sqrtf(d.x*d.x + d.y*d.y + d.z*d.z), d = rays[i].direction (makeUnitVector,
 * Vector3.cuh:162-165: correctly rounded sqrt and divisions); the scene-space origin is
 * (origin - translation) * scale, as in a render.
 *
 * No ray is rejected.  A zero, NaN or infinite direction or origin gives the record the
 * reference's walk gives for it (a zero direction normalises to NaN; from inside the scene the
 * original walk then never finishes: VR_HIT_NEVER): no status is promised for such rays, only
 * that the record equals the reference's.
 *
 * order (vr_trace_order) decides only the execution order: the records are byte for byte the
 * same under every order and hits[i] always belongs to rays[i].  COHERENT computes a 64-bit key
 * per ray and sorts (key, index) on the device; its scratch (12 bytes per ray for keys and
 * indices, twice, plus the sort's temporary) is allocated on the scene's device for the call
 * and released before it returns.
 *
 * rays: n records, on the scene's device (16-byte aligned) when inputs_on_device != 0; hits: n
 * records, on the device (16-byte aligned) when outputs_on_device != 0.  Host arrays are
 * staged through device buffers the call allocates and frees; GIVEN with everything on the
 * device allocates nothing.  The work runs on `stream` and the call returns when hits[0..n) are
 * written.  n == 0 returns VR_OK and does nothing.  As a pick, a trace is not a render launch:
 * no ring slot, nothing learned or forgotten.
 *
 * VR_E_INVALID (nothing is written to hits): s or translation NULL; rays or hits NULL with
 * n > 0; n >= 2^31; an unknown algorithm; an unknown order; a misaligned device array; a
 * stream that is capturing a HIP graph. */
int vr_trace(const vr_scene* s, vr_algo algo, const float translation[3], uint32_t scale,
             const vr_ray* rays, size_t n, int inputs_on_device,
             vr_hit* hits, int outputs_on_device, uint32_t order, void* stream);

/* Lit colours, and on request hits, for arbitrary rays: colors[i] is the packed 0x00RRGGBB word
 * vr_render writes for a pixel whose ray is rays[i] -- applyLighting at the primary hit
 * (Renderer.cuh:249-258), times !shadow when lit->use_shadows.  The primary walk is vr_trace's,
 * bit for bit (from (origin - translation) * scale along makeUnitVector(direction), correctly
 * rounded sqrt and divisions); the shadow walk is the render's, from the hit's point in the
 * hit's region towards the light.  A miss gives 0; so does a primary or a shadow walk the
 * reference would never finish, which is what the render writes.  With vr_camera_rays' rays
 * of a frame's pixels the colours are that frame's render, word for word: any other set of
 * rays (a mirror bounce from a hit's point, an orthographic, fisheye or stereo view, a
 * jittered sample pattern, a light probe) gets what that render would have given it.
 *
 * hits (may be NULL): when given, hits[i] is byte for byte the record vr_trace writes for
 * rays[i], from the same walk -- a bounce ray's origin, normal and colour in one call.  Its
 * status is VR_HIT_NEVER only for a PRIMARY walk that never ends; a shadow walk that never
 * ends leaves the primary's VOXEL record beside colour 0.  The colours are the same words
 * with and without it.
 *
 * No ray is rejected (as vr_trace) and no lighting value is: light_dir is taken as plain data,
 * as vr_render takes it.  order is a vr_trace_order with vr_trace's meaning: the execution
 * order only, never a word or a record; AUTO is GIVEN.
 *
 * rays: n records, on the scene's device (16-byte aligned) when inputs_on_device != 0; colors
 * (n words, 4-byte aligned) and hits (n records, 16-byte aligned) both on the device when
 * outputs_on_device != 0, both on the host otherwise.  Host arrays are staged through device
 * buffers the call allocates and frees; GIVEN with everything on the device allocates
 * nothing.  The work runs on `stream` and the call returns when the outputs are written.
 * n == 0 returns VR_OK and does nothing.  As a trace, a shade is not a render launch: no ring
 * slot, nothing learned or forgotten.
 *
 * VR_E_INVALID (nothing is written): s, lit or translation NULL; rays or colors NULL with
 * n > 0; n >= 2^31; an unknown algorithm; an unknown order; a misaligned device array; a
 * stream that is capturing a HIP graph. */
int vr_shade(const vr_scene* s, vr_algo algo, const vr_lighting* lit,
             const float translation[3], uint32_t scale,
             const vr_ray* rays, size_t n, int inputs_on_device,
             uint32_t* colors, vr_hit* hits /* may be NULL */, int outputs_on_device,
             uint32_t order, void* stream);

/* vr_shade under several lights and an ambient term, from ONE primary walk per ray: L calls of
 * vr_shade walk every primary ray L times; this walks it once and runs one lighting-and-shadow
 * pass per light over the hits.
 *
 * Terms.  For ray i and light k, T_k(i) is the word vr_shade writes for rays[i] under lights[k]
 * -- a plain vr_lighting, taken as data exactly as vr_shade takes it: applyLighting at the
 * primary hit, times !shadow when lights[k].use_shadows, the shadow walk along that light's
 * light_dir from the hit's point in the hit's region.  T_k(i) is 0 for a miss, 0 for a primary
 * walk that never ends, and 0 for a shadow walk of light k that never ends (the other lights'
 * terms still count).  Each light keeps every quirk of the reference: a point light's shadow
 * walk still follows light_dir (Renderer.cuh:174-235).
 * The ambient term T_a(i) exists when ambient != NULL: at a primary VOXEL hit with stored colour
 * col, each channel c of col gives f2u((div255(c) * ambient[ch]) * 255.0f) -- the directional
 * formula of applyLighting with the diffuse factor 1.0f and the light's colour replaced by
 * ambient, the same fp32 operations in the same order, no contraction (f2u: NaN and negatives
 * give 0) -- packed R << 16 | G << 8 | B.  It is 0 for a miss or a primary walk that never ends,
 * and it has no shadow walk.
 *
 * Sum.  colors[i] = min(255, sum R) << 16 | min(255, sum G) << 8 | min(255, sum B) over every
 * term, with R(w) = (w >> 16) & 0xFF, G(w) = (w >> 8) & 0xFF, B(w) = w & 0xFF.  Bits 24-31 of a
 * term are dropped: they are non-zero only where light_color or an un-normalised light_dir pushes
 * a channel past 255, which bleeds in the reference's packing.  The sums are of integers, so
 * colors[i] does not depend on the order of the lights.  Hence: with n_lights == 1 and no ambient,
 * colors[i] is vr_shade's word whenever that word is below 2^24; with n_lights == 0, colors[i]
 * is the ambient term alone (bits 24-31 dropped), and 0 without ambient.
 *
 * hits (may be NULL): when given, hits[i] is byte for byte vr_shade's and vr_trace's record for
 * rays[i]; status VR_HIT_NEVER is for a primary walk only.  The colours are the same words with
 * and without it.  order is a vr_trace_order with vr_trace's meaning: the execution order only,
 * never a word or a record; AUTO is GIVEN.  No ray and no lighting value is rejected.
 *
 * lights (n_lights blocks, at most VR_MAX_LIGHTS) and ambient (three floats, or NULL) are host
 * arrays, read before the call returns.  rays, colors and hits are vr_shade's: n records on the
 * scene's device (rays and hits 16-byte, colors 4-byte aligned) when the flag says so, host
 * arrays staged through device buffers otherwise.  The call also allocates its per-ray hit
 * state (32 bytes per ray) on the scene's device and frees it before it returns, on every
 * path; a failure there is VR_E_NOMEM or VR_E_HIP.  The work runs on `stream` -- one primary
 * kernel and one kernel per light -- and the call returns when the outputs are written.
 * n == 0 returns VR_OK and does nothing.  Not a render launch: no ring slot, nothing learned or
 * forgotten.
 *
 * VR_E_INVALID (nothing is written): s or translation NULL; lights NULL with n_lights > 0;
 * n_lights > VR_MAX_LIGHTS; rays or colors NULL with n > 0; n >= 2^31; an unknown algorithm; an
 * unknown order; a misaligned device array; a stream that is capturing a HIP graph. */
#define VR_MAX_LIGHTS 64u
int vr_shade_lights(const vr_scene* s, vr_algo algo,
                    const vr_lighting* lights, size_t n_lights,
                    const float ambient[3] /* may be NULL */,
                    const float translation[3], uint32_t scale,
                    const vr_ray* rays, size_t n, int inputs_on_device,
                    uint32_t* colors, vr_hit* hits /* may be NULL */, int outputs_on_device,
                    uint32_t order, void* stream);

/* Voxel ambient occlusion: how open the face of a hit is at the hit point, from the eight voxels
 * around the cell in front of the face.  ao[i] is ao(hits[i]), 0..255, VR_AO_OPEN (255) = open.
 * It takes the records of vr_pick, vr_trace, vr_shade and vr_shade_lights, and records the caller
 * made up: no record is rejected and any 64 bytes are safe.
 *
 * ao(h) is 255 unless h.status == VR_HIT_VOXEL and h.normal has exactly one component +1 or -1
 * and the other two 0.  Otherwise, with all int32 arithmetic wrapping:
 *   axes       a is the normal's axis; the tangent axes (u, w) are (1, 2), (2, 0), (0, 1) for
 *              a = 0, 1, 2.
 *   plane cell p = h.voxel + h.normal.
 *   occupancy  o(du, dw) = 1 when world voxel p + du * e_u + dw * e_w is stored (vr_scene_lookup's
 *              meaning: outside the frame, a null region, an absent cluster and an absent key are
 *              empty), else 0.  The eight (du, dw) of {-1, 0, 1}^2 other than (0, 0) are read; p
 *              itself never is.
 *   corners    for (su, sw) in {-1, +1}^2, with s1 = o(su, 0), s2 = o(0, sw), c = o(su, sw):
 *              L(su, sw) = (s1 & s2) ? 0 : 3 - (s1 + s2 + c).
 *   position   for t in {u, w}: f_t = h.point[t] - (float)(int32)(h.voxel[t] - 64 * h.region[t]),
 *              one fp32 subtraction; g = f_t * 256.0f (exact); q_t = 0 if !(g > 0) (NaN too), 256
 *              if g >= 256, else (int)g (truncated).
 *   sum        acc = (256 - q_u)(256 - q_w) L(-1,-1) + q_u (256 - q_w) L(+1,-1)
 *                    + (256 - q_u) q_w L(-1,+1) + q_u q_w L(+1,+1)        (at most 3 * 65536)
 *   result     ao = (acc * 255 + 98304) / 196608, an integer division.
 * Applied to a colour word with a strength in 0..255 (vr_shade_lights_ao):
 *   m = 255 - ((255 - ao) * strength + 127) / 255, and scale_rgb(word, m) replaces each of the
 *   bytes R, G and B of word by (b * m + 127) / 255 and drops bits 24-31.  strength 0 gives
 *   m = 255 and changes nothing; strength 255 gives m = ao.
 *
 * hits: n records, on the scene's device (16-byte aligned) when inputs_on_device != 0; ao: n
 * words, on the device (4-byte aligned) when outputs_on_device != 0.  Host arrays are staged
 * through device buffers the call allocates and frees; with everything on the device it
 * allocates nothing.  The work (one small kernel, one lane per record) runs on `stream` and the
 * call returns when ao[0..n) are written.  n == 0 returns VR_OK and does nothing.  As a trace, it
 * is not a render launch: no ring slot, nothing learned or forgotten.
 *
 * VR_E_INVALID (nothing is written): s NULL; hits or ao NULL with n > 0; n >= 2^31; a misaligned
 * device array; a stream that is capturing a HIP graph. */
#define VR_AO_OPEN 255u
int vr_occlusion(const vr_scene* s, const vr_hit* hits, size_t n, int inputs_on_device,
                 uint32_t* ao, int outputs_on_device, void* stream);

/* Where vr_shade_lights_ao applies the occlusion. */
typedef enum {
    VR_AO_AMBIENT = 0,   /* to the ambient term only: lit faces keep their light, the rest gains its corners */
    VR_AO_ALL = 1        /* to the whole word */
} vr_ao_apply;

/* vr_shade_lights with voxel ambient occlusion, from the same single primary walk.  With
 * m_i = the factor ao_strength (0..255) makes of ao(the hit of rays[i]) (vr_occlusion above):
 *   VR_AO_AMBIENT  colors[i] is vr_shade_lights' sum with the ambient term T_a(i) replaced by
 *                  scale_rgb(T_a(i), m_i) before summing;
 *   VR_AO_ALL      colors[i] = scale_rgb(w_i, m_i), w_i vr_shade_lights' word.
 * ao_out (may be NULL): ao_out[i] = ao(the hit of rays[i]) -- 255 for a miss and for a walk that
 * never ends -- n words on the same side as colors (4-byte aligned on the device).  hits stays
 * byte for byte vr_trace's record.  With ao_strength == 0 and ao_out == NULL the call is
 * vr_shade_lights, word for word.  Every other argument is vr_shade_lights'.
 *
 * The occlusion pass reads the primary walk's records: when hits is NULL the call allocates a
 * record buffer of its own (64 bytes per ray) beside vr_shade_lights' hit state and frees it
 * before it returns.  One more small kernel runs on `stream`: after the primary kernel (AMBIENT)
 * or after the last light (ALL).
 *
 * VR_E_INVALID (nothing is written): vr_shade_lights' cases; ao_strength > 255; an unknown
 * ao_apply; a misaligned device ao_out. */
int vr_shade_lights_ao(const vr_scene* s, vr_algo algo,
                       const vr_lighting* lights, size_t n_lights,
                       const float ambient[3] /* may be NULL */,
                       const float translation[3], uint32_t scale,
                       const vr_ray* rays, size_t n, int inputs_on_device,
                       uint32_t* colors, vr_hit* hits /* may be NULL */, int outputs_on_device,
                       uint32_t order, void* stream,
                       uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out /* may be NULL */);

/* The mirror bounce of a ray at its hit: out[i] = bounce(rays[i], hits[i]), the ray that leaves the
 * hit point along the incoming direction mirrored in the hit face.  It takes the records of
 * vr_pick, vr_trace, vr_shade and vr_shade_lights, and records the caller made up: no record is
 * rejected and any 64 bytes are safe.  No mirror test is applied: every VOXEL record bounces.
 *
 * bounce(ray, h) is defined when h.status == VR_HIT_VOXEL and h.normal has exactly one component +1
 * or -1 and the other two 0 (vr_occlusion's condition); a is the normal's axis.  Then
 *   origin[c]  = translation[c] + (((float)h.region[c] * 64.0f + h.point[c]) / (float)scale) for
 *                each component c: int-to-float, multiply, add and divide, then the translation's
 *                addition, each rounded to fp32 on its own in that order, the division correctly
 *                rounded, no contraction -- the hit point back in world space;
 *   direction  = ray.direction with the sign bit of component a flipped, the other two components
 *                bitwise unchanged.  Nothing is normalised: the magnitude survives every depth.
 *                For a direction without a zero component this is d - 2 (d . n) n to the bit; a
 *                zero, infinite or NaN component on the axis has its sign flipped all the same.
 *   reserved0 and reserved1 are 0.
 * For every other record the six floats are the quiet NaN 0x7FC00000, as vr_camera_rays writes for
 * a pixel outside the frame.  Such a ray is NOT harmless to trace: on the golden scene it gives
 * VR_HIT_NEVER under three store/algorithm pairs and a VOXEL record under the hash table with the
 * longest-axis walk.  A caller who traces the bounces must mask the results by the first
 * record's status (vr_shade_lights_reflect below does the descent on the device and walks no such
 * ray).  ray.origin is not read.
 *
 * Runs on `device` (no scene is needed) as one small kernel on `stream`, one lane per record, with
 * 16-byte loads and stores.  rays and hits are both host arrays, or both on the device (16-byte
 * aligned) when inputs_on_device != 0; out is on the device (16-byte aligned) when
 * outputs_on_device != 0; host arrays are staged as vr_camera_rays stages them.  Returns when
 * out[0..n) are written.  n == 0 returns VR_OK.
 *
 * VR_E_INVALID (nothing is written): translation NULL; rays, hits or out NULL with n > 0;
 * n >= 2^31; device outside 0..63 or not present; a misaligned device array; a stream that is
 * capturing a HIP graph. */
int vr_bounce_rays(int device, const float translation[3], uint32_t scale,
                   const vr_ray* rays, const vr_hit* hits, size_t n, int inputs_on_device,
                   vr_ray* out, int outputs_on_device, void* stream);

/* vr_shade_lights_ao with mirror reflections, the whole descent on the device: no record leaves
 * it and no ray that does not reflect is walked again.
 *
 * With B = bounces (at most VR_MAX_BOUNCES) and k = reflectivity (0..255), ray^0_i = rays[i] and
 * for depth j = 0..B:
 *   W^j_i     the word vr_shade_lights_ao writes for ray^j_i under the same lights, ambient,
 *             ao_strength and ao_apply, and H^j_i its record;
 *   refl^j_i  H^j_i.status == VR_HIT_VOXEL and (H^j_i.color & mirror_mask) == mirror_value and
 *             (j == 0 or refl^(j-1)_i);
 *   ray^(j+1)_i = bounce(ray^j_i, H^j_i) (vr_bounce_rays above) where refl^j_i and j < B.
 * Folded from the back: C^B_i = W^B_i, and for j = B - 1..0
 *   C^j_i = refl^j_i ? mix(W^j_i, C^(j+1)_i, k) : W^j_i,        colors[i] = C^0_i,
 * where mix(a, b, k) replaces each of the bytes R, G and B by (A * (255 - k) + B * k + 127) / 255,
 * an integer division, and drops bits 24-31: k = 0 gives a and k = 255 gives b.  A bounce that
 * misses, or whose walk never ends, contributes W = 0: a mirror shows the black background the
 * renderer writes there.
 *
 * mirror_mask = 0 and mirror_value = 0: every voxel reflects.  A material bit (mask 1, value 1) or
 * a key colour (mask 0xFFFFFF) selects the mirror voxels by their stored colour; vr_scene_paint
 * paints them.  hits and ao_out belong to depth 0: hits[i] stays byte for byte vr_trace's record for
 * rays[i].  order applies to depth 0; deeper depths run in the order of their lists, and no word
 * depends on either.  With reflectivity == 0 or bounces == 0 the call is vr_shade_lights_ao, word
 * for word: no extra kernel, allocation or readback.  Every other argument is vr_shade_lights_ao's.
 *
 * Per depth j >= 1 the call runs one small kernel that makes the bounce rays and the compact list
 * of the rays that reflected, reads the list's 4-byte count back on `stream` (a wait for the
 * stream per depth; a count of 0 ends the descent), runs vr_shade_lights_ao's kernels over the list
 * alone -- the occlusion kernel, where ao_strength != 0, over all n records -- and at the end one
 * small fold kernel per depth reached.  Beside vr_shade_lights_ao's buffers it allocates on the
 * scene's device, in one allocation, and frees before it returns on every path: one ray buffer
 * (two when bounces > 1; 32 bytes per ray each), per depth asked for a colour buffer and a list (4
 * bytes per ray each), the counts, and a record buffer (64 bytes per ray) when ao_strength != 0.
 * A failure there is VR_E_NOMEM or VR_E_HIP.  Not a render launch: no ring slot, nothing learned
 * or forgotten.
 *
 * VR_E_INVALID (nothing is written; every check comes before any device work): vr_shade_lights_ao's
 * cases; reflectivity > 255; bounces > VR_MAX_BOUNCES; mirror_value with a bit outside mirror_mask
 * (it could never match). */
#define VR_MAX_BOUNCES 4u
int vr_shade_lights_reflect(const vr_scene* s, vr_algo algo,
                            const vr_lighting* lights, size_t n_lights,
                            const float ambient[3] /* may be NULL */,
                            const float translation[3], uint32_t scale,
                            const vr_ray* rays, size_t n, int inputs_on_device,
                            uint32_t* colors, vr_hit* hits /* may be NULL */, int outputs_on_device,
                            uint32_t order, void* stream,
                            uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out /* may be NULL */,
                            uint32_t reflectivity, uint32_t bounces, uint32_t mirror_mask, uint32_t mirror_value);

/* Sky and distance fog: what a ray that hits nothing sees, and how a hit fades with its distance.
 * A vr_atmosphere is plain data: nothing in it is rejected but unknown flag bits, and nothing is
 * normalised. */
#define VR_ATMOS_SKY 1u   /* a MISS shows the sky in the direction of its ray */
#define VR_ATMOS_FOG 2u   /* a VOXEL hit is blended towards fog_color by its distance */
typedef struct {
    float zenith[3], horizon[3], nadir[3];  /* sky colours, 1.0 = 255, plain data */
    float up[3];                            /* plain data, NOT normalised by the library */
    float fog_color[3];
    float fog_start, fog_end;               /* world units, plain data */
    uint32_t flags;                         /* VR_ATMOS_SKY | VR_ATMOS_FOG */
    uint32_t reserved;                      /* 0 */
} vr_atmosphere;
/* A daylight sky: zenith (0.25, 0.45, 0.85), horizon (0.75, 0.85, 0.95), nadir (0.30, 0.28, 0.25),
 * up (0, 1, 0), fog_color the horizon's, fog_start 0, fog_end 16, flags VR_ATMOS_SKY (fog off),
 * reserved 0.  VR_E_INVALID for NULL. */
int vr_atmosphere_default(vr_atmosphere* atm);

/* out[i] = atmos(colors_in[i], rays[i], hits[i]): the colour word of a ray under an atmosphere.  It
 * takes the records of vr_pick, vr_trace, vr_shade and vr_shade_lights, and records the caller made
 * up: no record and no ray is rejected and any 64 bytes are safe.
 *
 * All floating-point arithmetic is fp32, each operation rounded on its own in the order written
 * (the parentheses are the order), no contraction, divisions and square roots correctly rounded.
 *   colour bytes  byte(x) = min(255, f2u(x * 255.0f)), f2u as in vr_shade_lights' ambient term: NaN
 *                 and values <= 0 give 0, everything else truncates.  Z, H, N and F are the words
 *                 byte(c[0]) << 16 | byte(c[1]) << 8 | byte(c[2]) of zenith, horizon, nadir and
 *                 fog_color, made once per call.
 *   q256(f)       g = f * 256.0f; 0 if !(g > 0) (NaN too), 256 if g >= 256, else (int)g, truncated:
 *                 vr_occlusion's position rule.
 *   lerp256(a, b, q)  each of the bytes R, G and B is (A * (256 - q) + B * q + 128) >> 8; bits 24-31
 *                 are dropped.  q = 0 gives a and q = 256 gives b (below 2^24).
 *   sky(d)        for a ray direction d of any length: len = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z),
 *                 h = ((d.x*up.x + d.y*up.y) + d.z*up.z) / len,
 *                 sky = lerp256(H, h < 0 ? N : Z, q256(fabsf(h))).  A zero, infinite or NaN direction
 *                 gives whatever these operations give; a NaN h gives H.
 *   fog(w, ray, h)  p[c] = translation[c] + (((float)h.region[c] * 64.0f + h.point[c]) / (float)scale),
 *                 vr_bounce_rays' origin: the hit point back in world space; e[c] = p[c] - ray.origin[c];
 *                 D = sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z);
 *                 f = (D - fog_start) / (fog_end - fog_start); fog = lerp256(w, F, q256(f)).
 *                 fog_end <= fog_start is taken as data: a step or an inverted ramp, as the operations
 *                 say.  The fog needs no unit normal: every VOXEL record has it.
 *   atmos(w, ray, h)  h.status == VR_HIT_MISS and flags has VR_ATMOS_SKY: sky(ray.direction);
 *                 h.status == VR_HIT_VOXEL and flags has VR_ATMOS_FOG: fog(w, ray, h);
 *                 every other case (NEVER, OUTSIDE, an unknown status, a flag not set): w, bit for bit.
 * The fog is linear on purpose: an exponential needs an exp that two implementations would not
 * share to the bit.
 *
 * Runs on `device` (no scene is needed) as one small kernel on `stream`, one lane per record, with
 * 16-byte loads of rays and records.  rays, hits and colors_in are all host arrays, or all on the
 * device (rays and hits 16-byte, colors_in 4-byte aligned) when inputs_on_device != 0; colors_out is
 * on the device (4-byte aligned) when outputs_on_device != 0, and may then be colors_in itself; host
 * arrays are staged as vr_bounce_rays stages them.  Returns when colors_out[0..n) are written.
 * n == 0 returns VR_OK.  Not a render launch.
 *
 * VR_E_INVALID (nothing is written): atm or translation NULL; atm->flags with a bit other than
 * VR_ATMOS_SKY | VR_ATMOS_FOG; rays, hits, colors_in or colors_out NULL with n > 0; n >= 2^31;
 * device outside 0..63 or not present; a misaligned device array; a stream that is capturing a HIP
 * graph. */
int vr_atmosphere_apply(int device, const vr_atmosphere* atm, const float translation[3], uint32_t scale,
                        const vr_ray* rays, const vr_hit* hits, const uint32_t* colors_in, size_t n,
                        int inputs_on_device, uint32_t* colors_out, int outputs_on_device, void* stream);

/* vr_shade_lights_reflect under an atmosphere, on the device: with atm == NULL or atm->flags == 0
 * the call is vr_shade_lights_reflect kernel for kernel -- no extra launch, allocation or readback.
 * Otherwise A^j_i = atmos(W^j_i, ray^j_i, H^j_i) (vr_atmosphere_apply above) replaces W^j_i everywhere
 * in vr_shade_lights_reflect's fold:
 *   C^B_i = A^B_i,   C^j_i = refl^j_i ? mix(A^j_i, C^(j+1)_i, k) : A^j_i,   colors[i] = C^0_i.
 * The fog is per leg: a bounce ray's origin is the previous hit point, so D is the length of that
 * leg alone.  A miss at any depth shows the sky in the direction of that depth's ray: a mirror
 * shows the sky.  The mirror test, hits and ao_out are untouched: they read stored colours and
 * records, never the tinted word.  A walk that never ends keeps its word 0.
 *
 * One more small kernel per depth reached runs on `stream`, after that depth's last colour pass; it
 * allocates nothing.  Every other argument is vr_shade_lights_reflect's.
 *
 * VR_E_INVALID (nothing is written; every check comes before any device work):
 * vr_shade_lights_reflect's cases; atm->flags with a bit other than VR_ATMOS_SKY | VR_ATMOS_FOG. */
int vr_shade_lights_atmosphere(const vr_scene* s, vr_algo algo,
                               const vr_lighting* lights, size_t n_lights,
                               const float ambient[3] /* may be NULL */,
                               const float translation[3], uint32_t scale,
                               const vr_ray* rays, size_t n, int inputs_on_device,
                               uint32_t* colors, vr_hit* hits /* may be NULL */, int outputs_on_device,
                               uint32_t order, void* stream,
                               uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out /* may be NULL */,
                               uint32_t reflectivity, uint32_t bounces, uint32_t mirror_mask, uint32_t mirror_value,
                               const vr_atmosphere* atm /* may be NULL */);

/* The ray a render or pick walks for pixel (px[i], py[i]) of a width x height frame (y = 0 the
 * top row): origin is the image-plane point lower_left + u * horizontal + v * vertical, with
 * the render's bits; direction is origin - cam->origin, NOT normalised -- vr_trace applies the
 * very division the render applies, so vr_trace(vr_camera_rays(px, py)) is byte-identical to
 * vr_pick(px, py) for every pixel inside the frame.  A pixel with px >= width or py >= height
 * gets a ray whose six floats are the quiet NaN 0x7FC00000.  reserved0 and reserved1 are
 * written as 0.
 *
 * Runs on `device` (no scene is needed) as one small kernel on `stream`; px, py and rays are
 * host arrays, or device arrays (rays 16-byte aligned) when the flags say so, staged as
 * vr_pick stages them; returns when rays[0..n) are written.  n == 0 returns VR_OK.
 *
 * VR_E_INVALID: cam NULL; px, py or rays NULL with n > 0; width or height outside 1..65536;
 * n >= 2^31; device outside 0..63 or not present; a stream that is capturing a HIP graph. */
int vr_camera_rays(int device, const vr_camera* cam, uint32_t width, uint32_t height,
                   const uint32_t* px, const uint32_t* py, size_t n, int inputs_on_device,
                   vr_ray* rays, int outputs_on_device, void* stream);

/* rayMarchSceneOriginal / rayMarchSceneJumpAxis (Renderer.cuh:1033-1063) as
 * launched by runRaymarchingKernel (Main.cu:105-163), for image rows
 * [row_begin, row_end) of a width x height frame.  out_dev: device buffer of
 * (row_end-row_begin)*width uint32, row-major, y = 0 the top row, each the
 * packed 0x00RRGGBB word the reference hands to writeColorToFramebuffer
 * (Renderer.cuh:1024-1031).  translation/scale = VoxelSceneInfo
 * (renderer/VoxelSceneInfo.cuh:5-15).  Asynchronous on `stream`. */
int vr_render(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
              const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
              uint32_t row_begin, uint32_t row_end, uint32_t* out_dev, void* stream);

/* Multi-GPU tile partition: the frame is cut into bands of band_rows rows;
 * band b belongs to rank b % nranks.  out_dev holds this rank's bands packed
 * in order: ceil(ceil(height/band_rows)/nranks)*band_rows*width uint32
 * (rows past the frame or past this rank's last band are written as 0), so
 * every rank's buffer has the same size for an RCCL gather. */
int vr_render_bands(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                    uint32_t band_rows, uint32_t rank, uint32_t nranks, uint32_t* out_dev,
                    void* stream);
/* Number of uint32 words vr_render_bands writes per rank. */
uint64_t vr_band_buffer_words(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t nranks);

/* The 2-D tile deal (vr_render_opts.tile_cols): every band_rows-row band of the frame is
 * cut into column blocks of tile_cols pixels, block j of band b -> rank (j + stride*b) %
 * nranks.  Row bands alone put a cluster of expensive rows (C5's crawl rows) on one or two
 * ranks; the deal gives every rank a share of every band while each 8x8 wave tile stays
 * whole.  out_dev: vr_tile_buffer_words(...) uint32 per rank (same for every rank). */
int vr_render_tiles(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                    uint32_t band_rows, uint32_t tile_cols, uint32_t rank, uint32_t nranks,
                    uint32_t* out_dev, void* stream);
uint64_t vr_tile_buffer_words(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t tile_cols,
                              uint32_t nranks);
/* The stride the deal uses when deal_stride is 0: 3 (a knight's-move deal) unless it
 * shares a factor with nranks, else 1. */
uint32_t vr_deal_stride_default(uint32_t nranks);
/* Rank 0's reassembly after the gather: parts_dev holds the nranks tile buffers back to
 * back (each vr_tile_buffer_words(...) pixels of elem_bytes bytes: 4 for the packed words,
 * 3 for RGB8), frame_dev receives the width x height image (row-major, elem_bytes per
 * pixel).  deal_stride 0 = the default.  Asynchronous on `stream`. */
int vr_assemble_tiles(const void* parts_dev, void* frame_dev, uint32_t elem_bytes, uint32_t width,
                      uint32_t height, uint32_t band_rows, uint32_t tile_cols, uint32_t nranks,
                      uint32_t deal_stride, void* stream);

/* Kernel implementations behind vr_render*: all produce identical pixels.
 * (Value 2 was a persistent state-machine kernel, retired in round 3: it was
 * never the fastest; it is rejected with VR_E_INVALID.) */
typedef enum {
    VR_KERNEL_AUTO = 0,         /* the fastest measured for the (store, algorithm) pair */
    VR_KERNEL_TILE = 1,         /* one lane per pixel, one wave per 8x8 tile (vr_march.hip) */
    VR_KERNEL_TILE_REWALK = 3   /* the tile kernel whose crawl pass walks every deferred pixel
                                   from its start instead of resuming it (cross-check) */
} vr_kernel;

/* Full-control render (the other vr_render* calls are wrappers of this):
 * rows [row_begin,row_end) of the frame cut into bands of band_rows rows,
 * band b rendered when b % nranks == rank; out_dev gets this rank's bands
 * packed as in vr_render_bands.  bytes_dev (optional, device uint64,
 * caller-zeroed) accumulates the SURVEY.md 8(d) algorithmic bytes.
 *
 * Versioned by its leading size: set struct_size = sizeof(vr_render_opts)
 * (vr_render_opts_init does, with every other field at its default).  The
 * library rejects (VR_E_INVALID) a struct_size below VR_RENDER_OPTS_MIN_SIZE --
 * the layout before this field existed began with `kernel` (0..3), so a caller
 * built against it is refused instead of having fields read past its struct --
 * and treats fields that lie past struct_size as zero (callers built against
 * an older, shorter version of this layout keep working). */
typedef struct {
    uint32_t struct_size; /* sizeof(vr_render_opts) as the caller was compiled */
    uint32_t kernel;      /* vr_kernel */
    uint32_t row_begin, row_end;
    uint32_t band_rows;   /* 0 = one band covering [row_begin,row_end) */
    uint32_t rank, nranks;
    uint32_t defer_cap;   /* records in the crawl pass's deferral list: 0 = the default (16384);
                             smaller values exercise its overflow path (tests) */
    uint64_t* bytes_dev;
    uint32_t schedule;    /* vr_schedule: the tile pass's work order (pixels never depend on it) */
    uint32_t reserved;    /* 0 */
    /* (optional, device uint64[2], caller-zeroed; read only with bytes_dev) the part of
     * bytes_dev's count that the kernels credit without loading it: [0] cluster-skip crawl
     * iterations fast-forwarded in closed form (Renderer.cuh:290-306, performVoxelSpaceJump
     * :707-725), [1] the existence-read bytes credited without a load -- 4 per fast-forwarded
     * iteration and 4 per crawl-pass skip step answered from its LDS copy of the region's
     * cluster-existence bits.  bytes_dev - [1] = the bytes the kernels' own loads stand for. */
    uint64_t* stats_dev;
    /* (round 5) vr_occupancy: which occupancy variant of the tile pass renders.  The
     * uninstrumented cuckoo `original` and VCS `longestaxis` walks have a higher-occupancy
     * variant for frames in flight; AUTO takes it when another stream's launch is still
     * running on the device.  Pixels never depend on it.  Instrumented launches (bytes_dev)
     * always run the lone variant. */
    uint32_t occupancy;
    /* (round 5) 2-D tile deal.  0: bands of whole rows, band b -> rank b % nranks (the layout
     * described at vr_render_bands).  > 0: the rows [row_begin,row_end) are cut into bands of
     * band_rows rows (0 = one band) and every band into column blocks of tile_cols pixels; block
     * j of band b belongs to rank (j + stride * b) % nranks, stride = deal_stride (0 =
     * vr_deal_stride_default(nranks)).  out_dev then holds, for every band in order, this rank's
     * blocks of that band in increasing j, each band_rows x tile_cols, as rows of
     * ceil(ceil(width/tile_cols)/nranks) * tile_cols words (vr_tile_buffer_words); pixels past
     * the frame are written as 0.  Every rank gets a share of every band, so expensive rows
     * (long walks are spatially clustered) are spread over all ranks. */
    uint32_t tile_cols;
    uint32_t deal_stride;
    uint32_t reserved2;   /* 0 */
} vr_render_opts;
/* The smallest struct_size accepted: the layout up to and including `reserved`. */
#define VR_RENDER_OPTS_MIN_SIZE 48u

typedef enum {
    VR_OCCUPANCY_AUTO = 0,
    VR_OCCUPANCY_LONE = 1,        /* the lone-frame variant (7 waves/SIMD original, 6 longest axis) */
    VR_OCCUPANCY_IN_FLIGHT = 2    /* the frames-in-flight variant where one exists (a build knob:
                                     since round 6 every walk runs its lone kernel in flight too,
                                     VR_ORIG_WAVES_HI / VR_LONG_WAVES_HI in vr_march.hip) */
} vr_occupancy;

/* Defaults: struct_size = sizeof(vr_render_opts), kernel AUTO, rows [0, UINT32_MAX) --
 * clipped to the frame by the render call -- one band, rank 0 of 1, schedule AUTO,
 * occupancy AUTO, no tile deal. */
int vr_render_opts_init(vr_render_opts* opts);

/* Work order of the tile pass.  A frame's time alone is set by its slowest tiles:
 * dispatched heaviest first (costs recorded by an earlier launch of the same grid
 * size on the device) they no longer start late -- C2 alone 0.151 -> 0.125 ms.
 * With frames in flight on several streams the next frame fills the tail anyway and
 * grid order is faster (C2 0.1124 vs 0.1151 ms per frame).  AUTO picks heaviest
 * first when the device's previous launch was on the same stream (serialised: each
 * launch's time adds up) or has finished, grid order when it is still running on
 * another stream. */
typedef enum {
    VR_SCHEDULE_AUTO = 0,
    VR_SCHEDULE_GRID = 1,
    VR_SCHEDULE_HEAVIEST_FIRST = 2
} vr_schedule;
/* Learned orders (round 5).  Besides the work order, every launch (any schedule) deals the
 * pixels of each 16x32 block to the block's eight waves heaviest first (the lane order: a
 * wave's lanes then walk about equally far) -- C2 per frame in flight 0.113 -> 0.101 ms.
 * Both are learned from the walk lengths of earlier launches of the SAME view (scene,
 * algorithm, camera, lights, transform, frame size, rows and band / tile deal) on the device
 * and used only for that view: a view's first launches, and a view that changes on every
 * launch, render with neither.  Neither ever changes a pixel.  A slot that has seen a view
 * defer no walk to the crawl pass skips that view's crawl pass (records carry their launch,
 * so a wrong skip could never shade another frame's pixels).  vr_forget_orders drops what a
 * device has learned, so the next launch renders as a first render (measurement). */
int vr_forget_orders(int device);
/* Test hook: the device's next launch skips its crawl pass as if its slot had seen the view
 * defer nothing.  For the crawl-skip safety net's test only (a launch that then defers a
 * pixel renders it as 0; the tile pass reports the deferral and the slot stops skipping, so
 * later launches are exact again).  Never needed by a renderer. */
int vr_debug_skip_next_crawl(int device);
/* Test hooks for the lane order.  After vr_debug_capture_lane_order the device's next launch
 * that makes a lane order (a repeated view) waits for its stream and keeps a host copy of the
 * order and of the per-pixel walk lengths it was made from.  vr_debug_lane_order returns them:
 * info = {row length LW, rows, tile-group columns, tile-group rows, block width, block height
 * (pixels), bytes per entry, seat rule (0 cost order, 1 Morton order)}; pcost (or NULL) takes
 * info[0] * info[1] words, row-major, (primary walk length << 16 | shadow walk length); perm
 * (or NULL) takes the order: per block (row-major over ceil(LW / width) x ceil(rows / height)
 * blocks) width * height entries, entry 64 q + i = row * width + column of the block pixel that
 * lane i of wave slot q renders (blocks cut by the frame's edge: unspecified).  Call it with
 * both NULL first for the sizes.  Never needed by a renderer. */
int vr_debug_capture_lane_order(int device);
int vr_debug_lane_order(int device, uint32_t info[8], uint32_t* pcost, uint64_t pcost_words, uint8_t* perm,
                        uint64_t perm_bytes);
/* Test hook: the work order of the captured launch (vr_debug_capture_lane_order).  When that
 * launch made its work order from the costs perm_kernel wrote under the new lane order, the
 * capture -- taken after the work order's kernel -- also keeps both: cost (or NULL) takes
 * 2 * info[2] * info[3] words, (tile-group row * info[2] + column) * 2 + wave, each
 * max(primary) + max(shadow) walk length over the wave's 64 pixels (a cut block's: over the 8x8
 * tile); order (or NULL) takes info[2] * info[3] words, (row << 16 | column) of the tile group
 * the tile pass's i-th workgroup renders, heaviest first.  info is vr_debug_lane_order's; call
 * with both NULL to ask whether a work order was captured.  VR_E_INVALID when none was (nothing
 * captured, or the launch made no work order from those costs), for a word count that is not
 * the captured one, or a device outside 0..63.  Host state only.  Never needed by a renderer. */
int vr_debug_work_order(int device, uint32_t* cost, uint64_t cost_words, uint32_t* order, uint64_t order_words);
/* Test hooks that run the two order kernels on the caller's input, in scratch device buffers
 * of their own, on the null stream: no slot of the device's ring, nothing learned and no
 * counter of vr_debug_order_uses is touched.  Each output buffer is followed by 256 guard bytes
 * of the hook's own; VR_E_HIP if the kernel changed one (it wrote past its output).  Never
 * needed by a renderer.
 * vr_debug_lane_order_from: the lane order and the waves' costs of a frame of LW x rows pixels
 * whose walk lengths are pcost_host (LW * rows words, row-major, primary << 16 | shadow).  info
 * is filled as by vr_debug_lane_order; perm takes the order (perm_bytes: blocks * width * height
 * * info[6]), cost 2 * info[2] * info[3] words, both laid out as vr_debug_lane_order and
 * vr_debug_work_order return them.  Both are filled with 0xFF bytes before the kernel runs, so
 * what it leaves unwritten shows (the perm entries of blocks cut by the frame's edge).  With
 * pcost_host, perm and cost all NULL only info is filled (the sizes) and nothing runs.
 * VR_E_INVALID for a NULL info, one of the three NULL, LW or rows outside 1..65536, a wrong
 * perm_bytes or cost_words, or a device outside 0..63 -- all checked before any device work.
 * vr_debug_work_order_from: the work order of a grid of `groups` tile groups in rows of
 * `columns`, from cost_host (2 * groups words, the two waves' costs per group); order takes
 * `groups` words, filled with 0xFF bytes before the kernel runs.  VR_E_INVALID for a NULL
 * pointer, columns outside 1..4096, groups that is 0 or no multiple of columns, more than 8192
 * rows, or a device outside 0..63 -- checked before any device work. */
int vr_debug_lane_order_from(int device, const uint32_t* pcost_host, uint32_t LW, uint32_t rows, uint32_t info[8],
                             uint8_t* perm, uint64_t perm_bytes, uint32_t* cost, uint64_t cost_words);
int vr_debug_work_order_from(int device, const uint32_t* cost_host, uint32_t columns, uint32_t groups, uint32_t* order);
/* Test hook: whether the device's launches rendered under learned orders.  Host counters kept
 * by the render launch, monotonic for the life of the process (vr_forget_orders does not reset
 * them); vr_pick moves none.  out[0] render launches that reached the tile pass, [1] lane
 * orders made, [2] launches whose tile pass had a lane order bound, [3] work orders made,
 * [4] launches whose tile pass had a work order bound, [5] launches whose crawl pass was
 * skipped, [6] the slots of the device's ring (a slot uses an order only when it comes round
 * again, so a view is under its orders from launch slots + 1 on), [7] lane block width << 16 |
 * height, in pixels.  Reads host state only and never initialises the device: for a device
 * that has not rendered, [0..5] are 0.  VR_E_INVALID for a NULL out or a device outside 0..63.
 * Never needed by a renderer. */
int vr_debug_order_uses(int device, uint64_t out[8]);
/* Test hook: while `on` is nonzero every render launch of the device plans as if another
 * stream's launch were running on it ("frames in flight": vr_schedule AUTO keeps grid order,
 * vr_occupancy AUTO takes the in-flight variant, the crawl pass takes its in-flight records per
 * wave), whatever the device is really doing.  Sticky until turned off with on = 0; nothing else
 * about a launch changes, and no pixel does.  Host state only: never initialises the device.
 * VR_E_INVALID for a device outside 0..63.  Never needed by a renderer. */
int vr_debug_force_in_flight(int device, int on);
/* Test hook: what the device's most recent render launch that reached the tile pass decided.
 * out[0] whether it planned as alone (no other stream's launch running), [1] whether its tile
 * pass dispatched heaviest first (a work order used or learned), [2] whether it took the
 * in-flight occupancy variant, [3] the crawl pass's records per wave, [4] the crawl pass's grid
 * in workgroups, [5] whether its crawl pass ran (0: skipped), [6] the record count that the
 * device's last completed crawl pass reported -- a hint the next launch sizes its grid by;
 * read it after waiting for the launch -- [7] 0.  Reads host state only and never initialises
 * the device: all 0 for a device that has not rendered.  VR_E_INVALID for a NULL out or a
 * device outside 0..63.  Never needed by a renderer. */
int vr_debug_last_launch(int device, uint64_t out[8]);
/* Every vr_render* call returns VR_E_INVALID on a stream that is capturing a HIP graph
 * (its per-device slot ring and work-order bookkeeping are host state that a graph replay
 * would not repeat). */
int vr_render_ex(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                 const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                 const vr_render_opts* opts, uint32_t* out_dev, void* stream);

/* Same render as vr_render, plus the SURVEY.md 8(d) algorithmic byte count of
 * the launch accumulated into *bytes_dev (device uint64, caller-zeroed).
 * Instrumented variant for measurement; pixels are identical. */
int vr_render_count(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                    uint32_t row_begin, uint32_t row_end, uint32_t* out_dev,
                    uint64_t* bytes_dev, void* stream);

/* writeColorToFramebuffer (Renderer.cuh:1024-1031): packed words -> RGB8
 * (3 bytes per pixel, R = word >> 16 truncated to 8 bits), on the device. */
int vr_pack_rgb8(const uint32_t* words_dev, uint8_t* rgb_dev, uint64_t n_pixels, void* stream);

/* Supersampled frames: the render at `samples` x `samples` samples per pixel, box-filtered.
 *
 * samples = S in {1, 2, 4, 8} per axis, N = S * S.  The FINE FRAME of a W x H frame is the
 * (S * W) x (S * H) render of the same scene, algorithm, camera, lighting, translation and scale:
 * vr_render's frame of that size, word for word.  Pixel (x, y) of the RESOLVED FRAME has, for each
 * channel c (R = bits 16-23, G = bits 8-15, B = bits 0-7 of a word; bits 24-31 of a fine word are
 * dropped, as vr_shade_lights drops them),
 *
 *   out_c(x, y) = (sum over 0 <= i, j < S of c(fine[(S * y + j) * (S * W) + S * x + i]) + N / 2) >> log2(N)
 *
 * packed R << 16 | G << 8 | B: the mean of the pixel's N samples, rounded half up.  The arithmetic
 * is of integers only, so no order of summation can matter.  With S = 1 the resolved word is the
 * fine word with bits 24-31 cleared: vr_render's word whenever that word is below 2^24.
 * (The reference's v = ((H - y) + 0.5) / H puts row 0 one row above the image plane; in the fine
 * frame that is one FINE row, so the resolved frame sits (S - 1) / (2 S) of a pixel lower than
 * the one-sample frame.  Deliberate: the resolved frame is exactly "the bigger render,
 * box-filtered")
 *
 * vr_aa_fine_words: the words of the fine frame of `rows` rows of a frame `width` wide,
 * (S * width) * (S * rows); 0 for arguments vr_render_aa rejects (samples not 1, 2, 4 or 8, width
 * outside 1..65536, rows above 65536, S * width or S * rows above 65536). */
uint64_t vr_aa_fine_words(uint32_t width, uint32_t rows, uint32_t samples);

/* The filter alone: resolves the fine frame at fine_dev -- (S * width) x (S * rows) words, row-major,
 * already on the current device: a vr_render, a frame of vr_shade_lights words or an assembled
 * multi-GPU frame -- to width x rows pixels.  out_dev (or NULL) receives the packed words,
 * width * rows of them; out_rgb8_dev (or NULL) the same pixels as RGB8, 3 bytes per pixel, R
 * first, as vr_pack_rgb8 writes them.  With both, both come from one read of the fine frame.  One
 * kernel on `stream`, asynchronous; allocates nothing.  Every fine word is read once, with 16-byte
 * loads when fine_dev is 16-byte aligned (and, at S = 2, width is even); a fine_dev that is only
 * 4-byte aligned is accepted and read word by word.
 *
 * VR_E_INVALID, before any device work: fine_dev NULL; both outputs NULL; samples not 1, 2, 4 or 8;
 * width or rows outside 1..65536; S * width or S * rows above 65536; fine_dev or out_dev not
 * 4-byte aligned; a stream that is capturing a HIP graph. */
int vr_resolve(const uint32_t* fine_dev, uint32_t width, uint32_t rows, uint32_t samples,
               uint32_t* out_dev /* or NULL */, uint8_t* out_rgb8_dev /* or NULL */, void* stream);

/* Rows [row_begin, row_end) of the resolved width x height frame.  Renders fine rows
 * [S * row_begin, S * row_end) of the fine frame into fine_dev through vr_render -- an ordinary
 * render launch of the (S * width) x (S * height) view, so a repeated view learns and uses its
 * orders as under vr_render -- and resolves them on the same stream into out_dev
 * ((row_end - row_begin) * width words) and/or out_rgb8_dev (3 bytes per pixel), as vr_resolve.
 * Asynchronous, as vr_render.  Afterwards fine_dev holds those fine rows, packed from its start.
 *
 * The caller owns fine_dev (fine_words words, at least vr_aa_fine_words(width, row_end -
 * row_begin, samples)) and must not reuse it while a launch that uses it is in flight on another
 * stream: two frames in flight need two buffers.
 *
 * VR_E_INVALID, every check before any device work: s, cam, lit, translation or fine_dev NULL;
 * both outputs NULL; samples not 1, 2, 4 or 8; width or height outside 1..65536; S * width or
 * S * height above 65536; row_begin <= row_end <= height violated (an empty range is VR_OK and
 * does nothing); fine_words too small; an unknown algorithm; fine_dev or out_dev not 4-byte
 * aligned; a stream that is capturing a HIP graph. */
int vr_render_aa(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                 const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                 uint32_t samples, uint32_t row_begin, uint32_t row_end,
                 uint32_t* fine_dev, uint64_t fine_words,
                 uint32_t* out_dev /* or NULL */, uint8_t* out_rgb8_dev /* or NULL */, void* stream);

/* ImageWriter::writeImage(filename, image, width, height, colorChannels)
 * (ImageWriter.cpp:8-16, stbi_write_png with tightly packed rows): 8-bit PNG
 * of 1-4 channels from HOST memory. Row chunks are deflated on parallel
 * threads (level 0-9, out-of-range = 6). Pixels are what stb would store; the
 * compressed bytes differ. */
int vr_png_write(const char* path, const uint8_t* image, uint32_t width, uint32_t height, int channels, int level);

/* Same encoder into memory. out == NULL: sets *out_len to an upper bound of
 * the encoded size (no encoding); otherwise encodes and sets the actual size.
 * threads <= 0: hardware threads, at most 16. */
int vr_png_encode(const uint8_t* image, uint32_t width, uint32_t height, int channels, int level, int threads,
                  uint8_t* out, size_t capacity, size_t* out_len);

/* Synthetic scene: with xyz == NULL only counts (*n_out); otherwise writes up
 * to `capacity` voxels (3 int32 + 1 colour each) and sets *n_out. */
int vr_synth_generate(const vr_synth_params* p, int32_t* xyz, uint32_t* rgb, size_t capacity,
                      size_t* n_out);

/* .vox CSV reader/writer ("x,y,z,color" per line, VoxelFile.cuh:11-35).
 * Reader: two-phase like vr_synth_generate. */
int vr_vox_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out);
int vr_vox_write(const char* path, const int32_t* xyz, const uint32_t* rgb, size_t n);

/* .vxb binary scene sidecar: 32-byte header {"VRVXB001",
 * u64 count, u64 reserved[2]}, then int32 xyz[3*count], uint32 rgb[count]
 * (little endian, insertion order).  Same two-call protocol as vr_vox_read. */
int vr_vxb_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out);
int vr_vxb_write(const char* path, const int32_t* xyz, const uint32_t* rgb, size_t n);
/* Either format, detected by the .vxb magic. */
int vr_scene_file_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out);

const char* vr_last_error(void);
const char* vr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VR_H */
