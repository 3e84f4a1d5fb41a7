// vr_scene.cpp -- scene build (region bucketing, VCS and cuckoo images) on the host or
// through the device builder, device upload, and the scene entry points of include/vr.h
// (create, digest, edit, voxels, and access by coordinate: lookup and paint).
//
// Replaces, on the host: VoxelSceneCPU (geometry/VoxelSceneCPU.cuh:13-131) and
// the VoxelClusterStore / CuckooHashTable constructors
// (storage/VoxelClusterStore.cuh:37-85, storage/CuckooHashTable.cuh:20-178).
// The nested unordered_maps of the reference become one sort of (region, key)
// records; pointers become 32-bit offsets.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "vr_build.h"
#include "vr_host.h"
#include "vr_staging.h"

namespace {

using vr::DevBuf;
using vr::DeviceGuard;
using vr::fail;
using vr::hip_fail;
using vr::Staging;

// static_cast<int32_t>(float) with the CUDA semantics used on the device.
inline int32_t f2i(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

// ------------------------------------------------------------- cuckoo hashing
const uint32_t kPrimes[14] = {668265261u, 12289u, 24593u, 49157u, 98317u, 196613u, 393241u,
                              786433u, 1572869u, 3145739u, 6291469u, 12582917u, 25165843u, 50331653u};

inline uint32_t hash1(uint32_t k, uint32_t offset) {   // CuckooHashTable.cuh:181-190
    k = (k + 0x7ed55d16u) + (k << 12);
    k = (k ^ 0xc761c23cu) ^ (uint32_t)((int32_t)k >> 19);
    k = (k + 0x165667b1u) + (k << 5);
    k = (k + 0xd3a2646cu) ^ (k << 9);
    k = (k + 0xfd7046c5u) + (k << 3);
    k = (k ^ 0xb55a4f09u) ^ (uint32_t)((int32_t)k >> 16);
    return k + offset;
}
inline uint32_t hash2(uint32_t k, uint32_t prime) {    // CuckooHashTable.cuh:193-202
    k = (k ^ 61u) ^ (uint32_t)((int32_t)k >> 16);
    k = k + (k << 3);
    k = k ^ (uint32_t)((int32_t)k >> 4);
    k = k * prime;
    k = k ^ (uint32_t)((int32_t)k >> 15);
    return k;
}

// createCuckooHashTable (CuckooHashTable.cuh:97-178) into interleaved
// {key,value} slots: table 1 at slots[0..M), table 2 at slots[M..2M).
// The rehash draws a new prime/offset from a seeded generator instead of
// rand() (Random.cuh:14-18): lookups do not depend on the placement.
bool cuckoo_build(const uint32_t* keys, const uint32_t* vals, uint32_t n, uint32_t* M_out,
                  uint32_t* prime_out, uint32_t* offset_out, std::vector<uint32_t>& slots,
                  size_t base_words) {
    const uint32_t M = (uint32_t)((double)n * 1.25);   // numElements * 1.25 (:23)
    uint32_t prime = kPrimes[0], offset = 0;
    uint64_t rng = 0x9E3779B97F4A7C15ull ^ (uint64_t)n ^ ((uint64_t)keys[0] << 20);
    uint32_t* t = nullptr;
    for (int attempt = 0; attempt < 4096; ++attempt) {
        slots.resize(base_words + 4 * (size_t)M);
        t = slots.data() + base_words;
        for (uint32_t i = 0; i < 2 * M; ++i) { t[2 * i] = vr::kEmpty; t[2 * i + 1] = 0; }
        bool rehash = false;
        for (uint32_t i = 0; i < n && !rehash; ++i) {
            uint32_t code = keys[i], value = vals[i], bucket = 0, it = 0;
            for (;;) {
                if (it >= 300000u) { rehash = true; break; }
                uint32_t* slot = bucket == 0 ? t + 2 * (size_t)(hash1(code, offset) % M)
                                             : t + 2 * ((size_t)M + hash2(code, prime) % M);
                if (slot[0] == vr::kEmpty) { slot[0] = code; slot[1] = value; break; }
                std::swap(slot[0], code);
                std::swap(slot[1], value);
                bucket ^= 1u;
                ++it;
            }
        }
        if (!rehash) {
            *M_out = M; *prime_out = prime; *offset_out = offset;
            return true;
        }
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        prime = kPrimes[(rng >> 33) % 14u];
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        offset = (uint32_t)((rng >> 33) % 25u);
    }
    return false;
}

void free_scene(vr_scene* s) {
    if (!s) return;
    DevBuf* bufs[] = {&s->region_slot, &s->vcs_mask, &s->vcs_vals, &s->ht_meta, &s->ht_slots, &s->vcs_cbits,
                      &s->ht_filter};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (s->paint_stat) (void)hipFree(s->paint_stat);
    delete s;
}

// A scene under construction: an early return frees its device buffers.  (Declared after
// the builder's DeviceGuard, so that it is freed with the scene's device current.)
struct SceneDeleter {
    void operator()(vr_scene* s) const { free_scene(s); }
};
using ScenePtr = std::unique_ptr<vr_scene, SceneDeleter>;

std::atomic<uint64_t> g_scene_serial{0};
ScenePtr new_scene(int device, vr_store store) {
    ScenePtr s(new vr_scene(++g_scene_serial));
    s->device = device;
    s->store = store;
    return s;
}

int upload(DevBuf& b, const void* src, size_t bytes) {
    b.bytes = bytes;
    if (bytes == 0) return VR_OK;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(VR_E_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy H2D");
    return VR_OK;
}

// One record per inserted voxel: (region index, local key) sort key.
struct Rec {
    uint64_t k;       // region << 32 | key
    uint32_t val;
    uint32_t idx;     // insertion order (later wins)
};

// Host build from host voxel arrays (build_scene_raw has checked the arguments).
int build_scene_host(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, vr_scene** out) {
    // VoxelSceneCPU::insertVoxel (VoxelSceneCPU.cuh:16-46)
    std::vector<int32_t> rc(3 * n);
    int32_t minc = 0, maxc = 0;
    for (size_t i = 0; i < n; ++i) {
        if (rgb[i] > 0xFFFFFFu)
            return fail(VR_E_INVALID, "voxel colour " + std::to_string(rgb[i]) + " at index " + std::to_string(i) +
                                          " exceeds 24-bit RGB");
        for (int a = 0; a < 3; ++a) {
            int32_t c = f2i(std::floor((float)xyz[3 * i + a] / 64.0f));   // :19-21
            rc[3 * i + a] = c;
            minc = std::min(minc, c);
            maxc = std::max(maxc, c);
        }
    }
    const int64_t D64 = (int64_t)maxc - (int64_t)minc + 1;
    if (D64 > 1024) return fail(VR_E_INVALID, "scene spans more than 1024 regions per axis");
    const uint32_t D = (uint32_t)D64;
    const uint64_t D3 = (uint64_t)D * D * D;

    std::vector<Rec> recs(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t l[3];
        for (int a = 0; a < 3; ++a) {
            int32_t c = xyz[3 * i + a];
            l[a] = (uint32_t)(((c % vr::kBlock) + vr::kBlock) % vr::kBlock);    // :24-26
        }
        uint64_t ax = (uint64_t)(rc[3 * i] - minc), ay = (uint64_t)(rc[3 * i + 1] - minc),
                 az = (uint64_t)(rc[3 * i + 2] - minc);
        uint64_t region = ax + ay * D + az * (uint64_t)D * D;
        uint32_t key = (l[0] << 20) | (l[1] << 10) | l[2];                     // generate3DPoint
        recs[i] = Rec{(region << 32) | key, rgb[i], (uint32_t)i};
    }
    std::vector<int32_t>().swap(rc);
    std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.k < b.k || (a.k == b.k && a.idx < b.idx); });
    size_t m = 0;   // duplicates: the later insertion wins (map assignment, :46)
    for (size_t i = 0; i < n; ++i) {
        if (m && recs[m - 1].k == recs[i].k) recs[m - 1] = recs[i];
        else recs[m++] = recs[i];
    }
    recs.resize(m);

    std::vector<uint32_t> region_slot(D3, vr::kNone);
    std::vector<size_t> region_begin;
    for (size_t i = 0; i < m; ++i)
        if (i == 0 || (recs[i].k >> 32) != (recs[i - 1].k >> 32)) {
            region_slot[recs[i].k >> 32] = (uint32_t)region_begin.size();
            region_begin.push_back(i);
        }
    const uint32_t nr = (uint32_t)region_begin.size();
    region_begin.push_back(m);
    if (store == VR_STORE_VCS && nr > vr::kVcsMaxRegions)     // (cuckoo scenes have no region bound)
        return fail(VR_E_INVALID, "VCS scene with " + std::to_string(nr) + " occupied 64^3 regions (at most " +
                                      std::to_string(vr::kVcsMaxRegions) + ")");

    DeviceGuard dg(device);
    ScenePtr s = new_scene(device, store);
    s->D = D; s->min_coord = minc; s->n_regions = nr; s->n_voxels = m;
    int rc_up = upload(s->region_slot, region_slot.data(), region_slot.size() * 4);
    if (rc_up) return rc_up;

    if (store == VR_STORE_VCS) {
        // VoxelClusterStore ctor (VoxelClusterStore.cuh:37-85): per region 512
        // cluster slots; a cluster's sorted keys become a 512-bit occupancy
        // mask over in-cluster indices (same order) with a running value index
        // per 32-bit word, its values follow in key order (vr_internal.h "VCS").
        if ((uint64_t)nr * 512u * 16u * sizeof(uint2) > (1ull << 40)) return fail(VR_E_BUILD, "VCS mask table too large");
        std::vector<uint2> mask((size_t)nr * 512 * 16, uint2{0u, vr::kNone});
        std::vector<uint32_t> vals;
        vals.reserve(m);
        for (uint32_t r = 0; r < nr; ++r) {
            size_t b = region_begin[r], e = region_begin[r + 1];
            uint32_t bits[512][16];
            uint32_t cnt[512] = {0};
            memset(bits, 0, sizeof bits);
            for (size_t i = b; i < e; ++i) {
                uint32_t key = (uint32_t)recs[i].k;
                uint32_t x = key >> 20, y = (key >> 10) & 0x3FFu, z = key & 0x3FFu;
                uint32_t c = ((x / 8u) << 6) | ((y / 8u) << 3) | (z / 8u);
                uint32_t q = ((x & 7u) << 6) | ((y & 7u) << 3) | (z & 7u);
                bits[c][q >> 5] |= 1u << (q & 31u);
                cnt[c]++;
            }
            // values: cluster by cluster, each in key order (keys arrive ascending
            // within a region, and one cluster's keys ascend with q)
            uint32_t start[512];
            uint32_t acc = (uint32_t)vals.size();
            for (uint32_t c = 0; c < 512; ++c) { start[c] = acc; acc += cnt[c]; }
            vals.resize(acc);
            uint32_t fill[512] = {0};
            for (size_t i = b; i < e; ++i) {
                uint32_t key = (uint32_t)recs[i].k;
                uint32_t x = key >> 20, y = (key >> 10) & 0x3FFu, z = key & 0x3FFu;
                uint32_t c = ((x / 8u) << 6) | ((y / 8u) << 3) | (z / 8u);
                vals[start[c] + fill[c]++] = recs[i].val;
            }
            for (uint32_t c = 0; c < 512; ++c) {
                if (!cnt[c]) continue;
                // slot order z3..5 | y3..5 | x3..5 (vr_device.h word_index)
                const uint32_t slot = (c >> 6) | (((c >> 3) & 7u) << 3) | ((c & 7u) << 6);
                uint2* w = &mask[((size_t)r * 512 + slot) * 16];
                uint32_t run = start[c];
                for (uint32_t j = 0; j < 16; ++j) {
                    w[j] = uint2{bits[c][j], run};
                    run += (uint32_t)__builtin_popcount(bits[c][j]);
                }
            }
        }
        if (mask.empty()) mask.assign(16, uint2{0u, vr::kNone});
        if (vals.empty()) vals.assign(1, 0u);
        if ((rc_up = upload(s->vcs_mask, mask.data(), mask.size() * sizeof(uint2))) ||
            (rc_up = upload(s->vcs_vals, vals.data(), vals.size() * 4)))
            return rc_up;
    } else {
        // CuckooHashTable ctor (CuckooHashTable.cuh:20-49) per region.
        std::vector<uint32_t> meta((size_t)nr * 4);
        std::vector<uint32_t> slots;
        std::vector<uint32_t> keys, vals;
        for (uint32_t r = 0; r < nr; ++r) {
            size_t b = region_begin[r], e = region_begin[r + 1];
            keys.resize(e - b); vals.resize(e - b);
            for (size_t i = b; i < e; ++i) { keys[i - b] = (uint32_t)recs[i].k; vals[i - b] = recs[i].val; }
            size_t base_words = slots.size();
            uint32_t M = 0, prime = 0, offset = 0;
            if (!cuckoo_build(keys.data(), vals.data(), (uint32_t)(e - b), &M, &prime, &offset, slots, base_words))
                return fail(VR_E_BUILD, "cuckoo hash table build failed for region " + std::to_string(r));
            if (base_words / 2 >= 0xFFFFFFFFull) return fail(VR_E_BUILD, "hash slots exceed 32-bit offsets");
            meta[4 * r + 0] = (uint32_t)(base_words / 2);
            meta[4 * r + 1] = M;
            meta[4 * r + 2] = prime;
            meta[4 * r + 3] = offset;
        }
        if (slots.empty()) slots.assign(2, vr::kEmpty);
        if (meta.empty()) meta.assign(4, 0);
        if ((rc_up = upload(s->ht_meta, meta.data(), meta.size() * 4)) ||
            (rc_up = upload(s->ht_slots, slots.data(), slots.size() * 4)))
            return rc_up;
    }
    *out = s.release();
    return VR_OK;
}

// The n voxels (xyz, rgb) on the device: the caller's own arrays, or host arrays staged in two
// buffers (both made, then both filled).  Null after an error (sg.err).
const int32_t* voxels_on_device(Staging& sg, const int32_t* xyz, const uint32_t* rgb, size_t n, const uint32_t*& drgb) {
    void* tx = sg.make(3 * n * sizeof(int32_t));
    void* tc = sg.make(n * sizeof(uint32_t));
    sg.put(tx, xyz, 3 * n * sizeof(int32_t));
    sg.put(tc, rgb, n * sizeof(uint32_t));
    drgb = (const uint32_t*)tc;
    return sg.err == hipSuccess ? (const int32_t*)tx : nullptr;
}

// A scene that owns what a device builder made (vr_build.h): whatever `g` holds, after a failed
// build too, is freed with the scene.
ScenePtr adopt_scene(int device, vr_store store, const vr::GpuScene& g) {
    ScenePtr s = new_scene(device, store);
    s->D = g.D; s->min_coord = g.min_coord;
    s->n_regions = g.n_regions; s->n_voxels = g.n_voxels;
    s->region_slot = DevBuf{g.region_slot, g.region_slot_bytes};
    s->vcs_mask = DevBuf{g.vcs_mask, g.vcs_mask_bytes};
    s->vcs_vals = DevBuf{g.vcs_vals, g.vcs_vals_bytes};
    s->ht_meta = DevBuf{g.ht_meta, g.ht_meta_bytes};
    s->ht_slots = DevBuf{g.ht_slots, g.ht_slots_bytes};
    return s;
}

// What the device builders return (vr_build.h), as the C ABI's code.
int builder_code(int rc) { return rc == -1 ? VR_E_INVALID : rc == -5 ? VR_E_BUILD : VR_E_HIP; }

// Device build (vr_build.hip) from host or device voxel arrays.
int build_scene_device(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, bool on_device,
                       hipStream_t stream, vr_scene** out) {
    DeviceGuard dg(device);
    Staging sg(stream);
    const int32_t* dxyz = xyz;
    const uint32_t* drgb = rgb;
    if (!on_device && n) dxyz = voxels_on_device(sg, xyz, rgb, n, drgb);
    if (sg.err != hipSuccess) return hip_fail(sg.err, "voxel upload");
    vr::GpuScene g;
    std::string err;
    const int rc = vr::build_scene_gpu((int)store, dxyz, drgb, n, stream, g, err);
    if (rc == 0) sg.drained();   // (a build that succeeds returns after the stream has drained)
    ScenePtr s = adopt_scene(device, store, g);
    if (rc) return fail(builder_code(rc), "scene build: " + err);
    *out = s.release();
    return VR_OK;
}

// The derived bits of a scene (vr_internal.h KScene), made on the device from the tables
// either builder wrote: a VCS scene's per-region cluster-existence bits (vcs_cbits), a
// cuckoo scene's per-region key-presence bits (ht_filter).
int add_derived_bits(vr_scene* s, hipStream_t stream) {
    const bool vcs = s->store == VR_STORE_VCS;
    DevBuf& b = vcs ? s->vcs_cbits : s->ht_filter;
    const std::string what = vcs ? "cluster bits" : "hash filter";
    DeviceGuard dg(s->device);
    const uint32_t nr = std::max(1u, s->n_regions);
    const size_t bytes = (size_t)nr * (vcs ? 16u : vr::kHashFilterWords) * sizeof(uint32_t);
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return hip_fail(e, ("hipMalloc(" + what + ")").c_str());
    }
    b.bytes = bytes;
    e = hipMemsetAsync(b.p, 0, bytes, stream);
    if (e == hipSuccess && s->n_regions)
        e = vcs ? vr::launch_cluster_bits((const uint2*)s->vcs_mask.p, s->n_regions, (uint32_t*)b.p, stream)
                : vr::launch_hash_filter((const uint4*)s->ht_meta.p, (const uint2*)s->ht_slots.p, s->n_regions,
                                         (uint32_t*)b.p, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, what.c_str());
    return VR_OK;
}

// The scene as vr_edit.hip's kernels read it.
vr::GpuImage gpu_image(const vr_scene* s) {
    return vr::GpuImage{(int)s->store, s->D, s->min_coord, s->n_regions, s->n_voxels, s->region_slot.p, s->vcs_mask.p,
                        s->vcs_vals.p, s->ht_meta.p, s->ht_slots.p, s->ht_filter.p};
}

int build_scene_raw(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, bool on_device,
                    vr_build mode, void* stream, vr_scene** out) {
    if (!out) return fail(VR_E_INVALID, "out is NULL");
    *out = nullptr;
    if (store != VR_STORE_VCS && store != VR_STORE_HASHTABLE) return fail(VR_E_INVALID, "unknown store");
    if (n && (!xyz || !rgb)) return fail(VR_E_INVALID, "xyz/rgb NULL");
    if (n >= 0xFFFFFFFFull) return fail(VR_E_INVALID, "too many voxels");
    if (mode != VR_BUILD_AUTO && mode != VR_BUILD_DEVICE && mode != VR_BUILD_HOST) return fail(VR_E_INVALID, "unknown build mode");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VR_E_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(VR_E_INVALID, "device index out of range");
    if (mode == VR_BUILD_HOST) {
        if (!on_device) return build_scene_host(device, store, xyz, rgb, n, out);
        DeviceGuard dg(device);
        std::vector<int32_t> hx(3 * n + 3);
        std::vector<uint32_t> hc(n + 1);
        if (n) {
            hipError_t e = hipMemcpy(hx.data(), xyz, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(hc.data(), rgb, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(e, "voxel download");
        }
        return build_scene_host(device, store, hx.data(), hc.data(), n, out);
    }
    return build_scene_device(device, store, xyz, rgb, n, on_device, (hipStream_t)stream, out);
}

}  // namespace

namespace vr {

int build_scene(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, bool on_device,
                vr_build mode, void* stream, vr_scene** out) {
    int rc = build_scene_raw(device, store, xyz, rgb, n, on_device, mode, stream, out);
    if (rc) return rc;
    rc = add_derived_bits(*out, (hipStream_t)stream);
    if (rc) {
        vr_scene_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

KScene kscene(const vr_scene* s) {
    KScene k{};
    k.region_slot = (const uint32_t*)s->region_slot.p;
    k.vcs_mask = (const uint2*)s->vcs_mask.p;
    k.vcs_vals = (const uint32_t*)s->vcs_vals.p;
    k.vcs_cbits = (const uint32_t*)s->vcs_cbits.p;
    k.ht_meta = (const uint4*)s->ht_meta.p;
    k.ht_slots = (const uint2*)s->ht_slots.p;
    k.ht_filter = (const uint32_t*)s->ht_filter.p;
    k.D = s->D;
    k.min_coord = s->min_coord;
    k.n_regions = s->n_regions;
    return k;
}

}  // namespace vr

using vr::build_scene;

extern "C" {

int vr_scene_create(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, vr_scene** out) {
    return build_scene(device, store, xyz, rgb, n, false, VR_BUILD_AUTO, nullptr, out);
}

int vr_scene_create_ex(int device, vr_store store, const int32_t* xyz, const uint32_t* rgb, size_t n, int inputs_on_device,
                       vr_build build, void* stream, vr_scene** out) {
    return build_scene(device, store, xyz, rgb, n, inputs_on_device != 0, build, stream, out);
}

int vr_scene_digest(const vr_scene* s, uint64_t out[5]) {
    if (!s || !out) return fail(VR_E_INVALID, "NULL argument");
    DeviceGuard dg(s->device);
    const DevBuf* bufs[5] = {&s->region_slot, &s->vcs_mask, &s->vcs_vals, &s->ht_meta, &s->ht_slots};
    for (int i = 0; i < 5; ++i) {
        uint64_t h = vr::kFnvBasis ^ bufs[i]->bytes;     // FNV-1a over the buffer bytes
        if (bufs[i]->p && bufs[i]->bytes) {
            std::vector<unsigned char> host(bufs[i]->bytes);
            hipError_t e = hipMemcpy(host.data(), bufs[i]->p, bufs[i]->bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpy D2H");
            h = vr::fnv1a(h, host.data(), host.size());
        }
        out[i] = h;
    }
    return VR_OK;
}

int vr_scene_load_vox(int device, vr_store store, const char* path, vr_scene** out) {
    if (!path) return fail(VR_E_INVALID, "NULL argument");
    vr::VoxParse vp;
    const int rc = vr::read_voxels(path, vp);
    if (rc) return rc;
    return build_scene(device, store, vp.xyz.data(), vp.rgb.data(), vp.rgb.size(), false, VR_BUILD_AUTO, nullptr, out);
}

int vr_scene_get_info(const vr_scene* s, vr_scene_info* out) {
    if (!s || !out) return fail(VR_E_INVALID, "NULL argument");
    out->diameter = s->D;
    out->min_coord = s->min_coord;
    out->region_count = s->n_regions;
    out->store = (uint32_t)s->store;
    out->voxel_count = s->n_voxels;
    out->device_bytes = s->device_bytes();
    out->device = s->device;
    return VR_OK;
}

int vr_scene_edit(vr_scene* s, const int32_t* xyz, const uint32_t* rgb, size_t n, int inputs_on_device, void* stream) {
    if (!s) return fail(VR_E_INVALID, "vr_scene_edit: scene is NULL");
    if (n && (!xyz || !rgb)) return fail(VR_E_INVALID, "vr_scene_edit: xyz/rgb NULL");
    if (n == 0) return VR_OK;
    if (n >= 0xFFFFFFFFull) return fail(VR_E_INVALID, "vr_scene_edit: too many edits");
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_scene_edit")) return rc;
    // the new image as a scene of its own: freed whole if anything fails, swapped in otherwise
    ScenePtr t;
    {
        Staging sg(st);
        const int32_t* dxyz = xyz;
        const uint32_t* drgb = rgb;
        if (!inputs_on_device) dxyz = voxels_on_device(sg, xyz, rgb, n, drgb);
        if (sg.err != hipSuccess) return hip_fail(sg.err, "edit upload");
        vr::GpuScene g;
        std::string err;
        const int rc = vr::edit_scene_gpu(gpu_image(s), dxyz, drgb, n, st, g, err);
        if (rc == 0) sg.drained();   // (as a build: an edit that succeeds has drained the stream)
        t = adopt_scene(s->device, s->store, g);
        if (rc) return fail(builder_code(rc), "scene edit: " + err);
    }
    if (const int rd = add_derived_bits(t.get(), st)) return rd;
    // the stream has drained (add_derived_bits): renders queued on it before the edit are done
    std::swap(s->n_regions, t->n_regions);
    std::swap(s->n_voxels, t->n_voxels);
    DevBuf vr_scene::*bufs[] = {&vr_scene::region_slot, &vr_scene::vcs_mask, &vr_scene::vcs_vals, &vr_scene::ht_meta,
                                &vr_scene::ht_slots, &vr_scene::vcs_cbits, &vr_scene::ht_filter};
    for (auto b : bufs) std::swap(s->*b, (*t).*b);
    ++s->revision;
    return VR_OK;   // t, now the old image, is freed here
}

// The colour stored at each coordinate (vr.h; kernel: vr_access.hip).  As the queries of
// vr_query_api.cpp it is no render launch: nothing the render path keeps per device is touched.
int vr_scene_lookup(const vr_scene* s, const int32_t* xyz, size_t n, int inputs_on_device, uint32_t* rgb,
                    int outputs_on_device, void* stream) {
    static_assert(VR_VOXEL_ABSENT == VR_VOXEL_REMOVE, "vr_scene_edit(xyz, vr_scene_lookup(xyz)) changes nothing");
    if (!s) return fail(VR_E_INVALID, "vr_scene_lookup: scene is NULL");
    if (n && (!xyz || !rgb)) return fail(VR_E_INVALID, "vr_scene_lookup: xyz/rgb NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_scene_lookup: too many queries");
    if (n == 0) return VR_OK;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_scene_lookup")) return rc;
    Staging sg(st);
    const int32_t* dxyz = inputs_on_device ? xyz : (const int32_t*)sg.upload(xyz, 3 * n * sizeof(int32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_scene_lookup: query upload");
    uint32_t* drgb = outputs_on_device ? rgb : (uint32_t*)sg.make(n * sizeof(uint32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_scene_lookup: colour buffer");
    hipError_t e = vr::launch_lookup((int)s->store, vr::kscene(s), dxyz, (uint32_t)n, drgb, st);
    if (e == hipSuccess && drgb != rgb) {
        sg.fetch(rgb, drgb, n * sizeof(uint32_t));
        e = sg.err;
    }
    const hipError_t es = sg.sync();
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "vr_scene_lookup");
    return VR_OK;
}

// Recolour stored voxels in place (vr.h; kernels: vr_access.hip).  One store per voxel into the
// live image: no buffer is replaced and the revision stays, so the views' learned orders and
// crawl skips stay bound -- no walk reads a colour except to compare it with kEmpty, so a
// recolour moves no deferral and no walk length.
int vr_scene_paint(vr_scene* s, const int32_t* xyz, const uint32_t* rgb, size_t n, int inputs_on_device, void* stream,
                   size_t* n_absent) {
    if (!s) return fail(VR_E_INVALID, "vr_scene_paint: scene is NULL");
    if (n && (!xyz || !rgb)) return fail(VR_E_INVALID, "vr_scene_paint: xyz/rgb NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_scene_paint: too many edits");
    if (n_absent) *n_absent = 0;
    if (n == 0) return VR_OK;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_scene_paint")) return rc;
    if (!s->paint_stat) {
        const hipError_t e = hipMalloc((void**)&s->paint_stat, 2 * sizeof(uint32_t));
        if (e != hipSuccess) {
            s->paint_stat = nullptr;
            return hip_fail(e, "vr_scene_paint: hipMalloc");
        }
    }
    Staging sg(st);
    const int32_t* dxyz = xyz;
    const uint32_t* drgb = rgb;
    if (!inputs_on_device) dxyz = voxels_on_device(sg, xyz, rgb, n, drgb);
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_scene_paint: edit upload");
    const vr::KScene k = vr::kscene(s);
    // every check before any write: the first colour that is no colour, and the absent count
    uint32_t stat[2] = {0u, 0u};
    hipError_t e = vr::launch_paint_check((int)s->store, k, dxyz, drgb, (uint32_t)n, s->paint_stat, st);
    if (e == hipSuccess) e = hipMemcpyAsync(stat, s->paint_stat, sizeof stat, hipMemcpyDeviceToHost, st);
    hipError_t es = sg.sync();
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "vr_scene_paint: check");
    if (stat[0] != 0xFFFFFFFFu) {
        uint32_t c = 0;
        if (!inputs_on_device) c = rgb[stat[0]];
        else if ((e = hipMemcpy(&c, rgb + stat[0], sizeof c, hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(e, "vr_scene_paint: check");
        return fail(VR_E_INVALID, "vr_scene_paint: voxel colour " + std::to_string(c) + " at index " +
                                      std::to_string(stat[0]) + " exceeds 24-bit RGB (a paint never removes)");
    }
    e = vr::launch_paint_apply((int)s->store, k, dxyz, drgb, (uint32_t)n, st);
    es = sg.sync();      // (whatever e is: the tag kernel may be queued on the staged arrays)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "vr_scene_paint (the colours of the batch's voxels are unspecified)");
    if (n_absent) *n_absent = (size_t)(0xFFFFFFFFu - stat[1]);
    return VR_OK;
}

int vr_scene_voxels(const vr_scene* s, int32_t* xyz, uint32_t* rgb, size_t capacity, int outputs_on_device, void* stream,
                    size_t* n_out) {
    if (!s || !n_out) return fail(VR_E_INVALID, "vr_scene_voxels: NULL argument");
    const size_t m = (size_t)s->n_voxels;
    *n_out = m;
    if (!xyz) return VR_OK;
    if (!rgb) return fail(VR_E_INVALID, "vr_scene_voxels: rgb NULL");
    if (capacity < m)
        return fail(VR_E_INVALID, "vr_scene_voxels: capacity " + std::to_string(capacity) + " below the scene's " +
                                      std::to_string(m) + " voxels");
    if (m == 0) return VR_OK;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    // (No vr::refuse_capture here, unlike every other entry point that stages: vr_scene_voxels
    // never refused a capturing stream, and that is left as it was.)
    Staging sg(st);
    int32_t* dxyz = outputs_on_device ? xyz : (int32_t*)sg.make(3 * m * sizeof(int32_t));
    uint32_t* drgb = outputs_on_device ? rgb : (uint32_t*)sg.make(m * sizeof(uint32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "voxel export buffers");
    std::string err;
    const int rc = vr::export_scene_gpu(gpu_image(s), dxyz, drgb, st, err);
    if (rc) return fail(builder_code(rc), "scene export: " + err);
    if (outputs_on_device) return VR_OK;
    sg.fetch(xyz, dxyz, 3 * m * sizeof(int32_t));
    sg.fetch(rgb, drgb, m * sizeof(uint32_t));
    const hipError_t e = sg.err == hipSuccess ? sg.sync() : sg.err;
    if (e != hipSuccess) return hip_fail(e, "voxel download");
    return VR_OK;
}

void vr_scene_destroy(vr_scene* s) {
    if (!s) return;
    DeviceGuard dg(s->device);
    free_scene(s);
}

}  // extern "C"
