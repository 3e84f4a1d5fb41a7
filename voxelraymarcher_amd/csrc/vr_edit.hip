// vr_edit.hip -- editing a scene image in place (vr_scene_edit) and reading its voxels
// back (vr_scene_voxels), on the GPU.  DESIGN.md 4d.
//
// The image already holds every voxel in the build's key order (vr_build.hip step 2), so
// an edit never sorts the scene:
//
//   1. export: the image's sorted unique (key, colour) list.  VCS: a mask word's value
//      index IS the list position of its first voxel (the colours lie in key order), so
//      every mask word writes its own voxels, no scan.  Cuckoo: a thread per (region, x, y)
//      counts the 64 z bits of the region's key-presence filter, one scan gives the
//      positions (thread order = key order x<<20|y<<10|z), the colours come from the
//      ordinary two-slot lookup.
//   2. the batch: keys as k_keys makes them, against the scene's own frame; a stable radix
//      sort of the n edits; the last edit of each key wins.
//   3. merge: each edit binary-searches the old keys -> overwrite (colour written into the
//      exported list), delete (keep flag cleared), insert (counted at its lower bound) or
//      nothing.  Two scans (kept old voxels; inserts at or before each old voxel) give every
//      survivor and every insert its place in the new list; two scatters write it.
//   4. emit: vr_build.hip's step 5 (emit_scene_gpu) on the new list.  Cuckoo regions whose
//      key set did not change keep their tables (k_cuckoo_copy); recoloured voxels of such
//      regions are then written into their slot.
#include <hip/hip_runtime.h>
#include <cstring>

#include "vr.h"
#include "vr_build_kernels.h"

namespace vr {
namespace {

// region_of[slot] = grid region index, the inverse of region_slot.
__global__ void k_region_of(const uint32_t* __restrict__ region_slot, uint64_t D3, uint32_t nr,
                            uint32_t* __restrict__ region_of) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= D3) return;
    const uint32_t r = region_slot[g];
    if (r < nr) region_of[r] = (uint32_t)g;
}

// VCS export: one thread per mask word (region r, cluster slot, word w).
__global__ void k_export_vcs(const uint2* __restrict__ mask, const uint32_t* __restrict__ vals,
                             const uint32_t* __restrict__ region_of, uint64_t words, uint64_t m,
                             uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= words) return;
    const uint2 rec = mask[t];
    uint32_t bits = rec.x;
    if (!bits || rec.y == kNone) return;
    const uint32_t r = (uint32_t)(t >> 13), slot = (uint32_t)(t >> 4) & 511u, w = (uint32_t)t & 15u;
    const uint32_t cid = ((slot & 7u) << 6) | (((slot >> 3) & 7u) << 3) | (slot >> 6);
    const uint64_t hi = ((uint64_t)region_of[r] << 18) | ((uint64_t)cid << 9) | (w << 5);
    uint64_t j = rec.y;
    while (bits && j < m) {
        const uint32_t b = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        key[j] = hi | b;
        val[j] = vals[j];
        ++j;
    }
}

// The 64 z bits of column (x, y) of a cuckoo region's key-presence filter (vr_internal.h
// ht_filter: word y2 | x<<1 | (y>>3)<<7 | (z>>3)<<10, bit (y&3)<<3 | z&7).
__device__ __forceinline__ uint64_t filter_column(const uint32_t* __restrict__ f, uint32_t x, uint32_t y) {
    const uint32_t w0 = ((y >> 2) & 1u) | (x << 1) | ((y >> 3) << 7), sh = (y & 3u) << 3;
    uint64_t z = 0;
    for (uint32_t zc = 0; zc < 8; ++zc) z |= (uint64_t)((f[w0 | (zc << 10)] >> sh) & 0xFFu) << (zc * 8u);
    return z;
}

// Cuckoo export, pass 1: thread t = r * 4096 + x * 64 + y counts its column's keys.
__global__ void k_count_hash(const uint32_t* __restrict__ filter, uint64_t cols, uint32_t* __restrict__ cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cols) return;
    const uint32_t x = (uint32_t)(t >> 6) & 63u, y = (uint32_t)t & 63u;
    cnt[t] = (uint32_t)__popcll(filter_column(filter + (t >> 12) * kHashFilterWords, x, y));
}

// Pass 2: the column's keys at off[t].., their colours by CuckooHashTable::lookupVoxel.
__global__ void k_export_hash(const uint32_t* __restrict__ filter, const uint32_t* __restrict__ off,
                              const uint32_t* __restrict__ region_of, const uint4* __restrict__ meta,
                              const uint2* __restrict__ slots, uint64_t cols, uint64_t m, uint64_t* __restrict__ key,
                              uint32_t* __restrict__ val) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cols) return;
    const uint32_t r = (uint32_t)(t >> 12), x = (uint32_t)(t >> 6) & 63u, y = (uint32_t)t & 63u;
    uint64_t zs = filter_column(filter + (uint64_t)r * kHashFilterWords, x, y);
    if (!zs) return;
    const uint4 mt = meta[r];
    const uint64_t hi = (uint64_t)region_of[r] << 26;
    uint64_t j = off[t];
    while (zs && j < m) {
        const uint32_t z = (uint32_t)__ffsll((unsigned long long)zs) - 1u;
        zs &= zs - 1u;
        const uint32_t k = (x << 20) | (y << 10) | z;
        const uint2 e1 = slots[mt.x + hash1(k, mt.w) % mt.y];
        const uint2 e2 = slots[mt.x + mt.y + hash2(k, mt.z) % mt.y];
        key[j] = hi | k;
        val[j] = e1.x == k ? e1.y : e2.y;
        ++j;
    }
}

// World coordinates of key j: the inverse of k_keys.
__global__ void k_key_xyz(const uint64_t* __restrict__ key, uint64_t m, int store, uint32_t D, int32_t minc,
                          int32_t* __restrict__ xyz) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint64_t k = key[j];
    uint32_t l[3];
    uint64_t g;
    if (store == STORE_VCS) {
        const uint32_t cid = (uint32_t)(k >> 9) & 511u, q = (uint32_t)k & 511u;
        l[0] = ((cid >> 6) << 3) | (q >> 6);
        l[1] = (((cid >> 3) & 7u) << 3) | ((q >> 3) & 7u);
        l[2] = ((cid & 7u) << 3) | (q & 7u);
        g = k >> 18;
    } else {
        l[0] = (uint32_t)(k >> 20) & 63u;
        l[1] = (uint32_t)(k >> 10) & 63u;
        l[2] = (uint32_t)k & 63u;
        g = k >> 26;
    }
    for (int a = 0; a < 3; ++a) {
        const int32_t rc = (int32_t)(g % D) + minc;
        g /= D;
        xyz[3 * j + a] = rc * kBlock + (int32_t)l[a];
    }
}

__device__ inline bool edit_ok(const int32_t* c, uint32_t col, int32_t minc, uint32_t D) {
    if (col > 0xFFFFFFu && col != VR_VOXEL_REMOVE) return false;
    for (int a = 0; a < 3; ++a)
        if ((uint32_t)(f2i(floorf((float)c[a] / 64.0f)) - minc) >= D) return false;
    return true;
}

// The first edit that the scene cannot take (edit_ok).
__global__ void k_edit_check(const int32_t* __restrict__ xyz, const uint32_t* __restrict__ rgb, uint64_t n, int32_t minc,
                             uint32_t D, unsigned long long* bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t c[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (!edit_ok(c, rgb[i], minc, D)) atomicMin(bad, (unsigned long long)i);
}

__device__ __forceinline__ uint32_t key_lower_bound(const uint64_t* __restrict__ a, uint32_t n, uint64_t k) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

enum : uint32_t { ACT_NONE = 0, ACT_OVERWRITE = 1, ACT_DELETE = 2, ACT_INSERT = 3 };

// What unique edit j does to the old list (okey/oval, m entries; keep = 1 and inscnt = 0 on
// entry).  lb[j] = its lower bound there; `changed` gets the regions whose key set changes.
__global__ void k_classify(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ eidx,
                           const uint32_t* __restrict__ rgb, uint32_t ne, const uint64_t* __restrict__ okey,
                           uint32_t* __restrict__ oval, uint32_t m, uint32_t shift, uint32_t* __restrict__ keep,
                           uint32_t* __restrict__ inscnt, uint32_t* __restrict__ ins, uint32_t* __restrict__ act,
                           uint32_t* __restrict__ lb, uint8_t* __restrict__ changed) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ne) return;
    const uint64_t k = ekey[j];
    const uint32_t col = rgb[eidx[j]];
    const uint32_t p = key_lower_bound(okey, m, k);
    const bool found = p < m && okey[p] == k;
    uint32_t a = ACT_NONE;
    if (found) {
        if (col == VR_VOXEL_REMOVE) {
            keep[p] = 0u;
            a = ACT_DELETE;
        } else {
            oval[p] = col;
            a = ACT_OVERWRITE;
        }
    } else if (col != VR_VOXEL_REMOVE) {
        atomicAdd(&inscnt[p], 1u);
        a = ACT_INSERT;
    }
    if (a >= ACT_DELETE) changed[k >> shift] = 1;
    ins[j] = a == ACT_INSERT ? 1u : 0u;
    act[j] = a;
    lb[j] = p;
}

// Old voxel i, kept, goes to (kept before it) + (inserts below it).
__global__ void k_scatter_old(const uint64_t* __restrict__ okey, const uint32_t* __restrict__ oval, uint32_t m,
                              const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kpos,
                              const uint32_t* __restrict__ sins, uint64_t* __restrict__ nkey, uint32_t* __restrict__ nval) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !keep[i]) return;
    const uint32_t d = kpos[i] + sins[i];
    nkey[d] = okey[i];
    nval[d] = oval[i];
}

// Insert j goes to (kept old voxels below it) + (inserts before it).
__global__ void k_scatter_ins(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ eidx,
                              const uint32_t* __restrict__ rgb, uint32_t ne, const uint32_t* __restrict__ ins,
                              const uint32_t* __restrict__ ipos, const uint32_t* __restrict__ lb,
                              const uint32_t* __restrict__ kpos, uint64_t* __restrict__ nkey, uint32_t* __restrict__ nval) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ne || !ins[j]) return;
    const uint32_t d = kpos[lb[j]] + ipos[j];
    nkey[d] = ekey[j];
    nval[d] = rgb[eidx[j]];
}

// A recoloured voxel of a cuckoo region that kept its tables: write the colour into its slot.
__global__ void k_recolour(const uint64_t* __restrict__ ekey, const uint32_t* __restrict__ eidx,
                           const uint32_t* __restrict__ rgb, uint32_t ne, const uint32_t* __restrict__ act,
                           const uint32_t* __restrict__ region_slot, const uint4* __restrict__ meta,
                           uint2* __restrict__ slots) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ne || act[j] != ACT_OVERWRITE) return;
    const uint32_t k = (uint32_t)ekey[j] & 0x3FFFFFFu;
    const uint4 mt = meta[region_slot[ekey[j] >> 26]];
    uint2* e1 = slots + mt.x + hash1(k, mt.w) % mt.y;
    uint2* e2 = slots + mt.x + mt.y + hash2(k, mt.z) % mt.y;
    if (e1->x == k) e1->y = rgb[eidx[j]];
    else if (e2->x == k) e2->y = rgb[eidx[j]];
}

// Step 1: the image's sorted unique list into key[m], val[m] (device).
int export_list(const GpuImage& g, Scratch& s, uint64_t* key, uint32_t* val, hipStream_t stream, std::string& err) {
    const uint64_t m = g.n_voxels;
    const uint32_t nr = g.n_regions;
    if (!m || !nr) return 0;
    const uint64_t D3 = (uint64_t)g.D * g.D * g.D;
    uint32_t* region_of;
    BUILD_CHECK(s.alloc(&region_of, nr));
    hipLaunchKernelGGL(k_region_of, blocks_for(D3), dim3(kThreads), 0, stream, (const uint32_t*)g.region_slot, D3, nr, region_of);
    if (g.store == STORE_VCS) {
        const uint64_t words = (uint64_t)nr * 8192u;
        hipLaunchKernelGGL(k_export_vcs, blocks_for(words), dim3(kThreads), 0, stream, (const uint2*)g.vcs_mask,
                           (const uint32_t*)g.vcs_vals, region_of, words, m, key, val);
        BUILD_CHECK(hipGetLastError());
    } else {
        const uint64_t cols = (uint64_t)nr * 4096u;
        if (cols >= 0xFFFFFFFFull * kThreads) { err = "too many regions to export"; return -1; }
        uint32_t *cnt, *off;
        BUILD_CHECK(s.alloc(&cnt, cols));
        BUILD_CHECK(s.alloc(&off, cols));
        hipLaunchKernelGGL(k_count_hash, blocks_for(cols), dim3(kThreads), 0, stream, (const uint32_t*)g.ht_filter, cols, cnt);
        BUILD_CHECK(hipGetLastError());
        if (int rc = scan(false, cnt, off, cols, stream, err)) return rc;
        hipLaunchKernelGGL(k_export_hash, blocks_for(cols), dim3(kThreads), 0, stream, (const uint32_t*)g.ht_filter, off,
                           region_of, (const uint4*)g.ht_meta, (const uint2*)g.ht_slots, cols, m, key, val);
        BUILD_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

int export_scene_gpu(const GpuImage& img, int32_t* xyz, uint32_t* rgb, hipStream_t stream, std::string& err) {
    const uint64_t m = img.n_voxels;
    if (!m) return 0;
    Scratch s;
    uint64_t* key;
    BUILD_CHECK(s.alloc(&key, m));
    if (int rc = export_list(img, s, key, rgb, stream, err)) return rc;
    hipLaunchKernelGGL(k_key_xyz, blocks_for(m), dim3(kThreads), 0, stream, key, m, img.store, img.D, img.min_coord, xyz);
    BUILD_CHECK(hipGetLastError());
    BUILD_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int edit_scene_gpu(const GpuImage& old, const int32_t* xyz, const uint32_t* rgb, uint64_t n, hipStream_t stream,
                   GpuScene& out, std::string& err) {
    out = GpuScene{};
    out.D = old.D;
    out.min_coord = old.min_coord;
    const int store = old.store;
    const uint64_t m = old.n_voxels;
    if (n >= 0xFFFFFFFFull || m + n >= 0xFFFFFFFFull) { err = "too many voxels"; return -1; }
    Scratch s;
    // the edits the scene cannot take: none is applied
    unsigned long long* bad;
    BUILD_CHECK(s.alloc(&bad, 1));
    const unsigned long long bad0 = ~0ull;
    BUILD_CHECK(hipMemcpyAsync(bad, &bad0, sizeof bad0, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_edit_check, blocks_for(n), dim3(kThreads), 0, stream, xyz, rgb, n, old.min_coord, old.D, bad);
    BUILD_CHECK(hipGetLastError());
    const unsigned long long badh = read_back(bad, stream);
    if (badh != ~0ull) {
        int32_t c[3];
        BUILD_CHECK(hipMemcpyAsync(c, xyz + 3 * badh, sizeof c, hipMemcpyDeviceToHost, stream));
        const uint32_t v = read_back(rgb + badh, stream);
        if (v > 0xFFFFFFu && v != VR_VOXEL_REMOVE)
            err = "edit colour " + std::to_string(v) + " at index " + std::to_string(badh) +
                  " is neither 24-bit RGB nor VR_VOXEL_REMOVE";
        else
            err = "edit at index " + std::to_string(badh) + " (" + std::to_string(c[0]) + "," + std::to_string(c[1]) + "," +
                  std::to_string(c[2]) + ") lies outside the scene's frame (min_coord " + std::to_string(old.min_coord) +
                  ", diameter " + std::to_string(old.D) + ")";
        return -1;
    }
    const uint64_t D3 = (uint64_t)old.D * old.D * old.D;
    uint32_t rbits = 1;
    while (rbits < 64 && (D3 - 1) >> rbits) ++rbits;
    const uint32_t shift = store == STORE_VCS ? 18u : 26u;

    // 1. the old list
    uint64_t* okey;
    uint32_t* oval;
    BUILD_CHECK(s.alloc(&okey, m));
    BUILD_CHECK(s.alloc(&oval, m));
    if (int rc = export_list(old, s, okey, oval, stream, err)) return rc;

    // 2. the batch: keys, stable sort, last edit of a key
    uint64_t *key_a, *key_b, *ekey;
    uint32_t *idx_a, *idx_b, *eidx, *flag, *pos;
    BUILD_CHECK(s.alloc(&key_a, n));
    BUILD_CHECK(s.alloc(&key_b, n));
    BUILD_CHECK(s.alloc(&idx_a, n));
    BUILD_CHECK(s.alloc(&idx_b, n));
    hipLaunchKernelGGL(k_keys, blocks_for(n), dim3(kThreads), 0, stream, xyz, n, old.min_coord, old.D, store, key_a, idx_a);
    BUILD_CHECK(hipGetLastError());
    size_t sort_bytes = 0;
    const unsigned end_bit = shift + rbits;
    BUILD_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_a, key_b, idx_a, idx_b, (size_t)n, 0, end_bit, stream));
    void* sort_tmp = nullptr;
    BUILD_CHECK(s.alloc((char**)&sort_tmp, sort_bytes));
    BUILD_CHECK(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, key_a, key_b, idx_a, idx_b, (size_t)n, 0, end_bit, stream));
    BUILD_CHECK(s.alloc(&flag, n));
    BUILD_CHECK(s.alloc(&pos, n));
    hipLaunchKernelGGL(k_flag_last, blocks_for(n), dim3(kThreads), 0, stream, key_b, n, flag);
    BUILD_CHECK(hipGetLastError());
    if (int rc = scan(false, flag, pos, n, stream, err)) return rc;
    const uint32_t ne = read_back(pos + n - 1, stream) + read_back(flag + n - 1, stream);
    BUILD_CHECK(s.alloc(&ekey, ne));
    BUILD_CHECK(s.alloc(&eidx, ne));
    hipLaunchKernelGGL(k_compact, blocks_for(n), dim3(kThreads), 0, stream, key_b, idx_b, flag, pos, n, ekey, eidx);
    BUILD_CHECK(hipGetLastError());

    // 3. merge
    uint32_t *keep, *kpos, *inscnt, *sins, *ins, *ipos, *act, *lb;
    uint8_t* changed;
    BUILD_CHECK(s.alloc(&keep, m + 1));
    BUILD_CHECK(s.alloc(&kpos, m + 1));
    BUILD_CHECK(s.alloc(&inscnt, m + 1));
    BUILD_CHECK(s.alloc(&sins, m + 1));
    BUILD_CHECK(s.alloc(&ins, ne));
    BUILD_CHECK(s.alloc(&ipos, ne));
    BUILD_CHECK(s.alloc(&act, ne));
    BUILD_CHECK(s.alloc(&lb, ne));
    BUILD_CHECK(s.alloc(&changed, D3));
    hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)std::min<uint64_t>(4096, (m + kThreads) / kThreads)), dim3(kThreads), 0, stream,
                       keep, m, 1u);
    BUILD_CHECK(hipGetLastError());
    BUILD_CHECK(hipMemsetAsync(keep + m, 0, sizeof(uint32_t), stream));
    BUILD_CHECK(hipMemsetAsync(inscnt, 0, (m + 1) * sizeof(uint32_t), stream));
    BUILD_CHECK(hipMemsetAsync(changed, 0, D3, stream));
    hipLaunchKernelGGL(k_classify, blocks_for(ne), dim3(kThreads), 0, stream, ekey, eidx, rgb, ne, okey, oval, (uint32_t)m, shift,
                       keep, inscnt, ins, act, lb, changed);
    BUILD_CHECK(hipGetLastError());
    if (int rc = scan(false, keep, kpos, m + 1, stream, err)) return rc;
    if (int rc = scan(true, inscnt, sins, m + 1, stream, err)) return rc;
    if (int rc = scan(false, ins, ipos, (uint64_t)ne, stream, err)) return rc;
    const uint64_t m2 = (uint64_t)read_back(kpos + m, stream) + read_back(sins + m, stream);
    uint64_t* nkey;
    uint32_t* nval;
    BUILD_CHECK(s.alloc(&nkey, m2));
    BUILD_CHECK(s.alloc(&nval, m2));
    if (m) hipLaunchKernelGGL(k_scatter_old, blocks_for(m), dim3(kThreads), 0, stream, okey, oval, (uint32_t)m, keep, kpos, sins, nkey, nval);
    hipLaunchKernelGGL(k_scatter_ins, blocks_for(ne), dim3(kThreads), 0, stream, ekey, eidx, rgb, ne, ins, ipos, lb, kpos, nkey, nval);
    BUILD_CHECK(hipGetLastError());

    // 4. emit; unchanged cuckoo regions keep their tables
    const CuckooReuse reuse{changed, (const uint32_t*)old.region_slot, old.ht_meta, old.ht_slots};
    if (int rc = emit_scene_gpu(store, nkey, nullptr, nval, m2, stream, out, err, store == STORE_VCS ? nullptr : &reuse)) return rc;
    if (store != STORE_VCS && out.n_regions) {
        hipLaunchKernelGGL(k_recolour, blocks_for(ne), dim3(kThreads), 0, stream, ekey, eidx, rgb, ne, act,
                           (const uint32_t*)out.region_slot, (const uint4*)out.ht_meta, (uint2*)out.ht_slots);
        BUILD_CHECK(hipGetLastError());
        BUILD_CHECK(hipStreamSynchronize(stream));
    }
    return 0;
}

}  // namespace vr
