// vr_build.hip -- the scene build on the GPU:
// VoxelSceneCPU::insertVoxel / generateVoxelScene (VoxelSceneCPU.cuh:16-93),
// the VoxelClusterStore image (VoxelClusterStore.cuh:37-85) and the
// CuckooHashTable images (CuckooHashTable.cuh:20-49, 97-178), producing the
// same device layout as the host builder in vr_scene.cpp (vr_internal.h):
//
//   1. region coordinates, the min/max coordinate (minCoord/maxCoord start at 0)
//      and the first colour above 24 bits                       (reduction)
//   2. one 64-bit sort key per voxel: region | (cluster, in-cluster index) for
//      the VCS, region | x<<20|y<<10|z for the hash table           (map)
//   3. stable radix sort of (key, insertion index)                  (rocPRIM)
//   4. keep the LAST insertion of each key (unordered_map assignment, :46)
//   5. region slots in region order; VCS: colours in (region, cluster, key)
//      order and one 16-word mask record per present cluster (a thread per
//      cluster); cuckoo: per region the host's sequential insertion with the
//      same seeded rehash (one lane per region), so every key lands in the
//      same table as in the host build -- which the lookup's algorithmic byte
//      count (key found in table 1 or 2) depends on.
#include <hip/hip_runtime.h>
#include <cstring>

#include "vr_build_kernels.h"

namespace vr {
namespace {

__global__ void k_minmax(const int32_t* __restrict__ xyz, const uint32_t* __restrict__ rgb, uint64_t n,
                         int32_t* mm, unsigned long long* bad) {
    int32_t lo = 0, hi = 0;                       // minCoord / maxCoord start at 0 (VoxelSceneCPU.cuh)
    unsigned long long first_bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        for (int a = 0; a < 3; ++a) {
            const int32_t c = f2i(floorf((float)xyz[3 * i + a] / 64.0f));   // :19-21
            lo = min(lo, c);
            hi = max(hi, c);
        }
        if (rgb[i] > 0xFFFFFFu && i < first_bad) first_bad = i;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_down(lo, off, 64));
        hi = max(hi, __shfl_down(hi, off, 64));
        first_bad = min(first_bad, __shfl_down(first_bad, off, 64));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
        if (first_bad != ~0ull) atomicMin(bad, first_bad);
    }
}

}  // namespace

int build_scene_gpu(int store, const int32_t* xyz, const uint32_t* rgb, uint64_t n, hipStream_t stream,
                    GpuScene& out, std::string& err) {
    out = GpuScene{};
    Scratch s;
    // 1. min / max region coordinate, first colour above 24 bits
    int32_t* mm;
    unsigned long long* bad;
    BUILD_CHECK(s.alloc(&mm, 2));
    BUILD_CHECK(s.alloc(&bad, 1));
    const int32_t mm0[2] = {0, 0};
    const unsigned long long bad0 = ~0ull;
    BUILD_CHECK(hipMemcpyAsync(mm, mm0, sizeof mm0, hipMemcpyHostToDevice, stream));
    BUILD_CHECK(hipMemcpyAsync(bad, &bad0, sizeof bad0, hipMemcpyHostToDevice, stream));
    if (n) {
        hipLaunchKernelGGL(k_minmax, dim3((unsigned)std::min<uint64_t>(2048, (n + kThreads - 1) / kThreads)), dim3(kThreads),
                           0, stream, xyz, rgb, n, mm, bad);
        BUILD_CHECK(hipGetLastError());
    }
    int32_t mmh[2];
    BUILD_CHECK(hipMemcpyAsync(mmh, mm, sizeof mmh, hipMemcpyDeviceToHost, stream));
    const unsigned long long badh = read_back(bad, stream);
    if (badh != ~0ull) {
        const uint32_t v = read_back(rgb + badh, stream);
        err = "voxel colour " + std::to_string(v) + " at index " + std::to_string(badh) + " exceeds 24-bit RGB";
        return -1;
    }
    const int64_t D64 = (int64_t)mmh[1] - (int64_t)mmh[0] + 1;
    if (D64 > 1024) {
        err = "scene spans more than 1024 regions per axis";
        return -1;
    }
    out.D = (uint32_t)D64;
    out.min_coord = mmh[0];
    const uint64_t D3 = (uint64_t)out.D * out.D * out.D;
    uint32_t rbits = 1;
    while (rbits < 64 && (D3 - 1) >> rbits) ++rbits;
    const uint32_t shift = store == STORE_VCS ? 18u : 26u;          // key >> shift = region

    uint64_t m = 0;
    uint64_t *key_a = nullptr, *key_b = nullptr, *ukey = nullptr;
    uint32_t *idx_a = nullptr, *idx_b = nullptr, *uidx = nullptr, *flag = nullptr, *pos = nullptr;
    if (n) {
        // 2-3. keys and a stable radix sort by key
        BUILD_CHECK(s.alloc(&key_a, n));
        BUILD_CHECK(s.alloc(&key_b, n));
        BUILD_CHECK(s.alloc(&idx_a, n));
        BUILD_CHECK(s.alloc(&idx_b, n));
        hipLaunchKernelGGL(k_keys, blocks_for(n), dim3(kThreads), 0, stream, xyz, n, out.min_coord, out.D, store, key_a, idx_a);
        BUILD_CHECK(hipGetLastError());
        size_t sort_bytes = 0;
        const unsigned end_bit = shift + rbits;
        BUILD_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_a, key_b, idx_a, idx_b, (size_t)n, 0, end_bit, stream));
        void* sort_tmp = nullptr;
        BUILD_CHECK(s.alloc((char**)&sort_tmp, sort_bytes));
        BUILD_CHECK(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, key_a, key_b, idx_a, idx_b, (size_t)n, 0, end_bit, stream));
        // 4. keep the last insertion of every key
        BUILD_CHECK(s.alloc(&flag, n));
        BUILD_CHECK(s.alloc(&pos, n));
        hipLaunchKernelGGL(k_flag_last, blocks_for(n), dim3(kThreads), 0, stream, key_b, n, flag);
        BUILD_CHECK(hipGetLastError());
        if (int rc = scan(false, flag, pos, n, stream, err)) return rc;
        m = (uint64_t)read_back(pos + n - 1, stream) + read_back(flag + n - 1, stream);
        BUILD_CHECK(s.alloc(&ukey, m));
        BUILD_CHECK(s.alloc(&uidx, m));
        hipLaunchKernelGGL(k_compact, blocks_for(n), dim3(kThreads), 0, stream, key_b, idx_b, flag, pos, n, ukey, uidx);
        BUILD_CHECK(hipGetLastError());
    }
    return emit_scene_gpu(store, ukey, uidx, rgb, m, stream, out, err);
}

int emit_scene_gpu(int store, const uint64_t* ukey, const uint32_t* uidx, const uint32_t* rgb, uint64_t m,
                   hipStream_t stream, GpuScene& out, std::string& err, const CuckooReuse* reuse) {
    Scratch s;
    const uint64_t D3 = (uint64_t)out.D * out.D * out.D;
    const uint32_t shift = store == STORE_VCS ? 18u : 26u;          // key >> shift = region
    // region table (all null) even for an empty scene
    BUILD_CHECK(hipMalloc(&out.region_slot, D3 * sizeof(uint32_t)));
    out.region_slot_bytes = D3 * sizeof(uint32_t);
    hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)std::min<uint64_t>(4096, (D3 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       stream, (uint32_t*)out.region_slot, D3, kNone);
    BUILD_CHECK(hipGetLastError());

    uint32_t *flag = nullptr, *pos = nullptr;
    uint32_t nr = 0;
    uint32_t *rstart = nullptr, *rslot_of = nullptr;
    if (m) {
        // 5. regions: starts, slots (region order), the slot of every voxel
        BUILD_CHECK(s.alloc(&flag, m));
        BUILD_CHECK(s.alloc(&pos, m));
        hipLaunchKernelGGL(k_flag_first, blocks_for(m), dim3(kThreads), 0, stream, ukey, m, shift, flag);
        BUILD_CHECK(hipGetLastError());
        if (int rc = scan(false, flag, pos, m, stream, err)) return rc;
        nr = read_back(pos + m - 1, stream) + read_back(flag + m - 1, stream);
        BUILD_CHECK(s.alloc(&rstart, nr));
        hipLaunchKernelGGL(k_starts, blocks_for(m), dim3(kThreads), 0, stream, flag, pos, m, rstart);
        hipLaunchKernelGGL(k_region_slots, blocks_for(nr), dim3(kThreads), 0, stream, ukey, rstart, nr, shift, (uint32_t*)out.region_slot);
        BUILD_CHECK(hipGetLastError());
        if (store == STORE_VCS) {
            BUILD_CHECK(s.alloc(&rslot_of, m));
            if (int rc = scan(true, flag, rslot_of, m, stream, err)) return rc;
            hipLaunchKernelGGL(k_minus_one, blocks_for(m), dim3(kThreads), 0, stream, rslot_of, m);
            BUILD_CHECK(hipGetLastError());
        }
    }
    out.n_regions = nr;
    out.n_voxels = m;
    if (store == STORE_VCS && nr > kVcsMaxRegions) {   // (cuckoo scenes have no region bound)
        err = "VCS scene with " + std::to_string(nr) + " occupied 64^3 regions (at most " +
              std::to_string(kVcsMaxRegions) + ")";
        return -1;
    }

    if (store == STORE_VCS) {
        const uint64_t words = std::max<uint64_t>((uint64_t)nr * 8192u, 16u);
        BUILD_CHECK(hipMalloc(&out.vcs_mask, words * sizeof(uint2)));
        out.vcs_mask_bytes = words * sizeof(uint2);
        hipLaunchKernelGGL(k_fill_u2, dim3((unsigned)std::min<uint64_t>(8192, (words + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, (uint2*)out.vcs_mask, words, make_uint2(0u, kNone));
        BUILD_CHECK(hipGetLastError());
        BUILD_CHECK(hipMalloc(&out.vcs_vals, std::max<uint64_t>(m, 1) * sizeof(uint32_t)));
        out.vcs_vals_bytes = std::max<uint64_t>(m, 1) * sizeof(uint32_t);
        if (m) {
            hipLaunchKernelGGL(k_gather_vals, blocks_for(m), dim3(kThreads), 0, stream, rgb, uidx, m, (uint32_t*)out.vcs_vals);
            // clusters: starts, then one thread per cluster writes its record
            hipLaunchKernelGGL(k_flag_first, blocks_for(m), dim3(kThreads), 0, stream, ukey, m, 9u, flag);
            BUILD_CHECK(hipGetLastError());
            if (int rc = scan(false, flag, pos, m, stream, err)) return rc;
            const uint32_t nc = read_back(pos + m - 1, stream) + read_back(flag + m - 1, stream);
            uint32_t* cstart;
            BUILD_CHECK(s.alloc(&cstart, nc));
            hipLaunchKernelGGL(k_starts, blocks_for(m), dim3(kThreads), 0, stream, flag, pos, m, cstart);
            hipLaunchKernelGGL(k_cluster_records, blocks_for(nc), dim3(kThreads), 0, stream, ukey, cstart, nc, m, rslot_of,
                               (uint2*)out.vcs_mask);
            BUILD_CHECK(hipGetLastError());
        } else {
            const uint32_t zero = 0;
            BUILD_CHECK(hipMemcpyAsync(out.vcs_vals, &zero, 4, hipMemcpyHostToDevice, stream));
        }
    } else {
        uint32_t *M = nullptr, *slots2 = nullptr, *base2 = nullptr, *failed = nullptr;
        uint64_t total = 2;
        if (nr) {
            BUILD_CHECK(s.alloc(&M, nr));
            BUILD_CHECK(s.alloc(&slots2, nr));
            BUILD_CHECK(s.alloc(&base2, nr));
            hipLaunchKernelGGL(k_region_sizes, blocks_for(nr), dim3(kThreads), 0, stream, rstart, nr, m, M, slots2);
            BUILD_CHECK(hipGetLastError());
            if (int rc = scan(false, slots2, base2, (uint64_t)nr, stream, err)) return rc;
            total = (uint64_t)read_back(base2 + nr - 1, stream) + read_back(slots2 + nr - 1, stream);
            if (total >= 0xFFFFFFFFull) { err = "hash slots exceed 32-bit offsets"; return -5; }
            total = std::max<uint64_t>(total, 2);
        }
        BUILD_CHECK(hipMalloc(&out.ht_slots, total * sizeof(uint2)));
        out.ht_slots_bytes = total * sizeof(uint2);
        hipLaunchKernelGGL(k_fill_u2, dim3((unsigned)std::min<uint64_t>(8192, (total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, (uint2*)out.ht_slots, total, make_uint2(kEmpty, 0u));
        const uint64_t metas = std::max<uint32_t>(nr, 1);
        BUILD_CHECK(hipMalloc(&out.ht_meta, metas * sizeof(uint4)));
        out.ht_meta_bytes = metas * sizeof(uint4);
        BUILD_CHECK(hipMemsetAsync(out.ht_meta, 0, metas * sizeof(uint4), stream));
        if (nr) {
            BUILD_CHECK(s.alloc(&failed, 1));
            BUILD_CHECK(hipMemsetAsync(failed, 0, 4, stream));
            hipLaunchKernelGGL(k_cuckoo, dim3(nr), dim3(64), 0, stream, ukey, uidx, rgb, rstart, nr, m, M, base2,
                               (uint2*)out.ht_slots, (uint4*)out.ht_meta, failed, reuse ? reuse->changed : nullptr);
            if (reuse)
                hipLaunchKernelGGL(k_cuckoo_copy, dim3(nr), dim3(kThreads), 0, stream, ukey, rstart, nr, M, base2, reuse->changed,
                                   reuse->region_slot, (const uint4*)reuse->ht_meta, (const uint2*)reuse->ht_slots,
                                   (uint2*)out.ht_slots, (uint4*)out.ht_meta);
            BUILD_CHECK(hipGetLastError());
            if (read_back(failed, stream)) { err = "cuckoo hash table build failed"; return -5; }
        }
    }
    BUILD_CHECK(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace vr
