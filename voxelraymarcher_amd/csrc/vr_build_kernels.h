// vr_build_kernels.h -- the kernels and small host helpers that the scene build
// (vr_build.hip) and the in-place edit (vr_edit.hip) share: sort keys, the
// last-insertion dedupe, group starts, and the emit of the VCS records and the
// cuckoo tables from a sorted unique (key, colour) list.  Everything is in an
// anonymous namespace: each of the two translation units gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "vr_build.h"
#include "vr_device.h"

namespace vr {
namespace {

constexpr uint32_t kThreads = 256;

// Sort key of voxel i and its insertion index.
__global__ void k_keys(const int32_t* __restrict__ xyz, uint64_t n, int32_t minc, uint32_t D, int store,
                       uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t l[3];
    uint64_t region = 0, mul = 1;
    for (int a = 0; a < 3; ++a) {
        const int32_t c = xyz[3 * i + a];
        const int32_t rc = f2i(floorf((float)c / 64.0f));
        l[a] = (uint32_t)(((c % kBlock) + kBlock) % kBlock);                // :24-26
        region += (uint64_t)(uint32_t)(rc - minc) * mul;
        mul *= D;
    }
    uint64_t k;
    if (store == STORE_VCS) {
        const uint32_t cid = ((l[0] >> 3) << 6) | ((l[1] >> 3) << 3) | (l[2] >> 3);
        const uint32_t q = ((l[0] & 7u) << 6) | ((l[1] & 7u) << 3) | (l[2] & 7u);
        k = (region << 18) | ((uint64_t)cid << 9) | q;
    } else {
        k = (region << 26) | ((l[0] << 20) | (l[1] << 10) | l[2]);          // generate3DPoint
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
}

// 1 where this sorted entry is the last of its key (the winning insertion).
__global__ void k_flag_last(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ f) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f[i] = (i + 1 == n || key[i] != key[i + 1]) ? 1u : 0u;
}

// 1 where key >> shift differs from the previous entry's (first of a group).
__global__ void k_flag_first(const uint64_t* __restrict__ key, uint64_t n, uint32_t shift, uint32_t* __restrict__ f) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f[i] = (i == 0 || (key[i] >> shift) != (key[i - 1] >> shift)) ? 1u : 0u;
}

__global__ void k_compact(const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ f,
                          const uint32_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ ukey, uint32_t* __restrict__ uidx) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && f[i]) {
        ukey[pos[i]] = key[i];
        uidx[pos[i]] = idx[i];
    }
}

// Group starts: start[pos[i]] = i where f[i].
__global__ void k_starts(const uint32_t* __restrict__ f, const uint32_t* __restrict__ pos, uint64_t n, uint32_t* __restrict__ start) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && f[i]) start[pos[i]] = (uint32_t)i;
}

__global__ void k_fill_u32(uint32_t* __restrict__ p, uint64_t n, uint32_t v) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void k_fill_u2(uint2* __restrict__ p, uint64_t n, uint2 v) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = v;
}

// region_slot[region] = slot, for the first voxel of each region.
__global__ void k_region_slots(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ rstart, uint32_t nr,
                               uint32_t shift, uint32_t* __restrict__ region_slot) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nr) region_slot[ukey[rstart[r]] >> shift] = r;
}

// vals[j] = rgb[uidx[j]], or rgb[j] without an index list (uidx null).
__global__ void k_gather_vals(const uint32_t* __restrict__ rgb, const uint32_t* __restrict__ uidx, uint64_t m,
                              uint32_t* __restrict__ vals) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) vals[j] = rgb[uidx ? uidx[j] : (uint32_t)j];
}

// One thread per present cluster: its 16 mask words {occupancy bits, value
// index of the word's first voxel}, in the record of slot perm(cid) of its region.
__global__ void k_cluster_records(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ cstart, uint32_t nc,
                                  uint64_t m, const uint32_t* __restrict__ rslot_of, uint2* __restrict__ mask) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const uint32_t b = cstart[c];
    const uint32_t e = c + 1 < nc ? cstart[c + 1] : (uint32_t)m;
    const uint32_t r = rslot_of[b];
    const uint32_t cid = (uint32_t)(ukey[b] >> 9) & 511u;
    const uint32_t slot = (cid >> 6) | (((cid >> 3) & 7u) << 3) | ((cid & 7u) << 6);
    uint2* rec = mask + ((size_t)r * 512 + slot) * 16;
    uint32_t j = b, run = b;
    for (uint32_t w = 0; w < 16; ++w) {
        uint32_t bits = 0;
        while (j < e && (((uint32_t)ukey[j] & 511u) >> 5) == w) {
            bits |= 1u << ((uint32_t)ukey[j] & 31u);
            ++j;
        }
        rec[w] = make_uint2(bits, run);
        run += (uint32_t)__popc(bits);
    }
}

// Region slot of every unique voxel: (inclusive scan of region starts) - 1.
__global__ void k_minus_one(uint32_t* __restrict__ p, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] -= 1u;
}

// Per region: n_r, M_r = (u32)(n_r * 1.25) (CuckooHashTable.cuh:23) and 2 M_r slots.
__global__ void k_region_sizes(const uint32_t* __restrict__ rstart, uint32_t nr, uint64_t m, uint32_t* __restrict__ M,
                               uint32_t* __restrict__ slots2) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const uint32_t b = rstart[r], e = r + 1 < nr ? rstart[r + 1] : (uint32_t)m;
    const uint32_t Mr = (uint32_t)((double)(e - b) * 1.25);
    M[r] = Mr;
    slots2[r] = 2u * Mr;
}

__constant__ uint32_t c_primes[14] = {668265261u, 12289u, 24593u, 49157u, 98317u, 196613u, 393241u,
                                      786433u, 1572869u, 3145739u, 6291469u, 12582917u, 25165843u, 50331653u};

// One wave per region: lane 0 inserts the region's keys in sorted order with
// the host builder's algorithm (bucket alternation, 300 000-step eviction
// limit, seeded prime/offset rehash, at most 4096 attempts); the wave clears
// the tables before each attempt.  Values are rgb[uidx[i]], or rgb[i] without
// an index list.  With `changed` (the edit: one byte per grid region) only
// regions whose byte is set are built; the others are k_cuckoo_copy's.
__global__ void k_cuckoo(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ uidx, const uint32_t* __restrict__ rgb,
                         const uint32_t* __restrict__ rstart, uint32_t nr, uint64_t m, const uint32_t* __restrict__ M,
                         const uint32_t* __restrict__ base2, uint2* __restrict__ slots, uint4* __restrict__ meta,
                         uint32_t* __restrict__ failed, const uint8_t* __restrict__ changed) {
    const uint32_t r = blockIdx.x;
    if (r >= nr) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t b = rstart[r], e = r + 1 < nr ? rstart[r + 1] : (uint32_t)m, n = e - b;
    if (changed && !changed[ukey[b] >> 26]) return;
    const uint32_t Mr = M[r];
    uint2* t = slots + base2[r];
    __shared__ uint32_t s_prime, s_offset, s_done;
    if (lane == 0) {
        s_prime = c_primes[0];
        s_offset = 0;
        s_done = 0;
    }
    __syncthreads();
    const uint32_t key0 = (uint32_t)ukey[b] & 0x3FFFFFFu;
    uint64_t rng = 0x9E3779B97F4A7C15ull ^ (uint64_t)n ^ ((uint64_t)key0 << 20);
    for (int attempt = 0; attempt < 4096; ++attempt) {
        for (uint32_t i = lane; i < 2u * Mr; i += blockDim.x) t[i] = make_uint2(kEmpty, 0u);
        __threadfence_block();
        __syncthreads();
        if (lane == 0) {
            const uint32_t prime = s_prime, offset = s_offset;
            bool rehash = false;
            for (uint32_t i = b; i < e && !rehash; ++i) {
                uint32_t code = (uint32_t)ukey[i] & 0x3FFFFFFu, value = rgb[uidx ? uidx[i] : i], bucket = 0, it = 0;
                for (;;) {
                    if (it >= 300000u) { rehash = true; break; }
                    uint2* slot = bucket == 0 ? t + hash1(code, offset) % Mr : t + Mr + hash2(code, prime) % Mr;
                    const uint2 old = *slot;
                    *slot = make_uint2(code, value);
                    if (old.x == kEmpty) break;
                    code = old.x;
                    value = old.y;
                    bucket ^= 1u;
                    ++it;
                }
            }
            if (!rehash) {
                meta[r] = make_uint4(base2[r], Mr, prime, offset);
                s_done = 1;
            } else {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                s_prime = c_primes[(rng >> 33) % 14u];
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                s_offset = (uint32_t)((rng >> 33) % 25u);
            }
        }
        __syncthreads();
        if (s_done) return;
    }
    if (lane == 0) atomicAdd(failed, 1u);
}

// The edit's other half of k_cuckoo: a region whose key set did not change keeps its
// tables (the same keys inserted in the same order land in the same slots), copied to the
// region's new base; its meta keeps {M, prime, offset}.  One workgroup per region.
__global__ void k_cuckoo_copy(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ rstart, uint32_t nr,
                              const uint32_t* __restrict__ M, const uint32_t* __restrict__ base2,
                              const uint8_t* __restrict__ changed, const uint32_t* __restrict__ old_region_slot,
                              const uint4* __restrict__ old_meta, const uint2* __restrict__ old_slots,
                              uint2* __restrict__ slots, uint4* __restrict__ meta) {
    const uint32_t r = blockIdx.x;
    if (r >= nr) return;
    const uint64_t g = ukey[rstart[r]] >> 26;
    if (changed[g]) return;
    const uint4 om = old_meta[old_region_slot[g]];
    const uint32_t Mr = M[r];               // == om.y: the region has as many keys as before
    const uint2* src = old_slots + om.x;
    uint2* dst = slots + base2[r];
    for (uint32_t i = threadIdx.x; i < 2u * Mr; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x == 0) meta[r] = make_uint4(base2[r], Mr, om.z, om.w);
}

inline dim3 blocks_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, (n + kThreads - 1) / kThreads)); }

struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T>
    hipError_t alloc(T** p, uint64_t count) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<uint64_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) { ptrs.push_back(q); *p = (T*)q; }
        return e;
    }
};

#define BUILD_CHECK(expr)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
            return -2;                                                                      \
        }                                                                                   \
    } while (0)

template <class T>
int scan(bool inclusive, const T* in, T* out, uint64_t n, hipStream_t stream, std::string& err) {
    size_t bytes = 0;
    void* tmp = nullptr;
    if (inclusive) BUILD_CHECK(rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)n, rocprim::plus<T>(), stream));
    else BUILD_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), stream));
    BUILD_CHECK(hipMalloc(&tmp, std::max<size_t>(bytes, 1)));
    hipError_t e = inclusive ? rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<T>(), stream)
                             : rocprim::exclusive_scan(tmp, bytes, in, out, T(0), (size_t)n, rocprim::plus<T>(), stream);
    (void)hipStreamSynchronize(stream);
    (void)hipFree(tmp);
    BUILD_CHECK(e);
    return 0;
}

template <class T>
T read_back(const T* p, hipStream_t stream) {
    T v{};
    (void)hipMemcpyAsync(&v, p, sizeof(T), hipMemcpyDeviceToHost, stream);
    (void)hipStreamSynchronize(stream);
    return v;
}

}  // namespace
}  // namespace vr
