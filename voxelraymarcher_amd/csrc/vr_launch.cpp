// vr_launch.cpp -- the render launch: the per-device slot ring, the learned orders and the
// crawl-pass skip kept per slot (their decisions: vr_launch_plan.h), the render entry points of
// include/vr.h with the view they render (make_view; vr_query_api.cpp's pick shares it, its
// shade the lighting block, view_lighting, and nothing else), the band and tile helpers and the
// vr_debug_* functions.
//
// Replaces runRaymarchingKernel (main/Main.cu:105-163).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "vr_host.h"
#pragma GCC visibility push(hidden)
#include "vr_launch_plan.h"
#pragma GCC visibility pop

namespace vr {

void view_camera(KView& v, const vr_camera* cam, uint32_t width, uint32_t height) {
    for (int i = 0; i < 3; ++i) {
        v.llc[i] = cam->lower_left[i]; v.hor[i] = cam->horizontal[i]; v.ver[i] = cam->vertical[i];
        v.org[i] = cam->origin[i];
    }
    v.W = width;
    v.H = height;
    v.LW = width;
}

void view_lighting(KView& v, const vr_lighting* lit) {
    for (int i = 0; i < 3; ++i) {
        v.L[i] = lit->light_dir[i]; v.LC[i] = lit->light_color[i]; v.LP[i] = lit->light_pos[i];
    }
    v.L_fast = 1u;
    for (int i = 0; i < 3; ++i) {
        const float a = std::fabs(v.L[i]);
        v.Lr[i] = 1.0f / v.L[i];
        if (!(a >= 0x1p-64f && a <= 0x1p+20f)) v.L_fast = 0u;
    }
    {
        // the light's longest-axis frame, in the device's fp32 order (-ffp-contract=off)
        const float ax = std::fabs(v.L[0]), ay = std::fabs(v.L[1]), az = std::fabs(v.L[2]);
        const uint32_t order =
            (ax > ay && ax > az) ? (ay > az ? 0u : 1u) : (ay > az ? (ax > az ? 2u : 3u) : (ax > ay ? 4u : 5u));
        const float k = 1.0f / (order < 2u ? ax : (order < 4u ? ay : az));
        uint32_t cls = 0;
        bool unit = order == 5u && ax == ay && ay == az;
        for (int i = 0; i < 3; ++i) {
            v.Lw[i] = k * v.L[i];
            cls |= (uint32_t)(v.Lw[i] > 0.0f) << (2 * i) | (uint32_t)(v.Lw[i] < 0.0f) << (2 * i + 1);
            unit = unit && std::fabs(v.Lw[i]) == 1.0f;
        }
        v.L_order = order;
        v.L_cls = cls;
        v.L_unit = unit ? 1u : 0u;
        v.L_eq = (v.L[0] == v.L[1] && v.L[1] == v.L[2]) ? 1u : 0u;
    }
    v.use_point_light = lit->use_point_light ? 1 : 0;
    v.use_shadows = lit->use_shadows ? 1 : 0;
}

int make_view(const vr_scene* s, const vr_camera* cam, const vr_lighting* lit, const float translation[3],
              uint32_t scale, uint32_t width, uint32_t height, KView& v) {
    if (!s) return fail(VR_E_INVALID, "scene is NULL");
    if (!cam || !lit) return fail(VR_E_INVALID, "camera/lighting NULL");
    if (width == 0 || height == 0 || width > 65536 || height > 65536) return fail(VR_E_INVALID, "bad image size");
    memset(&v, 0, sizeof v);
    view_camera(v, cam, width, height);
    view_lighting(v, lit);
    for (int i = 0; i < 3; ++i) v.translation[i] = translation ? translation[i] : 0.0f;
    v.scale_f = (float)scale;          // static_cast<float>(scale) (Ray.cuh:16)
    return VR_OK;
}

}  // namespace vr

namespace {

using vr::DeviceGuard;
using vr::fail;
using vr::hip_fail;
using vr::make_view;

// ---------------------------------------------------------------- environment knobs
// Each is read once per process (a function-local static): none is on the per-launch path.
// A flag that defaults on is turned off by "0...", one that defaults off is turned on by "1...".
bool env_flag(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}
// An integer in lo..hi, or dflt when unset or out of range.
uint32_t env_uint(const char* name, long lo, long hi, uint32_t dflt) {
    const char* e = std::getenv(name);
    const long v = e ? std::strtol(e, nullptr, 10) : lo - 1;
    return v >= lo && v <= hi ? (uint32_t)v : dflt;
}
// VR_ORDER_REFRESH=N (experiments): remake the learned orders every N uses of a slot.
uint32_t order_refresh() { static const uint32_t r = env_uint("VR_ORDER_REFRESH", 1, LONG_MAX, 0); return r; }
// VR_ORDER=0 / VR_LANE_ORDER=0 (A/B runs): no work order / 8x8 tiles, no per-pixel lane order.
bool order_enabled() { static const bool on = env_flag("VR_ORDER", true); return on; }
bool lane_order_enabled() { static const bool on = env_flag("VR_LANE_ORDER", true); return on; }
// VR_CRAWL_SKIP=0 (A/B runs): every launch runs its crawl pass.
bool crawl_skip_enabled() { static const bool on = env_flag("VR_CRAWL_SKIP", true); return on; }
// The launch policy's knobs (vr_launch_plan.h launch_policy), A/B runs:
//  VR_INFLIGHT_HEAVY=1       AUTO dispatches heaviest first with frames in flight too
//  VR_INFLIGHT_WAVES=0       frames in flight keep the lone-frame occupancy
//  VR_CRAWL_RPW=1..64        crawl records per wave for every launch, instead of
//  VR_CRAWL_RPW_IN_FLIGHT=1..64  (default 32) with frames in flight and 2 for a lone frame
const vr::PolicyKnobs& policy_knobs() {
    static const vr::PolicyKnobs k = {env_flag("VR_INFLIGHT_HEAVY", false), env_flag("VR_INFLIGHT_WAVES", true),
                                      env_uint("VR_CRAWL_RPW", 1, 64, 0), env_uint("VR_CRAWL_RPW_IN_FLIGHT", 1, 64, 32)};
    return k;
}

// Per-device ring of device scratch slots that a launch borrows: the deferral
// list of the crawl pass (vr::kDeferWords uint32, zeroed once; the crawl pass
// resets it at its end).  A slot belongs to ONE launch at a time: the launch
// that takes it waits (on its own stream, hipStreamWaitEvent) for the event
// the slot's previous launch recorded after its last kernel, and records the
// slot's event again after its own.  The device's lock is held from taking the
// slot to recording the event, so two launches in flight -- on any streams,
// from any threads -- never share a slot however many slots there are (a wait
// on an event of the same stream or one that has completed costs nothing).
// Launches on different devices take different locks.
struct SlotRing {
    const size_t words = vr::kDeferWords;   // uint32 per slot
    const uint32_t nslots = 16;
    // what a slot has learned about the view it last rendered (vr_launch_plan.h)
    struct Slot {
        vr::WorkOrder work;
        vr::LaneOrder lane;
        vr::CrawlSkip skip;
    };
    struct Dev {
        std::mutex mu;
        uint32_t* base = nullptr;
        std::vector<hipEvent_t> ev;
        std::vector<bool> used;
        uint32_t next = 0;
        // host-mapped: [0] the last crawl pass's record count (any slot); then per slot the
        // {launch id, record count} its last crawl pass reported (two words, 8-B aligned)
        uint32_t* stat_host = nullptr;
        uint32_t* stat_dev = nullptr;
        uint32_t launch_serial = 0;
        std::vector<Slot> slot;
        bool any = false;                  // the device's previous launch: its stream and slot
        hipStream_t last_stream = nullptr;
        uint32_t last_idx = 0;
        uint64_t last_key = 0;             // the view of the device's previous launch
        bool force_skip = false;           // vr_debug_skip_next_crawl (tests)
        bool force_in_flight = false;      // vr_debug_force_in_flight (tests): launches plan as not alone
        // vr_debug_last_launch (tests): the plan of the device's latest render launch -- alone,
        // heavy, hi, crawl_rpw, the crawl pass's grid, whether the crawl pass ran
        uint32_t last_plan[6] = {0, 0, 0, 0, 0, 0};
        // vr_debug_order_uses (tests): render launches, lane orders made, launches with a lane
        // order bound, work orders made, launches with a work order bound, crawl passes skipped
        uint64_t uses[6] = {0, 0, 0, 0, 0, 0};
        // vr_debug_capture_lane_order (tests): the next lane order made on the device is kept
        // here with the walk lengths it was made from, for vr_debug_lane_order; with it the
        // waves' costs perm_kernel wrote and the work order that launch made from them, for
        // vr_debug_work_order (empty when the launch made no work order from those costs)
        bool capture_lane = false;
        struct LaneCapture {
            uint32_t LW = 0, rows = 0, gx = 0, gy = 0;
            std::vector<uint32_t> pcost;
            std::vector<uint8_t> perm;
            std::vector<uint32_t> cost, order;
        } lane_capture;
        // No other stream's launch is running on the device.  (The lock orders launches:
        // "previous" is well defined.  The event is queried only when there is a previous
        // launch and it was on another stream: this is on the enqueue path.)
        bool alone(hipStream_t st) const {
            return !any || last_stream == st || hipEventQuery(ev[last_idx]) == hipSuccess;
        }
        // This launch becomes the device's previous one; returns whether its view repeats.
        bool follow(hipStream_t st, uint32_t idx, uint64_t key) {
            const bool repeat = last_key == key;
            any = true;
            last_stream = st;
            last_idx = idx;
            last_key = key;
            return repeat;
        }
    } dev[64];
} g_defer_ring;

// First use of a device: the slots and their events.  On a
// failure everything made so far is released and the next launch tries again.
int ring_init(SlotRing& r, SlotRing::Dev& D) {
    void* q = nullptr;
    const size_t bytes = (size_t)r.nslots * r.words * sizeof(uint32_t);
    std::vector<hipEvent_t> made;
    auto undo = [&](hipError_t e, const char* what) {
        for (hipEvent_t x : made) (void)hipEventDestroy(x);
        if (q) (void)hipFree(q);
        return hip_fail(e, what);
    };
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { q = nullptr; return undo(e, "hipMalloc(slot ring)"); }
    e = hipMemset(q, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return undo(e, "hipMemset(slot ring)");
    std::vector<hipEvent_t> ev(r.nslots);
    for (uint32_t i = 0; i < r.nslots; ++i) {
        e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e != hipSuccess) return undo(e, "hipEventCreate(slot ring)");
        made.push_back(ev[i]);
    }
    void* h = nullptr;
    void* hd = nullptr;
    const size_t stat_words = 2u + 2u * (size_t)r.nslots;
    e = hipHostMalloc(&h, sizeof(uint32_t) * stat_words, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {
        for (size_t i = 0; i < stat_words; ++i) ((volatile uint32_t*)h)[i] = 0u;
        e = hipHostGetDevicePointer(&hd, h, 0);
        if (e != hipSuccess) (void)hipHostFree(h);
    }
    if (e != hipSuccess) return undo(e, "hipHostMalloc(crawl statistics)");
    D.ev = std::move(ev);
    D.used.assign(r.nslots, false);
    D.slot.assign(r.nslots, SlotRing::Slot{});
    D.stat_host = (uint32_t*)h;
    D.stat_dev = (uint32_t*)hd;
    D.base = (uint32_t*)q;
    return VR_OK;
}

// The borrowed slot; the device's lock is held until release() (or destruction).
struct SlotLease {
    SlotRing* ring = nullptr;
    std::unique_lock<std::mutex> lk;
    int dev = -1;
    uint32_t idx = 0;
    uint32_t* p = nullptr;
    int acquire(SlotRing& r, int d, hipStream_t stream) {
        if (d < 0 || d >= 64) return fail(VR_E_INVALID, "device index too large");
        SlotRing::Dev& D = r.dev[d];
        lk = std::unique_lock<std::mutex>(D.mu);
        if (!D.base) {
            int rc = ring_init(r, D);
            if (rc) return rc;
        }
        ring = &r;
        dev = d;
        idx = D.next;
        D.next = (D.next + 1u) % r.nslots;
        if (D.used[idx]) {
            hipError_t e = hipStreamWaitEvent(stream, D.ev[idx], 0);
            if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent(slot ring)");
        }
        p = D.base + r.words * idx;
        return VR_OK;
    }
    SlotRing::Dev& D() const { return ring->dev[dev]; }
    // after the launch's last kernel on `stream`
    int release(hipStream_t stream) {
        hipError_t e = hipEventRecord(D().ev[idx], stream);
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord(slot ring)");
        D().used[idx] = true;
        lk.unlock();
        return VR_OK;
    }
};

// The view a launch renders, for the learned orders and the crawl-pass skip: an FNV-1a hash
// of the scene (its per-process serial and its revision, which every vr_scene_edit that
// changes it bumps: an edit changes which pixels defer), the algorithm and every value field of the view --
// the KView prefix above `out`: camera (llc, hor, ver, org), lights (L, LC, LP and the
// host-made Lr, L_fast, Lw, L_order, L_cls, L_unit, L_eq), transform (translation, scale_f),
// use_point_light, use_shadows, frame size (W, H), the launch's rows (row0, band_rows, rank,
// nranks, local_rows, row_limit, band_minv) and its tile deal (LW, tile_cols, tile_minv,
// col_R, col_rank, col_stride).  make_view zeroes the struct, so its padding is 0.  These,
// with the compile-time tile budget (vr::kTileBudget), are every input of which pixels the
// tile pass defers (vr_internal.h KView: a field added after `out` fails a static_assert
// until reviewed).  The per-launch buffers (out and after) are not part of it.
uint64_t view_key(const vr_scene* s, vr_algo algo, const vr::KView& v) {
    const uint32_t a = (uint32_t)algo;
    uint64_t h = vr::fnv1a(vr::kFnvBasis, &s->serial, sizeof s->serial);
    h = vr::fnv1a(h, &s->revision, sizeof s->revision);
    h = vr::fnv1a(h, &a, sizeof a);
    return vr::fnv1a(h, &v, offsetof(vr::KView, out));
}

// The crawl-pass skip's key: the view, plus the per-launch knobs that change how the crawl
// pass resumes deferred pixels (the list's capacity, walk-from-the-start records).  Which
// pixels defer is a function of the view alone: the tile pass's budget is compile-time
// (vr::kTileBudget) and everything else it reads is in the view (vr_internal.h KView).
uint64_t crawl_key(uint64_t key, const vr::KView& v) {
    const uint32_t knobs[2] = {v.defer_cap, v.crawl_rewalk};
    return vr::fnv1a(key, knobs, sizeof knobs);
}

// Buffers of a slot's order that a larger grid outgrew, freed and allocated again with
// `bytes` each.  Stream-ordered: the slot's previous launch -- the last user of the old
// buffers -- is fenced on this stream (SlotLease::acquire), so freeing them on it needs no
// host synchronisation.  Every path frees what it allocated: on an error all are null.
struct Regrow {
    void** p;
    size_t bytes;
};
hipError_t regrow(std::initializer_list<Regrow> bufs, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (const Regrow& b : bufs) {
        const hipError_t e2 = *b.p ? hipFreeAsync(*b.p, st) : hipSuccess;
        if (e == hipSuccess) e = e2;
        *b.p = nullptr;
    }
    for (const Regrow& b : bufs)
        if (e == hipSuccess) e = hipMallocAsync(b.p, b.bytes, st);
    if (e != hipSuccess)
        for (const Regrow& b : bufs) {
            if (*b.p) (void)hipFreeAsync(*b.p, st);
            *b.p = nullptr;
        }
    return e;
}

// The work order: this slot's order if it was made for this view (v.order), made (v.cost:
// from this launch's costs, after its passes; `remake`) when missing and the view repeats.
// It only permutes the tile groups: any order renders the same pixels.
hipError_t bind_work_order(vr::WorkOrder& W, uint32_t gx, uint32_t gy, uint64_t key, bool repeat, hipStream_t st,
                           vr::KView& v, bool& remake) {
    const uint32_t n = gx * gy;
    if (n > W.cap) {
        W.cap = 0;               // (the work order's fields only: the lane order's are its own)
        W.valid = false;
        const hipError_t e = regrow({{(void**)&W.cost, sizeof(uint32_t) * vr::kWavesPerTileGroup * (size_t)n},
                                     {(void**)&W.order, sizeof(uint32_t) * (size_t)n}}, st);
        if (e != hipSuccess) return e;
        W.cap = n;
    }
    const bool match = W.matches(gx, gy, key);
    v.order = match ? W.order : nullptr;
    // (a work order made from costs walked under another lane order is remade: the lane
    // order moves the heavy pixels of a block into one of its two tile groups)
    remake = vr::remake_due(match, W.relaned, repeat, W.age, order_refresh());
    v.cost = remake ? W.cost : nullptr;
    return hipSuccess;
}

// The lane order, kept like the work order but for every schedule: this slot's if it was
// made for this view (v.perm), made from this launch's per-pixel walk lengths (v.pcost;
// `relane`) when missing and the view repeats.  It permutes pixels within lane blocks (16x32)
// only: any permutation renders the same pixels.  On an error `what` names the step.
hipError_t bind_lane_order(vr::LaneOrder& L, uint32_t gx, uint32_t gy, uint64_t key, bool repeat, hipStream_t st,
                           vr::KView& v, bool& relane, const char*& what) {
    const size_t nperm = vr::perm_bytes(gx, gy);
    if (nperm > L.bcap) {
        L.bcap = 0;
        L.valid = false;
        what = "lane order buffer";
        const hipError_t e = regrow({{(void**)&L.perm, nperm}}, st);
        if (e != hipSuccess) return e;
        L.bcap = nperm;
    }
    const bool match = L.matches(gx, gy, key);
    v.perm = match ? L.perm : nullptr;
    relane = vr::remake_due(match, false, repeat, L.age, order_refresh());
    if (!relane) return hipSuccess;
    // 4 B per pixel, only between this launch's tile pass and its perm_kernel (freed
    // stream-ordered after it): the slots keep 2 B per pixel each, not 6
    what = "lane order walk lengths";
    return hipMallocAsync((void**)&v.pcost, sizeof(uint32_t) * (size_t)v.LW * v.local_rows, st);
}

// VR_HOST_PROF (measurement builds only, profiles/build_variant.sh -- -DVR_HOST_PROF): host
// clock stamps at the stages of each launch, fetched with vr_host_prof_fetch.
#ifdef VR_HOST_PROF
}  // namespace
static uint64_t g_hp[4096][8];
static uint32_t g_hp_n = 0;
static inline uint64_t hp_now() { return (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count(); }
extern "C" int vr_host_prof_fetch(uint64_t* out, int n) {
    const uint32_t k = g_hp_n < 4096u ? g_hp_n : 4096u;
    const uint32_t m = (uint32_t)n < k ? (uint32_t)n : k;
    for (uint32_t i = 0; i < m; ++i)
        for (int j = 0; j < 8; ++j) out[8 * i + j] = g_hp[(g_hp_n - m + i) % 4096u][j];
    return (int)m;
}
namespace {
#define VR_HP(i) hp_row[i] = hp_now()
#else
#define VR_HP(i) do { } while (0)
#endif

// One render: validate, lease a slot, plan (vr_launch_plan.h), bind the slot's buffers into
// the view, the passes, the lane order and the work order learned from them, release.
int launch(const vr_scene* s, vr_algo algo, uint32_t kernel, uint32_t schedule, uint32_t occupancy, vr::KView& v,
           void* stream) {
#ifdef VR_HOST_PROF
    uint64_t* hp_row = g_hp[g_hp_n++ % 4096u];
    for (int j = 0; j < 8; ++j) hp_row[j] = 0;
#endif
    VR_HP(0);
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS) return fail(VR_E_INVALID, "unknown algorithm");
    if (kernel != VR_KERNEL_AUTO && kernel != VR_KERNEL_TILE && kernel != VR_KERNEL_TILE_REWALK)
        return fail(VR_E_INVALID, "unknown kernel (2, the persistent kernel, was retired)");
    if (occupancy > VR_OCCUPANCY_IN_FLIGHT) return fail(VR_E_INVALID, "unknown occupancy");
    if (v.local_rows == 0 || v.LW == 0) return VR_OK;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    // A launch is not capturable into a graph: the slot ring's event wait/record and the
    // work order's host-side bookkeeping would be baked into it and not replay (no test
    // captures one), so capture is refused before anything is enqueued.
    int rc = vr::refuse_capture(st, "vr_render*");
    if (rc) return rc;
    // the deferral list of the crawl pass (cluster-skip crawls, walks over the tile budget)
    SlotLease lease;
    rc = lease.acquire(g_defer_ring, s->device, st);
    if (rc) return rc;
    VR_HP(1);
    // An error after the slot was taken: the slot's event is recorded again on `st` first (a
    // stream-ordered free of its old buffers may already be queued there), then the error.
    auto bail = [&](hipError_t err, const char* what) {
        (void)lease.release(st);
        return hip_fail(err, what);
    };
    SlotRing::Dev& D = lease.D();
    SlotRing::Slot& S = D.slot[lease.idx];
    v.crawl_rewalk = kernel == VR_KERNEL_TILE_REWALK ? 1u : 0u;
    v.defer = lease.p;
    v.defer_cap = (v.defer_cap && v.defer_cap < vr::kDeferCap) ? v.defer_cap : vr::kDeferCap;
    v.defer_stat = D.stat_dev;
    v.slot_stat = D.stat_dev + 2 + 2 * (size_t)lease.idx;
    const uint32_t expect = *(volatile uint32_t*)D.stat_host;   // an earlier launch's count (a hint)
    uint32_t gx = 0, gy = 0;
    vr::march_grid(v, gx, gy);
    const uint32_t n = gx * gy;
    const bool alone = D.alone(st) && !D.force_in_flight;
    VR_HP(2);
    const vr::LaunchPolicy pol = vr::launch_policy(schedule, occupancy, alone, policy_knobs());
    v.crawl_rpw = pol.crawl_rpw;
    const uint64_t key = view_key(s, algo, v);
    const bool repeat = D.follow(st, lease.idx, key);
    VR_HP(3);
    bool remake = false, relane = false;
    hipError_t e = hipSuccess;
    if (pol.heavy && order_enabled() && n != 0) {
        e = bind_work_order(S.work, gx, gy, key, repeat, st, v, remake);
        if (e != hipSuccess) return bail(e, "work order buffers");
    }
    if (lane_order_enabled() && n != 0) {
        const char* what = "";
        e = bind_lane_order(S.lane, gx, gy, key, repeat, st, v, relane, what);
        if (e != hipSuccess) return bail(e, what);
    }
    VR_HP(4);
    v.launch_id = vr::next_launch_id(D.launch_serial);
    const uint64_t report = *reinterpret_cast<volatile uint64_t*>(D.stat_host + 2 + 2 * (size_t)lease.idx);
    const bool crawl = S.skip.step(crawl_key(key, v), report, v.launch_id, D.force_skip, crawl_skip_enabled());
    VR_HP(5);
    // crawl pass grid from the records an earlier launch deferred (a hint: any grid renders
    // the same pixels)
    const vr::KScene ks = vr::kscene(s);
    const uint32_t cwgs = vr::crawl_grid(expect, v.crawl_rpw);
    D.uses[0] += 1u;
    D.uses[2] += v.perm != nullptr;
    D.uses[4] += v.order != nullptr;
    D.uses[5] += !crawl;
    const uint32_t plan[6] = {alone, pol.heavy, pol.hi, v.crawl_rpw, cwgs, crawl};
    std::memcpy(D.last_plan, plan, sizeof plan);
    VR_HP(6);
    e = vr::launch_march((int)s->store, (int)algo, v.bytes != nullptr, ks, v, st, cwgs, pol.hi, crawl);
    VR_HP(7);
    // The lane order first: when the slot has work-order buffers for this grid, perm_kernel
    // also writes the waves' costs under the new lane order and the work order is remade from
    // them at once -- an order made from costs walked under another lane order puts the light
    // half of a block first as often as the heavy one (C2 lone launch 0.125 -> 0.185 ms with
    // it, 0.116 without, profiles/r05/lane_order/).
    bool with_costs = false;
    if (e == hipSuccess && relane) {
        with_costs = order_enabled() && S.work.cost && S.work.cap >= n;
        e = vr::launch_perm(v.pcost, v.LW, v.local_rows, gx, gy, S.lane.perm, with_costs ? S.work.cost : nullptr, st);
        S.lane.learned(gx, gy, key, e == hipSuccess);
        D.uses[1] += e == hipSuccess;
        S.work.relaned = !with_costs;
    }
    const bool capture = e == hipSuccess && relane && D.capture_lane;
    if (e == hipSuccess && (remake || with_costs)) {
        // (on a side stream instead -- one more stream than the box's 4 hardware queues
        // serialised the two render streams: C2 0.1124 -> 0.1277 ms per frame in flight,
        // profiles/r03/ab_order_C2_C3.txt)
        e = vr::launch_order(S.work.cost, n, gx, S.work.order, st);
        S.work.learned(gx, gy, key, e == hipSuccess);
        D.uses[3] += e == hipSuccess;
    }
    if (capture && e == hipSuccess) {     // (tests only: waits for the stream)
        D.capture_lane = false;
        SlotRing::Dev::LaneCapture& C = D.lane_capture;
        C.LW = v.LW, C.rows = v.local_rows, C.gx = gx, C.gy = gy;
        C.pcost.resize((size_t)v.LW * v.local_rows);
        C.perm.resize(vr::perm_bytes(gx, gy));
        // (the work order only when this launch made it from perm_kernel's costs)
        C.cost.resize(with_costs ? (size_t)vr::kWavesPerTileGroup * n : 0);
        C.order.resize(with_costs ? (size_t)n : 0);
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(C.pcost.data(), v.pcost, sizeof(uint32_t) * C.pcost.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(C.perm.data(), S.lane.perm, C.perm.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess && with_costs) e = hipMemcpy(C.cost.data(), S.work.cost, sizeof(uint32_t) * C.cost.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess && with_costs) e = hipMemcpy(C.order.data(), S.work.order, sizeof(uint32_t) * C.order.size(), hipMemcpyDeviceToHost);
    }
    if (v.pcost) {      // (a relaning launch's per-pixel walk lengths: transient)
        const hipError_t ef = hipFreeAsync(v.pcost, st);
        if (e == hipSuccess) e = ef;
    }
    // (on a failed launch the slot is still fenced: a kernel of it may be queued)
    rc = lease.release(st);
    if (e != hipSuccess) return hip_fail(e, "ray-march launch");
    return rc;
}

}  // namespace

extern "C" {

int vr_render_ex(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                 const float translation[3], uint32_t scale, uint32_t width, uint32_t height,
                 const vr_render_opts* opts, uint32_t* out_dev, void* stream) {
    if (!opts) return fail(VR_E_INVALID, "opts is NULL");
    // Versioned struct (vr.h): a caller built before struct_size existed passes `kernel`
    // (0..3) in the first word and is refused; fields past the caller's struct read as 0.
    // (checked first: only the caller's own struct_size bytes are ever read)
    if (opts->struct_size < VR_RENDER_OPTS_MIN_SIZE)
        return fail(VR_E_INVALID, "vr_render_opts.struct_size is " + std::to_string(opts->struct_size) +
                                      ": set it to sizeof(vr_render_opts) (vr_render_opts_init); a struct built "
                                      "against the layout without struct_size is not accepted");
    vr_render_opts o{};
    std::memcpy(&o, opts, std::min<size_t>(opts->struct_size, sizeof o));
    if (o.reserved != 0u) return fail(VR_E_INVALID, "vr_render_opts.reserved must be 0");
    vr::KView v;
    int rc = make_view(s, cam, lit, translation, scale, width, height, v);
    if (rc) return rc;
    if (!out_dev) return fail(VR_E_INVALID, "out_dev is NULL");
    const uint32_t row_end = o.row_end == 0xFFFFFFFFu ? height : o.row_end;
    if (o.row_begin > row_end || row_end > height) return fail(VR_E_INVALID, "bad row range");
    if (!o.nranks || o.rank >= o.nranks) return fail(VR_E_INVALID, "bad band partition");
    if (o.reserved2 != 0u) return fail(VR_E_INVALID, "vr_render_opts.reserved2 must be 0");
    const uint32_t rows = row_end - o.row_begin;
    const uint32_t band = o.band_rows ? o.band_rows : std::max(1u, rows);
    v.row0 = o.row_begin;
    v.row_limit = row_end;
    v.band_rows = band;
    v.band_minv = band == 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / band);
    if (o.tile_cols == 0u) {
        v.rank = o.rank;
        v.nranks = o.nranks;
        v.local_rows = (uint32_t)(vr_band_buffer_words(width, rows, band, o.nranks) / width);
    } else {
        // 2-D tile deal: every band is this rank's; its columns are dealt (KView)
        if (o.tile_cols > width) return fail(VR_E_INVALID, "tile_cols larger than the frame width");
        v.rank = 0;
        v.nranks = 1;
        v.local_rows = (uint32_t)(((uint64_t)rows + band - 1) / band * band);
        const uint32_t nblk = (width + o.tile_cols - 1) / o.tile_cols;
        v.LW = (nblk + o.nranks - 1) / o.nranks * o.tile_cols;
        v.tile_cols = o.tile_cols;
        v.tile_minv = o.tile_cols == 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / o.tile_cols);
        v.col_R = o.nranks;
        v.col_rank = o.rank;
        v.col_stride = (o.deal_stride ? o.deal_stride : vr_deal_stride_default(o.nranks)) % o.nranks;
        if (v.local_rows > 65535u || v.LW > 65535u) return fail(VR_E_INVALID, "tile buffer too large");
    }
    v.out = out_dev;
    v.bytes = (unsigned long long*)o.bytes_dev;
    v.stats = o.bytes_dev ? (unsigned long long*)o.stats_dev : nullptr;
    v.defer_cap = o.defer_cap;
    if (o.schedule > VR_SCHEDULE_HEAVIEST_FIRST) return fail(VR_E_INVALID, "unknown schedule");
    return launch(s, algo, o.kernel, o.schedule, o.occupancy, v, stream);
}

int vr_render_opts_init(vr_render_opts* opts) {
    if (!opts) return fail(VR_E_INVALID, "NULL argument");
    *opts = vr_render_opts{};
    opts->struct_size = (uint32_t)sizeof(vr_render_opts);
    opts->kernel = VR_KERNEL_AUTO;
    opts->row_begin = 0;
    opts->row_end = 0xFFFFFFFFu;
    opts->band_rows = 0;
    opts->rank = 0;
    opts->nranks = 1;
    opts->schedule = VR_SCHEDULE_AUTO;
    return VR_OK;
}

namespace {
vr_render_opts opts_rows(uint32_t row_begin, uint32_t row_end) {
    vr_render_opts o;
    vr_render_opts_init(&o);
    o.row_begin = row_begin;
    o.row_end = row_end;
    return o;
}
}  // namespace

int vr_render(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit, const float translation[3],
              uint32_t scale, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t* out_dev,
              void* stream) {
    const vr_render_opts o = opts_rows(row_begin, row_end);
    return vr_render_ex(s, algo, cam, lit, translation, scale, width, height, &o, out_dev, stream);
}

uint64_t vr_band_buffer_words(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t nranks) {
    if (!band_rows || !nranks) return 0;
    uint64_t nb = (height + (uint64_t)band_rows - 1) / band_rows;
    uint64_t per = (nb + nranks - 1) / nranks;
    return per * band_rows * (uint64_t)width;
}

uint32_t vr_deal_stride_default(uint32_t nranks) {
    return (nranks % 3u == 0u) ? 1u : 3u;
}

int vr_forget_orders(int device) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    for (SlotRing::Slot& S : D.slot) {
        S.work.forget();
        S.lane.forget();
        S.skip.forget();
    }
    D.last_key = 0;
    return VR_OK;
}

int vr_debug_skip_next_crawl(int device) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    D.force_skip = true;
    return VR_OK;
}

int vr_debug_order_uses(int device, uint64_t out[8]) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    if (!out) return fail(VR_E_INVALID, "out is NULL");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    const vr::LaneShape sh = vr::lane_shape();
    std::lock_guard<std::mutex> lk(D.mu);
    for (int i = 0; i < 6; ++i) out[i] = D.uses[i];
    out[6] = g_defer_ring.nslots;
    out[7] = (uint64_t)sh.block_x << 16 | sh.block_y;
    return VR_OK;
}

int vr_debug_force_in_flight(int device, int on) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    D.force_in_flight = on != 0;
    return VR_OK;
}

int vr_debug_last_launch(int device, uint64_t out[8]) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    if (!out) return fail(VR_E_INVALID, "out is NULL");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    for (int i = 0; i < 6; ++i) out[i] = D.last_plan[i];
    // (host-mapped: written by the device's last completed crawl pass; none before the ring exists)
    out[6] = D.stat_host ? *(volatile uint32_t*)D.stat_host : 0u;
    out[7] = 0;
    return VR_OK;
}

int vr_debug_capture_lane_order(int device) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    D.capture_lane = true;
    D.lane_capture = {};
    return VR_OK;
}

int vr_debug_lane_order(int device, uint32_t info[8], uint32_t* pcost, uint64_t pcost_words, uint8_t* perm,
                        uint64_t perm_bytes) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    if (!info) return fail(VR_E_INVALID, "info is NULL");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    const SlotRing::Dev::LaneCapture& C = D.lane_capture;
    if (C.perm.empty()) return fail(VR_E_INVALID, "no lane order captured (vr_debug_capture_lane_order, then a repeated view)");
    const vr::LaneShape sh = vr::lane_shape();
    const uint32_t words[8] = {C.LW, C.rows, C.gx, C.gy, sh.block_x, sh.block_y, sh.entry_bytes, sh.seat};
    std::memcpy(info, words, sizeof words);
    if (pcost) {
        if (pcost_words != C.pcost.size()) return fail(VR_E_INVALID, "pcost_words is not info[0] * info[1]");
        std::memcpy(pcost, C.pcost.data(), sizeof(uint32_t) * C.pcost.size());
    }
    if (perm) {
        if (perm_bytes != C.perm.size()) return fail(VR_E_INVALID, "perm_bytes is not the captured order's size");
        std::memcpy(perm, C.perm.data(), C.perm.size());
    }
    return VR_OK;
}

int vr_debug_work_order(int device, uint32_t* cost, uint64_t cost_words, uint32_t* order, uint64_t order_words) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    SlotRing::Dev& D = g_defer_ring.dev[device];
    std::lock_guard<std::mutex> lk(D.mu);
    const SlotRing::Dev::LaneCapture& C = D.lane_capture;
    if (C.order.empty())
        return fail(VR_E_INVALID, "no work order captured (vr_debug_capture_lane_order, then a repeated view whose "
                                  "launch makes its work order from the lane order's costs)");
    if (cost) {
        if (cost_words != C.cost.size()) return fail(VR_E_INVALID, "cost_words is not 2 * info[2] * info[3]");
        std::memcpy(cost, C.cost.data(), sizeof(uint32_t) * C.cost.size());
    }
    if (order) {
        if (order_words != C.order.size()) return fail(VR_E_INVALID, "order_words is not info[2] * info[3]");
        std::memcpy(order, C.order.data(), sizeof(uint32_t) * C.order.size());
    }
    return VR_OK;
}

namespace {
// A scratch device buffer of a test hook, freed when it returns.  An output (fill) is followed
// by kGuardBytes more and all of it is filled with 0xFF bytes before the kernel runs: fetch
// copies the output back and reports whether the guard behind it is still as filled (a kernel
// that wrote past its output is caught inside memory the hook owns).
struct Scratch {
    static constexpr size_t kGuardBytes = 256;
    void* p = nullptr;
    size_t bytes = 0;
    ~Scratch() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { bytes = n; return hipMalloc(&p, n + kGuardBytes); }
    hipError_t fill() { return hipMemset(p, 0xFF, bytes + kGuardBytes); }
    hipError_t fetch(void* host, bool& guard_ok) {
        unsigned char g[kGuardBytes];
        hipError_t e = hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(g, (const char*)p + bytes, kGuardBytes, hipMemcpyDeviceToHost);
        for (size_t i = 0; e == hipSuccess && i < kGuardBytes; ++i) guard_ok = guard_ok && g[i] == 0xFFu;
        return e;
    }
};
}  // namespace

int vr_debug_lane_order_from(int device, const uint32_t* pcost_host, uint32_t LW, uint32_t rows, uint32_t info[8],
                             uint8_t* perm, uint64_t perm_bytes, uint32_t* cost, uint64_t cost_words) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    if (!info) return fail(VR_E_INVALID, "info is NULL");
    if (LW == 0 || rows == 0 || LW > 65536 || rows > 65536) return fail(VR_E_INVALID, "bad frame size");
    vr::KView v{};
    v.LW = LW;
    v.local_rows = rows;
    uint32_t gx = 0, gy = 0;
    vr::march_grid(v, gx, gy);
    const vr::LaneShape sh = vr::lane_shape();
    const uint32_t words[8] = {LW, rows, gx, gy, sh.block_x, sh.block_y, sh.entry_bytes, sh.seat};
    std::memcpy(info, words, sizeof words);
    if (!pcost_host && !perm && !cost) return VR_OK;       // (the sizes only)
    if (!pcost_host || !perm || !cost) return fail(VR_E_INVALID, "pcost_host, perm or cost is NULL");
    const size_t nperm = vr::perm_bytes(gx, gy), ncost = (size_t)vr::kWavesPerTileGroup * gx * gy;
    if (perm_bytes != nperm) return fail(VR_E_INVALID, "perm_bytes is not the order's size");
    if (cost_words != ncost) return fail(VR_E_INVALID, "cost_words is not 2 * info[2] * info[3]");
    DeviceGuard dg(device);
    const size_t npc = sizeof(uint32_t) * (size_t)LW * rows;
    Scratch dp, dperm, dcost;
    hipError_t e = dp.alloc(npc);
    if (e == hipSuccess) e = dperm.alloc(nperm);
    if (e == hipSuccess) e = dcost.alloc(sizeof(uint32_t) * ncost);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(lane order scratch)");
    e = hipMemcpy(dp.p, pcost_host, npc, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dperm.fill();
    if (e == hipSuccess) e = dcost.fill();
    if (e == hipSuccess)
        e = vr::launch_perm((const uint32_t*)dp.p, LW, rows, gx, gy, (uint8_t*)dperm.p, (uint32_t*)dcost.p, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    bool guard_ok = true;
    if (e == hipSuccess) e = dperm.fetch(perm, guard_ok);
    if (e == hipSuccess) e = dcost.fetch(cost, guard_ok);
    if (e != hipSuccess) return hip_fail(e, "vr_debug_lane_order_from");
    if (!guard_ok) return fail(VR_E_HIP, "vr_debug_lane_order_from: perm_kernel wrote past perm or cost (guard bytes changed)");
    return VR_OK;
}

int vr_debug_work_order_from(int device, const uint32_t* cost_host, uint32_t columns, uint32_t groups, uint32_t* order) {
    if (device < 0 || device >= 64) return fail(VR_E_INVALID, "device index out of range");
    if (!cost_host || !order) return fail(VR_E_INVALID, "cost_host or order is NULL");
    if (columns == 0 || columns > 4096 || groups == 0 || groups % columns != 0 || groups / columns > 8192)
        return fail(VR_E_INVALID, "bad grid (columns 1..4096, groups a multiple of columns, at most 8192 rows)");
    DeviceGuard dg(device);
    const size_t ncost = sizeof(uint32_t) * (size_t)vr::kWavesPerTileGroup * groups, nord = sizeof(uint32_t) * (size_t)groups;
    Scratch dcost, dord;
    hipError_t e = dcost.alloc(ncost);
    if (e == hipSuccess) e = dord.alloc(nord);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(work order scratch)");
    e = hipMemcpy(dcost.p, cost_host, ncost, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dord.fill();
    if (e == hipSuccess) e = vr::launch_order((const uint32_t*)dcost.p, groups, columns, (uint32_t*)dord.p, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    bool guard_ok = true;
    if (e == hipSuccess) e = dord.fetch(order, guard_ok);
    if (e != hipSuccess) return hip_fail(e, "vr_debug_work_order_from");
    if (!guard_ok) return fail(VR_E_HIP, "vr_debug_work_order_from: order_kernel wrote past order (guard bytes changed)");
    return VR_OK;
}

uint64_t vr_tile_buffer_words(uint32_t width, uint32_t height, uint32_t band_rows, uint32_t tile_cols, uint32_t nranks) {
    if (!nranks || !tile_cols || !width || !height) return 0;
    const uint64_t band = band_rows ? band_rows : height;
    const uint64_t rows = (height + band - 1) / band * band;
    const uint64_t nblk = ((uint64_t)width + tile_cols - 1) / tile_cols;
    return rows * ((nblk + nranks - 1) / nranks * tile_cols);
}

int vr_render_tiles(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height, uint32_t band_rows,
                    uint32_t tile_cols, uint32_t rank, uint32_t nranks, uint32_t* out_dev, void* stream) {
    if (!band_rows || !tile_cols) return fail(VR_E_INVALID, "band_rows and tile_cols must be > 0");
    vr_render_opts o = opts_rows(0, height);
    o.band_rows = band_rows;
    o.tile_cols = tile_cols;
    o.rank = rank;
    o.nranks = nranks;
    return vr_render_ex(s, algo, cam, lit, translation, scale, width, height, &o, out_dev, stream);
}

int vr_assemble_tiles(const void* parts_dev, void* frame_dev, uint32_t elem_bytes, uint32_t width, uint32_t height,
                      uint32_t band_rows, uint32_t tile_cols, uint32_t nranks, uint32_t deal_stride, void* stream) {
    if (!parts_dev || !frame_dev) return fail(VR_E_INVALID, "NULL device buffer");
    if (elem_bytes < 1u || elem_bytes > 4u) return fail(VR_E_INVALID, "elem_bytes must be 1..4");
    if (!width || !height || !band_rows || !tile_cols || !nranks || tile_cols > width)
        return fail(VR_E_INVALID, "bad tile layout");
    vr::TileLayout t{};
    t.W = width;
    t.H = height;
    t.band_rows = band_rows;
    t.tile_cols = tile_cols;
    t.R = nranks;
    t.stride = (deal_stride ? deal_stride : vr_deal_stride_default(nranks)) % nranks;
    t.LW = (uint32_t)(vr_tile_buffer_words(width, band_rows, band_rows, tile_cols, nranks) / band_rows);
    t.rank_words = vr_tile_buffer_words(width, height, band_rows, tile_cols, nranks);
    hipError_t e = vr::launch_assemble_tiles(parts_dev, frame_dev, elem_bytes, t, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "assemble_tiles launch");
    return VR_OK;
}

int vr_render_bands(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height, uint32_t band_rows,
                    uint32_t rank, uint32_t nranks, uint32_t* out_dev, void* stream) {
    if (!band_rows) return fail(VR_E_INVALID, "band_rows must be > 0");
    vr_render_opts o = opts_rows(0, height);
    o.band_rows = band_rows;
    o.rank = rank;
    o.nranks = nranks;
    return vr_render_ex(s, algo, cam, lit, translation, scale, width, height, &o, out_dev, stream);
}

int vr_render_count(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                    const float translation[3], uint32_t scale, uint32_t width, uint32_t height, uint32_t row_begin,
                    uint32_t row_end, uint32_t* out_dev, uint64_t* bytes_dev, void* stream) {
    if (!bytes_dev) return fail(VR_E_INVALID, "bytes_dev is NULL");
    vr_render_opts o = opts_rows(row_begin, row_end);
    o.bytes_dev = bytes_dev;
    return vr_render_ex(s, algo, cam, lit, translation, scale, width, height, &o, out_dev, stream);
}

int vr_pack_rgb8(const uint32_t* words_dev, uint8_t* rgb_dev, uint64_t n_pixels, void* stream) {
    if (n_pixels && (!words_dev || !rgb_dev)) return fail(VR_E_INVALID, "NULL device buffer");
    hipError_t e = vr::launch_pack_rgb8(words_dev, rgb_dev, n_pixels, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "pack_rgb8 launch");
    return VR_OK;
}

}  // extern "C"
