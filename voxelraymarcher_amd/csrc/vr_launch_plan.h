// vr_launch_plan.h -- the decisions of a launch (vr_launch.cpp launch) as pure functions
// of plain values: no HIP, no environment, no clock.  Knob values come in as arguments.
// tools/launch_plan_check.cpp checks them on a CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vr.h"

namespace vr {

// ---------------------------------------------------------------- launch policy
struct PolicyKnobs {
    bool inflight_heavy;        // VR_INFLIGHT_HEAVY
    bool in_flight_occupancy;   // VR_INFLIGHT_WAVES
    uint32_t rpw_override;      // VR_CRAWL_RPW (0 = none)
    uint32_t rpw_in_flight;     // VR_CRAWL_RPW_IN_FLIGHT
};
struct LaunchPolicy {
    bool heavy;           // the tile pass dispatches heaviest first (the work order is used / learned)
    bool hi;              // the tile pass's in-flight occupancy variant (vr_occupancy)
    uint32_t crawl_rpw;   // crawl records per wave
};
// The three choices that hang on `alone` (no other stream's launch is running on the
// device).  heavy: AUTO dispatches heaviest first for a lone frame.  hi: AUTO takes the
// in-flight occupancy variant while another stream's launch is running.  crawl_rpw: a lone
// frame ends with the crawl pass's longest chain (2 per wave since round 4's shorter chains:
// C5 alone 0.767 -> 0.759 ms vs 4, profiles/r04/crawl/scene_lds_ab.txt,
// rpw_multi_cluster.txt); with frames in flight the pass's issue cycles are what count (32
// per wave since round 6: fewer crawl waves for the other frames' tile passes to share the
// CUs with.  C5 per frame in flight is bimodal from run to run -- 0.541-0.543 ms in some
// processes, 0.561-0.567 in others -- and the fast mode showed up in 6 of 20 runs at 32 or
// more and in none of 22 at 8 or 16; never slower; profiles/r06/ab/ab_C5_crawl_rpw.txt).
inline LaunchPolicy launch_policy(uint32_t schedule, uint32_t occupancy, bool alone, const PolicyKnobs& k) {
    LaunchPolicy p;
    p.heavy = schedule == VR_SCHEDULE_HEAVIEST_FIRST || (schedule == VR_SCHEDULE_AUTO && (alone || k.inflight_heavy));
    p.hi = occupancy == VR_OCCUPANCY_IN_FLIGHT || (occupancy == VR_OCCUPANCY_AUTO && !alone && k.in_flight_occupancy);
    p.crawl_rpw = k.rpw_override ? k.rpw_override : (alone ? 2u : k.rpw_in_flight);
    return p;
}

// ---------------------------------------------------------------- learned orders
// Heaviest-first work order and lane order: made once per slot and view -- a
// view's walk lengths do not change (scenes are immutable), so they are not remade unless
// VR_ORDER_REFRESH=N (experiments; `refresh`, 0 = never) asks for a remake every N uses of
// a slot.  Orders are learned per view: one made for another view (e.g. the previous rank
// of a one-GPU rank emulation, or a moved camera) would deal the wrong pixels together.  A
// view whose previous launch on the device was the same view (`repeat`) gets its orders
// made (on each slot's first such launch); a view that changes every launch never does,
// and renders as a first render does.
inline bool refresh_due(uint32_t& age, uint32_t refresh) { return refresh != 0 && ++age >= refresh; }
// Whether a launch (re)makes an order: a matching one when it is stale or due for a
// refresh (age advances only then), a missing one when the view repeats.
inline bool remake_due(bool match, bool stale, bool repeat, uint32_t& age, uint32_t refresh) {
    return match ? (stale || refresh_due(age, refresh)) : repeat;
}

// What a slot's order was learned on: a grid of gx x gy and a view (view_key).
struct Learned {
    uint32_t gx = 0, gy = 0, age = 0;
    uint64_t key = 0;
    bool valid = false;
    bool matches(uint32_t x, uint32_t y, uint64_t k) const { return valid && gx == x && gy == y && key == k; }
    void learned(uint32_t x, uint32_t y, uint64_t k, bool ok) { valid = ok; gx = x; gy = y; key = k; age = 0; }
    void forget() { valid = false; }               // (buffers kept)
};
// Per slot: the tile pass's work order (heaviest tile groups first) made from the costs of
// the slot's last launch that recorded them.
struct WorkOrder : Learned {
    uint32_t* cost = nullptr;      // kWavesPerTileGroup words per tile group
    uint32_t* order = nullptr;     // one word per tile group
    uint32_t cap = 0;
    bool relaned = false;          // the lane order changed after the work order's costs
    void learned(uint32_t x, uint32_t y, uint64_t k, bool ok) { Learned::learned(x, y, k, ok); relaned = false; }
    void forget() { valid = relaned = false; }
};
// Per slot: the lane order (vr_march.hip lane_pixel, vr_order.hip perm_kernel): per lane block (16x32 pixels) its pixels heaviest first.
struct LaneOrder : Learned {
    uint8_t* perm = nullptr;       // vr::perm_bytes(gx, gy)
    size_t bcap = 0;
};

// ---------------------------------------------------------------- crawl-pass skip
// Launch ids are nonzero (0 = "no crawl pass yet" in CrawlSkip::cid and the report words).
inline uint32_t next_launch_id(uint32_t& serial) { return ++serial ? serial : ++serial; }

// The crawl pass is skipped for a view this slot has seen defer nothing: whether a walk
// is deferred is a pure function of its ray, so a view defers the same pixels on every
// launch.  Every record carries its launch's id and a crawl pass shades only its own,
// so even a wrong skip cannot put another frame's pixels into a frame; the records it
// leaves raise the count the next crawl pass of the slot reports, which ends the skipping.
// (C2 lone launch: the 4-us empty crawl pass and a kernel boundary.)
//   The safety net: every tile pass that defers a pixel writes {launch id, 1}
// into the slot's report word (vr_walk.h deferral_report), skipped launches included.
// While the slot skips, nothing else writes that word (its last crawl pass left
// {id, 0}), so a nonzero count there means a skipped launch deferred: the skipping ends,
// and the slot's next launch runs the crawl pass, which drops the stale records (they
// carry another launch's id) and resets the list.  What the net cannot repair is the
// frames of the skipped launches that deferred before the host saw the report (their
// deferred pixels stay 0): that needs a deferral that is not a function of the crawl key,
// which the kernels do not have (vr_internal.h KView, "end of the view's identity");
// tests/test_gpu_slots.py forces one (vr_debug_skip_next_crawl) to test the net.
struct CrawlSkip {
    // the slot's last launch that ran a crawl pass (id, crawl key), and whether a completed
    // one reported that this view defers nothing
    uint32_t cid = 0;
    uint64_t ckey = 0;
    bool czero = false;
    // One launch of the slot: `report` is the slot's report word {low: launch id, high:
    // records deferred}, `lid` this launch's id, `force` vr_debug_skip_next_crawl's flag
    // (consumed), `enabled` VR_CRAWL_SKIP.  Returns whether the crawl pass runs.
    bool step(uint64_t key, uint64_t report, uint32_t lid, bool& force, bool enabled) {
        const uint32_t rid = (uint32_t)report, count = (uint32_t)(report >> 32);
        if (ckey != key) {
            czero = false;
        } else if (czero) {
            if (count != 0u) czero = false;   // a skipped launch deferred
        } else if (cid != 0u) {
            czero = rid == cid && count == 0u;
        }
        if (force) {
            force = false;
            czero = true;
            ckey = key;
        }
        const bool crawl = !(czero && enabled);
        if (crawl) {
            cid = lid;
            ckey = key;
        }
        return crawl;
    }
    void forget() { cid = 0; czero = false; }
};

}  // namespace vr
