// launch_plan_check -- the launch decisions of vr_launch_plan.h against literal tables, on a
// CPU.  Returns 0, or prints the failing cases and returns 1.
#include "vr_launch_plan.h"

#include <stdio.h>

static int g_bad = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            ++g_bad;                              \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                  \
            printf("  [%s]\n", #cond);            \
        }                                         \
    } while (0)

// ---------------------------------------------------------------- policy
// schedule: 0 AUTO, 1 GRID, 2 HEAVIEST_FIRST; occupancy: 0 AUTO, 1 LONE, 2 IN_FLIGHT
static const bool kHeavy[3][2][2] = {   // [schedule][alone][inflight_heavy]
    {{false, true}, {true, true}},
    {{false, false}, {false, false}},
    {{true, true}, {true, true}},
};
static const bool kHi[3][2][2] = {      // [occupancy][alone][in_flight_occupancy]
    {{false, true}, {false, false}},
    {{false, false}, {false, false}},
    {{true, true}, {true, true}},
};
static const uint32_t kOverride[2] = {0, 5};
static const uint32_t kRpw[2][2] = {    // [override index][alone], in-flight rpw 32
    {32, 2},
    {5, 5},
};

static void check_policy() {
    int cases = 0;
    for (uint32_t sch = 0; sch < 3; ++sch)
        for (uint32_t occ = 0; occ < 3; ++occ)
            for (int alone = 0; alone < 2; ++alone)
                for (int ih = 0; ih < 2; ++ih)
                    for (int ifo = 0; ifo < 2; ++ifo)
                        for (int ov = 0; ov < 2; ++ov) {
                            const vr::PolicyKnobs k = {ih != 0, ifo != 0, kOverride[ov], 32};
                            const vr::LaunchPolicy p = vr::launch_policy(sch, occ, alone != 0, k);
                            CHECK(p.heavy == kHeavy[sch][alone][ih] && p.hi == kHi[occ][alone][ifo] &&
                                      p.crawl_rpw == kRpw[ov][alone],
                                  "policy schedule %u occupancy %u alone %d inflight_heavy %d in_flight_occupancy %d "
                                  "override %u: heavy %d hi %d rpw %u",
                                  sch, occ, alone, ih, ifo, kOverride[ov], p.heavy, p.hi, p.crawl_rpw);
                            ++cases;
                        }
    CHECK(cases == 144, "policy cases %d", cases);
    CHECK(VR_SCHEDULE_AUTO == 0 && VR_SCHEDULE_GRID == 1 && VR_SCHEDULE_HEAVIEST_FIRST == 2, "schedule values");
    CHECK(VR_OCCUPANCY_AUTO == 0 && VR_OCCUPANCY_LONE == 1 && VR_OCCUPANCY_IN_FLIGHT == 2, "occupancy values");
}

// ---------------------------------------------------------------- crawl skip
static uint64_t report(uint32_t id, uint32_t count) { return (uint64_t)count << 32 | id; }

// One step from state {cid, ckey, czero} and the expected result and state after it.
struct SkipCase {
    const char* name;
    uint32_t cid; uint64_t ckey; bool czero;                 // before
    uint64_t key; uint32_t rid, rcount, lid; bool force, enabled;
    bool crawl; uint32_t cid2; uint64_t ckey2; bool czero2; // after (force is always consumed)
};
static const SkipCase kSkip[] = {
    // name                         cid ckey czero  key  rid rcount lid force enabled  crawl cid2 ckey2 czero2
    {"new key crawls, adopts",        7, 100, false, 200,  7, 0,  9, false, true,   true,  9, 200, false},
    {"new key ends skipping",         7, 100, true,  200,  7, 0,  9, false, true,   true,  9, 200, false},
    {"{cid,0} starts skipping",       7, 100, false, 100,  7, 0,  9, false, true,   false, 7, 100, true},
    {"report of another id crawls",   7, 100, false, 100,  6, 0,  9, false, true,   true,  9, 100, false},
    {"{cid,n>0} crawls",              7, 100, false, 100,  7, 3,  9, false, true,   true,  9, 100, false},
    {"skipping, nonzero count ends",  7, 100, true,  100,  8, 1,  9, false, true,   true,  9, 100, false},
    {"skipping, zero count keeps",    7, 100, true,  100,  7, 0,  9, false, true,   false, 7, 100, true},
    {"cid 0 (forgotten) crawls",      0, 100, false, 100,  0, 0,  9, false, true,   true,  9, 100, false},
    {"forced skip, fresh state",      0,   0, false, 200,  0, 0,  9, true,  true,   false, 0, 200, true},
    {"forced skip, other key",        7, 100, false, 200,  7, 5,  9, true,  true,   false, 7, 200, true},
    {"forced skip, same key, count",  7, 100, true,  100,  8, 1,  9, true,  true,   false, 7, 100, true},
    {"disabled: {cid,0} crawls",      7, 100, false, 100,  7, 0,  9, false, false,  true,  9, 100, true},
    {"disabled: czero kept, crawls",  7, 100, true,  100,  7, 0,  9, false, false,  true,  9, 100, true},
    {"disabled: nonzero count ends",  7, 100, true,  100,  8, 1,  9, false, false,  true,  9, 100, false},
    {"disabled: new key",             7, 100, true,  200,  7, 0,  9, false, false,  true,  9, 200, false},
    {"disabled: forced, consumed",    7, 100, false, 200,  7, 0,  9, true,  false,  true,  9, 200, true},
};

static void check_crawl_skip() {
    for (const SkipCase& c : kSkip) {
        vr::CrawlSkip s;
        s.cid = c.cid; s.ckey = c.ckey; s.czero = c.czero;
        bool force = c.force;
        const bool crawl = s.step(c.key, report(c.rid, c.rcount), c.lid, force, c.enabled);
        CHECK(crawl == c.crawl && s.cid == c.cid2 && s.ckey == c.ckey2 && s.czero == c.czero2 && !force,
              "crawl skip '%s': crawl %d cid %u ckey %llu czero %d force %d", c.name, crawl, s.cid,
              (unsigned long long)s.ckey, s.czero, force);
    }
    // a slot's life: crawl, report {id, 0}, skip, skip, a skipped launch defers, crawl again
    vr::CrawlSkip s;
    bool force = false;
    CHECK(s.step(100, report(0, 0), 1, force, true) && s.cid == 1, "life: first launch crawls");
    CHECK(s.step(100, report(0, 0), 2, force, true) && s.cid == 2, "life: no report yet, crawls");
    CHECK(!s.step(100, report(2, 0), 3, force, true) && s.cid == 2, "life: {2, 0} reported, skips");
    CHECK(!s.step(100, report(2, 0), 4, force, true), "life: keeps skipping");
    CHECK(s.step(100, report(4, 1), 5, force, true) && s.cid == 5 && !s.czero, "life: launch 4 deferred, crawls");
    s.forget();
    CHECK(s.cid == 0 && !s.czero && s.ckey == 100, "forget");

    uint32_t serial = 0;
    CHECK(vr::next_launch_id(serial) == 1 && serial == 1, "launch id after 0");
    serial = 0xFFFFFFFEu;
    CHECK(vr::next_launch_id(serial) == 0xFFFFFFFFu, "launch id after 0xFFFFFFFE");
    CHECK(vr::next_launch_id(serial) == 1 && serial == 1, "launch id after 0xFFFFFFFF is 1");
}

// ---------------------------------------------------------------- orders
template <class Order>
static void check_matches(const char* name) {
    Order o;
    CHECK(!o.matches(0, 0, 0), "%s: a fresh order matches", name);
    o.learned(5, 7, 99, true);
    o.age = 3;
    CHECK(o.valid && o.gx == 5 && o.gy == 7 && o.key == 99, "%s: learned", name);
    CHECK(o.matches(5, 7, 99), "%s: same grid and key", name);
    CHECK(!o.matches(6, 7, 99), "%s: changed gx", name);
    CHECK(!o.matches(5, 8, 99), "%s: changed gy", name);
    CHECK(!o.matches(5, 7, 98), "%s: changed key", name);
    o.forget();
    CHECK(!o.matches(5, 7, 99) && o.gx == 5 && o.gy == 7 && o.key == 99 && o.age == 3, "%s: forgotten", name);
    o.learned(5, 7, 99, false);
    CHECK(!o.matches(5, 7, 99) && o.age == 0, "%s: a failed build is invalid", name);
}

struct RemakeCase {
    bool match, stale, repeat;
    uint32_t refresh, age;
    bool remake;
    uint32_t age2;
};
static const RemakeCase kRemake[] = {
    // match stale  repeat refresh age  remake age2
    {false, false, false, 0, 0, false, 0}, {false, false, true, 0, 0, true, 0},
    {false, true, false, 0, 0, false, 0},  {false, true, true, 0, 0, true, 0},
    {false, false, false, 2, 1, false, 1}, {false, false, true, 2, 1, true, 1},
    {false, true, false, 2, 1, false, 1},  {false, true, true, 2, 1, true, 1},
    {true, false, false, 0, 0, false, 0},  {true, false, true, 0, 0, false, 0},
    {true, false, false, 0, 5, false, 5},  {true, false, true, 0, 5, false, 5},
    {true, true, false, 0, 0, true, 0},    {true, true, true, 0, 0, true, 0},
    {true, false, false, 2, 0, false, 1},  {true, false, true, 2, 0, false, 1},
    {true, false, false, 2, 1, true, 2},   {true, false, true, 2, 1, true, 2},
    {true, true, false, 2, 0, true, 0},    {true, true, true, 2, 0, true, 0},
    {true, true, false, 2, 1, true, 1},    {true, true, true, 2, 1, true, 1},
};

static void check_orders() {
    check_matches<vr::WorkOrder>("work order");
    check_matches<vr::LaneOrder>("lane order");
    vr::WorkOrder w;
    w.relaned = true;
    w.learned(1, 1, 1, true);
    CHECK(!w.relaned, "work order: learned clears relaned");
    w.relaned = true;
    w.forget();
    CHECK(!w.relaned && !w.valid, "work order: forget clears relaned");
    for (const RemakeCase& c : kRemake) {
        uint32_t age = c.age;
        const bool r = vr::remake_due(c.match, c.stale, c.repeat, age, c.refresh);
        CHECK(r == c.remake && age == c.age2, "remake match %d stale %d repeat %d refresh %u age %u: %d, age %u", c.match,
              c.stale, c.repeat, c.refresh, c.age, r, age);
    }
}

int main() {
    check_policy();
    check_crawl_skip();
    check_orders();
    if (g_bad) printf("launch_plan_check: %d failed\n", g_bad);
    return g_bad ? 1 : 0;
}
