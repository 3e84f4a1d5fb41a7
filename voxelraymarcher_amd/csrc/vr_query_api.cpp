// vr_query_api.cpp -- the query entry points of include/vr.h: vr_pick, vr_trace, vr_shade,
// vr_shade_lights, vr_shade_lights_ao, vr_shade_lights_reflect, vr_shade_lights_atmosphere,
// vr_occlusion, vr_bounce_rays, vr_atmosphere_apply and vr_camera_rays (their kernels: vr_query.hip,
// vr_trace.hip, vr_shade.hip, vr_lights.hip, vr_occlusion.hip, vr_reflect.hip, vr_atmos.hip).  None
// is a render launch: no slot
// lease, no view key, nothing the render path keeps per device (vr_launch.cpp) is touched.  Each
// takes its arrays on the host or on the device (vr_staging.h), and in each every argument
// check comes before any device work.
#include <cstddef>
#include <cstring>

#include "vr_atmos_math.h"
#include "vr_host.h"
#include "vr_staging.h"

namespace {

using vr::DeviceGuard;
using vr::fail;
using vr::hip_fail;
using vr::Staging;

// The rows of a whole-frame render: one band, rank 0 of 1 (in a zeroed view).
void whole_frame(vr::KView& v, uint32_t height) {
    v.row_limit = height;
    v.band_rows = height;
    v.band_minv = height == 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / height);
    v.nranks = 1;
    v.local_rows = height;
}

// The n pixels (px[i], py[i]) on the device: the caller's own arrays, or host arrays staged in
// one buffer, py behind px.  Null after an error (sg.err).
const uint32_t* pixels_on_device(Staging& sg, const uint32_t* px, const uint32_t* py, size_t n, const uint32_t*& dpy) {
    uint32_t* q = (uint32_t*)sg.make(2 * n * sizeof(uint32_t));
    sg.put(q, px, n * sizeof(uint32_t));
    sg.put(q + n, py, n * sizeof(uint32_t));
    dpy = q + n;
    return sg.err == hipSuccess ? q : nullptr;
}

// The end of every query: the records' way back to a host array, the wait for the stream, and
// the first error of kernel launch `e`, copy and wait under the entry point's name.
int finish(Staging& sg, hipError_t e, void* host, const void* dev, size_t bytes, const char* who) {
    if (e == hipSuccess && host != dev) {
        sg.fetch(host, dev, bytes);
        e = sg.err;
    }
    const hipError_t es = sg.sync();
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, who);
    return VR_OK;
}

// What vr_shade_lights_ao adds to vr_shade_lights' arguments.
struct AoArgs {
    uint32_t strength, apply;
    uint32_t* out;
};

// What vr_shade_lights_reflect adds to vr_shade_lights_ao's arguments.
struct ReflectArgs {
    uint32_t reflectivity, bounces, mask, value;
};

// The kernels' form of a vr_atmosphere whose flags are not 0 (the colour bytes and the fog's span
// are made here, once per call).
vr::AtmosParams atmos_of(const vr_atmosphere* atm) {
    return vr::atmos_params(atm->zenith, atm->horizon, atm->nadir, atm->up, atm->fog_color, atm->fog_start, atm->fog_end,
                            atm->flags);
}

// One light pass per light over the rays of idx (null: all n), as vr_shade takes each light: the
// render's lighting block in the primary walk's view.
hipError_t light_terms(const vr_scene* s, vr_algo algo, const vr::KView& v, const vr_lighting* lights, size_t n_lights,
                       const uint32_t* idx, uint32_t n, const void* state, uint32_t* colors, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < n_lights && e == hipSuccess; ++k) {
        vr::KView lv = v;
        vr::view_lighting(lv, &lights[k]);
        e = vr::launch_light_term((int)s->store, (int)algo, vr::kscene(s), lv, idx, n, state, colors, st);
    }
    return e;
}

// The depths below the first of vr_shade_lights_reflect, after depth 0's kernels on `st`: state holds
// depth 0's hit state and colors0 its words W^0.  Per depth j >= 1 one bounce-and-compact pass
// (vr_reflect.hip) makes ray^j and the list of the rays that reflected at depth j - 1, the list's
// count comes back to the host (4 bytes, a wait for the stream: a count of 0 ends the descent),
// and vr_lights.hip's launches run over the list as they ran over all rays at depth 0, into a
// colour buffer of the depth.  The occlusion pass takes no list: it runs over all n records of a
// record buffer of this call, in which only the list's rays hold this depth's records -- whatever
// bytes the others hold are safe to read (vr_occlusion.hip) and their words are never read again.
// Then the folds, deepest first.  All scratch is one allocation of sg's, cut into 256-byte aligned
// parts -- the counts, the ray buffer(s), the record buffer, a list and a colour buffer per depth
// asked for -- so the descent costs one hipMalloc and one hipFree whatever its depth (each costs
// more than a depth's small kernels); it is freed on every path.  Under an atmosphere (at not null)
// one atmosphere pass (vr_atmos.hip) follows each depth's last colour pass, over that depth's list.
hipError_t reflect_descend(Staging& sg, const vr_scene* s, vr_algo algo, const vr::KView& v, const vr_lighting* lights,
                           size_t n_lights, const float* ambient, const AoArgs* ao, const ReflectArgs& rf, const vr::AtmosParams* at,
                           const void* rays0, uint32_t n, void* state, uint32_t* colors0, hipStream_t st) {
    const bool occlude = ao && ao->strength != 0u;       // (ao_out belongs to depth 0)
    const vr::KScene ks = vr::kscene(s);
    const auto part = [](size_t bytes) { return (bytes + 255u) & ~(size_t)255u; };
    const size_t counts_b = part(VR_MAX_BOUNCES * sizeof(uint32_t)), rays_b = part((size_t)n * sizeof(vr_ray)),
                 rec_b = occlude ? part((size_t)n * sizeof(vr_hit)) : 0u, words_b = part((size_t)n * sizeof(uint32_t));
    const size_t n_raybufs = rf.bounces > 1u ? 2u : 1u;
    char* base = (char*)sg.make(counts_b + n_raybufs * rays_b + rec_b + 2u * rf.bounces * words_b);
    if (sg.err != hipSuccess) return sg.err;
    uint32_t* counts = (uint32_t*)base;
    void* raybuf[2] = {base + counts_b, n_raybufs > 1u ? base + counts_b + rays_b : nullptr};
    void* rec = occlude ? base + counts_b + n_raybufs * rays_b : nullptr;
    char* per_depth = base + counts_b + n_raybufs * rays_b + rec_b;      // depth j: its list, then its colours
    hipError_t e = hipMemsetAsync(counts, 0, VR_MAX_BOUNCES * sizeof(uint32_t), st);
    uint32_t* col[VR_MAX_BOUNCES + 1] = {colors0};
    const uint32_t* list[VR_MAX_BOUNCES + 1] = {nullptr};
    uint32_t cnt[VR_MAX_BOUNCES + 1] = {n};
    const void* rays_prev = rays0;
    uint32_t depth = 0;
    for (uint32_t j = 1; j <= rf.bounces && e == hipSuccess; ++j) {
        uint32_t* lj = (uint32_t*)(per_depth + 2u * (j - 1u) * words_b);
        col[j] = (uint32_t*)(per_depth + (2u * (j - 1u) + 1u) * words_b);
        void* rays_j = raybuf[(j - 1u) & 1u];
        e = vr::launch_bounce_compact(state, rays_prev, list[j - 1], cnt[j - 1], rf.mask, rf.value, v.translation, v.scale_f,
                                      rays_j, lj, counts + (j - 1u), st);
        uint32_t c = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&c, counts + (j - 1u), sizeof c, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess || c == 0u) break;
        if (c > cnt[j - 1]) return hipErrorUnknown;     // (cannot happen: a list never grows)
        list[j] = lj;
        cnt[j] = c;
        depth = j;
        e = vr::launch_lights_primary((int)s->store, (int)algo, ks, v, rays_j, lj, c, ambient, state, col[j], rec, st);
        if (occlude && ao->apply == VR_AO_AMBIENT && e == hipSuccess)
            e = vr::launch_occlusion_apply((int)s->store, ks, rec, n, ao->strength, col[j], nullptr, st);
        if (e == hipSuccess) e = light_terms(s, algo, v, lights, n_lights, lj, c, state, col[j], st);
        if (occlude && ao->apply == VR_AO_ALL && e == hipSuccess)
            e = vr::launch_occlusion_apply((int)s->store, ks, rec, n, ao->strength, col[j], nullptr, st);
        // (over the list alone: the state of a ray outside it is an earlier depth's)
        if (at && e == hipSuccess) e = vr::launch_atmos_state(state, rays_j, lj, c, *at, v.translation, v.scale_f, col[j], st);
        rays_prev = rays_j;
    }
    for (uint32_t j = depth; j >= 1u && e == hipSuccess; --j)
        e = vr::launch_fold(list[j], cnt[j], col[j - 1], col[j], rf.reflectivity, st);
    return e;
}

// The body of vr_shade_lights (ao null), vr_shade_lights_ao and vr_shade_lights_reflect (rf not
// null; with a reflectivity or a depth of 0 it is vr_shade_lights_ao's call, kernel for kernel),
// under the name `who` in every
// message.  The occlusion pass (vr_occlusion.hip launch_occlusion_apply) runs over the records of
// the primary walk -- the caller's, or an internal buffer when hits is NULL -- straight after the
// primary kernel, when colors holds the ambient term alone (VR_AO_AMBIENT), or after the last
// light (VR_AO_ALL).  With strength 0 and no ao_out it does not run, no record buffer is made and
// the call is vr_shade_lights'.
int shade_lights(const char* who_c, const vr_scene* s, vr_algo algo, const vr_lighting* lights, size_t n_lights,
                 const float ambient[3], const float translation[3], uint32_t scale, const vr_ray* rays, size_t n,
                 int inputs_on_device, uint32_t* colors, vr_hit* hits, int outputs_on_device, uint32_t order, void* stream,
                 const AoArgs* ao, const ReflectArgs* rf = nullptr, const vr_atmosphere* atm = nullptr) {
    const std::string who(who_c);
    if (!s) return fail(VR_E_INVALID, who + ": scene is NULL");
    if (!translation) return fail(VR_E_INVALID, who + ": translation NULL");
    if (n_lights && !lights) return fail(VR_E_INVALID, who + ": lights NULL");
    if (n_lights > VR_MAX_LIGHTS) return fail(VR_E_INVALID, who + ": too many lights (VR_MAX_LIGHTS)");
    if (n && (!rays || !colors)) return fail(VR_E_INVALID, who + ": rays/colors NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, who + ": too many rays");
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS)
        return fail(VR_E_INVALID, who + ": unknown algorithm");
    if (order != VR_TRACE_ORDER_AUTO && order != VR_TRACE_ORDER_GIVEN && order != VR_TRACE_ORDER_COHERENT)
        return fail(VR_E_INVALID, who + ": unknown order");
    if (ao && ao->strength > 255u) return fail(VR_E_INVALID, who + ": ao_strength above 255");
    if (ao && ao->apply != VR_AO_AMBIENT && ao->apply != VR_AO_ALL) return fail(VR_E_INVALID, who + ": unknown ao_apply");
    if (rf && rf->reflectivity > 255u) return fail(VR_E_INVALID, who + ": reflectivity above 255");
    if (rf && rf->bounces > VR_MAX_BOUNCES) return fail(VR_E_INVALID, who + ": too many bounces (VR_MAX_BOUNCES)");
    if (rf && (rf->value & ~rf->mask) != 0u)
        return fail(VR_E_INVALID, who + ": mirror_value has bits outside mirror_mask (it could never match)");
    if (atm && (atm->flags & ~(VR_ATMOS_SKY | VR_ATMOS_FOG)) != 0u)
        return fail(VR_E_INVALID, who + ": unknown atmosphere flags");
    if (n == 0) return VR_OK;
    if (inputs_on_device && ((uintptr_t)rays & 15u) != 0u)
        return fail(VR_E_INVALID, who + ": device rays must be 16-byte aligned");
    if (outputs_on_device && ((uintptr_t)colors & 3u) != 0u)
        return fail(VR_E_INVALID, who + ": device colors must be 4-byte aligned");
    if (outputs_on_device && hits && ((uintptr_t)hits & 15u) != 0u)
        return fail(VR_E_INVALID, who + ": device hits must be 16-byte aligned");
    if (outputs_on_device && ao && ao->out && ((uintptr_t)ao->out & 3u) != 0u)
        return fail(VR_E_INVALID, who + ": device ao_out must be 4-byte aligned");
    // the trace's view for the primary walk (no camera, no light, no frame)
    vr::KView v;
    memset(&v, 0, sizeof v);
    for (int i = 0; i < 3; ++i) v.translation[i] = translation[i];
    v.scale_f = (float)scale;          // static_cast<float>(scale) (Ray.cuh:16)
    // AUTO is GIVEN, as vr_trace's (vr.h)
    const bool coherent = order == VR_TRACE_ORDER_COHERENT;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, who_c)) return rc;
    Staging sg(st);           // (owns every buffer below: freed on every path, after the stream has drained)
    const void* dr = inputs_on_device ? rays : sg.upload(rays, n * sizeof(vr_ray));
    if (sg.err != hipSuccess) return hip_fail(sg.err, (who + ": ray upload").c_str());
    uint32_t* dc = outputs_on_device ? colors : (uint32_t*)sg.make(n * sizeof(uint32_t));
    void* dh = (outputs_on_device || !hits) ? hits : sg.make(n * sizeof(vr_hit));
    // the occlusion pass reads the primary walk's records: the caller's, or a buffer of this call
    const bool occlude = ao && (ao->strength != 0u || ao->out);
    void* rec = dh;
    if (occlude && !rec) rec = sg.make(n * sizeof(vr_hit));
    uint32_t* da = nullptr;
    if (occlude && ao->out) da = outputs_on_device ? ao->out : (uint32_t*)sg.make(n * sizeof(uint32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, (who + ": output buffers").c_str());
    // the per-ray hit state between the primary pass and the light passes (32 bytes per ray)
    void* state = sg.make(n * 32u);
    if (sg.err == hipErrorOutOfMemory) return fail(VR_E_NOMEM, who + ": hit state: " + std::string(hipGetErrorString(sg.err)));
    if (sg.err != hipSuccess) return hip_fail(sg.err, (who + ": hit state").c_str());
    hipError_t e = hipSuccess;
    const uint32_t* idx = nullptr;
    if (coherent) {
        void* scratch = nullptr;
        e = vr::trace_order(vr::kscene(s), v, dr, (uint32_t)n, st, &scratch, &idx);
        sg.adopt(scratch);
    }
    if (e == hipSuccess)
        e = vr::launch_lights_primary((int)s->store, (int)algo, vr::kscene(s), v, dr, idx, (uint32_t)n, ambient, state, dc,
                                      rec, st);
    if (occlude && ao->apply == VR_AO_AMBIENT && e == hipSuccess)     // (colors holds the ambient term alone)
        e = vr::launch_occlusion_apply((int)s->store, vr::kscene(s), rec, (uint32_t)n, ao->strength, dc, da, st);
    if (e == hipSuccess) e = light_terms(s, algo, v, lights, n_lights, idx, (uint32_t)n, state, dc, st);
    if (occlude && ao->apply == VR_AO_ALL && e == hipSuccess)
        e = vr::launch_occlusion_apply((int)s->store, vr::kscene(s), rec, (uint32_t)n, ao->strength, dc, da, st);
    // the atmosphere over depth 0: elementwise over all n, so no order can matter
    vr::AtmosParams at;
    const bool tint = atm && atm->flags != 0u;
    if (tint) at = atmos_of(atm);
    if (tint && e == hipSuccess)
        e = vr::launch_atmos_state(state, dr, nullptr, (uint32_t)n, at, v.translation, v.scale_f, dc, st);
    if (rf && rf->reflectivity != 0u && rf->bounces != 0u && e == hipSuccess) {
        e = reflect_descend(sg, s, algo, v, lights, n_lights, ambient, ao, *rf, tint ? &at : nullptr, dr, (uint32_t)n, state,
                            dc, st);
        if (e == hipErrorOutOfMemory) return fail(VR_E_NOMEM, who + ": reflection buffers: " + std::string(hipGetErrorString(e)));
    }
    if (e == hipSuccess && da && ao->out != da) {
        sg.fetch(ao->out, da, n * sizeof(uint32_t));
        e = sg.err;
    }
    if (e == hipSuccess && hits != dh) {        // (the records' way back; the colours': finish)
        sg.fetch(hits, dh, n * sizeof(vr_hit));
        e = sg.err;
    }
    return finish(sg, e, colors, dc, n * sizeof(uint32_t), who_c);
}

}  // namespace

extern "C" {

// The hit behind each pixel (vr.h).
int vr_pick(const vr_scene* s, vr_algo algo, const vr_camera* cam, const float translation[3], uint32_t scale,
            uint32_t width, uint32_t height, const uint32_t* px, const uint32_t* py, size_t n, int inputs_on_device,
            vr_hit* hits, int outputs_on_device, void* stream) {
    static_assert(sizeof(vr_hit) == 64 && offsetof(vr_hit, voxel) == 8 && offsetof(vr_hit, normal) == 20 &&
                      offsetof(vr_hit, region) == 32 && offsetof(vr_hit, point) == 44 && offsetof(vr_hit, reserved) == 56,
                  "vr_hit: the record pick_kernel writes");
    static_assert(vr::kPickMiss == VR_HIT_MISS && vr::kPickVoxel == VR_HIT_VOXEL && vr::kPickNever == VR_HIT_NEVER &&
                      vr::kPickOutside == VR_HIT_OUTSIDE, "VR_HIT_*");
    if (!s) return fail(VR_E_INVALID, "vr_pick: scene is NULL");
    if (!cam || !translation) return fail(VR_E_INVALID, "vr_pick: camera/translation NULL");
    if (n && (!px || !py || !hits)) return fail(VR_E_INVALID, "vr_pick: px/py/hits NULL");
    if (width == 0 || height == 0 || width > 65536 || height > 65536) return fail(VR_E_INVALID, "vr_pick: bad image size");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_pick: too many queries");
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS) return fail(VR_E_INVALID, "vr_pick: unknown algorithm");
    if (n == 0) return VR_OK;
    if (outputs_on_device && ((uintptr_t)hits & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_pick: device hits must be 16-byte aligned");
    // the view of a whole-frame render (the lights are never read)
    vr_lighting lit;
    vr_lighting_default(&lit);
    vr::KView v;
    int rc = vr::make_view(s, cam, &lit, translation, scale, width, height, v);
    if (rc) return rc;
    whole_frame(v, height);
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if ((rc = vr::refuse_capture(st, "vr_pick"))) return rc;
    Staging sg(st);
    const uint32_t *dpx = px, *dpy = py;
    if (!inputs_on_device) dpx = pixels_on_device(sg, px, py, n, dpy);
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_pick: query upload");
    void* dh = outputs_on_device ? hits : sg.make(n * sizeof(vr_hit));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_pick: hit buffer");
    const hipError_t e = vr::launch_pick((int)s->store, (int)algo, vr::kscene(s), v, dpx, dpy, (uint32_t)n, dh, st);
    return finish(sg, e, hits, dh, n * sizeof(vr_hit), "vr_pick");
}

// The closest hit of arbitrary rays (vr.h).
int vr_trace(const vr_scene* s, vr_algo algo, const float translation[3], uint32_t scale, const vr_ray* rays, size_t n,
             int inputs_on_device, vr_hit* hits, int outputs_on_device, uint32_t order, void* stream) {
    static_assert(sizeof(vr_ray) == 32 && offsetof(vr_ray, reserved0) == 12 && offsetof(vr_ray, direction) == 16 &&
                      offsetof(vr_ray, reserved1) == 28, "vr_ray: the record trace_kernel loads");
    if (!s) return fail(VR_E_INVALID, "vr_trace: scene is NULL");
    if (!translation) return fail(VR_E_INVALID, "vr_trace: translation NULL");
    if (n && (!rays || !hits)) return fail(VR_E_INVALID, "vr_trace: rays/hits NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_trace: too many rays");
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS) return fail(VR_E_INVALID, "vr_trace: unknown algorithm");
    if (order != VR_TRACE_ORDER_AUTO && order != VR_TRACE_ORDER_GIVEN && order != VR_TRACE_ORDER_COHERENT)
        return fail(VR_E_INVALID, "vr_trace: unknown order");
    if (n == 0) return VR_OK;
    if (inputs_on_device && ((uintptr_t)rays & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_trace: device rays must be 16-byte aligned");
    if (outputs_on_device && ((uintptr_t)hits & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_trace: device hits must be 16-byte aligned");
    // the walk reads the view's translation and scale only (no camera, no light, no frame)
    vr::KView v;
    memset(&v, 0, sizeof v);
    for (int i = 0; i < 3; ++i) v.translation[i] = translation[i];
    v.scale_f = (float)scale;          // static_cast<float>(scale) (Ray.cuh:16)
    // AUTO is GIVEN at every n: COHERENT won at no measured size (vr.h, profiles/trace/README.md)
    const bool coherent = order == VR_TRACE_ORDER_COHERENT;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_trace")) return rc;
    Staging sg(st);
    const void* dr = inputs_on_device ? rays : sg.upload(rays, n * sizeof(vr_ray));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_trace: ray upload");
    void* dh = outputs_on_device ? hits : sg.make(n * sizeof(vr_hit));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_trace: hit buffer");
    hipError_t e = hipSuccess;
    const uint32_t* idx = nullptr;
    if (coherent) {
        void* scratch = nullptr;
        e = vr::trace_order(vr::kscene(s), v, dr, (uint32_t)n, st, &scratch, &idx);
        sg.adopt(scratch);
    }
    if (e == hipSuccess) e = vr::launch_trace((int)s->store, (int)algo, vr::kscene(s), v, dr, idx, (uint32_t)n, dh, st);
    return finish(sg, e, hits, dh, n * sizeof(vr_hit), "vr_trace");
}

// The render's colour, and on request the trace's record, for arbitrary rays (vr.h).
int vr_shade(const vr_scene* s, vr_algo algo, const vr_lighting* lit, const float translation[3], uint32_t scale,
             const vr_ray* rays, size_t n, int inputs_on_device, uint32_t* colors, vr_hit* hits, int outputs_on_device,
             uint32_t order, void* stream) {
    if (!s) return fail(VR_E_INVALID, "vr_shade: scene is NULL");
    if (!lit || !translation) return fail(VR_E_INVALID, "vr_shade: lighting/translation NULL");
    if (n && (!rays || !colors)) return fail(VR_E_INVALID, "vr_shade: rays/colors NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_shade: too many rays");
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS) return fail(VR_E_INVALID, "vr_shade: unknown algorithm");
    if (order != VR_TRACE_ORDER_AUTO && order != VR_TRACE_ORDER_GIVEN && order != VR_TRACE_ORDER_COHERENT)
        return fail(VR_E_INVALID, "vr_shade: unknown order");
    if (n == 0) return VR_OK;
    if (inputs_on_device && ((uintptr_t)rays & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_shade: device rays must be 16-byte aligned");
    if (outputs_on_device && ((uintptr_t)colors & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_shade: device colors must be 4-byte aligned");
    if (outputs_on_device && hits && ((uintptr_t)hits & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_shade: device hits must be 16-byte aligned");
    // the trace's view and the render's lighting block (no camera, no frame)
    vr::KView v;
    memset(&v, 0, sizeof v);
    vr::view_lighting(v, lit);
    for (int i = 0; i < 3; ++i) v.translation[i] = translation[i];
    v.scale_f = (float)scale;          // static_cast<float>(scale) (Ray.cuh:16)
    // AUTO is GIVEN, as vr_trace's (vr.h)
    const bool coherent = order == VR_TRACE_ORDER_COHERENT;
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_shade")) return rc;
    Staging sg(st);
    const void* dr = inputs_on_device ? rays : sg.upload(rays, n * sizeof(vr_ray));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_shade: ray upload");
    uint32_t* dc = outputs_on_device ? colors : (uint32_t*)sg.make(n * sizeof(uint32_t));
    void* dh = (outputs_on_device || !hits) ? hits : sg.make(n * sizeof(vr_hit));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_shade: output buffers");
    hipError_t e = hipSuccess;
    const uint32_t* idx = nullptr;
    if (coherent) {
        void* scratch = nullptr;
        e = vr::trace_order(vr::kscene(s), v, dr, (uint32_t)n, st, &scratch, &idx);
        sg.adopt(scratch);
    }
    if (e == hipSuccess)
        e = vr::launch_shade((int)s->store, (int)algo, vr::kscene(s), v, dr, idx, (uint32_t)n, dc, dh, st);
    if (e == hipSuccess && hits != dh) {        // (the records' way back; the colours': finish)
        sg.fetch(hits, dh, n * sizeof(vr_hit));
        e = sg.err;
    }
    return finish(sg, e, colors, dc, n * sizeof(uint32_t), "vr_shade");
}

// vr_shade's colours under several lights and an ambient term, from one primary walk (vr.h).
int vr_shade_lights(const vr_scene* s, vr_algo algo, const vr_lighting* lights, size_t n_lights, const float ambient[3],
                    const float translation[3], uint32_t scale, const vr_ray* rays, size_t n, int inputs_on_device,
                    uint32_t* colors, vr_hit* hits, int outputs_on_device, uint32_t order, void* stream) {
    return shade_lights("vr_shade_lights", s, algo, lights, n_lights, ambient, translation, scale, rays, n, inputs_on_device,
                        colors, hits, outputs_on_device, order, stream, nullptr);
}

// vr_shade_lights with the ambient term, or the whole word, scaled by the hit's occlusion (vr.h).
int vr_shade_lights_ao(const vr_scene* s, vr_algo algo, const vr_lighting* lights, size_t n_lights, const float ambient[3],
                       const float translation[3], uint32_t scale, const vr_ray* rays, size_t n, int inputs_on_device,
                       uint32_t* colors, vr_hit* hits, int outputs_on_device, uint32_t order, void* stream,
                       uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out) {
    const AoArgs ao{ao_strength, ao_apply, ao_out};
    return shade_lights("vr_shade_lights_ao", s, algo, lights, n_lights, ambient, translation, scale, rays, n,
                        inputs_on_device, colors, hits, outputs_on_device, order, stream, &ao);
}

// vr_shade_lights_ao with mirror reflections: the bounces' words folded into the first hit's (vr.h).
int vr_shade_lights_reflect(const vr_scene* s, vr_algo algo, const vr_lighting* lights, size_t n_lights,
                            const float ambient[3], const float translation[3], uint32_t scale, const vr_ray* rays, size_t n,
                            int inputs_on_device, uint32_t* colors, vr_hit* hits, int outputs_on_device, uint32_t order,
                            void* stream, uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out, uint32_t reflectivity,
                            uint32_t bounces, uint32_t mirror_mask, uint32_t mirror_value) {
    const AoArgs ao{ao_strength, ao_apply, ao_out};
    const ReflectArgs rf{reflectivity, bounces, mirror_mask, mirror_value};
    return shade_lights("vr_shade_lights_reflect", s, algo, lights, n_lights, ambient, translation, scale, rays, n,
                        inputs_on_device, colors, hits, outputs_on_device, order, stream, &ao, &rf);
}

// vr_shade_lights_reflect under a sky and a distance fog (vr.h).
int vr_shade_lights_atmosphere(const vr_scene* s, vr_algo algo, const vr_lighting* lights, size_t n_lights,
                               const float ambient[3], const float translation[3], uint32_t scale, const vr_ray* rays,
                               size_t n, int inputs_on_device, uint32_t* colors, vr_hit* hits, int outputs_on_device,
                               uint32_t order, void* stream, uint32_t ao_strength, uint32_t ao_apply, uint32_t* ao_out,
                               uint32_t reflectivity, uint32_t bounces, uint32_t mirror_mask, uint32_t mirror_value,
                               const vr_atmosphere* atm) {
    const AoArgs ao{ao_strength, ao_apply, ao_out};
    const ReflectArgs rf{reflectivity, bounces, mirror_mask, mirror_value};
    return shade_lights("vr_shade_lights_atmosphere", s, algo, lights, n_lights, ambient, translation, scale, rays, n,
                        inputs_on_device, colors, hits, outputs_on_device, order, stream, &ao, &rf, atm);
}

// How open the face of each hit is at the hit point (vr.h).
int vr_occlusion(const vr_scene* s, const vr_hit* hits, size_t n, int inputs_on_device, uint32_t* ao, int outputs_on_device,
                 void* stream) {
    static_assert(VR_AO_OPEN == 255u, "VR_AO_OPEN: vr_occlusion_math.h kAoOpen");
    if (!s) return fail(VR_E_INVALID, "vr_occlusion: scene is NULL");
    if (n && (!hits || !ao)) return fail(VR_E_INVALID, "vr_occlusion: hits/ao NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_occlusion: too many records");
    if (n == 0) return VR_OK;
    if (inputs_on_device && ((uintptr_t)hits & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_occlusion: device hits must be 16-byte aligned");
    if (outputs_on_device && ((uintptr_t)ao & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_occlusion: device ao must be 4-byte aligned");
    DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_occlusion")) return rc;
    Staging sg(st);
    const void* dh = inputs_on_device ? hits : sg.upload(hits, n * sizeof(vr_hit));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_occlusion: record upload");
    uint32_t* da = outputs_on_device ? ao : (uint32_t*)sg.make(n * sizeof(uint32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_occlusion: ao buffer");
    const hipError_t e = vr::launch_occlusion((int)s->store, vr::kscene(s), dh, (uint32_t)n, da, st);
    return finish(sg, e, ao, da, n * sizeof(uint32_t), "vr_occlusion");
}

// The mirror bounce of each ray at its hit record (vr.h): needs no scene.
int vr_bounce_rays(int device, const float translation[3], uint32_t scale, const vr_ray* rays, const vr_hit* hits, size_t n,
                   int inputs_on_device, vr_ray* out, int outputs_on_device, void* stream) {
    if (!translation) return fail(VR_E_INVALID, "vr_bounce_rays: translation NULL");
    if (n && (!rays || !hits || !out)) return fail(VR_E_INVALID, "vr_bounce_rays: rays/hits/out NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_bounce_rays: too many records");
    if (device < 0 || device > 63) return fail(VR_E_INVALID, "vr_bounce_rays: bad device");
    if (n == 0) return VR_OK;
    if (inputs_on_device && (((uintptr_t)rays | (uintptr_t)hits) & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_bounce_rays: device rays and hits must be 16-byte aligned");
    if (outputs_on_device && ((uintptr_t)out & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_bounce_rays: device out must be 16-byte aligned");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return fail(VR_E_INVALID, "vr_bounce_rays: no such device");
    DeviceGuard dg(device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_bounce_rays")) return rc;
    Staging sg(st);
    const void *dr = rays, *dh = hits;
    if (!inputs_on_device) {
        dr = sg.upload(rays, n * sizeof(vr_ray));
        dh = sg.upload(hits, n * sizeof(vr_hit));
    }
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_bounce_rays: record upload");
    void* dout = outputs_on_device ? out : sg.make(n * sizeof(vr_ray));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_bounce_rays: ray buffer");
    const hipError_t e = vr::launch_bounce_rays(dr, dh, (uint32_t)n, translation, (float)scale, dout, st);
    return finish(sg, e, out, dout, n * sizeof(vr_ray), "vr_bounce_rays");
}

// A daylight sky, fog off (vr.h).
int vr_atmosphere_default(vr_atmosphere* atm) {
    static_assert(sizeof(vr_atmosphere) == 76 && offsetof(vr_atmosphere, up) == 36 && offsetof(vr_atmosphere, fog_start) == 60 &&
                      offsetof(vr_atmosphere, flags) == 68, "vr_atmosphere");
    static_assert(vr::kAtmosSky == VR_ATMOS_SKY && vr::kAtmosFog == VR_ATMOS_FOG && vr::kAtmosStatusMiss == VR_HIT_MISS &&
                      vr::kBounceStatusVoxel == VR_HIT_VOXEL, "VR_ATMOS_*, VR_HIT_*");
    if (!atm) return fail(VR_E_INVALID, "vr_atmosphere_default: atm NULL");
    const vr_atmosphere d = {{0.25f, 0.45f, 0.85f}, {0.75f, 0.85f, 0.95f}, {0.30f, 0.28f, 0.25f}, {0.0f, 1.0f, 0.0f},
                             {0.75f, 0.85f, 0.95f}, 0.0f, 16.0f, VR_ATMOS_SKY, 0u};
    *atm = d;
    return VR_OK;
}

// The colour word of each ray under an atmosphere, from its hit record (vr.h): needs no scene.
int vr_atmosphere_apply(int device, const vr_atmosphere* atm, const float translation[3], uint32_t scale, const vr_ray* rays,
                        const vr_hit* hits, const uint32_t* colors_in, size_t n, int inputs_on_device, uint32_t* colors_out,
                        int outputs_on_device, void* stream) {
    if (!atm || !translation) return fail(VR_E_INVALID, "vr_atmosphere_apply: atm/translation NULL");
    if ((atm->flags & ~(VR_ATMOS_SKY | VR_ATMOS_FOG)) != 0u) return fail(VR_E_INVALID, "vr_atmosphere_apply: unknown atmosphere flags");
    if (n && (!rays || !hits || !colors_in || !colors_out))
        return fail(VR_E_INVALID, "vr_atmosphere_apply: rays/hits/colors_in/colors_out NULL");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_atmosphere_apply: too many records");
    if (device < 0 || device > 63) return fail(VR_E_INVALID, "vr_atmosphere_apply: bad device");
    if (n == 0) return VR_OK;
    if (inputs_on_device && (((uintptr_t)rays | (uintptr_t)hits) & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_atmosphere_apply: device rays and hits must be 16-byte aligned");
    if (inputs_on_device && ((uintptr_t)colors_in & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_atmosphere_apply: device colors_in must be 4-byte aligned");
    if (outputs_on_device && ((uintptr_t)colors_out & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_atmosphere_apply: device colors_out must be 4-byte aligned");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return fail(VR_E_INVALID, "vr_atmosphere_apply: no such device");
    DeviceGuard dg(device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_atmosphere_apply")) return rc;
    Staging sg(st);
    const void *dr = rays, *dh = hits;
    const uint32_t* din = colors_in;
    if (!inputs_on_device) {
        dr = sg.upload(rays, n * sizeof(vr_ray));
        dh = sg.upload(hits, n * sizeof(vr_hit));
        din = (const uint32_t*)sg.upload(colors_in, n * sizeof(uint32_t));
    }
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_atmosphere_apply: record upload");
    uint32_t* dout = outputs_on_device ? colors_out : (uint32_t*)sg.make(n * sizeof(uint32_t));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_atmosphere_apply: colour buffer");
    const vr::AtmosParams at = atmos_of(atm);
    const hipError_t e = vr::launch_atmos_records(dr, dh, din, (uint32_t)n, at, translation, (float)scale, dout, st);
    return finish(sg, e, colors_out, dout, n * sizeof(uint32_t), "vr_atmosphere_apply");
}

// The rays a render or pick walks for pixels of a frame (vr.h): needs no scene.
int vr_camera_rays(int device, const vr_camera* cam, uint32_t width, uint32_t height, const uint32_t* px,
                   const uint32_t* py, size_t n, int inputs_on_device, vr_ray* rays, int outputs_on_device, void* stream) {
    if (!cam) return fail(VR_E_INVALID, "vr_camera_rays: camera NULL");
    if (n && (!px || !py || !rays)) return fail(VR_E_INVALID, "vr_camera_rays: px/py/rays NULL");
    if (width == 0 || height == 0 || width > 65536 || height > 65536)
        return fail(VR_E_INVALID, "vr_camera_rays: bad image size");
    if (n >= (1ull << 31)) return fail(VR_E_INVALID, "vr_camera_rays: too many pixels");
    if (device < 0 || device > 63) return fail(VR_E_INVALID, "vr_camera_rays: bad device");
    if (n == 0) return VR_OK;
    if (outputs_on_device && ((uintptr_t)rays & 15u) != 0u)
        return fail(VR_E_INVALID, "vr_camera_rays: device rays must be 16-byte aligned");
    // the view of a whole-frame render, as vr_pick's; only the camera is read
    vr::KView v;
    memset(&v, 0, sizeof v);
    vr::view_camera(v, cam, width, height);
    whole_frame(v, height);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return fail(VR_E_INVALID, "vr_camera_rays: no such device");
    DeviceGuard dg(device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_camera_rays")) return rc;
    Staging sg(st);
    const uint32_t *dpx = px, *dpy = py;
    if (!inputs_on_device) dpx = pixels_on_device(sg, px, py, n, dpy);
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_camera_rays: pixel upload");
    void* dr = outputs_on_device ? rays : sg.make(n * sizeof(vr_ray));
    if (sg.err != hipSuccess) return hip_fail(sg.err, "vr_camera_rays: ray buffer");
    const hipError_t e = vr::launch_camera_rays(v, dpx, dpy, (uint32_t)n, dr, st);
    return finish(sg, e, rays, dr, n * sizeof(vr_ray), "vr_camera_rays");
}

}  // extern "C"
