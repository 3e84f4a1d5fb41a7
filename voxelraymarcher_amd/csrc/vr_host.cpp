// vr_host.cpp -- the thread's error string and the camera and lighting maths of the C ABI
// (include/vr.h).  The rest of libvr.so's host side: vr_scene.cpp (scene build and upload),
// vr_scene_io.cpp (synthetic grids, .vox/.vxb files), vr_launch.cpp (the render launch),
// vr_query_api.cpp (vr_pick, vr_trace, vr_camera_rays).
//
// Replaces Camera::Camera (renderer/camera/Camera.cuh:11-23).
#include <cmath>
#include <string>

#include "vr_host.h"

namespace {

using vr::fail;

thread_local std::string g_err = "";

// ---------------------------------------------------------------- camera math
struct f3 { float x, y, z; };
inline f3 add(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline f3 sub(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline f3 scl(float t, f3 a) { return {t * a.x, t * a.y, t * a.z}; }
inline f3 unit(f3 a) {
    float len = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return {a.x / len, a.y / len, a.z / len};
}
inline f3 cross(f3 a, f3 b) {   // Vector3.cuh:154-159
    return {(a.y * b.z - a.z * b.y), (-(a.x * b.z - a.z * b.x)), (a.x * b.y - a.y * b.x)};
}

}  // namespace

namespace vr {
int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace vr

extern "C" {

const char* vr_last_error(void) { return g_err.c_str(); }
const char* vr_version(void) { return "voxelraymarcher_amd 0.1 (gfx950)"; }

int vr_camera_make(const float eye[3], const float look_at[3], const float up[3], float fov_deg, float aspect,
                   vr_camera* out) {
    if (!eye || !look_at || !up || !out) return fail(VR_E_INVALID, "NULL argument");
    const float PI = 3.141592f;                                 // MathConstants.cuh:3
    float half_h = std::tan((fov_deg * PI / 180.f) / 2.0f);     // Camera.cuh:13
    float half_w = half_h * aspect;
    f3 o{eye[0], eye[1], eye[2]};
    f3 w = unit(sub(f3{look_at[0], look_at[1], look_at[2]}, o));
    f3 u = unit(cross(w, f3{up[0], up[1], up[2]}));
    f3 v = cross(u, w);
    f3 llc = add(sub(sub(o, scl(half_w, u)), scl(half_h, v)), w);   // :19
    f3 hor = scl(2 * half_w, u), ver = scl(2 * half_h, v);
    const f3* src[5] = {&o, &llc, &hor, &ver, &w};
    float* dst[5] = {out->origin, out->lower_left, out->horizontal, out->vertical, out->forward};
    for (int i = 0; i < 5; ++i) { dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z; }
    return VR_OK;
}

int vr_lighting_default(vr_lighting* out) {
    if (!out) return fail(VR_E_INVALID, "NULL argument");
    f3 L = unit(f3{1.0f, 1.0f, 1.0f});                          // Main.cu:28
    out->light_dir[0] = L.x; out->light_dir[1] = L.y; out->light_dir[2] = L.z;
    for (int i = 0; i < 3; ++i) out->light_color[i] = 1.0f;    // :31
    out->light_pos[0] = 10.0f; out->light_pos[1] = 10.0f; out->light_pos[2] = -10.0f;   // :34
    out->use_point_light = 0;                                   // :37
    out->use_shadows = 1;                                       // :40
    return VR_OK;
}

int vr_lighting_set_direction(vr_lighting* lit, const float dir[3]) {
    if (!lit || !dir) return fail(VR_E_INVALID, "NULL argument");
    f3 L = unit(f3{dir[0], dir[1], dir[2]});                     // Main.cu:28 makeUnitVector
    if (!std::isfinite(L.x) || !std::isfinite(L.y) || !std::isfinite(L.z))
        return fail(VR_E_INVALID, "light direction must be a finite non-zero vector");
    lit->light_dir[0] = L.x; lit->light_dir[1] = L.y; lit->light_dir[2] = L.z;
    return VR_OK;
}

}  // extern "C"
