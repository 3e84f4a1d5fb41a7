// vr.hpp -- C++ host interface over the C ABI (vr.h), mirroring the
// reference's host-side names so code written against
// lukeduball/VoxelRaymarcher reads the same:
//   StorageType            (geometry/VoxelFunctions.cuh:37)
//   Camera                 (renderer/camera/Camera.cuh:8-40)
//   VoxelSceneInfo         (renderer/VoxelSceneInfo.cuh:5-15)
//   VoxelSceneCPU          (geometry/VoxelSceneCPU.cuh:13-131)
//   VoxelFile::readVoxelFile (geometry/VoxelFile.cuh:6-37)
//   runRaymarchingKernel   (main/Main.cu:105-163)
// Errors surface as vrx::Error (the reference ignores them).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "vr.h"

namespace vrx {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc, const char* where) {
    if (rc != VR_OK) throw Error(rc, std::string(where) + ": " + vr_last_error());
}

enum class StorageType { VOXEL_CLUSTER_STORE = VR_STORE_VCS, HASH_TABLE = VR_STORE_HASHTABLE };
enum class RayMarchAlgorithm { LONGEST_AXIS = VR_ALGO_LONGESTAXIS, ORIGINAL = VR_ALGO_ORIGINAL };

struct Vector3f {
    float x = 0, y = 0, z = 0;
};

class Camera {
public:
    Camera(Vector3f o, Vector3f lookAt, Vector3f globalUp, float fieldOfView, float aspectRatio) {
        float e[3] = {o.x, o.y, o.z}, l[3] = {lookAt.x, lookAt.y, lookAt.z}, u[3] = {globalUp.x, globalUp.y, globalUp.z};
        check(vr_camera_make(e, l, u, fieldOfView, aspectRatio, &cam_), "Camera");
    }
    const vr_camera& raw() const { return cam_; }

private:
    vr_camera cam_{};
};

struct VoxelSceneInfo {
    Vector3f translationVector{};
    uint32_t scale = 1;
    VoxelSceneInfo() = default;
    VoxelSceneInfo(Vector3f location, uint32_t s = 1) : translationVector(location), scale(s) {}
};

// Owns one device scene (the reference's deviceVoxelScene + per-region stores).
class DeviceScene {
public:
    DeviceScene() = default;
    explicit DeviceScene(vr_scene* s) : s_(s) {}
    DeviceScene(const DeviceScene&) = delete;
    DeviceScene& operator=(const DeviceScene&) = delete;
    DeviceScene(DeviceScene&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    DeviceScene& operator=(DeviceScene&& o) noexcept {
        if (this != &o) { vr_scene_destroy(s_); s_ = o.s_; o.s_ = nullptr; }
        return *this;
    }
    ~DeviceScene() { vr_scene_destroy(s_); }
    const vr_scene* get() const { return s_; }
    vr_scene* get() { return s_; }
    vr_scene_info info() const {
        vr_scene_info i{};
        check(vr_scene_get_info(s_, &i), "vr_scene_get_info");
        return i;
    }

private:
    vr_scene* s_ = nullptr;
};

class VoxelSceneCPU {
public:
    void insertVoxel(int32_t x, int32_t y, int32_t z, uint32_t color) {
        xyz_.push_back(x); xyz_.push_back(y); xyz_.push_back(z);
        rgb_.push_back(color);
    }
    // Builds the storage structures and uploads them (generateVoxelScene).
    DeviceScene generateVoxelScene(StorageType storageType, int device = 0) const {
        vr_scene* s = nullptr;
        check(vr_scene_create(device, (vr_store)storageType, xyz_.data(), rgb_.data(), rgb_.size(), &s),
              "generateVoxelScene");
        return DeviceScene(s);
    }
    size_t size() const { return rgb_.size(); }
    const std::vector<int32_t>& coords() const { return xyz_; }
    const std::vector<uint32_t>& colors() const { return rgb_; }

private:
    std::vector<int32_t> xyz_;
    std::vector<uint32_t> rgb_;
};

struct VoxelFile {
    // .vox CSV or, detected by its magic, the .vxb binary sidecar.
    static void readVoxelFile(VoxelSceneCPU& scene, const std::string& path) {
        size_t n = 0;
        check(vr_scene_file_read(path.c_str(), nullptr, nullptr, 0, &n), "readVoxelFile");
        std::vector<int32_t> xyz(3 * n + 3);
        std::vector<uint32_t> rgb(n + 1);
        check(vr_scene_file_read(path.c_str(), xyz.data(), rgb.data(), n, &n), "readVoxelFile");
        for (size_t i = 0; i < n; ++i) scene.insertVoxel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], rgb[i]);
    }
    // Write the binary sidecar of a scene file (vr_vxb_write).
    static void writeBinary(const std::string& src, const std::string& dst) {
        size_t n = 0;
        check(vr_scene_file_read(src.c_str(), nullptr, nullptr, 0, &n), "readVoxelFile");
        std::vector<int32_t> xyz(3 * n + 3);
        std::vector<uint32_t> rgb(n + 1);
        check(vr_scene_file_read(src.c_str(), xyz.data(), rgb.data(), n, &n), "readVoxelFile");
        check(vr_vxb_write(dst.c_str(), xyz.data(), rgb.data(), n), "vr_vxb_write");
    }
};

inline vr_lighting defaultLighting() {
    vr_lighting l{};
    check(vr_lighting_default(&l), "setupConstantValues");
    return l;
}

// LIGHT_DIRECTION = makeUnitVector(dir) (Main.cu:28).
inline void setLightDirection(vr_lighting& l, float x, float y, float z) {
    const float d[3] = {x, y, z};
    check(vr_lighting_set_direction(&l, d), "setLightDirection");
}

// Launch on `stream` (hipStream_t as void*); asynchronous.
inline void runRaymarchingKernel(uint32_t width, uint32_t height, RayMarchAlgorithm algo, const Camera& camera,
                                 const VoxelSceneInfo& info, const DeviceScene& scene, const vr_lighting& lighting,
                                 uint32_t* framebufferDev, void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    check(vr_render(scene.get(), (vr_algo)algo, &camera.raw(), &lighting, t, info.scale, width, height, 0, height,
                    framebufferDev, stream),
          "runRaymarchingKernel");
}

// vr_render_aa: the frame at samples x samples (1, 2, 4 or 8 per axis) samples per pixel, box-filtered
// with round half up -- runRaymarchingKernel of the (samples * width) x (samples * height) frame
// into fineDev (vr_aa_fine_words(width, height, samples) words, the caller's), resolved on the same
// stream into framebufferDev (width * height words) and/or rgb8Dev (3 bytes per pixel); asynchronous.
inline void runRaymarchingKernelAA(uint32_t width, uint32_t height, uint32_t samples, RayMarchAlgorithm algo,
                                   const Camera& camera, const VoxelSceneInfo& info, const DeviceScene& scene,
                                   const vr_lighting& lighting, uint32_t* fineDev, uint32_t* framebufferDev,
                                   uint8_t* rgb8Dev = nullptr, void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    check(vr_render_aa(scene.get(), (vr_algo)algo, &camera.raw(), &lighting, t, info.scale, width, height, samples, 0,
                       height, fineDev, vr_aa_fine_words(width, height, samples), framebufferDev, rgb8Dev, stream),
          "runRaymarchingKernelAA");
}

// vr_resolve: the filter alone, for any fine frame of (samples * width) x (samples * rows) words
// already on the device (a render, a frame of shadeLights words, an assembled multi-GPU frame);
// asynchronous, allocates nothing.
inline void resolve(const uint32_t* fineDev, uint32_t width, uint32_t rows, uint32_t samples, uint32_t* framebufferDev,
                    uint8_t* rgb8Dev = nullptr, void* stream = nullptr) {
    check(vr_resolve(fineDev, width, rows, samples, framebufferDev, rgb8Dev, stream), "resolve");
}

// vr_pick: the hit behind each pixel (px[i], py[i]) of the frame runRaymarchingKernel renders
// for the same arguments -- the voxel (what vr_scene_edit takes), the reference's shading
// normal and the hit point.  Host arrays in, host records out; returns when they are written.
inline std::vector<vr_hit> pick(uint32_t width, uint32_t height, RayMarchAlgorithm algo, const Camera& camera,
                                const VoxelSceneInfo& info, const DeviceScene& scene, const std::vector<uint32_t>& px,
                                const std::vector<uint32_t>& py, void* stream = nullptr) {
    if (px.size() != py.size()) throw Error(VR_E_INVALID, "pick: px and py lengths differ");
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<vr_hit> hits(px.size());
    check(vr_pick(scene.get(), (vr_algo)algo, &camera.raw(), t, info.scale, width, height, px.data(), py.data(), px.size(),
                  0, hits.data(), 0, stream),
          "pick");
    return hits;
}

// vr_scene_lookup: the stored colour of each world voxel xyz[3i..3i+2] (what pick()'s `voxel` and
// vr_scene_edit use), or VR_VOXEL_ABSENT -- e.g. whether a pick's voxel + normal is free to build
// on.  Host array in, host colours out; returns when they are written.
inline std::vector<uint32_t> lookup(const DeviceScene& scene, const std::vector<int32_t>& xyz, void* stream = nullptr) {
    if (xyz.size() % 3 != 0) throw Error(VR_E_INVALID, "lookup: xyz needs three coordinates per voxel");
    std::vector<uint32_t> rgb(xyz.size() / 3);
    check(vr_scene_lookup(scene.get(), xyz.data(), rgb.size(), 0, rgb.data(), 0, stream), "lookup");
    return rgb;
}

// vr_scene_paint: recolour the stored voxels among xyz in place (later edits of a coordinate win);
// returns how many of the edits named a voxel that is not stored (they do nothing).  The scene's
// views keep their learned orders: a painter's loop is pick -> paint -> render.
inline size_t paint(DeviceScene& scene, const std::vector<int32_t>& xyz, const std::vector<uint32_t>& rgb,
                    void* stream = nullptr) {
    if (xyz.size() != 3 * rgb.size()) throw Error(VR_E_INVALID, "paint: xyz and rgb lengths differ");
    size_t absent = 0;
    check(vr_scene_paint(scene.get(), xyz.data(), rgb.data(), rgb.size(), 0, stream, &absent), "paint");
    return absent;
}

// vr_trace: the closest hit of each ray (any origin, any direction length), as vr_hit records --
// what pick() gives for a pixel, for rays that are no pixel of a camera.  Host arrays in, host
// records out; returns when they are written.  The order never changes a record.
inline std::vector<vr_hit> trace(RayMarchAlgorithm algo, const VoxelSceneInfo& info, const DeviceScene& scene,
                                 const std::vector<vr_ray>& rays, vr_trace_order order = VR_TRACE_ORDER_AUTO,
                                 void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<vr_hit> hits(rays.size());
    check(vr_trace(scene.get(), (vr_algo)algo, t, info.scale, rays.data(), rays.size(), 0, hits.data(), 0, (uint32_t)order,
                   stream),
          "trace");
    return hits;
}

// vr_shade: the colour runRaymarchingKernel writes for a pixel whose ray is rays[i] (0x00RRGGBB:
// lit, and shadowed when lighting.use_shadows; 0 for a miss) -- for rays that are no pixel of a
// camera.  hits (optional): filled with the records trace() gives for the same rays, from the
// same walk.  Host arrays in, host arrays out; returns when they are written.
inline std::vector<uint32_t> shade(RayMarchAlgorithm algo, const VoxelSceneInfo& info, const vr_lighting& lighting,
                                   const DeviceScene& scene, const std::vector<vr_ray>& rays,
                                   std::vector<vr_hit>* hits = nullptr, vr_trace_order order = VR_TRACE_ORDER_AUTO,
                                   void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> colors(rays.size());
    if (hits) hits->assign(rays.size(), vr_hit{});
    check(vr_shade(scene.get(), (vr_algo)algo, &lighting, t, info.scale, rays.data(), rays.size(), 0, colors.data(),
                   hits ? hits->data() : nullptr, 0, (uint32_t)order, stream),
          "shade");
    return colors;
}

// vr_shade_lights: shade() under several lights (at most VR_MAX_LIGHTS) and an optional ambient
// term (three floats, or nullptr), from one primary walk per ray: the lights' words and the
// ambient term summed per channel with a clamp at 255.  hits as for shade().  Host arrays in, host
// arrays out; returns when they are written.
inline std::vector<uint32_t> shadeLights(RayMarchAlgorithm algo, const VoxelSceneInfo& info,
                                         const std::vector<vr_lighting>& lights, const float* ambient,
                                         const DeviceScene& scene, const std::vector<vr_ray>& rays,
                                         std::vector<vr_hit>* hits = nullptr, vr_trace_order order = VR_TRACE_ORDER_AUTO,
                                         void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> colors(rays.size());
    if (hits) hits->assign(rays.size(), vr_hit{});
    check(vr_shade_lights(scene.get(), (vr_algo)algo, lights.data(), lights.size(), ambient, t, info.scale, rays.data(),
                          rays.size(), 0, colors.data(), hits ? hits->data() : nullptr, 0, (uint32_t)order, stream),
          "shadeLights");
    return colors;
}

// vr_occlusion: voxel ambient occlusion of hit records (pick(), trace(), shade()'s, or made up): how
// open each hit's face is at the hit point, 0..255 (VR_AO_OPEN = 255).  Host records in, host
// values out; returns when they are written.
inline std::vector<uint32_t> occlusion(const DeviceScene& scene, const std::vector<vr_hit>& hits, void* stream = nullptr) {
    std::vector<uint32_t> ao(hits.size());
    check(vr_occlusion(scene.get(), hits.data(), hits.size(), 0, ao.data(), 0, stream), "occlusion");
    return ao;
}

// vr_shade_lights_ao: shadeLights() with the ambient term (VR_AO_AMBIENT) or the whole word
// (VR_AO_ALL) scaled by the factor aoStrength (0..255) makes of each hit's occlusion; aoOut (or
// nullptr) receives the occlusion values.
inline std::vector<uint32_t> shadeLightsAo(RayMarchAlgorithm algo, const VoxelSceneInfo& info,
                                           const std::vector<vr_lighting>& lights, const float* ambient,
                                           const DeviceScene& scene, const std::vector<vr_ray>& rays, uint32_t aoStrength,
                                           vr_ao_apply aoApply = VR_AO_AMBIENT, std::vector<uint32_t>* aoOut = nullptr,
                                           std::vector<vr_hit>* hits = nullptr, vr_trace_order order = VR_TRACE_ORDER_AUTO,
                                           void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> colors(rays.size());
    if (hits) hits->assign(rays.size(), vr_hit{});
    if (aoOut) aoOut->assign(rays.size(), VR_AO_OPEN);
    check(vr_shade_lights_ao(scene.get(), (vr_algo)algo, lights.data(), lights.size(), ambient, t, info.scale, rays.data(),
                             rays.size(), 0, colors.data(), hits ? hits->data() : nullptr, 0, (uint32_t)order, stream,
                             aoStrength, (uint32_t)aoApply, aoOut ? aoOut->data() : nullptr),
          "shadeLightsAo");
    return colors;
}

// vr_bounce_rays: the mirror bounce of rays[i] at the hit record hits[i] (origin the hit point in
// world units, direction the incoming one with the sign of the normal's axis flipped); an all-NaN
// ray for a record that is no VOXEL hit -- mask what you trace by the records' status.
inline std::vector<vr_ray> bounceRays(const VoxelSceneInfo& info, const std::vector<vr_ray>& rays,
                                      const std::vector<vr_hit>& hits, int device = 0, void* stream = nullptr) {
    if (rays.size() != hits.size()) throw Error(VR_E_INVALID, "bounceRays: rays and hits lengths differ");
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<vr_ray> out(rays.size());
    check(vr_bounce_rays(device, t, info.scale, rays.data(), hits.data(), rays.size(), 0, out.data(), 0, stream), "bounceRays");
    return out;
}

// vr_shade_lights_reflect: shadeLightsAo() (aoStrength 0: shadeLights()) with mirror reflections --
// rays whose hit voxel has (stored colour & mirrorMask) == mirrorValue bounce up to `bounces` times
// (at most VR_MAX_BOUNCES), every depth shaded as the first, and the words are blended from the back
// by reflectivity (0..255).  hits and aoOut are the first hit's.  The descent stays on the device.
inline std::vector<uint32_t> shadeLightsReflect(RayMarchAlgorithm algo, const VoxelSceneInfo& info,
                                                const std::vector<vr_lighting>& lights, const float* ambient,
                                                const DeviceScene& scene, const std::vector<vr_ray>& rays,
                                                uint32_t reflectivity, uint32_t bounces = 1, uint32_t mirrorMask = 0,
                                                uint32_t mirrorValue = 0, uint32_t aoStrength = 0,
                                                vr_ao_apply aoApply = VR_AO_AMBIENT, std::vector<uint32_t>* aoOut = nullptr,
                                                std::vector<vr_hit>* hits = nullptr,
                                                vr_trace_order order = VR_TRACE_ORDER_AUTO, void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> colors(rays.size());
    if (hits) hits->assign(rays.size(), vr_hit{});
    if (aoOut) aoOut->assign(rays.size(), VR_AO_OPEN);
    check(vr_shade_lights_reflect(scene.get(), (vr_algo)algo, lights.data(), lights.size(), ambient, t, info.scale,
                                  rays.data(), rays.size(), 0, colors.data(), hits ? hits->data() : nullptr, 0,
                                  (uint32_t)order, stream, aoStrength, (uint32_t)aoApply, aoOut ? aoOut->data() : nullptr,
                                  reflectivity, bounces, mirrorMask, mirrorValue),
          "shadeLightsReflect");
    return colors;
}

// vr_atmosphere_default: a daylight sky with up = (0, 1, 0), fog off.
inline vr_atmosphere atmosphereDefault() {
    vr_atmosphere atm;
    check(vr_atmosphere_default(&atm), "atmosphereDefault");
    return atm;
}

// vr_atmosphere_apply: colors[i] under the atmosphere -- the sky in the direction of rays[i] where
// hits[i] is a MISS (VR_ATMOS_SKY), colors[i] blended towards the fog's colour by the distance from
// rays[i]'s origin to the hit point where it is a VOXEL record (VR_ATMOS_FOG), colors[i] otherwise.
inline std::vector<uint32_t> atmosphereApply(const VoxelSceneInfo& info, const vr_atmosphere& atm,
                                             const std::vector<vr_ray>& rays, const std::vector<vr_hit>& hits,
                                             const std::vector<uint32_t>& colors, int device = 0, void* stream = nullptr) {
    if (rays.size() != hits.size() || rays.size() != colors.size())
        throw Error(VR_E_INVALID, "atmosphereApply: rays, hits and colors lengths differ");
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> out(rays.size());
    check(vr_atmosphere_apply(device, &atm, t, info.scale, rays.data(), hits.data(), colors.data(), rays.size(), 0, out.data(), 0,
                              stream),
          "atmosphereApply");
    return out;
}

// vr_shade_lights_atmosphere: shadeLightsReflect() (reflectivity 0: shadeLightsAo()) under a sky and
// a distance fog -- at every depth a miss shows the sky in the direction of that depth's ray and a
// hit fades with the length of its leg, before the depths are blended.  hits and aoOut are untouched.
inline std::vector<uint32_t> shadeLightsAtmosphere(RayMarchAlgorithm algo, const VoxelSceneInfo& info,
                                                   const std::vector<vr_lighting>& lights, const float* ambient,
                                                   const DeviceScene& scene, const std::vector<vr_ray>& rays,
                                                   const vr_atmosphere& atm, uint32_t reflectivity = 0, uint32_t bounces = 1,
                                                   uint32_t mirrorMask = 0, uint32_t mirrorValue = 0, uint32_t aoStrength = 0,
                                                   vr_ao_apply aoApply = VR_AO_AMBIENT, std::vector<uint32_t>* aoOut = nullptr,
                                                   std::vector<vr_hit>* hits = nullptr,
                                                   vr_trace_order order = VR_TRACE_ORDER_AUTO, void* stream = nullptr) {
    float t[3] = {info.translationVector.x, info.translationVector.y, info.translationVector.z};
    std::vector<uint32_t> colors(rays.size());
    if (hits) hits->assign(rays.size(), vr_hit{});
    if (aoOut) aoOut->assign(rays.size(), VR_AO_OPEN);
    check(vr_shade_lights_atmosphere(scene.get(), (vr_algo)algo, lights.data(), lights.size(), ambient, t, info.scale,
                                     rays.data(), rays.size(), 0, colors.data(), hits ? hits->data() : nullptr, 0,
                                     (uint32_t)order, stream, aoStrength, (uint32_t)aoApply, aoOut ? aoOut->data() : nullptr,
                                     reflectivity, bounces, mirrorMask, mirrorValue, &atm),
          "shadeLightsAtmosphere");
    return colors;
}

// vr_camera_rays: the rays a render or pick walks for pixels (px[i], py[i]) of a width x height
// frame; trace(camera_rays(px, py)) equals pick(px, py) for pixels inside the frame.
inline std::vector<vr_ray> camera_rays(uint32_t width, uint32_t height, const Camera& camera, const std::vector<uint32_t>& px,
                                       const std::vector<uint32_t>& py, int device = 0, void* stream = nullptr) {
    if (px.size() != py.size()) throw Error(VR_E_INVALID, "camera_rays: px and py lengths differ");
    std::vector<vr_ray> rays(px.size());
    check(vr_camera_rays(device, &camera.raw(), width, height, px.data(), py.data(), px.size(), 0, rays.data(), 0, stream),
          "camera_rays");
    return rays;
}

}  // namespace vrx
