// VoxelRaymarcher CLI -- the reference's command line (main/Main.cu:176-229)
// on the MI355X renderer:
//   VoxelRaymarcher [scale] {hashtable|vcs} {original|longestaxis}
//                   [--scene resources/scene.vox] [--width 1920] [--height 1080]
//                   [--out output.png] [--device 0] [--synth N] [--repeat K]
//                   [--write-vxb F]   (convert the scene to the .vxb sidecar and exit)
//                   [--no-shadows] [--point-light X,Y,Z] [--light-dir X,Y,Z] [--light-color R,G,B]
//                   (the setupConstantValues toggles, Main.cu:26-42, as flags)
//                   [--gpus N]   (the frame image-tiled over devices 0..N-1 of the node and
//                                 gathered to device 0 over RCCL: multi_gpu.h; N = 1 takes the
//                                 same RCCL path with one rank)
//                   [--pick X,Y]...  (after the frame is rendered: one line per pick with the
//                                 voxel, stored colour and shading normal behind pixel (X, Y),
//                                 y = 0 the top row -- vr_pick; not with --gpus N > 1)
//                   [--trace OX,OY,OZ,DX,DY,DZ]...  (beside the picks: one line per ray with the
//                                 voxel, colour, normal and hit point it reaches from world origin
//                                 O in direction D (any length) -- vr_trace, with the scale above
//                                 and a zero translation; not with --gpus N > 1)
//                   [--shade OX,OY,OZ,DX,DY,DZ]...  (after the traces: one line per ray with the colour
//                                 the render would give it -- vr_shade, with the run's scale and
//                                 lighting flags and a zero translation -- then the --trace text
//                                 of its hit; not with --gpus N > 1)
//                   [--lookup X,Y,Z]...  (after the shades: one line per query with the colour
//                                 stored at world voxel (X, Y, Z), signed integers, or "absent"
//                                 -- vr_scene_lookup; not with --gpus N > 1)
//                   [--paint X,Y,Z,RRGGBB]...  (before the render, so output.png shows it: set
//                                 the colour (hex) of stored voxel (X, Y, Z) -- vr_scene_paint, all
//                                 of them as one batch in the order given; a voxel that is not
//                                 stored gets a line on stderr; not with --gpus)
//                   [--add-light DX,DY,DZ,R,G,B]...  (one more directional light of colour R,G,B, its
//                                 direction normalised as --light-dir's, its shadows following
//                                 --no-shadows) [--ambient R,G,B]  (an ambient term): with either,
//                                 output.png is the vr_shade_lights frame -- the run's own light
//                                 first, then the added ones, the terms summed per channel with a
//                                 clamp at 255 -- and a line "lights <N> ambient <r> <g> <b>" is
//                                 printed before "Wrote"; not with --gpus
//                   [--ao STRENGTH] [--ao-all]  (voxel ambient occlusion, vr_shade_lights_ao: STRENGTH
//                                 0..255 scales the ambient term -- with --ao-all the whole word --
//                                 of the lights frame by each hit's occlusion; --ao selects the
//                                 lights frame as --ambient does, and the "lights" line then ends
//                                 in " ao <strength> <ambient|all>"; not with --gpus)
//                   [--reflect K] [--bounces B] [--mirror RRGGBB]  (mirror reflections,
//                                 vr_shade_lights_reflect: K 0..255 blends up to B (default 1, at most 4)
//                                 bounces into the lights frame's words; --mirror makes only voxels
//                                 of that stored colour (hex) mirrors, the default is every voxel;
//                                 --reflect selects the lights frame as --ambient does and works with
//                                 --add-light, --ambient, --ao and --aa; the "lights" line then ends in
//                                 " reflect <K> bounces <B> mirror <every|rrggbb>"; not with --gpus)
//                   [--sky ZZZZZZ,HHHHHH,NNNNNN] [--fog RRGGBB,START,END]  (sky and distance fog,
//                                 vr_shade_lights_atmosphere: --sky gives the colours (hex) a ray that
//                                 hits nothing shows straight up, level and straight down, up being
//                                 (0, 1, 0); --fog blends every hit towards RRGGBB between START and END
//                                 world units from its ray's origin; a colour byte b is handed over as
//                                 the float (b + 0.5) / 255, which the library truncates back to b;
//                                 either selects the lights frame as --ambient does and works with
//                                 --add-light, --ambient, --ao, --reflect and --aa; the "lights" line
//                                 then ends in " sky <zzzzzz> <hhhhhh> <nnnnnn>" and / or
//                                 " fog <rrggbb> <start> <end>"; not with --gpus)
//                   [--aa S]     (S = 1, 2, 4 or 8 samples per axis: output.png is the resolved frame --
//                                 the (S * width) x (S * height) render box-filtered with round half
//                                 up, vr_render_aa; with --add-light / --ambient the lights frame is
//                                 made at that size and resolved, vr_resolve; the time printed is
//                                 the fine render plus the filter; not with --gpus)
// Defaults follow Main.cu: VCS unless "hashtable", longest axis unless
// "original" (:45-68), 1920x1080 (:195-196), camera (6,2,6)->(0,0,-1) fov 60
// (:199), translation 0 (:215), scene file resources/scene.vox (:96-103).
// The kernel time is measured with HIP events (the reference: std::chrono
// around launch + sync, :114,160-162).
#include <hip/hip_runtime.h>

#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "multi_gpu.h"
#include "vr.hpp"

namespace {

// "x,y,z" -> 3 floats; false on malformed input.
bool parse_vec3(const char* s, float out[3]) {
    char* end = nullptr;
    for (int i = 0; i < 3; ++i) {
        out[i] = std::strtof(s, &end);
        if (end == s) return false;
        s = end;
        if (i < 2) {
            if (*s != ',') return false;
            ++s;
        }
    }
    return *s == 0;
}

// "ox,oy,oz,dx,dy,dz" -> a vr_ray; false on malformed input.
bool parse_ray(const char* s, vr_ray& ray) {
    float f[6];
    char* end = nullptr;
    for (int i = 0; i < 6; ++i) {
        f[i] = std::strtof(s, &end);
        if (end == s) return false;
        s = end;
        if (i < 5) {
            if (*s != ',') return false;
            ++s;
        }
    }
    ray = vr_ray{{f[0], f[1], f[2]}, 0u, {f[3], f[4], f[5]}, 0u};
    return *s == 0;
}

// "X,Y" -> two unsigned 32-bit decimals; false on malformed input.
bool parse_pixel(const char* s, uint32_t& x, uint32_t& y) {
    uint32_t* out[2] = {&x, &y};
    for (int i = 0; i < 2; ++i) {
        if (*s < '0' || *s > '9') return false;
        char* end = nullptr;
        const unsigned long long v = std::strtoull(s, &end, 10);
        if (v > 0xFFFFFFFFull) return false;
        *out[i] = (uint32_t)v;
        s = end;
        if (i == 0) {
            if (*s != ',') return false;
            ++s;
        }
    }
    return *s == 0;
}

// "X,Y,Z" -> three signed 32-bit decimals, then (colour != null) ",RRGGBB" -> a hex colour below
// 2^32 (vr_scene_paint refuses one above 24 bits); false on malformed input.
bool parse_voxel(const char* s, int32_t xyz[3], uint32_t* colour) {
    char* end = nullptr;
    for (int i = 0; i < 3; ++i) {
        const long long v = std::strtoll(s, &end, 10);
        if (end == s || v < INT32_MIN || v > INT32_MAX) return false;
        xyz[i] = (int32_t)v;
        s = end;
        if (i < 2 || colour) {
            if (*s != ',') return false;
            ++s;
        }
    }
    if (colour) {
        if (*s == '-' || *s == '+' || *s == ' ') return false;
        const unsigned long long v = std::strtoull(s, &end, 16);
        if (end == s || v > 0xFFFFFFFFull) return false;
        *colour = (uint32_t)v;
        s = end;
    }
    return *s == 0;
}

bool is_integer(const char* s) {
    if (!s || !*s) return false;
    if (*s == '-' || *s == '+') ++s;
    if (!*s) return false;
    for (; *s; ++s)
        if (*s < '0' || *s > '9') return false;
    return true;
}

#define HIP_OK(x)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            std::cerr << #x << ": " << hipGetErrorString(e_) << std::endl;               \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

}  // namespace

int main(int argc, char* argv[]) {
    std::vector<const char*> pos;
    std::string scene_path = "resources/scene.vox", out_path = "output.png", vxb_path;
    uint32_t width = 1920, height = 1080, synth = 0;
    int device = 0, repeat = 1, gpus = 0;
    uint32_t aa = 0;                         // --aa S: samples per axis (0: not given)
    bool multi = false;                      // --gpus given: the RCCL-tiled frame
    bool shadows = true, point_light = false, has_dir = false;
    std::vector<uint32_t> pick_x, pick_y;    // --pick X,Y (repeatable)
    std::vector<vr_ray> trace_rays;          // --trace OX,OY,OZ,DX,DY,DZ (repeatable)
    std::vector<vr_ray> shade_rays;          // --shade OX,OY,OZ,DX,DY,DZ (repeatable)
    std::vector<int32_t> lookup_xyz;         // --lookup X,Y,Z (repeatable)
    std::vector<int32_t> paint_xyz;          // --paint X,Y,Z,RRGGBB (repeatable)
    std::vector<uint32_t> paint_rgb;
    std::vector<vr_ray> added_lights;        // --add-light DX,DY,DZ,R,G,B (repeatable): direction, colour
    bool has_ambient = false;                // --ambient R,G,B
    float ambient[3] = {0.0f, 0.0f, 0.0f};
    bool has_ao = false, ao_all = false;     // --ao STRENGTH, --ao-all
    uint32_t ao_strength = 0;
    bool has_reflect = false, has_bounces = false, has_mirror = false;     // --reflect K, --bounces B, --mirror RRGGBB
    uint32_t reflect_k = 0, bounces = 1, mirror_rgb = 0;
    bool has_sky = false, has_fog = false;   // --sky ZZZZZZ,HHHHHH,NNNNNN, --fog RRGGBB,START,END
    uint32_t sky_rgb[3] = {0, 0, 0}, fog_rgb = 0;
    float fog_start = 0.0f, fog_end = 0.0f;
    // RRGGBB: one to six hexadecimal digits and nothing else
    auto parse_rgb = [](const std::string& v, uint32_t& out) {
        if (v.empty() || v.size() > 6) return false;
        for (const char c : v)
            if (!std::isxdigit((unsigned char)c)) return false;
        out = (uint32_t)std::strtoul(v.c_str(), nullptr, 16);
        return true;
    };
    auto split_commas = [](const char* v) {
        std::vector<std::string> parts(1);
        for (const char* c = v; *c; ++c) {
            if (*c == ',') parts.emplace_back();
            else parts.back().push_back(*c);
        }
        return parts;
    };
    float light_pos[3] = {10.0f, 10.0f, -10.0f}, light_dir[3] = {1.0f, 1.0f, 1.0f}, light_color[3] = {1.0f, 1.0f, 1.0f};
    auto vec3 = [](const char* name, const char* v, float out[3]) {
        if (!parse_vec3(v, out)) { std::cerr << name << " needs X,Y,Z" << std::endl; std::exit(2); }
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << name << " needs a value" << std::endl; std::exit(2); }
            return argv[++i];
        };
        if (a == "--scene") scene_path = next("--scene");
        else if (a == "--out") out_path = next("--out");
        else if (a == "--width") width = (uint32_t)std::strtoul(next("--width"), nullptr, 10);
        else if (a == "--height") height = (uint32_t)std::strtoul(next("--height"), nullptr, 10);
        else if (a == "--device") device = std::atoi(next("--device"));
        else if (a == "--synth") synth = (uint32_t)std::strtoul(next("--synth"), nullptr, 10);
        else if (a == "--gpus") { multi = true; gpus = std::atoi(next("--gpus")); }
        else if (a == "--aa") {
            const char* v = next("--aa");
            if (std::strcmp(v, "1") && std::strcmp(v, "2") && std::strcmp(v, "4") && std::strcmp(v, "8")) {
                std::cerr << "--aa needs 1, 2, 4 or 8 (samples per axis)" << std::endl;
                std::exit(2);
            }
            aa = (uint32_t)std::atoi(v);
        }
        else if (a == "--repeat") repeat = std::max(1, std::atoi(next("--repeat")));
        else if (a == "--write-vxb") vxb_path = next("--write-vxb");
        else if (a == "--no-shadows") shadows = false;
        else if (a == "--point-light") { point_light = true; vec3("--point-light", next("--point-light"), light_pos); }
        else if (a == "--light-dir") { has_dir = true; vec3("--light-dir", next("--light-dir"), light_dir); }
        else if (a == "--light-color") vec3("--light-color", next("--light-color"), light_color);
        else if (a == "--pick") {
            const char* v = next("--pick");
            uint32_t x = 0, y = 0;
            if (!parse_pixel(v, x, y)) {
                std::cerr << "--pick needs X,Y (pixel coordinates)" << std::endl;
                std::exit(2);
            }
            pick_x.push_back(x);
            pick_y.push_back(y);
        }
        else if (a == "--trace") {
            vr_ray ray;
            if (!parse_ray(next("--trace"), ray)) {
                std::cerr << "--trace needs OX,OY,OZ,DX,DY,DZ" << std::endl;
                std::exit(2);
            }
            trace_rays.push_back(ray);
        }
        else if (a == "--shade") {
            vr_ray ray;
            if (!parse_ray(next("--shade"), ray)) {
                std::cerr << "--shade needs OX,OY,OZ,DX,DY,DZ" << std::endl;
                std::exit(2);
            }
            shade_rays.push_back(ray);
        }
        else if (a == "--lookup") {
            int32_t v[3];
            if (!parse_voxel(next("--lookup"), v, nullptr)) {
                std::cerr << "--lookup needs X,Y,Z (voxel coordinates)" << std::endl;
                std::exit(2);
            }
            lookup_xyz.insert(lookup_xyz.end(), v, v + 3);
        }
        else if (a == "--paint") {
            int32_t v[3];
            uint32_t c = 0;
            if (!parse_voxel(next("--paint"), v, &c)) {
                std::cerr << "--paint needs X,Y,Z,RRGGBB (voxel coordinates and a hex colour)" << std::endl;
                std::exit(2);
            }
            paint_xyz.insert(paint_xyz.end(), v, v + 3);
            paint_rgb.push_back(c);
        }
        else if (a == "--add-light") {
            vr_ray l;                        // (six floats: the direction in `origin`, the colour in `direction`)
            if (!parse_ray(next("--add-light"), l)) {
                std::cerr << "--add-light needs DX,DY,DZ,R,G,B (a direction and a colour)" << std::endl;
                std::exit(2);
            }
            added_lights.push_back(l);
        }
        else if (a == "--ambient") {
            if (!parse_vec3(next("--ambient"), ambient)) {
                std::cerr << "--ambient needs R,G,B" << std::endl;
                std::exit(2);
            }
            has_ambient = true;
        }
        else if (a == "--ao") {
            const char* v = next("--ao");
            if (!is_integer(v) || std::atol(v) < 0 || std::atol(v) > 255) {
                std::cerr << "--ao needs STRENGTH (0..255)" << std::endl;
                std::exit(2);
            }
            ao_strength = (uint32_t)std::atol(v);
            has_ao = true;
        }
        else if (a == "--ao-all") ao_all = true;
        else if (a == "--reflect") {
            const char* v = next("--reflect");
            if (!is_integer(v) || std::atol(v) < 0 || std::atol(v) > 255) {
                std::cerr << "--reflect needs K (0..255)" << std::endl;
                std::exit(2);
            }
            reflect_k = (uint32_t)std::atol(v);
            has_reflect = true;
        }
        else if (a == "--bounces") {
            const char* v = next("--bounces");
            if (!is_integer(v) || std::atol(v) < 0 || std::atol(v) > (long)VR_MAX_BOUNCES) {
                std::cerr << "--bounces needs B (0.." << VR_MAX_BOUNCES << ")" << std::endl;
                std::exit(2);
            }
            bounces = (uint32_t)std::atol(v);
            has_bounces = true;
        }
        else if (a == "--mirror") {
            const char* v = next("--mirror");
            char* end = nullptr;
            const unsigned long c = std::strtoul(v, &end, 16);
            if (*v == '\0' || *end != '\0' || std::strlen(v) > 6) {
                std::cerr << "--mirror needs RRGGBB (a stored colour, hex)" << std::endl;
                std::exit(2);
            }
            mirror_rgb = (uint32_t)c;
            has_mirror = true;
        }
        else if (a == "--sky") {
            const std::vector<std::string> parts = split_commas(next("--sky"));
            if (parts.size() != 3 || !parse_rgb(parts[0], sky_rgb[0]) || !parse_rgb(parts[1], sky_rgb[1]) ||
                !parse_rgb(parts[2], sky_rgb[2])) {
                std::cerr << "--sky needs ZZZZZZ,HHHHHH,NNNNNN (zenith, horizon and nadir colours, hex)" << std::endl;
                std::exit(2);
            }
            has_sky = true;
        }
        else if (a == "--fog") {
            const std::vector<std::string> parts = split_commas(next("--fog"));
            char *e1 = nullptr, *e2 = nullptr;
            bool ok = parts.size() == 3 && parse_rgb(parts[0], fog_rgb) && !parts[1].empty() && !parts[2].empty();
            if (ok) {
                fog_start = std::strtof(parts[1].c_str(), &e1);
                fog_end = std::strtof(parts[2].c_str(), &e2);
                ok = *e1 == '\0' && *e2 == '\0';
            }
            if (!ok) {
                std::cerr << "--fog needs RRGGBB,START,END (the fog's colour, hex, and its bounds in world units)" << std::endl;
                std::exit(2);
            }
            has_fog = true;
        }
        else if (a == "-h" || a == "--help") {
            std::cout << "usage: VoxelRaymarcher [scale] {hashtable|vcs} {original|longestaxis} [--scene F] "
                         "[--width W] [--height H] [--out F] [--device N] [--synth N] [--repeat K] [--write-vxb F] "
                         "[--no-shadows] [--point-light X,Y,Z] [--light-dir X,Y,Z] [--light-color R,G,B] [--gpus N] "
                         "[--pick X,Y]... [--trace OX,OY,OZ,DX,DY,DZ]... [--shade OX,OY,OZ,DX,DY,DZ]... "
                         "[--lookup X,Y,Z]... [--paint X,Y,Z,RRGGBB]... [--add-light DX,DY,DZ,R,G,B]... "
                         "[--ambient R,G,B] [--ao STRENGTH] [--ao-all] [--reflect K] [--bounces B] [--mirror RRGGBB] "
                         "[--sky ZZZZZZ,HHHHHH,NNNNNN] [--fog RRGGBB,START,END] [--aa S]" << std::endl;
            return 0;
        } else pos.push_back(argv[i]);
    }
    if (!vxb_path.empty()) {                 // scene conversion only: no GPU needed
        try {
            vrx::VoxelFile::writeBinary(scene_path, vxb_path);
        } catch (const vrx::Error& e) {
            std::cerr << e.what() << std::endl;
            return 1;
        }
        std::cout << "wrote " << vxb_path << std::endl;
        return 0;
    }
    if (!pick_x.empty() && multi && gpus > 1) {
        std::cerr << "ERROR: --pick is a single-GPU query: not with --gpus " << gpus << std::endl;
        return 2;
    }
    if (!trace_rays.empty() && multi && gpus > 1) {
        std::cerr << "ERROR: --trace is a single-GPU query: not with --gpus " << gpus << std::endl;
        return 2;
    }
    if (!shade_rays.empty() && multi && gpus > 1) {
        std::cerr << "ERROR: --shade is a single-GPU query: not with --gpus " << gpus << std::endl;
        return 2;
    }
    if (!lookup_xyz.empty() && multi && gpus > 1) {
        std::cerr << "ERROR: --lookup is a single-GPU query: not with --gpus " << gpus << std::endl;
        return 2;
    }
    if (!paint_rgb.empty() && multi) {       // (every rank renders a replica of its own)
        std::cerr << "ERROR: --paint changes this process's single-GPU scene: not with --gpus" << std::endl;
        return 2;
    }
    if (ao_all && !has_ao) {
        std::cerr << "ERROR: --ao-all needs --ao STRENGTH" << std::endl;
        return 2;
    }
    if ((has_bounces || has_mirror) && !has_reflect) {
        std::cerr << "ERROR: --bounces and --mirror need --reflect K" << std::endl;
        return 2;
    }
    const bool has_atmos = has_sky || has_fog;
    const bool lights_frame = !added_lights.empty() || has_ambient || has_ao || has_reflect || has_atmos;
    if (lights_frame && multi) {             // (the frame is one device's vr_shade_lights call)
        std::cerr << "ERROR: --add-light, --ambient, --ao, --reflect, --sky and --fog shade a single-GPU frame: not with --gpus"
                  << std::endl;
        return 2;
    }
    if (aa && multi) {                       // (a resolved frame dealt over several GPUs: a later change)
        std::cerr << "ERROR: --aa resolves a single-GPU frame: not with --gpus" << std::endl;
        return 2;
    }
    if (added_lights.size() + 1u > VR_MAX_LIGHTS) {
        std::cerr << "ERROR: --add-light: at most " << (VR_MAX_LIGHTS - 1u) << " added lights" << std::endl;
        return 2;
    }
    // argv[1] = scale (Main.cu:181-186); optional here (README.md:22-25 omits it).
    uint32_t scale = 1;
    size_t p = 0;
    if (p < pos.size() && is_integer(pos[p])) scale = (uint32_t)std::atoi(pos[p++]);
    const char* store_arg = p < pos.size() ? pos[p++] : "";
    const char* algo_arg = p < pos.size() ? pos[p++] : "";
    vrx::StorageType store = vrx::StorageType::VOXEL_CLUSTER_STORE;
    if (std::strcmp(store_arg, "hashtable") == 0) {          // Main.cu:45-55
        std::cout << "Storage Type: Cuckoo Hash Table" << std::endl;
        store = vrx::StorageType::HASH_TABLE;
    } else {
        std::cout << "Storage Type: Voxel Cluster Storage" << std::endl;
    }
    vrx::RayMarchAlgorithm algo = vrx::RayMarchAlgorithm::LONGEST_AXIS;
    if (std::strcmp(algo_arg, "original") == 0) {            // Main.cu:58-68
        std::cout << "Raymarching Algorithm: Original" << std::endl;
        algo = vrx::RayMarchAlgorithm::ORIGINAL;
    } else {
        if (std::strcmp(algo_arg, "optimized") == 0)          // :71-80 launches nothing; we render
            std::cout << "Optimized functions are currently disabled" << std::endl;
        std::cout << "Raymarching Algorithm: Longest Axis" << std::endl;
    }

    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    std::printf("Device Count: %d\n", ndev);                   // pickCudaDevice (:82-94)
    if (device >= ndev) { std::cerr << "no such device" << std::endl; return 1; }
    if (multi && (gpus < 1 || gpus > ndev)) {
        std::cerr << "ERROR: --gpus " << gpus << ": " << ndev << " HIP device(s) visible (need 1.." << ndev << ")"
                  << std::endl;
        return 2;
    }
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    std::printf("Device: %s (%s)\n", prop.name, prop.gcnArchName);
    HIP_OK(hipSetDevice(device));

    try {
        vrx::VoxelSceneCPU cpu;
        if (synth) {
            vr_synth_params sp{synth, 1.0, 0.3, 0.08, 0x256};
            size_t n = 0;
            vrx::check(vr_synth_generate(&sp, nullptr, nullptr, 0, &n), "synth");
            std::vector<int32_t> xyz(3 * n + 3);
            std::vector<uint32_t> rgb(n + 1);
            vrx::check(vr_synth_generate(&sp, xyz.data(), rgb.data(), n, &n), "synth");
            for (size_t i = 0; i < n; ++i) cpu.insertVoxel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], rgb[i]);
        } else {
            vrx::VoxelFile::readVoxelFile(cpu, scene_path);
        }
        vrx::DeviceScene scene = cpu.generateVoxelScene(store, device);
        vr_scene_info info = scene.info();
        uint64_t slots = (uint64_t)info.diameter * info.diameter * info.diameter;
        std::cout << "There are : " << info.region_count << "/" << slots << " regions that are filled" << std::endl;

        // --paint: recolour stored voxels before anything is rendered (vr_scene_paint, one batch)
        if (!paint_rgb.empty() && vrx::paint(scene, paint_xyz, paint_rgb) != 0) {
            const std::vector<uint32_t> stored = vrx::lookup(scene, paint_xyz);
            for (size_t i = 0; i < stored.size(); ++i)
                if (stored[i] == VR_VOXEL_ABSENT)
                    std::cerr << "paint " << paint_xyz[3 * i] << " " << paint_xyz[3 * i + 1] << " " << paint_xyz[3 * i + 2]
                              << " absent: nothing painted" << std::endl;
        }

        float aspect = (float)width / (float)height;             // Main.cu:197
        vrx::Camera camera({6.0f, 2.0f, 6.0f}, {0.0f, 0.0f, -1.0f}, {0.0f, 1.0f, 0.0f}, 60.0f, aspect);
        vrx::VoxelSceneInfo sinfo({0.0f, 0.0f, 0.0f}, scale);
        vr_lighting lit = vrx::defaultLighting();
        if (has_dir) vrx::setLightDirection(lit, light_dir[0], light_dir[1], light_dir[2]);
        for (int i = 0; i < 3; ++i) {
            lit.light_color[i] = light_color[i];
            lit.light_pos[i] = light_pos[i];
        }
        lit.use_point_light = point_light;                       // Main.cu:37
        lit.use_shadows = shadows;                               // Main.cu:40

        // --trace: the closest hit of each given ray (vr_trace), printed after the picks
        auto print_record = [](const vr_hit& h) {      // (the rest of a --trace or --shade line)
            if (h.status == VR_HIT_VOXEL)
                std::printf("voxel %d %d %d color 0x%06X normal %d %d %d point %.9g %.9g %.9g\n", h.voxel[0], h.voxel[1],
                            h.voxel[2], h.color, h.normal[0], h.normal[1], h.normal[2], h.point[0], h.point[1], h.point[2]);
            else
                std::printf("%s\n", h.status == VR_HIT_MISS ? "miss" : "never");
        };
        auto print_traces = [&]() {
            if (trace_rays.empty()) return;
            const std::vector<vr_hit> hits = vrx::trace(algo, sinfo, scene, trace_rays);
            for (size_t i = 0; i < hits.size(); ++i) {
                std::printf("trace %zu ", i);
                print_record(hits[i]);
            }
            std::fflush(stdout);
        };
        // --shade: the colour the render would give each given ray, and its hit (vr_shade, with
        // the run's lighting), printed after the traces
        auto print_shades = [&]() {
            if (shade_rays.empty()) return;
            std::vector<vr_hit> hits;
            const std::vector<uint32_t> colors = vrx::shade(algo, sinfo, lit, scene, shade_rays, &hits);
            for (size_t i = 0; i < colors.size(); ++i) {
                std::printf("shade %zu color 0x%06X ", i, colors[i]);
                print_record(hits[i]);
            }
            std::fflush(stdout);
        };
        // --pick: the hit each picked pixel of the rendered frame was shaded from (vr_pick)
        auto print_picks = [&]() {
            if (pick_x.empty()) return;
            const std::vector<vr_hit> hits = vrx::pick(width, height, algo, camera, sinfo, scene, pick_x, pick_y);
            for (size_t i = 0; i < hits.size(); ++i) {
                const vr_hit& h = hits[i];
                if (h.status == VR_HIT_VOXEL)
                    std::printf("pick %u %u voxel %d %d %d color 0x%06X normal %d %d %d\n", pick_x[i], pick_y[i], h.voxel[0],
                                h.voxel[1], h.voxel[2], h.color, h.normal[0], h.normal[1], h.normal[2]);
                else
                    std::printf("pick %u %u %s\n", pick_x[i], pick_y[i],
                                h.status == VR_HIT_MISS ? "miss" : (h.status == VR_HIT_NEVER ? "never" : "outside"));
            }
            std::fflush(stdout);
        };
        // --lookup: the colour stored at each given voxel (vr_scene_lookup), printed after the shades
        auto print_lookups = [&]() {
            if (lookup_xyz.empty()) return;
            const std::vector<uint32_t> stored = vrx::lookup(scene, lookup_xyz);
            for (size_t i = 0; i < stored.size(); ++i) {
                std::printf("lookup %d %d %d ", lookup_xyz[3 * i], lookup_xyz[3 * i + 1], lookup_xyz[3 * i + 2]);
                if (stored[i] == VR_VOXEL_ABSENT) std::printf("absent\n");
                else std::printf("color 0x%06X\n", stored[i]);
            }
            std::fflush(stdout);
        };
        if (multi) {
            // The frame image-tiled over devices 0..gpus-1, RCCL-gathered to device 0 (multi_gpu.h)
            vrx::MultiGpuFrame mg;
            if (!mg.init(gpus, (vr_store)store, cpu.coords(), cpu.colors(), width, height)) {
                std::cerr << "ERROR: " << mg.error() << std::endl;
                return 1;
            }
            const float t[3] = {sinfo.translationVector.x, sinfo.translationVector.y, sinfo.translationVector.z};
            vrx::MultiGpuTiming best, tm;
            best.frame_ms = 1e30;
            for (int r = 0; r < repeat; ++r) {
                if (!mg.render((vr_algo)algo, camera.raw(), lit, t, sinfo.scale, &tm)) {
                    std::cerr << "ERROR: " << mg.error() << std::endl;
                    return 1;
                }
                if (tm.frame_ms < best.frame_ms) best = tm;
            }
            std::cout << "Execution Time for Ray Marching Algorithm is: " << (long long)(best.frame_ms * 1000.0)
                      << " microseconds on " << gpus << " GPU(s), tiled + RCCL gather + assembly ("
                      << (double)width * height / (best.frame_ms * 1e3) << " Mrays/s)" << std::endl;
            for (size_t i = 0; i < best.rank_render_ms.size(); ++i)
                std::cout << "  rank " << i << " render " << (long long)(best.rank_render_ms[i] * 1000.0f)
                          << " microseconds" << std::endl;
            print_picks();                   // (--gpus 1: the scene of this process's device)
            print_traces();
            print_shades();
            print_lookups();
            std::vector<uint8_t> host;
            if (!mg.download(host)) {
                std::cerr << "ERROR: " << mg.error() << std::endl;
                return 1;
            }
            if (vr_png_write(out_path.c_str(), host.data(), width, height, 3, 6) != VR_OK) {
                std::cerr << "ERROR: Failed to write image to: " << out_path << " (" << vr_last_error() << ")" << std::endl;
                return 1;
            }
            std::cout << "Wrote " << out_path << std::endl;
            return 0;
        }
        uint32_t* fb = nullptr;
        uint8_t* rgb = nullptr;
        // --aa: the fine frame of S x S samples per pixel, resolved into fb
        const uint32_t S = aa ? aa : 1u;
        const uint64_t fine_words = aa ? vr_aa_fine_words(width, height, S) : 0;
        uint32_t* fine = nullptr;
        if (aa) {
            if (fine_words == 0) {
                std::cerr << "ERROR: --aa " << S << ": the fine frame of " << width << "x" << height
                          << " is too large (at most 65536 samples per axis)" << std::endl;
                return 2;
            }
            HIP_OK(hipMalloc(&fine, fine_words * 4));
        }
        HIP_OK(hipMalloc(&fb, (size_t)width * height * 4));
        HIP_OK(hipMalloc(&rgb, (size_t)width * height * 3));
        hipEvent_t e0, e1;
        HIP_OK(hipEventCreate(&e0));
        HIP_OK(hipEventCreate(&e1));
        float best_ms = 1e30f;
        for (int r = 0; r < repeat; ++r) {
            HIP_OK(hipEventRecord(e0, nullptr));
            if (aa) vrx::runRaymarchingKernelAA(width, height, S, algo, camera, sinfo, scene, lit, fine, fb, nullptr, nullptr);
            else vrx::runRaymarchingKernel(width, height, algo, camera, sinfo, scene, lit, fb, nullptr);
            HIP_OK(hipEventRecord(e1, nullptr));
            HIP_OK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, e0, e1));
            best_ms = std::min(best_ms, ms);
        }
        std::cout << hipGetErrorString(hipGetLastError()) << std::endl;
        std::cout << "Execution Time for Ray Marching Algorithm is: " << (long long)(best_ms * 1000.0f)
                  << " microseconds (" << (double)width * height / (best_ms * 1e3) << " Mrays/s)" << std::endl;
        print_picks();
        print_traces();
        print_shades();
        print_lookups();
        // --add-light / --ambient: the frame written is the vr_shade_lights one -- the camera rays
        // of every pixel in 8x8-tile order (the order in which a frame's rays walk fastest), the
        // run's own light first and then the added ones, the words scattered back to their pixels
        // (with --aa: the frame of S * width x S * height pixels, resolved into fb)
        if (lights_frame) {
            const uint32_t lw = S * width, lh = S * height;
            std::vector<vr_lighting> lights(1, lit);
            for (const vr_ray& l : added_lights) {
                vr_lighting k = vrx::defaultLighting();
                vrx::setLightDirection(k, l.origin[0], l.origin[1], l.origin[2]);
                for (int i = 0; i < 3; ++i) k.light_color[i] = l.direction[i];
                k.use_shadows = shadows;
                lights.push_back(k);
            }
            const size_t n = (size_t)lw * lh;
            std::vector<uint32_t> px, py;
            px.reserve(n);
            py.reserve(n);
            for (uint32_t ty = 0; ty < lh; ty += 8)
                for (uint32_t tx = 0; tx < lw; tx += 8)
                    for (uint32_t y = ty; y < std::min(ty + 8u, lh); ++y)
                        for (uint32_t x = tx; x < std::min(tx + 8u, lw); ++x) {
                            px.push_back(x);
                            py.push_back(y);
                        }
            vr_ray* rays = nullptr;
            HIP_OK(hipMalloc(&rays, n * sizeof(vr_ray)));
            const float t[3] = {sinfo.translationVector.x, sinfo.translationVector.y, sinfo.translationVector.z};
            std::vector<uint32_t> words(n), frame(n);
            int rc = vr_camera_rays(device, &camera.raw(), lw, lh, px.data(), py.data(), n, 0, rays, 1, nullptr);
            if (rc == VR_OK && has_atmos) {
                // (a byte b as (b + 0.5) / 255: the library's truncation gives b back)
                vr_atmosphere atm = vrx::atmosphereDefault();
                const auto put = [](float out[3], uint32_t rgb) {
                    for (int c = 0; c < 3; ++c) out[c] = ((float)((rgb >> (16 - 8 * c)) & 0xFFu) + 0.5f) / 255.0f;
                };
                if (has_sky) {
                    put(atm.zenith, sky_rgb[0]);
                    put(atm.horizon, sky_rgb[1]);
                    put(atm.nadir, sky_rgb[2]);
                }
                if (has_fog) {
                    put(atm.fog_color, fog_rgb);
                    atm.fog_start = fog_start;
                    atm.fog_end = fog_end;
                }
                atm.flags = (has_sky ? VR_ATMOS_SKY : 0u) | (has_fog ? VR_ATMOS_FOG : 0u);
                rc = vr_shade_lights_atmosphere(scene.get(), (vr_algo)algo, lights.data(), lights.size(),
                                                has_ambient ? ambient : nullptr, t, sinfo.scale, rays, n, 1, words.data(), nullptr,
                                                0, VR_TRACE_ORDER_AUTO, nullptr, has_ao ? ao_strength : 0u,
                                                ao_all ? VR_AO_ALL : VR_AO_AMBIENT, nullptr, has_reflect ? reflect_k : 0u,
                                                has_reflect ? bounces : 0u, has_mirror ? 0xFFFFFFu : 0u,
                                                has_mirror ? mirror_rgb : 0u, &atm);
            } else if (rc == VR_OK && has_reflect)
                rc = vr_shade_lights_reflect(scene.get(), (vr_algo)algo, lights.data(), lights.size(),
                                             has_ambient ? ambient : nullptr, t, sinfo.scale, rays, n, 1, words.data(), nullptr,
                                             0, VR_TRACE_ORDER_AUTO, nullptr, has_ao ? ao_strength : 0u,
                                             ao_all ? VR_AO_ALL : VR_AO_AMBIENT, nullptr, reflect_k, bounces,
                                             has_mirror ? 0xFFFFFFu : 0u, has_mirror ? mirror_rgb : 0u);
            else if (rc == VR_OK && has_ao)
                rc = vr_shade_lights_ao(scene.get(), (vr_algo)algo, lights.data(), lights.size(),
                                        has_ambient ? ambient : nullptr, t, sinfo.scale, rays, n, 1, words.data(), nullptr, 0,
                                        VR_TRACE_ORDER_AUTO, nullptr, ao_strength, ao_all ? VR_AO_ALL : VR_AO_AMBIENT, nullptr);
            else if (rc == VR_OK)
                rc = vr_shade_lights(scene.get(), (vr_algo)algo, lights.data(), lights.size(), has_ambient ? ambient : nullptr,
                                     t, sinfo.scale, rays, n, 1, words.data(), nullptr, 0, VR_TRACE_ORDER_AUTO, nullptr);
            (void)hipFree(rays);
            vrx::check(rc, "lights frame");
            for (size_t i = 0; i < n; ++i) frame[(size_t)py[i] * lw + px[i]] = words[i];
            HIP_OK(hipMemcpy(aa ? fine : fb, frame.data(), n * 4, hipMemcpyHostToDevice));
            if (aa) vrx::resolve(fine, width, height, S, fb);
            std::printf("lights %zu ambient %.9g %.9g %.9g", lights.size(), has_ambient ? ambient[0] : 0.0f,
                        has_ambient ? ambient[1] : 0.0f, has_ambient ? ambient[2] : 0.0f);
            if (has_ao) std::printf(" ao %u %s", ao_strength, ao_all ? "all" : "ambient");
            if (has_reflect && has_mirror) std::printf(" reflect %u bounces %u mirror %06x", reflect_k, bounces, mirror_rgb);
            else if (has_reflect) std::printf(" reflect %u bounces %u mirror every", reflect_k, bounces);
            if (has_sky) std::printf(" sky %06x %06x %06x", sky_rgb[0], sky_rgb[1], sky_rgb[2]);
            if (has_fog) std::printf(" fog %06x %.9g %.9g", fog_rgb, fog_start, fog_end);
            std::printf("\n");
            std::fflush(stdout);
        }
        // writeResultingImageToDisk (Main.cu:165-174): RGB8 pack on the device,
        // async copy into pinned memory, parallel PNG encode (vr_png_write).
        const size_t nbytes = (size_t)width * height * 3;
        uint8_t* host = nullptr;
        HIP_OK(hipHostMalloc((void**)&host, nbytes, hipHostMallocDefault));
        auto t0 = std::chrono::steady_clock::now();
        vrx::check(vr_pack_rgb8(fb, rgb, (uint64_t)width * height, nullptr), "pack");
        HIP_OK(hipMemcpyAsync(host, rgb, nbytes, hipMemcpyDeviceToHost, nullptr));
        HIP_OK(hipStreamSynchronize(nullptr));
        auto t1 = std::chrono::steady_clock::now();
        int rc = vr_png_write(out_path.c_str(), host, width, height, 3, 6);
        auto t2 = std::chrono::steady_clock::now();
        (void)hipHostFree(host);
        (void)hipFree(fb);
        (void)hipFree(rgb);
        (void)hipFree(fine);
        if (rc != VR_OK) {
            std::cerr << "ERROR: Failed to write image to: " << out_path << " (" << vr_last_error() << ")" << std::endl;
            return 1;
        }
        std::cout << "Wrote " << out_path << " (pack+copy "
                  << std::chrono::duration<double, std::milli>(t1 - t0).count() << " ms, png "
                  << std::chrono::duration<double, std::milli>(t2 - t1).count() << " ms)" << std::endl;
    } catch (const vrx::Error& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}
