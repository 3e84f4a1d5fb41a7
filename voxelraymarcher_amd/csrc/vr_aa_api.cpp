// vr_aa_api.cpp -- the supersampling entry points of include/vr.h: vr_aa_fine_words, vr_resolve and
// vr_render_aa (the kernel: vr_resolve.hip).  vr_render_aa is an ordinary vr_render of the fine
// frame followed by the resolve on the same stream; vr_resolve is the filter alone, for any fine
// frame already on the device.  Neither stages an array or allocates, and in both every argument
// check comes before any device work.
#include <string>

#include "vr_host.h"

namespace {

using vr::fail;
using vr::hip_fail;

bool good_samples(uint32_t s) { return s == 1u || s == 2u || s == 4u || s == 8u; }

// The frame checks the two entry points share: `who` names the caller in the message.
int check_frame(const char* who, uint32_t width, uint32_t rows, uint32_t samples) {
    const std::string w(who);
    if (!good_samples(samples)) return fail(VR_E_INVALID, w + ": samples must be 1, 2, 4 or 8");
    if (width == 0 || rows == 0 || width > 65536 || rows > 65536) return fail(VR_E_INVALID, w + ": bad image size");
    if ((uint64_t)samples * width > 65536 || (uint64_t)samples * rows > 65536)
        return fail(VR_E_INVALID, w + ": fine frame too large (samples * width and samples * height at most 65536)");
    return VR_OK;
}

}  // namespace

extern "C" {

uint64_t vr_aa_fine_words(uint32_t width, uint32_t rows, uint32_t samples) {
    if (!good_samples(samples) || width == 0 || width > 65536 || rows > 65536) return 0;
    if ((uint64_t)samples * width > 65536 || (uint64_t)samples * rows > 65536) return 0;
    return (uint64_t)samples * width * ((uint64_t)samples * rows);
}

int vr_resolve(const uint32_t* fine_dev, uint32_t width, uint32_t rows, uint32_t samples, uint32_t* out_dev,
               uint8_t* out_rgb8_dev, void* stream) {
    if (!fine_dev) return fail(VR_E_INVALID, "vr_resolve: fine_dev is NULL");
    if (!out_dev && !out_rgb8_dev) return fail(VR_E_INVALID, "vr_resolve: out_dev and out_rgb8_dev both NULL");
    if (const int rc = check_frame("vr_resolve", width, rows, samples)) return rc;
    if (((uintptr_t)fine_dev & 3u) != 0u || ((uintptr_t)out_dev & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_resolve: device words must be 4-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_resolve")) return rc;
    const hipError_t e = vr::launch_resolve(fine_dev, width, rows, samples, out_dev, out_rgb8_dev, st);
    if (e != hipSuccess) return hip_fail(e, "vr_resolve launch");
    return VR_OK;
}

int vr_render_aa(const vr_scene* s, vr_algo algo, const vr_camera* cam, const vr_lighting* lit,
                 const float translation[3], uint32_t scale, uint32_t width, uint32_t height, uint32_t samples,
                 uint32_t row_begin, uint32_t row_end, uint32_t* fine_dev, uint64_t fine_words, uint32_t* out_dev,
                 uint8_t* out_rgb8_dev, void* stream) {
    if (!s) return fail(VR_E_INVALID, "vr_render_aa: scene is NULL");
    if (!cam || !lit || !translation) return fail(VR_E_INVALID, "vr_render_aa: camera/lighting/translation NULL");
    if (!fine_dev) return fail(VR_E_INVALID, "vr_render_aa: fine_dev is NULL");
    if (!out_dev && !out_rgb8_dev) return fail(VR_E_INVALID, "vr_render_aa: out_dev and out_rgb8_dev both NULL");
    if (const int rc = check_frame("vr_render_aa", width, height, samples)) return rc;
    if (row_begin > row_end || row_end > height) return fail(VR_E_INVALID, "vr_render_aa: bad row range");
    const uint32_t rows = row_end - row_begin;
    if (fine_words < vr_aa_fine_words(width, rows, samples))
        return fail(VR_E_INVALID, "vr_render_aa: fine_words is " + std::to_string(fine_words) + ", needs " +
                                      std::to_string(vr_aa_fine_words(width, rows, samples)) + " (vr_aa_fine_words)");
    if (algo != VR_ALGO_ORIGINAL && algo != VR_ALGO_LONGESTAXIS) return fail(VR_E_INVALID, "vr_render_aa: unknown algorithm");
    if (((uintptr_t)fine_dev & 3u) != 0u || ((uintptr_t)out_dev & 3u) != 0u)
        return fail(VR_E_INVALID, "vr_render_aa: device words must be 4-byte aligned");
    if (rows == 0) return VR_OK;
    vr::DeviceGuard dg(s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = vr::refuse_capture(st, "vr_render_aa")) return rc;
    // the fine frame: an ordinary render launch of the (S * W) x (S * H) view (a ring slot, the
    // view's learned orders), rows [S * row_begin, S * row_end)
    if (const int rc = vr_render(s, algo, cam, lit, translation, scale, samples * width, samples * height,
                                 samples * row_begin, samples * row_end, fine_dev, stream))
        return rc;
    const hipError_t e = vr::launch_resolve(fine_dev, width, rows, samples, out_dev, out_rgb8_dev, st);
    if (e != hipSuccess) return hip_fail(e, "vr_render_aa: resolve launch");
    return VR_OK;
}

}  // extern "C"
