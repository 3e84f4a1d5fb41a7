// vr_scene_io.cpp -- voxel lists without a device: the synthetic grid generator and the
// .vox CSV / .vxb readers and writers of include/vr.h.  Makes no HIP call.
//
// Replaces VoxelFile::readVoxelFile (geometry/VoxelFile.cuh:9-35).
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "vr_host.h"

namespace {

using vr::fail;
using vr::VoxParse;

// ------------------------------------------------------------- synthetic grid
inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
inline bool draw(uint64_t seed, uint64_t stream, uint64_t k, double p) {
    uint64_t h = splitmix64((seed << 34) | (stream << 32) | k);
    return (double)(h >> 40) * (1.0 / 16777216.0) < p;
}

// std::stoi as used by VoxelFile.cuh:18-21: skip leading whitespace, optional
// sign, at least one digit, stop at the first non-digit; out of int range or
// no digits throws in the reference -> VR_E_PARSE here.
bool stoi_like(const char* b, const char* e, int32_t* out) {
    while (b < e && (*b == ' ' || *b == '\t' || *b == '\n' || *b == '\v' || *b == '\f' || *b == '\r')) ++b;
    bool neg = false;
    if (b < e && (*b == '+' || *b == '-')) { neg = *b == '-'; ++b; }
    if (b >= e || *b < '0' || *b > '9') return false;
    int64_t v = 0;
    while (b < e && *b >= '0' && *b <= '9') {
        v = v * 10 + (*b - '0');
        if (v > 2147483648ll) return false;
        ++b;
    }
    if (neg) v = -v;
    if (v > 2147483647ll || v < -2147483648ll) return false;
    *out = (int32_t)v;
    return true;
}

// VoxelFile::readVoxelFile (VoxelFile.cuh:11-35) for one line: comma-separated
// fields with empty fields skipped (find_first_not_of(",")), lines with <= 3
// fields ignored, each of the first four fields converted like std::stoi.
// Returns 1 = voxel, 0 = ignored line, -1 = std::stoi would throw.
int parse_vox_line(const char* p, const char* e, int32_t v[4]) {
    const char* fb[4] = {nullptr, nullptr, nullptr, nullptr};
    const char* fe[4] = {nullptr, nullptr, nullptr, nullptr};
    int nf = 0;
    while (p < e) {
        while (p < e && *p == ',') ++p;
        if (p >= e) break;
        const char* q = p;
        while (q < e && *q != ',') ++q;
        if (nf < 4) { fb[nf] = p; fe[nf] = q; }
        ++nf;
        p = q;
    }
    if (nf <= 3) return 0;                     // lineEntries.size() > 3 (VoxelFile.cuh:25)
    for (int i = 0; i < 4; ++i)
        if (!stoi_like(fb[i], fe[i], &v[i])) return -1;
    return 1;
}

// .vxb: the binary scene sidecar -- 32-byte header {"VRVXB001", u64 count,
// u64 reserved x2}, then int32 xyz[3 * count] and uint32 rgb[count], little
// endian, in insertion order (duplicates resolve exactly as in the CSV).
constexpr char kVxbMagic[9] = "VRVXB001";
struct VxbHeader {
    char magic[8];
    uint64_t count = 0;
    uint64_t reserved[2] = {0, 0};
};
static_assert(sizeof(VxbHeader) == 32, "vxb header");

int read_vxb_header(FILE* f, const char* path, VxbHeader& hd) {
    if (std::fread(&hd, sizeof hd, 1, f) != 1 || std::memcmp(hd.magic, kVxbMagic, 8) != 0)
        return fail(VR_E_PARSE, std::string(path) + ": not a .vxb scene (bad header)");
    if (hd.count >= 0xFFFFFFFFull) return fail(VR_E_PARSE, std::string(path) + ": .vxb voxel count too large");
    return VR_OK;
}

int open_file(const char* path, const char* mode, FILE*& f) {
    f = std::fopen(path, mode);
    if (!f) return fail(VR_E_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    return VR_OK;
}

// Whole-file read (the .vox parser splits the text across threads).
int read_file(const char* path, std::vector<char>& out) {
    FILE* f;
    if (int rc = open_file(path, "rb", f)) return rc;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    const bool err = std::ferror(f) != 0;
    std::fclose(f);
    if (err) return fail(VR_E_IO, std::string("read failed: ") + path);
    return VR_OK;
}

// The text is cut at newlines into one chunk per worker; chunks are parsed in
// parallel and concatenated in file order (later duplicates must stay later).
// The first error in file order is reported with its line number.
int parse_vox_text(const char* path, const std::vector<char>& text, VoxParse& out) {
    const size_t len = text.size();
    const char* base = text.data();
    unsigned hw = std::thread::hardware_concurrency();
    size_t workers = std::max<size_t>(1, std::min<size_t>({(size_t)(hw ? hw : 1), (size_t)16, len / (1u << 20) + 1}));
    std::vector<size_t> cut(workers + 1, len);
    cut[0] = 0;
    for (size_t w = 1; w < workers; ++w) {
        size_t c = std::max(cut[w - 1], len * w / workers);
        while (c < len && base[c - 1] != '\n') ++c;
        cut[w] = c;
    }
    struct Part {
        VoxParse vp;
        size_t lines = 0;            // newline-terminated or final lines seen
        size_t bad_line = 0;         // 1-based within the chunk, 0 = none
    };
    std::vector<Part> parts(workers);
    auto run = [&](size_t w) {
        Part& pt = parts[w];
        const char* p = base + cut[w];
        const char* end = base + cut[w + 1];
        pt.vp.xyz.reserve((size_t)(end - p) / 8 * 3);
        pt.vp.rgb.reserve((size_t)(end - p) / 24);
        while (p < end) {
            const char* q = (const char*)std::memchr(p, '\n', (size_t)(end - p));
            const char* le = q ? q : end;
            ++pt.lines;
            int32_t v[4];
            const int r = parse_vox_line(p, le, v);
            if (r < 0) { pt.bad_line = pt.lines; return; }
            if (r > 0) {
                pt.vp.xyz.insert(pt.vp.xyz.end(), {v[0], v[1], v[2]});
                pt.vp.rgb.push_back((uint32_t)v[3]);
            }
            p = q ? q + 1 : end;
        }
    };
    if (workers == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        for (size_t w = 0; w < workers; ++w) th.emplace_back(run, w);
        for (auto& t : th) t.join();
    }
    size_t line0 = 0, n = 0;
    for (size_t w = 0; w < workers; ++w) {
        if (parts[w].bad_line) {
            // lines before this chunk: every earlier chunk ends with a newline
            return fail(VR_E_PARSE, std::string(path) + ":" + std::to_string(line0 + parts[w].bad_line) +
                                        ": std::stoi would throw");
        }
        line0 += parts[w].lines;
        n += parts[w].vp.rgb.size();
    }
    out.xyz.reserve(3 * n);
    out.rgb.reserve(n);
    for (auto& pt : parts) {
        out.xyz.insert(out.xyz.end(), pt.vp.xyz.begin(), pt.vp.xyz.end());
        out.rgb.insert(out.rgb.end(), pt.vp.rgb.begin(), pt.vp.rgb.end());
    }
    return VR_OK;
}

bool is_vxb(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    char m[8];
    const bool yes = std::fread(m, 1, 8, f) == 8 && std::memcmp(m, kVxbMagic, 8) == 0;
    std::fclose(f);
    return yes;
}

int read_vox(const char* path, VoxParse& out) {
    std::vector<char> text;
    const int rc = read_file(path, text);
    return rc ? rc : parse_vox_text(path, text, out);
}

}  // namespace

int vr::read_voxels(const char* path, VoxParse& out) {
    if (!is_vxb(path)) return read_vox(path, out);
    size_t n = 0;
    const int rc = vr_vxb_read(path, nullptr, nullptr, 0, &n);
    if (rc) return rc;
    out.xyz.resize(3 * n);          // (empty vectors: null arrays, which only count again)
    out.rgb.resize(n);
    return vr_vxb_read(path, out.xyz.data(), out.rgb.data(), n, &n);
}

extern "C" {

int vr_synth_generate(const vr_synth_params* p, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out) {
    if (!p || !n_out) return fail(VR_E_INVALID, "NULL argument");
    if (p->n == 0 || p->n % 64 || p->n > 1024) return fail(VR_E_INVALID, "grid side must be a multiple of 64 in [64,1024]");
    if (xyz && !rgb) return fail(VR_E_INVALID, "rgb NULL");
    const uint32_t NR = p->n / 64, NC = p->n / 8;
    size_t cnt = 0;
    for (uint32_t rz = 0; rz < NR; ++rz)
        for (uint32_t ry = 0; ry < NR; ++ry)
            for (uint32_t rx = 0; rx < NR; ++rx) {
                if (!draw(p->seed, 0, rx + ry * NR + rz * NR * NR, p->p_region)) continue;
                for (uint32_t cz = rz * 8; cz < rz * 8 + 8; ++cz)
                    for (uint32_t cy = ry * 8; cy < ry * 8 + 8; ++cy)
                        for (uint32_t cx = rx * 8; cx < rx * 8 + 8; ++cx) {
                            if (!draw(p->seed, 1, cx + cy * NC + (uint64_t)cz * NC * NC, p->p_cluster)) continue;
                            for (uint32_t z = cz * 8; z < cz * 8 + 8; ++z)
                                for (uint32_t y = cy * 8; y < cy * 8 + 8; ++y)
                                    for (uint32_t x = cx * 8; x < cx * 8 + 8; ++x) {
                                        uint64_t key = ((uint64_t)x << 20) | (y << 10) | z;
                                        if (!draw(p->seed, 2, key, p->p_voxel)) continue;
                                        if (xyz) {
                                            if (cnt >= capacity) return fail(VR_E_INVALID, "capacity too small");
                                            xyz[3 * cnt] = (int32_t)x; xyz[3 * cnt + 1] = (int32_t)y; xyz[3 * cnt + 2] = (int32_t)z;
                                            rgb[cnt] = (uint32_t)(splitmix64((p->seed << 34) | (3ull << 32) | key) & 0xFFFFFFu);
                                        }
                                        ++cnt;
                                    }
                        }
            }
    *n_out = cnt;
    return VR_OK;
}

int vr_vox_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out) {
    if (!path || !n_out) return fail(VR_E_INVALID, "NULL argument");
    VoxParse vp;
    const int rc = read_vox(path, vp);
    if (rc) return rc;
    const size_t n = vp.rgb.size();
    if (xyz) {
        if (!rgb) return fail(VR_E_INVALID, "rgb NULL");
        if (n > capacity) return fail(VR_E_INVALID, "capacity too small");
        std::memcpy(xyz, vp.xyz.data(), 3 * n * sizeof(int32_t));
        std::memcpy(rgb, vp.rgb.data(), n * sizeof(uint32_t));
    }
    *n_out = n;
    return VR_OK;
}

int vr_vxb_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out) {
    if (!path || !n_out) return fail(VR_E_INVALID, "NULL argument");
    FILE* f;
    if (int rc = open_file(path, "rb", f)) return rc;
    VxbHeader hd;
    int rc = read_vxb_header(f, path, hd);
    if (!rc && xyz) {
        if (!rgb) rc = fail(VR_E_INVALID, "rgb NULL");
        else if (hd.count > capacity) rc = fail(VR_E_INVALID, "capacity too small");
        else if (std::fread(xyz, sizeof(int32_t), 3 * (size_t)hd.count, f) != 3 * (size_t)hd.count ||
                 std::fread(rgb, sizeof(uint32_t), (size_t)hd.count, f) != (size_t)hd.count)
            rc = fail(VR_E_PARSE, std::string(path) + ": truncated .vxb payload");
    }
    std::fclose(f);
    if (!rc) *n_out = (size_t)hd.count;
    return rc;
}

int vr_vxb_write(const char* path, const int32_t* xyz, const uint32_t* rgb, size_t n) {
    if (!path || (n && (!xyz || !rgb))) return fail(VR_E_INVALID, "NULL argument");
    FILE* f;
    if (int rc = open_file(path, "wb", f)) return rc;
    VxbHeader hd;
    std::memcpy(hd.magic, kVxbMagic, 8);
    hd.count = n;
    bool ok = std::fwrite(&hd, sizeof hd, 1, f) == 1 &&
              (n == 0 || (std::fwrite(xyz, sizeof(int32_t), 3 * n, f) == 3 * n &&
                          std::fwrite(rgb, sizeof(uint32_t), n, f) == n));
    if (std::fclose(f) != 0) ok = false;
    if (!ok) return fail(VR_E_IO, std::string("write failed: ") + path);
    return VR_OK;
}

int vr_scene_file_read(const char* path, int32_t* xyz, uint32_t* rgb, size_t capacity, size_t* n_out) {
    if (!path) return fail(VR_E_INVALID, "NULL argument");
    return is_vxb(path) ? vr_vxb_read(path, xyz, rgb, capacity, n_out) : vr_vox_read(path, xyz, rgb, capacity, n_out);
}

int vr_vox_write(const char* path, const int32_t* xyz, const uint32_t* rgb, size_t n) {
    if (!path || (n && (!xyz || !rgb))) return fail(VR_E_INVALID, "NULL argument");
    FILE* f;
    if (int rc = open_file(path, "wb", f)) return rc;
    for (size_t i = 0; i < n; ++i)
        std::fprintf(f, "%d,%d,%d,%d\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (int32_t)rgb[i]);
    if (std::fclose(f) != 0) return fail(VR_E_IO, std::string("write failed: ") + path);
    return VR_OK;
}

}  // extern "C"
