// C ABI, host only (no HIP, no device): the checkpoint file of a progressive render
// (include/raytrace_amd.h, rt_checkpoint_write / rt_checkpoint_read): main.rs:47-56 stopped in one
// process and continued in another.  A fixed little-endian header, then the f64 running sums
// (format version 1) or the sums and then the sums of squares of a moments accumulator (version 2:
// rt_checkpoint_write_moments / rt_checkpoint_read_moments; each reader refuses the other's file).
// Written and parsed byte by byte: no struct is read from the file, nothing of it is trusted
// before it is checked, and every size is computed in 64 bits with its overflow tested first.
// Compiled alone by tests/native/checkpoint_check.cpp and checkpoint2_check.cpp under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "raytrace_amd.h"

namespace rtamd {
void set_thread_error(const std::string& msg);   // host_color.cpp (rt_last_error(NULL))
}

namespace {

constexpr char kMagic[8] = {'R', 'T', 'A', 'M', 'D', 'C', 'K', 'P'};
constexpr size_t kHeaderBytes = 88;
constexpr uint64_t kMaxSamples = 1ull << 31;

int refuse(int code, const std::string& msg) {
    rtamd::set_thread_error(msg);
    return code;
}

void put32(unsigned char* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = static_cast<unsigned char>(v >> (8 * i)); }
void put64(unsigned char* p, uint64_t v) { for (int i = 0; i < 8; ++i) p[i] = static_cast<unsigned char>(v >> (8 * i)); }
uint32_t get32(const unsigned char* p) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= static_cast<uint32_t>(p[i]) << (8 * i); return v; }
uint64_t get64(const unsigned char* p) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i); return v; }

struct File {
    std::FILE* f = nullptr;
    ~File() { if (f) std::fclose(f); }
};

// One file of format `version`: the header, then the `arrays` (1: sums; 2: sums, squares) of n_doubles each.
int write_file(const char* who, uint32_t version, const char* path, const rt_render_opts* o, uint64_t scene_hash, uint32_t samples,
               const double* const* data, int arrays, size_t n_doubles) {
    const std::string w(who);
    const uint64_t pixels = static_cast<uint64_t>(o->tile_w) * o->tile_h;      // < 2^64: two 32-bit factors
    if (n_doubles != 3 * pixels) return refuse(RT_E_INVALID, w + ": n_doubles is not 3 * tile_w * tile_h");
    if (samples > kMaxSamples) return refuse(RT_E_INVALID, w + ": samples above 2^31");
    unsigned char h[kHeaderBytes];
    std::memcpy(h, kMagic, 8);
    put32(h + 8, version);
    const uint32_t u[10] = {o->width, o->height, o->x0, o->tile_w, o->y0, o->tile_h, o->band, o->band_stride, o->band_phase,
                            o->max_depth};
    for (int i = 0; i < 10; ++i) put32(h + 12 + 4 * i, u[i]);
    put32(h + 52, static_cast<uint32_t>(o->jitter));
    put32(h + 56, samples);
    put32(h + 60, 0);
    put64(h + 64, o->seed);
    put64(h + 72, scene_hash);
    put64(h + 80, pixels);
    // a temporary name beside the file, renamed over it: a reader never sees a half-written checkpoint
    const std::string tmp = std::string(path) + ".tmp";
    {
        File out;
        out.f = std::fopen(tmp.c_str(), "wb");
        if (!out.f) return refuse(RT_E_IO, "cannot create " + tmp);
        bool ok = std::fwrite(h, 1, kHeaderBytes, out.f) == kHeaderBytes;
        unsigned char buf[8 * 512];
        for (int a = 0; a < arrays; ++a)
            for (size_t i = 0; ok && i < n_doubles;) {
                const size_t k = n_doubles - i < 512 ? n_doubles - i : 512;
                for (size_t j = 0; j < k; ++j) {
                    uint64_t bits;
                    std::memcpy(&bits, &data[a][i + j], 8);
                    put64(buf + 8 * j, bits);
                }
                ok = std::fwrite(buf, 8, k, out.f) == k;
                i += k;
            }
        ok = ok && std::fflush(out.f) == 0;
        if (!ok) {
            std::fclose(out.f);
            out.f = nullptr;
            std::remove(tmp.c_str());
            return refuse(RT_E_IO, "error writing " + tmp);
        }
    }
    if (std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return refuse(RT_E_IO, std::string("cannot rename the checkpoint to ") + path);
    }
    return RT_OK;
}

// ... and its reader.  data[a] all set: the arrays are read; all null (want false): header only.
int read_file(uint32_t version, const char* path, rt_render_opts* o, uint64_t* scene_hash, uint32_t* samples, double* const* data,
              int arrays, bool want, size_t cap_doubles) {
    File in;
    in.f = std::fopen(path, "rb");
    if (!in.f) return refuse(RT_E_IO, std::string("cannot open ") + path);
    unsigned char h[kHeaderBytes];
    if (std::fread(h, 1, kHeaderBytes, in.f) != kHeaderBytes) return refuse(RT_E_INVALID, "checkpoint: truncated header");
    if (std::memcmp(h, kMagic, 8) != 0) return refuse(RT_E_INVALID, "checkpoint: wrong magic");
    if (get32(h + 8) != version) return refuse(RT_E_INVALID, "checkpoint: unknown format version");
    rt_render_opts r;
    std::memset(&r, 0, sizeof r);
    uint32_t* const u[10] = {&r.width, &r.height, &r.x0, &r.tile_w, &r.y0, &r.tile_h, &r.band, &r.band_stride, &r.band_phase,
                             &r.max_depth};
    for (int i = 0; i < 10; ++i) *u[i] = get32(h + 12 + 4 * i);
    r.jitter = static_cast<int32_t>(get32(h + 52));
    const uint32_t n_samples = get32(h + 56);
    r.seed = get64(h + 64);
    const uint64_t hash = get64(h + 72), pixels = get64(h + 80);
    if (n_samples > kMaxSamples) return refuse(RT_E_INVALID, "checkpoint: samples above 2^31");
    if (pixels != static_cast<uint64_t>(r.tile_w) * r.tile_h)
        return refuse(RT_E_INVALID, "checkpoint: the pixel count is not tile_w * tile_h");
    // 3 * pixels doubles of 8 bytes each, per array: a product of two 32-bit sides can pass 2^64 / 24 (2^61 pixels
    // would wrap to 0 bytes), so the bound is tested before anything is multiplied
    if (pixels > UINT64_MAX / (24 * static_cast<uint64_t>(arrays))) return refuse(RT_E_INVALID, "checkpoint: size overflows");
    const uint64_t n = 3 * pixels;
    if (n > SIZE_MAX / (8 * static_cast<uint64_t>(arrays))) return refuse(RT_E_INVALID, "checkpoint: size overflows");
    if (want) {
        if (cap_doubles < n) return refuse(RT_E_INVALID, "checkpoint: the sums buffer is too small");
        unsigned char buf[8 * 512];
        for (int a = 0; a < arrays; ++a)
            for (uint64_t i = 0; i < n;) {
                const size_t k = n - i < 512 ? static_cast<size_t>(n - i) : 512;
                if (std::fread(buf, 8, k, in.f) != k) return refuse(RT_E_INVALID, "checkpoint: truncated sums");
                for (size_t j = 0; j < k; ++j) {
                    const uint64_t bits = get64(buf + 8 * j);
                    std::memcpy(&data[a][i + j], &bits, 8);
                }
                i += k;
            }
    } else {
        // header only: still a whole file?  (the length is the header's claim, checked against the file)
        if (std::fseek(in.f, 0, SEEK_END) != 0) return refuse(RT_E_IO, "checkpoint: cannot seek");
        const long end = std::ftell(in.f);
        if (end < 0 || static_cast<uint64_t>(end) < kHeaderBytes + 8 * n * static_cast<uint64_t>(arrays))
            return refuse(RT_E_INVALID, "checkpoint: truncated sums");
    }
    *o = r;
    if (scene_hash) *scene_hash = hash;
    if (samples) *samples = n_samples;
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_checkpoint_write(const char* path, const rt_render_opts* o, uint64_t scene_hash, uint32_t samples, const double* sums,
                        size_t n_doubles) {
    if (!path || !o || (!sums && n_doubles)) return refuse(RT_E_INVALID, "rt_checkpoint_write: null argument");
    const double* const data[1] = {sums};
    return write_file("rt_checkpoint_write", 1, path, o, scene_hash, samples, data, 1, n_doubles);
}

int rt_checkpoint_read(const char* path, rt_render_opts* o, uint64_t* scene_hash, uint32_t* samples, double* sums,
                       size_t cap_doubles) {
    if (!path || !o) return refuse(RT_E_INVALID, "rt_checkpoint_read: null argument");
    double* const data[1] = {sums};
    return read_file(1, path, o, scene_hash, samples, data, 1, sums != nullptr, cap_doubles);
}

int rt_checkpoint_write_moments(const char* path, const rt_render_opts* o, uint64_t scene_hash, uint32_t samples, const double* sums,
                                const double* squares, size_t n_doubles) {
    if (!path || !o || ((!sums || !squares) && n_doubles)) return refuse(RT_E_INVALID, "rt_checkpoint_write_moments: null argument");
    const double* const data[2] = {sums, squares};
    return write_file("rt_checkpoint_write_moments", 2, path, o, scene_hash, samples, data, 2, n_doubles);
}

int rt_checkpoint_read_moments(const char* path, rt_render_opts* o, uint64_t* scene_hash, uint32_t* samples, double* sums,
                               double* squares, size_t cap_doubles) {
    if (!path || !o || (sums == nullptr) != (squares == nullptr))
        return refuse(RT_E_INVALID, "rt_checkpoint_read_moments: null argument");
    double* const data[2] = {sums, squares};
    return read_file(2, path, o, scene_hash, samples, data, 2, sums != nullptr, cap_doubles);
}

}  // extern "C"
