// The checkpoint file of a moments accumulator, format version 2 (csrc/host_checkpoint.cpp alone: no HIP, no
// device), built with -fsanitize=address,undefined: a round trip of sums and squares, each reader against the other
// version's file, and the version 2 reader against files it must refuse -- an empty file, a file cut at every
// header field boundary, inside the sums, at the boundary between sums and squares and inside the squares, a
// wrong magic, a pixel count one more than the tile's, pixel counts of 2^59 (48 * 2^59 wraps) and 2^61 -- without
// reading or writing out of bounds.
//   checkpoint2_check <scratch directory>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "raytrace_amd.h"

namespace rtamd {
static std::string g_err;
void set_thread_error(const std::string& msg) { g_err = msg; }     // what host_color.cpp gives the library
}

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

static std::vector<unsigned char> slurp(const std::string& path) {
    std::vector<unsigned char> v;
    if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
        unsigned char buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}

static void spill(const std::string& path, const std::vector<unsigned char>& v, size_t n) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { CHECK(!"cannot write the scratch file"); return; }
    if (n) CHECK(std::fwrite(v.data(), 1, n, f) == n);
    std::fclose(f);
}

static void put64(std::vector<unsigned char>& v, size_t at, uint64_t x) {
    for (int i = 0; i < 8; ++i) v[at + i] = static_cast<unsigned char>(x >> (8 * i));
}
static void put32(std::vector<unsigned char>& v, size_t at, uint32_t x) {
    for (int i = 0; i < 4; ++i) v[at + i] = static_cast<unsigned char>(x >> (8 * i));
}

// The version 2 reader on `path`, header only and with both buffers, each exactly as large as the tile needs, so
// the sanitizer sees any write past them.  Returns the two statuses (they must agree on a refusal).
static int read_both(const std::string& path, size_t n_doubles, int* header_only) {
    rt_render_opts o;
    std::memset(&o, 0x5A, sizeof o);
    uint64_t hash = 0;
    uint32_t samples = 0;
    *header_only = rt_checkpoint_read_moments(path.c_str(), &o, &hash, &samples, nullptr, nullptr, 0);
    std::vector<double> sums(n_doubles), squares(n_doubles);
    return rt_checkpoint_read_moments(path.c_str(), &o, &hash, &samples, sums.data(), squares.data(), n_doubles);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: checkpoint2_check DIR\n"); return 2; }
    const std::string dir = argv[1], good = dir + "/good2.ckpt", bad = dir + "/bad2.ckpt", v1 = dir + "/v1.ckpt";
    rt_render_opts o;
    std::memset(&o, 0, sizeof o);
    o.width = 40; o.height = 30; o.x0 = 3; o.tile_w = 7; o.y0 = 2; o.tile_h = 5;
    o.band = 1; o.band_stride = 2; o.band_phase = 1; o.max_depth = 4; o.jitter = RT_JITTER_RANDOM;
    o.seed = 0x0123456789abcdefull;
    o.spp = 99; o.flags = 3; o.algo = 6; o.bgr_pitch = 77;           // not bound: not stored
    const size_t n = 3 * 7 * 5;
    std::vector<double> sums(n), squares(n);
    for (size_t i = 0; i < n; ++i) {
        sums[i] = 0.125 * static_cast<double>(i) - 3.0;
        squares[i] = 1000.0 + static_cast<double>(i);
    }
    sums[1] = -0.0;
    sums[2] = std::numeric_limits<double>::quiet_NaN();
    squares[0] = std::numeric_limits<double>::infinity();
    squares[n - 1] = 4.9e-324;
    const uint64_t hash = 0xfeedfacecafef00dull;

    // ---- round trip ----
    CHECK(rt_checkpoint_write_moments(good.c_str(), &o, hash, 17, sums.data(), squares.data(), n) == RT_OK);
    const std::vector<unsigned char> file = slurp(good);
    CHECK(file.size() == 88 + 16 * n);
    CHECK(file.size() > 12 && file[8] == 2 && file[9] == 0 && file[10] == 0 && file[11] == 0);
    CHECK(slurp(good + ".tmp").empty());                             // renamed, not left behind
    {
        rt_render_opts r;
        uint64_t h = 0;
        uint32_t s = 0;
        std::vector<double> back(n, 1.0), back2(n, 1.0);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r, &h, &s, back.data(), back2.data(), n) == RT_OK);
        CHECK(h == hash && s == 17);
        CHECK(std::memcmp(back.data(), sums.data(), 8 * n) == 0);    // bit for bit: -0.0, NaN, inf, a subnormal
        CHECK(std::memcmp(back2.data(), squares.data(), 8 * n) == 0);
        CHECK(r.width == 40 && r.height == 30 && r.x0 == 3 && r.tile_w == 7 && r.y0 == 2 && r.tile_h == 5);
        CHECK(r.band == 1 && r.band_stride == 2 && r.band_phase == 1 && r.max_depth == 4 && r.jitter == RT_JITTER_RANDOM);
        CHECK(r.seed == o.seed);
        CHECK(r.spp == 0 && r.flags == 0 && r.algo == 0 && r.bgr_pitch == 0);
        // header only; larger buffers are fine, smaller ones are refused and nothing is written to them; one buffer
        // without the other is no call
        rt_render_opts r2;
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, &h, &s, nullptr, nullptr, 0) == RT_OK && s == 17 && r2.tile_w == 7);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, nullptr, nullptr, nullptr, nullptr, 0) == RT_OK);
        std::vector<double> big(n + 5, 2.0), big2(n + 5, 2.0), small(n - 1, 2.0), small2(n - 1, 2.0);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, &h, &s, big.data(), big2.data(), n + 5) == RT_OK);
        CHECK(big[n] == 2.0 && big2[n] == 2.0 && big2[n - 1] == 4.9e-324);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, &h, &s, small.data(), small2.data(), n - 1) == RT_E_INVALID);
        CHECK(small[0] == 2.0 && small2[0] == 2.0);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, &h, &s, back.data(), nullptr, n) == RT_E_INVALID);
        CHECK(rt_checkpoint_read_moments(good.c_str(), &r2, &h, &s, nullptr, back2.data(), n) == RT_E_INVALID);
    }
    // ---- each reader refuses the other version's file ----
    {
        rt_render_opts r;
        std::memset(&r, 0x5A, sizeof r);
        rt_render_opts untouched = r;
        std::vector<double> a(2 * n, 3.0), b(n, 3.0);
        CHECK(rt_checkpoint_read(good.c_str(), &r, nullptr, nullptr, nullptr, 0) == RT_E_INVALID);
        CHECK(rt_checkpoint_read(good.c_str(), &r, nullptr, nullptr, a.data(), a.size()) == RT_E_INVALID && a[0] == 3.0);
        CHECK(rt_checkpoint_write(v1.c_str(), &o, hash, 17, sums.data(), n) == RT_OK);
        CHECK(slurp(v1).size() == 88 + 8 * n);
        CHECK(rt_checkpoint_read_moments(v1.c_str(), &r, nullptr, nullptr, nullptr, nullptr, 0) == RT_E_INVALID);
        CHECK(rt_checkpoint_read_moments(v1.c_str(), &r, nullptr, nullptr, a.data(), b.data(), n) == RT_E_INVALID);
        CHECK(a[0] == 3.0 && b[0] == 3.0 && std::memcmp(&r, &untouched, sizeof r) == 0);
        // a version 1 file relabelled as 2 is a version 2 file cut where the squares begin
        std::vector<unsigned char> v = slurp(v1);
        put32(v, 8, 2);
        spill(bad, v, v.size());
        int ho = 0;
        CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
        std::remove(v1.c_str());
    }
    // the writer's own refusals
    CHECK(rt_checkpoint_write_moments(bad.c_str(), &o, hash, 1, sums.data(), squares.data(), n - 1) == RT_E_INVALID);
    CHECK(rt_checkpoint_write_moments(bad.c_str(), &o, hash, 1, sums.data(), squares.data(), n + 3) == RT_E_INVALID);
    CHECK(rt_checkpoint_write_moments(bad.c_str(), &o, hash, 0x80000001u, sums.data(), squares.data(), n) == RT_E_INVALID);
    CHECK(rt_checkpoint_write_moments((dir + "/no/such/dir/x.ckpt").c_str(), &o, hash, 1, sums.data(), squares.data(), n) == RT_E_IO);
    CHECK(rt_checkpoint_write_moments(nullptr, &o, hash, 1, sums.data(), squares.data(), n) == RT_E_INVALID);
    CHECK(rt_checkpoint_write_moments(bad.c_str(), &o, hash, 1, sums.data(), nullptr, n) == RT_E_INVALID);
    CHECK(rt_checkpoint_write_moments(bad.c_str(), &o, hash, 1, nullptr, squares.data(), n) == RT_E_INVALID);
    // an empty tile is a header alone
    {
        rt_render_opts e = o, r;
        e.tile_h = 0;
        CHECK(rt_checkpoint_write_moments(bad.c_str(), &e, hash, 0, nullptr, nullptr, 0) == RT_OK && slurp(bad).size() == 88);
        uint32_t s = 9;
        CHECK(rt_checkpoint_read_moments(bad.c_str(), &r, nullptr, &s, nullptr, nullptr, 0) == RT_OK && s == 0 && r.tile_h == 0);
    }

    // ---- the reader against bad files ----
    int ho = 0;
    rt_render_opts untouched;
    std::memset(&untouched, 0x5A, sizeof untouched);
    CHECK(read_both(dir + "/missing.ckpt", n, &ho) == RT_E_IO && ho == RT_E_IO);
    spill(bad, file, 0);                                             // empty
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    // cut at every header field boundary (and one byte into the file, and one byte short of the header)
    const size_t cuts[] = {1, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 72, 80, 87};
    for (size_t c : cuts) {
        spill(bad, file, c);
        const int rc = read_both(bad, n, &ho);
        if (rc != RT_E_INVALID || ho != RT_E_INVALID) { std::printf("cut at %zu: %d %d\n", c, rc, ho); ++failures; }
    }
    // cut in the sums, where the squares begin, inside the squares, inside the last double
    for (size_t c : {size_t(88), size_t(88 + 8 * (n / 2) + 3), size_t(88 + 8 * n - 1), size_t(88 + 8 * n), size_t(88 + 8 * n + 5),
                     size_t(88 + 8 * n + 8 * (n / 2)), file.size() - 1}) {
        spill(bad, file, c);
        const int rc = read_both(bad, n, &ho);
        if (rc != RT_E_INVALID || ho != RT_E_INVALID) { std::printf("cut at %zu: %d %d\n", c, rc, ho); ++failures; }
    }
    {   // a refused read leaves the caller's opts alone
        rt_render_opts r;
        std::memset(&r, 0x5A, sizeof r);
        CHECK(rt_checkpoint_read_moments(bad.c_str(), &r, nullptr, nullptr, nullptr, nullptr, 0) == RT_E_INVALID);
        CHECK(std::memcmp(&r, &untouched, sizeof r) == 0);
    }
    std::vector<unsigned char> v = file;
    v[0] ^= 0x20;                                                    // wrong magic
    spill(bad, v, v.size());
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    v = file;
    put32(v, 8, 3);                                                  // a format version of the future
    spill(bad, v, v.size());
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    v = file;
    put64(v, 80, 7 * 5 + 1);                                         // one pixel more than the tile has
    v.resize(v.size() + 48, 0);                                      // ... and the bytes to go with it
    spill(bad, v, v.size());
    CHECK(read_both(bad, n + 3, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    v = file;
    put64(v, 80, 1ull << 59);                                        // 2^59 pixels: 6 * 8 * 2^59 wraps (3 * 8 * 2^59 does not)
    put32(v, 24, 1u << 30);                                          // ... with a tile that agrees: 2^30 x 2^29
    put32(v, 32, 1u << 29);
    spill(bad, v, v.size());
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    v = file;
    put64(v, 80, 1ull << 61);                                        // 2^61 pixels, tile_w 2^31, tile_h 2^30
    put32(v, 24, 1u << 31);
    put32(v, 32, 1u << 30);
    spill(bad, v, v.size());
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    v = file;
    put32(v, 56, 0x80000001u);                                       // more samples than an accumulator can hold
    spill(bad, v, v.size());
    CHECK(read_both(bad, n, &ho) == RT_E_INVALID && ho == RT_E_INVALID);
    std::remove(bad.c_str());
    std::remove(good.c_str());
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("checkpoint2_check ok\n");
    return 0;
}
