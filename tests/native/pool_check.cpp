// CPU check of HostCopyPool (csrc/host_copy_pool.hpp alone), meant to be built with
// -fsanitize=thread and with -fsanitize=address,undefined: repeated copies of sizes that take
// the pooled path with full parts, a ragged last part, and the plain memcpy; run() with 1..13
// parts, each of which must run exactly once.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_copy_pool.hpp"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

int main() {
    rtamd::HostCopyPool pool;
    const size_t sizes[] = {size_t{24} << 20, (size_t{3} << 20) + 17, 1000};
    std::vector<uint8_t> src(sizes[0] + 64), dst(sizes[0] + 64);
    uint32_t x = 0x9E3779B9u;
    for (uint8_t& b : src) { x = x * 1664525u + 1013904223u; b = static_cast<uint8_t>(x >> 24); }
    for (int round = 0; round < 4; ++round) {
        for (const size_t len : sizes) {
            std::memset(dst.data(), 0xA5, dst.size());
            pool.copy(dst.data() + 1, src.data() + 3, len);            // unaligned on both sides
            CHECK(std::memcmp(dst.data() + 1, src.data() + 3, len) == 0);
            CHECK(dst[0] == 0xA5 && dst[len + 1] == 0xA5);             // nothing written outside the range
        }
    }
    for (int round = 0; round < 50; ++round)
        for (size_t parts = 1; parts <= 13; ++parts) {
            std::vector<std::atomic<int>> ran(parts);
            for (auto& r : ran) r.store(0, std::memory_order_relaxed);
            pool.run(parts, [&](size_t q) { ran[q].fetch_add(1, std::memory_order_relaxed); });
            for (size_t q = 0; q < parts; ++q) CHECK(ran[q].load(std::memory_order_relaxed) == 1);
        }
    pool.run(0, [&](size_t) { CHECK(false); });
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pool_check ok\n");
    return 0;
}
