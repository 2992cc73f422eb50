// exact_plan_main.cpp -- TEST INFRASTRUCTURE.  The exact-mode deflater
// (deflate_exact_core.h) in heap blocks of exactly exact_plan.h's sizes, for
// the address and undefined-behaviour sanitizers: zeros, random bytes and
// JSON-like text x levels 0, 1, 6, 9 x windowBits 9-15 x memLevel 1, 4, 5 x
// the lengths at the tier edges and in the queue's 64-byte band.  Every
// message runs in its own tier's arrays and in the generous ones; both must
// succeed with the same payload.  Built with clang++ (the core uses
// __builtin_bitreverse32) and run by tests/test_exact_plan.py.
#include "exact_host_backend.cpp"

#include <stdio.h>
#include <string.h>

#include <vector>

static std::vector<uint8_t> message(int kind, uint32_t len, uint32_t seed)
{
    std::vector<uint8_t> m(len, 0);
    uint32_t x = seed * 2654435761u + 12345u;
    auto next = [&x] { return (x = x * 1664525u + 1013904223u) >> 8; };
    if (kind == 1)
        for (auto& b : m) b = (uint8_t)next();
    if (kind == 2) {
        static const char* const keys[] = {"\"id\":", "\"user\":", "\"ts\":", "\"status\":\"ok\",", "\"items\":[", "],"};
        for (uint32_t i = 0; i < len;) {
            const uint32_t r = next();
            char buf[48];
            const int n = r % 3 ? snprintf(buf, sizeof buf, "%s%u,", keys[r % 6], next() % 100000u)
                                : snprintf(buf, sizeof buf, "{%s\"v%u\"}", keys[(r >> 4) % 6], next() % 64u);
            for (int j = 0; j < n && i < len; ++j) m[i++] = (uint8_t)buf[j];
        }
    }
    return m;
}

int main()
{
    const int levels[] = {0, 1, 6, 9}, mems[] = {1, 4, 5};
    const uint32_t lens[] = {0, 1, 4095, 4096, 4097, 7866, 7867, 7929, 7930, 7931, 7994, 9000};
    unsigned cases = 0, failures = 0, by_tier[3] = {0, 0, 0};
    for (int kind = 0; kind < 3; ++kind)
        for (uint32_t len : lens) {
            const std::vector<uint8_t> m = message(kind, len, len + 7u * (uint32_t)kind);
            const uint32_t cap = len + ((len + 7) >> 3) + ((len + 63) >> 6) + 11;
            // heap blocks of exactly cap bytes: a store past the slot is the sanitizer's to see
            std::vector<uint8_t> a(cap), b(cap);
            for (int level : levels)
                for (int wbits = 9; wbits <= 15; ++wbits)
                    for (int mem : mems) {
                        const int t = tier_of(len, make_cfg(level, wbits, mem, 0).hbits);
                        const int32_t ra = dx_host(level, wbits, mem, 0, m.data(), len, a.data(), cap, t);
                        const int32_t rb = dx_host(level, wbits, mem, 0, m.data(), len, b.data(), cap, -1);
                        ++cases;
                        ++by_tier[t];
                        if (ra < 0 || rb < 0 || ra != rb || memcmp(a.data(), b.data(), (size_t)ra) != 0) {
                            ++failures;
                            printf("FAIL kind %d len %u level %d wbits %d mem %d tier %d: %d vs %d\n", kind, len, level,
                                   wbits, mem, t, ra, rb);
                        }
                    }
        }
    printf("exact_plan_main: %u cases (tiers %u / %u / %u), %u failures\n", cases, by_tier[0], by_tier[1], by_tier[2],
           failures);
    return failures || cases != 3024 || !by_tier[0] || !by_tier[1] || !by_tier[2];
}
