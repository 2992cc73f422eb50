// hdr_list_main.cpp -- TEST INFRASTRUCTURE.  The run list of the lane
// kernel's dynamic headers (beast_amd/csrc/hdr_list.h) on the CPU:
//  1. the fit rule: for every (entries, coded literal/length symbols) the
//     list's bytes and the placed symbols' bytes are disjoint exactly when
//     list_fits() says so, and more entries than the area holds never fit;
//  2. placement: random code-length sequences are placed once by the walk
//     over every symbol and once from the list, PL entries read before any
//     of them is placed, in the one area both share; whenever the rule lets
//     the list path run, both give the same symbol order.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       hdr_list_main.cpp -o hl_asan && ./hl_asan
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../beast_amd/csrc/hdr_list.h"

namespace hl = bpmd::hl;

namespace {

int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            if (++fails < 10) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                             \
    } while (0)

void fit_rule()
{
    for (uint32_t e = 0; e <= 2 * hl::MAX_ENTRIES; ++e)
        for (uint32_t c = 0; c <= hl::AREA; ++c) {
            if (e > hl::MAX_ENTRIES) {
                CHECK(!hl::list_fits(e, c));
                continue;
            }
            uint8_t owner[hl::AREA] = {};
            for (uint32_t j = 0; j < e; ++j) {
                CHECK(hl::entry_off(j) + 2 <= hl::AREA);
                owner[hl::entry_off(j)] = owner[hl::entry_off(j) + 1] = 1;
            }
            bool disjoint = true;
            for (uint32_t b = 0; b < c; ++b) disjoint = disjoint && !owner[b];
            CHECK(disjoint == hl::list_fits(e, c));
        }
}

constexpr uint32_t PL = 16;

struct Header {
    uint32_t nlen, ndist;
    std::vector<uint8_t> len;                                  // per symbol, nlen + ndist
    std::vector<uint32_t> run_first, run_rep;                  // as pass 1 decodes them
};

// lengths in runs of 1 (a literal length) or 3-6 (a 16 repeat) and zero runs
Header random_header(std::mt19937& g, uint32_t coded_pct)
{
    Header h;
    h.nlen = 257 + g() % 30;
    h.ndist = 1 + g() % 30;
    const uint32_t want = h.nlen + h.ndist;
    while (h.len.size() < want) {
        const uint32_t left = want - (uint32_t)h.len.size();
        const bool zero = g() % 100 >= coded_pct;
        uint32_t rep = zero ? 1 + g() % (coded_pct < 50 ? 40 : 4) : (g() % 4 ? 1 : 3 + g() % 4);
        if (rep > left) rep = zero ? left : 1;
        const uint8_t v = zero ? 0 : (uint8_t)(1 + g() % 15);
        if (v) {
            h.run_first.push_back((uint32_t)h.len.size());
            h.run_rep.push_back(rep);
        }
        h.len.insert(h.len.end(), rep, v);
    }
    return h;
}

void placement(std::mt19937& g, uint32_t coded_pct, uint32_t& took_list, uint32_t& took_walk)
{
    const Header h = random_header(g, coded_pct);
    // first slot per length (literal/length and distance symbols apart)
    uint32_t cl[17] = {}, cd[17] = {};
    for (uint32_t i = 0; i < h.len.size(); ++i)
        if (h.len[i]) (i < h.nlen ? cl : cd)[h.len[i] + 1] += 1;
    uint32_t coded_lit = 0, coded_dist = 0;
    for (int l = 1; l <= 16; ++l) {
        coded_lit += cl[l];
        coded_dist += cd[l];
        cl[l] += cl[l - 1];
        cd[l] += cd[l - 1];
    }
    // the walk over every symbol
    std::vector<uint8_t> wl(hl::AREA, 0xee), wd(32, 0xee);
    {
        uint32_t a[17], d[17];
        std::memcpy(a, cl, sizeof a);
        std::memcpy(d, cd, sizeof d);
        for (uint32_t i = 0; i < h.len.size(); ++i) {
            const uint32_t l = h.len[i];
            if (!l) continue;
            if (i < h.nlen) wl[a[l]++] = (uint8_t)i;
            else wd[d[l]++] = (uint8_t)(i - h.nlen);
        }
    }
    const uint32_t entries = (uint32_t)h.run_first.size();
    if (!hl::list_fits(entries, coded_lit)) {
        ++took_walk;
        return;
    }
    ++took_list;
    // pass 1 leaves the list in the area; pass 2 places into the same area
    std::vector<uint8_t> area(hl::AREA, 0xee), dst(32, 0xee);
    for (uint32_t j = 0; j < entries; ++j) {
        const uint32_t e = hl::entry_pack(h.run_first[j], h.len[h.run_first[j]], h.run_rep[j]);
        CHECK(e < 0x10000u && hl::entry_first(e) == h.run_first[j] && hl::entry_rep(e) == h.run_rep[j]);
        area[hl::entry_off(j)] = (uint8_t)e;
        area[hl::entry_off(j) + 1] = (uint8_t)(e >> 8);
    }
    uint32_t a[17], d[17];
    std::memcpy(a, cl, sizeof a);
    std::memcpy(d, cd, sizeof d);
    for (uint32_t have = 0; have < entries; have += PL) {
        uint32_t en[PL];
        for (uint32_t j = 0; j < PL; ++j) {
            const uint32_t off = hl::entry_off(have + j);   // stays inside the area: MAX_ENTRIES is a multiple of PL
            CHECK(off + 2 <= hl::AREA);
            en[j] = have + j < entries ? area[off] | area[off + 1] << 8 : 0u;
        }
        for (uint32_t j = 0; j < PL; ++j) {
            const uint32_t l = hl::entry_len(en[j]);
            if (!l) continue;
            for (uint32_t t = 0; t < hl::entry_rep(en[j]); ++t) {
                const uint32_t i = hl::entry_first(en[j]) + t;
                if (i < h.nlen) {
                    CHECK(a[l] < coded_lit);
                    area[a[l]++] = (uint8_t)i;
                } else {
                    CHECK(d[l] < coded_dist);
                    dst[d[l]++] = (uint8_t)(i - h.nlen);
                }
            }
        }
    }
    CHECK(std::memcmp(area.data(), wl.data(), coded_lit) == 0);
    CHECK(std::memcmp(dst.data(), wd.data(), coded_dist) == 0);
}

}  // namespace

int main()
{
    fit_rule();
    std::mt19937 g(0x5eed);
    uint32_t list = 0, walk = 0;
    for (int i = 0; i < 6000; ++i) placement(g, 5 + (uint32_t)i % 95, list, walk);
    CHECK(list > 1000 && walk > 1000);
    std::printf("hdr_list: %u list, %u walk, %d failures\n", list, walk, fails);
    return fails ? 1 : 0;
}
