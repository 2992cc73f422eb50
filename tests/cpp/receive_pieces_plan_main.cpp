// The piece walk of the chained receive (beast_amd/csrc/receive_pieces_plan.h)
// under -fsanitize=address,undefined.  A connection's wire -- fragmented
// messages, control frames between the fragments, both short length forms, masked or
// not -- is fed in chunks of every size from one byte up, into out slots of
// several capacities.  Each call gets heap blocks of exactly the bytes it may
// touch: the unconsumed wire bytes, an out slot of `cap` bytes and a control
// slot of 125, so one byte read or written outside any of them aborts the
// program; the callbacks also check the walk's own bounds (data below cap - 4,
// the tail below cap).  The pieces, put together again, must be the messages
// that were framed, and the events must come in the order they were sent.
// Then the walk runs over random bytes from random states for its bounds alone.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "receive_pieces_plan.h"

using namespace bpmd;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            if (failures++ < 10) printf("line %d: %s\n", __LINE__, #c); \
        }                                                         \
    } while (0)

static std::mt19937_64 rng(20250517);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

struct Item {   // what the peer sent, in order
    uint32_t kind;   // 1 message, 2 ping, 3 pong, 4 close
    uint32_t op, deflated;
    std::string bytes;
};

static void put_frame(std::string& w, bool fin, bool rsv1, uint32_t op, const std::string& pay, bool masked, int form = 0)
{
    const size_t n = pay.size();
    if (!form) form = n <= 125 ? 7 : n <= 65535 ? 16 : 64;
    w.push_back((char)((fin ? 0x80 : 0) | (rsv1 ? 0x40 : 0) | op));
    const uint8_t m = masked ? 0x80 : 0;
    if (form == 7) w.push_back((char)(m | n));
    else if (form == 16) {
        w.push_back((char)(m | 126));
        w.push_back((char)(n >> 8));
        w.push_back((char)(n & 0xff));
    } else {
        w.push_back((char)(m | 127));
        for (int i = 7; i >= 0; --i) w.push_back((char)((uint64_t)n >> (8 * i)));
    }
    uint8_t key[4] = {0, 0, 0, 0};
    if (masked) {
        for (auto& k : key) k = (uint8_t)rnd(256);
        w.append((const char*)key, 4);
    }
    for (size_t i = 0; i < n; ++i) w.push_back((char)((uint8_t)pay[i] ^ key[i & 3]));
}

static std::string blob(uint32_t n)
{
    std::string s(n, '\0');
    for (auto& c : s) c = (char)rnd(256);
    return s;
}

static std::string make_wire(bool masked, std::vector<Item>& items)
{
    std::string w;
    const uint32_t msgs = 2 + rnd(3);
    for (uint32_t k = 0; k < msgs; ++k) {
        const uint32_t op = 1 + rnd(2), deflated = rnd(2), frags = 1 + rnd(4);
        Item msg{1, op, deflated, ""};
        for (uint32_t f = 0; f < frags; ++f) {
            const uint32_t lens[] = {0, 1, 3, 17, 125, 126, 200};
            const std::string pay = blob(lens[rnd(7)]);
            put_frame(w, f + 1 == frags, f == 0 && deflated, f == 0 ? op : 0, pay, masked);
            msg.bytes += pay;
            if (f + 1 < frags && rnd(3) == 0) {
                const std::string c = blob(rnd(126));
                const uint32_t cop = 9 + rnd(2);
                put_frame(w, true, false, cop, c, masked);
                items.push_back(Item{cop == 9 ? 2u : 3u, cop, 0, c});   // arrives before the message ends
            }
        }
        items.push_back(msg);
    }
    std::string reason = std::string("\x03\xe8", 2) + "bye";
    put_frame(w, true, false, 8, reason, masked);
    items.push_back(Item{4, 8, 0, reason});
    return w;
}

static unsigned long long calls = 0, stores = 0;

// one walk with exact-size blocks; returns the Stop, the piece in `piece`, the control payload in `ctl`
static rpp::Stop one_walk(const uint8_t* avail, uint32_t wl, uint32_t role, bool pmd_on, uint64_t msg_max, uint32_t cap,
                          rpp::PieceState& st, std::string& piece, std::string& ctl)
{
    uint8_t* w = (uint8_t*)malloc(wl ? wl : 1);
    if (wl) memcpy(w, avail, wl);
    uint8_t* slot = (uint8_t*)malloc(cap ? cap : 1);
    uint8_t* c = (uint8_t*)malloc(125);
    memset(slot, 0xA5, cap ? cap : 1);
    uint32_t end = 0;
    rpp::Stop s;
    rpp::walk(
        w, wl, role, pmd_on, msg_max, cap, st,
        [&](uint32_t at, const uint8_t* src, uint32_t len, uint32_t key) {
            CHECK(at == end && (uint64_t)at + len + rpp::TAIL <= cap);   // appended, the tail's room kept
            CHECK(src >= w && src + len <= w + wl);
            for (uint32_t t = 0; t < len; ++t) slot[at + t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
            end = at + len;
            stores += len;
        },
        [&](const uint8_t* src, uint32_t len, uint32_t key) {
            CHECK(len <= 125 && src >= w && src + len <= w + wl);
            for (uint32_t t = 0; t < len; ++t) c[t] = src[t] ^ (uint8_t)(key >> (8 * (t & 3u)));
        },
        [&](uint32_t at) {
            CHECK(at == end && (uint64_t)at + rpp::TAIL <= cap);
            memcpy(slot + at, "\x00\x00\xff\xff", 4);
        },
        s);
    ++calls;
    CHECK(s.piece_len == end && s.consumed <= wl);
    piece.assign((const char*)slot, s.piece_len);
    if (s.tail) CHECK(memcmp(slot + s.piece_len, "\x00\x00\xff\xff", 4) == 0);
    for (uint32_t t = s.piece_len + (s.tail ? 4u : 0u); t < cap; ++t) CHECK(slot[t] == 0xA5);
    ctl.assign((const char*)c, s.ctl_len);
    free(w);
    free(slot);
    free(c);
    return s;
}

static void replay(const std::string& w, const std::vector<Item>& items, uint32_t role, uint32_t chunk, uint32_t cap)
{
    rpp::PieceState st{};
    size_t fed = 0, used = 0, item = 0;
    std::string msg;
    while (used < w.size()) {
        fed = fed + chunk < w.size() ? fed + chunk : w.size();
        while (true) {
            std::string piece, ctl;
            const rpp::PieceState before = st;
            const rpp::Stop s =
                one_walk((const uint8_t*)w.data() + used, (uint32_t)(fed - used), role, true, 0, cap, st, piece, ctl);
            CHECK(s.status == 0);
            if (s.status) return;
            if (s.consumed == 0) CHECK(memcmp(&before, &st, sizeof st) == 0 && s.piece_len == 0);
            used += s.consumed;
            msg += piece;
            const bool last = s.event == fp::EV_MESSAGE;
            if (s.event != fp::EV_NEED_MORE) {
                CHECK(item < items.size());
                if (item >= items.size()) return;
                const Item& it = items[item++];
                if (last) {
                    CHECK(it.kind == 1 && it.bytes == msg && it.op == s.msg_op && it.deflated == s.msg_deflated);
                    CHECK(s.tail == it.deflated && st.rd_remain == 0 && st.rd_fin == 1);
                    msg.clear();
                } else {
                    CHECK(it.kind == s.event && it.kind >= 2 && it.bytes == ctl);
                    if (it.kind == 4) CHECK(s.close_code == 1000);
                }
            }
            const uint8_t none[3] = {0, 0, 0};
            rpp::commit(st, last, 0, 0, none);
            if (last) {
                const rpp::PieceState zero{};
                CHECK(memcmp(&zero, &st, sizeof st) == 0);
            }
            if (s.consumed == 0 && s.event == fp::EV_NEED_MORE) break;   // wants more bytes
        }
    }
    CHECK(item == items.size() && msg.empty());
}

int main()
{
    // EV_PING = 2, EV_PONG = 3, EV_CLOSE = 4 are the Item kinds
    static_assert(fp::EV_PING == 2 && fp::EV_PONG == 3 && fp::EV_CLOSE == 4, "kinds");
    for (int round = 0; round < 6; ++round) {
        const uint32_t role = round & 1;   // server reads masked frames
        std::vector<Item> items;
        const std::string w = make_wire(role == fp::ROLE_SERVER, items);
        const uint32_t caps[] = {8, 12, 13, 64, 4096};
        for (uint32_t cap : caps)
            for (uint32_t chunk = 1; chunk <= w.size(); chunk += (chunk < 40 ? 1 : 37)) replay(w, items, role, chunk, cap);
    }
    // a slot below the minimum gathers nothing
    for (uint32_t cap = 0; cap < rpp::MIN_CAP; ++cap) {
        std::vector<Item> items;
        const std::string w = make_wire(false, items);
        rpp::PieceState st{};
        std::string piece, ctl;
        const rpp::Stop s = one_walk((const uint8_t*)w.data(), (uint32_t)w.size(), fp::ROLE_CLIENT, true, 0, cap, st, piece, ctl);
        CHECK(s.status == fp::E_BUFFER_OVERFLOW && s.consumed == 0 && s.piece_len == 0);
    }
    // random bytes from random states: bounds only
    for (int k = 0; k < 20000; ++k) {
        const std::string w = blob(rnd(64));
        rpp::PieceState st{};
        st.rd_remain = rnd(3) ? rnd(100) : 0;
        st.rd_key = (uint32_t)rng();
        st.rd_cont = rnd(2), st.rd_op = 1 + rnd(2), st.rd_deflated = rnd(2), st.rd_fin = rnd(2);
        st.rd_size = rnd(2) ? rnd(1000) : ~0ull - rnd(4);
        std::string piece, ctl;
        std::string ww = w;
        if (rnd(2) && ww.size() >= 2) ww[1] = (char)((uint8_t)ww[1] | 0x80);
        (void)one_walk((const uint8_t*)ww.data(), (uint32_t)ww.size(), rnd(2), rnd(2) != 0, rnd(2) ? 0 : rnd(300),
                       rnd(40), st, piece, ctl);
    }
    // the UTF-8 carry: every split of a few strings gives the carry of the cut code point
    const char* texts[] = {"a\xc3\xa9z", "\xe2\x82\xac!", "x\xf0\x9f\x98\x80y", "\xf4\x8f\xbf\xbf"};
    for (const char* t : texts) {
        const uint32_t n = (uint32_t)strlen(t);
        for (uint32_t cut = 0; cut <= n; ++cut) {
            uint8_t* a = (uint8_t*)malloc(cut ? cut : 1);
            uint8_t* b = (uint8_t*)malloc(n - cut ? n - cut : 1);
            memcpy(a, t, cut);
            memcpy(b, t + cut, n - cut);
            const rpp::Utf8Head c = rpp::utf8_tail([&](uint32_t i) { return (uint32_t)a[i]; }, cut);
            const rpp::Utf8Head h = rpp::utf8_head(c.n, c.b, [&](uint32_t i) { return (uint32_t)b[i]; }, n - cut);
            CHECK(!h.bad && h.n == 0 && h.skip <= n - cut);
            const rpp::Utf8Head e = rpp::utf8_tail([&](uint32_t i) { return (uint32_t)b[h.skip + i]; }, n - cut - h.skip);
            CHECK(e.n == 0);
            free(a);
            free(b);
        }
    }
    printf("%llu walks, %llu payload bytes stored, %d failures\n", calls, stores, failures);
    return failures ? 1 : 0;
}
