// frame_parse.h -- the header step of the batch receive side: Beast's
// parse_fh (websocket/impl/stream_impl.hpp:701-913) restated as a pure
// function of the bytes at hand and the message state carried from frame to
// frame, with is_valid_close_code and read_close (websocket/detail/frame.hpp:
// 94-126, 196-240).  Host-compilable without HIP: tests/test_frame_parse.py
// compares it with a Python model, tests/cpp/frame_parse_main.cpp fuzzes it
// under the address sanitizer; unframe_kernel (pmd_frame.hip) calls the same
// functions, every lane of a wave with the same arguments.
//
// parse_fh changes rd_size / rd_op / rd_cont and the pmd's rd_set as it goes;
// here the step leaves the state alone and reports what it read, and the
// caller commits a frame (commit_data) only once the whole frame lies in its
// buffer, so a frame that is refused or cut leaves no trace.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BPMD_HD __host__ __device__ inline
#else
#define BPMD_HD inline
#endif

namespace bpmd {
namespace fp {

// Message state between frames (stream_impl.hpp:78-87 rd_size, rd_cont,
// rd_op; impl_base.hpp:61-78 rd_set).  The C ABI's bpmd_rd_state.
struct RdState {
    uint64_t rd_size;      // payload bytes of the current message gathered so far
    uint8_t rd_cont;       // a continuation frame is expected
    uint8_t rd_op;         // opcode of the current message (1 text, 2 binary)
    uint8_t rd_deflated;   // the current message's first frame had RSV1
    uint8_t reserved[5];
};
static_assert(sizeof(RdState) == 16, "RdState is 16 bytes");

// detail::opcode (frame.hpp:28-47)
enum : uint32_t { OP_CONT = 0, OP_TEXT = 1, OP_BINARY = 2, OP_CLOSE = 8, OP_PING = 9, OP_PONG = 10 };
// role_type: whose frames are read
enum : uint32_t { ROLE_SERVER = 0, ROLE_CLIENT = 1 };

// outcome of a header step: NEED_MORE, FRAME, or one of websocket::error
// (the C ABI's bpmd_ws_error values)
enum : int32_t {
    NEED_MORE = 0,
    FRAME = 1,
    E_BAD_FRAME_PAYLOAD = 256,
    E_BUFFER_OVERFLOW = 257,
    E_MESSAGE_TOO_BIG = 258,
    E_BAD_OPCODE = 259,
    E_BAD_DATA_FRAME = 260,
    E_BAD_CONTINUATION = 261,
    E_BAD_RESERVED_BITS = 262,
    E_BAD_CONTROL_FRAGMENT = 263,
    E_BAD_CONTROL_SIZE = 264,
    E_BAD_UNMASKED_FRAME = 265,
    E_BAD_MASKED_FRAME = 266,
    E_BAD_SIZE = 267,
    E_BAD_CLOSE_CODE = 268,
    E_BAD_CLOSE_SIZE = 269,
    E_BAD_CLOSE_PAYLOAD = 270,
};

// detail::frame_header (frame.hpp:50-60) of a FRAME outcome
struct Header {
    uint64_t len;       // payload length
    uint32_t hdr_len;   // header bytes, extended length and key included
    uint32_t key;       // masking key, little-endian from the wire; 0 when unmasked
    uint8_t fin, rsv1, op, masked;
};

BPMD_HD bool is_control(uint32_t op) { return op >= OP_CLOSE; }                        // frame.hpp:85-90
BPMD_HD bool is_reserved(uint32_t op) { return (op >= 3 && op <= 7) || op >= 11; }   // frame.hpp:69-76

// is_valid_close_code (frame.hpp:94-126)
BPMD_HD bool close_code_valid(uint16_t v)
{
    switch (v) {
    case 1000: case 1001: case 1002: case 1003: case 1007: case 1008: case 1009: case 1010: case 1011: case 1012:
    case 1013: case 1014:
        return true;
    case 1004: case 1005: case 1006: case 1015:   // explicitly reserved
        return false;
    }
    if (v >= 1016 && v <= 2999) return false;   // reserved
    if (v <= 999) return false;                 // not used
    return true;
}

// The header at p, of which `avail` bytes are there; no byte at or beyond
// p + avail is read.  role: ROLE_SERVER wants masked frames, ROLE_CLIENT
// unmasked ones.  pmd_on: RSV1 is legal on a message's first frame
// (impl_base.hpp:61-78; without the extension :381-390 refuses it).
// msg_max: rd_msg_max, 0 = no limit.  out_room: capacity of the slot the
// message is gathered into.  The checks run in parse_fh's order.
BPMD_HD int32_t parse_fh(const uint8_t* p, uint64_t avail, uint32_t role, bool pmd_on, uint64_t msg_max,
                         uint64_t out_room, const RdState& st, Header& h)
{
    if (avail < 2) return NEED_MORE;   // :706-711
    const uint32_t b0 = p[0], b1 = p[1];
    const uint32_t len7 = b1 & 0x7fu;
    uint32_t need = len7 == 126 ? 2u : len7 == 127 ? 8u : 0u;
    const bool masked = (b1 & 0x80u) != 0;
    if (masked) need += 4;
    if (avail - 2 < need) return NEED_MORE;   // :731-736
    const uint32_t op = b0 & 0x0fu;
    const bool fin = (b0 & 0x80u) != 0, rsv1 = (b0 & 0x40u) != 0, rsv2 = (b0 & 0x20u) != 0, rsv3 = (b0 & 0x10u) != 0;
    switch (op) {   // :744-804
    case OP_BINARY:
    case OP_TEXT:
        if (st.rd_cont) return E_BAD_DATA_FRAME;
        if (rsv2 || rsv3 || (rsv1 && !pmd_on)) return E_BAD_RESERVED_BITS;
        break;
    case OP_CONT:
        if (!st.rd_cont) return E_BAD_CONTINUATION;
        if (rsv1 || rsv2 || rsv3) return E_BAD_RESERVED_BITS;
        break;
    default:
        if (is_reserved(op)) return E_BAD_OPCODE;
        if (!fin) return E_BAD_CONTROL_FRAGMENT;
        if (len7 > 125) return E_BAD_CONTROL_SIZE;
        if (rsv1 || rsv2 || rsv3) return E_BAD_RESERVED_BITS;
        break;
    }
    if (role == ROLE_SERVER && !masked) return E_BAD_UNMASKED_FRAME;   // :805-810
    if (role == ROLE_CLIENT && masked) return E_BAD_MASKED_FRAME;      // :811-816
    // :817-823 keeps a control frame until its payload is there; the caller
    // does so for every frame (whole frames only), after this step
    uint64_t len = len7;
    uint32_t at = 2;
    if (len7 == 126) {   // :826-840
        len = (uint64_t)p[2] << 8 | p[3];
        at = 4;
        if (len < 126) return E_BAD_SIZE;
    } else if (len7 == 127) {   // :841-861
        len = 0;
        for (uint32_t i = 0; i < 8; ++i) len = len << 8 | p[2 + i];
        at = 10;
        if (len < 65536) return E_BAD_SIZE;
        if (len >> 63) return E_BAD_SIZE;
    }
    uint32_t key = 0;
    if (masked) {   // :863-871
        key = (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
        at += 4;
    }
    if (!is_control(op)) {   // :877-909
        uint64_t size = 0;
        bool deflated = pmd_on && rsv1;
        if (op == OP_CONT) {
            size = st.rd_size;
            deflated = pmd_on && st.rd_deflated;
            if (size > ~(uint64_t)0 - len) return E_MESSAGE_TOO_BIG;
        }
        // an inflated size is checked while inflating (:894-906)
        if (!deflated && msg_max && (len > msg_max || size > msg_max - len)) return E_MESSAGE_TOO_BIG;
        // this library's own: the gathered message must fit its slot, known
        // here, or a frame announcing 2^63 - 1 bytes would wait for them
        if (len > out_room || size > out_room - len) return E_BUFFER_OVERFLOW;
    }
    h.len = len;
    h.hdr_len = at;
    h.key = key;
    h.fin = fin, h.rsv1 = rsv1, h.op = (uint8_t)op, h.masked = masked;
    return FRAME;
}

// A data frame consumed (:877-909): returns the offset in the out slot its
// payload starts at.  On FIN the caller reports the message and resets.
BPMD_HD uint64_t commit_data(RdState& st, const Header& h, bool pmd_on)
{
    if (h.op != OP_CONT) {
        st.rd_size = 0;
        st.rd_op = h.op;
        st.rd_deflated = pmd_on && h.rsv1;
    }
    const uint64_t at = st.rd_size;
    st.rd_size += h.len;
    st.rd_cont = !h.fin;
    return at;
}

BPMD_HD void reset(RdState& st)
{
    st.rd_size = 0;
    st.rd_cont = st.rd_op = st.rd_deflated = 0;
    for (int i = 0; i < 5; ++i) st.reserved[i] = 0;
}

// check_utf8 (utf8_checker.ipp:317-324: write() then finish()) over n bytes
// that get(i) yields: well-formed UTF-8 of RFC 3629, complete at the end.
// Serial, for the at most 123 bytes of a close reason.
template <class Get>
BPMD_HD bool utf8_complete(Get get, uint32_t n)
{
    uint32_t i = 0;
    while (i < n) {
        const uint32_t c = get(i);
        if (c < 0x80) {
            ++i;
            continue;
        }
        uint32_t more, lo = 0x80, hi = 0xbf;
        if (c >= 0xc2 && c <= 0xdf) more = 1;
        else if (c >= 0xe0 && c <= 0xef) {
            more = 2;
            if (c == 0xe0) lo = 0xa0;
            if (c == 0xed) hi = 0x9f;
        } else if (c >= 0xf0 && c <= 0xf4) {
            more = 3;
            if (c == 0xf0) lo = 0x90;
            if (c == 0xf4) hi = 0x8f;
        } else
            return false;
        if (n - i <= more) return false;   // ends inside the code point (or is invalid before)
        for (uint32_t k = 1; k <= more; ++k) {
            const uint32_t d = get(i + k);
            if (d < (k == 1 ? lo : 0x80u) || d > (k == 1 ? hi : 0xbfu)) return false;
        }
        i += more + 1;
    }
    return true;
}

// read_close (frame.hpp:196-240) over the n <= 125 unmasked payload bytes
// get(i) yields: the close code (0 = none) and 0 or the error
template <class Get>
BPMD_HD int32_t read_close(Get get, uint32_t n, uint16_t& code)
{
    code = 0;
    if (n == 0) return 0;
    if (n == 1) return E_BAD_CLOSE_SIZE;
    code = (uint16_t)(get(0) << 8 | get(1));
    if (!close_code_valid(code)) return E_BAD_CLOSE_CODE;
    if (n > 2 && !utf8_complete([&](uint32_t i) { return get(i + 2); }, n - 2)) return E_BAD_CLOSE_PAYLOAD;
    return 0;
}

// what stopped a walk (the C ABI's bpmd_event)
enum : uint32_t { EV_NEED_MORE = 0, EV_MESSAGE = 1, EV_PING = 2, EV_PONG = 3, EV_CLOSE = 4 };

struct Stop {
    uint64_t msg_len;        // the message's payload bytes: complete after EV_MESSAGE, else gathered so far
    uint32_t consumed;       // wire bytes of the frames consumed
    uint32_t event;
    int32_t status;          // 0, a refused header's error, or read_close's
    uint32_t msg_op, msg_deflated;
    uint32_t ctl_len;        // payload bytes of the control frame that stopped the walk
    uint16_t close_code;
};

// One entry of bpmd_unframe_batch (include/beast_pmd.h): read_some's frame
// loop (read.hpp:1085-1283) over the wl bytes at p, whole frames only, up to
// the first complete message, control frame, refused header or the end of
// the bytes.  put_data(at, src, len, key) appends a data frame's payload
// (masked bytes at src, len of them) at offset `at` of the out slot, whose
// capacity `cap` the header step has checked; put_ctl(src, len, key) stores a
// control payload.  On the device every lane of a wave runs this with the
// same arguments and the two callbacks share the copy among the lanes.
template <class PutData, class PutCtl>
BPMD_HD void walk(const uint8_t* p, uint32_t wl, uint32_t role, bool pmd_on, uint64_t msg_max, uint32_t cap, RdState& st,
                  PutData put_data, PutCtl put_ctl, Stop& s)
{
    uint32_t pos = 0;
    s.event = EV_NEED_MORE;
    s.status = 0;
    s.ctl_len = 0;
    s.close_code = 0;
    bool message = false;
    while (true) {
        Header h;
        const int32_t r = parse_fh(p + pos, wl - pos, role, pmd_on, msg_max, cap, st, h);
        if (r == NEED_MORE) break;
        if (r != FRAME) {
            s.status = r;
            break;
        }
        if (h.len > (uint64_t)(wl - pos - h.hdr_len)) break;   // payload cut: the frame stays
        const uint8_t* src = p + pos + h.hdr_len;
        const uint32_t len = (uint32_t)h.len, key = h.key;
        pos += h.hdr_len + len;
        if (is_control(h.op)) {   // read.hpp:1117-1199
            put_ctl(src, len, key);
            s.ctl_len = len;
            s.event = h.op == OP_PING ? EV_PING : h.op == OP_PONG ? EV_PONG : EV_CLOSE;
            if (h.op == OP_CLOSE)
                s.status = read_close(
                    [&](uint32_t i) { return (uint32_t)(uint8_t)(src[i] ^ (uint8_t)(key >> (8 * (i & 3u)))); }, len,
                    s.close_code);
            break;
        }
        const uint64_t at = commit_data(st, h, pmd_on);
        put_data(at, src, len, key);
        if (h.fin) {   // read.hpp:1281-1283
            s.event = EV_MESSAGE;
            s.msg_len = st.rd_size, s.msg_op = st.rd_op, s.msg_deflated = st.rd_deflated;
            reset(st);
            message = true;
            break;
        }
    }
    if (!message) s.msg_len = st.rd_size, s.msg_op = st.rd_op, s.msg_deflated = st.rd_deflated;
    s.consumed = pos;
}

}  // namespace fp
}  // namespace bpmd
