// send_plan.h -- the plan of the batch send side: what write_some decides
// about one message before any payload byte moves (websocket/impl/write.hpp:
// 625-831, websocket/impl/stream_impl.hpp:225-252), restated as pure functions
// of the message's length and the stream's options, with the frame header
// writer (detail::write, websocket/detail/frame.hpp:134-175) and the control
// frames of write_ping / write_close (stream_impl.hpp:915-996).
// Host-compilable without HIP: tests/test_send_plan.py compares it with a
// Python model, tests/cpp/send_plan_main.cpp runs it under the address
// sanitizer; the kernels of pmd_send.hip call the same functions.
//
// frame_kernel (pmd_frame.hip) walks a message's frames one after the other
// and adds up where each starts.  Here every frame of a message but the last
// has the same payload and so the same header, which gives frame f's wire
// offset in closed form: any wave can start at any frame.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BPMD_SP_HD __host__ __device__ inline
#else
#define BPMD_SP_HD inline
#endif

namespace bpmd {
namespace sp {

// role_type of the sending end: a client masks (write.hpp:679-685)
enum : uint32_t { ROLE_SERVER = 0, ROLE_CLIENT = 1 };
// detail::opcode (frame.hpp:28-47)
enum : uint32_t { OP_CONT = 0, OP_TEXT = 1, OP_BINARY = 2, OP_CLOSE = 8, OP_PING = 9, OP_PONG = 10 };
// per-message outcomes, numbered as include/beast_pmd.h does
enum : int32_t { E_NEED_BUFFERS = 1, E_BUFFER_OVERFLOW = 257, E_BAD_OPCODE = 259, E_BAD_CONTROL_SIZE = 264 };

constexpr uint32_t CTL_SLOT = 128;    // bytes of a control payload slot (bpmd_unframe_batch's d_ctl)
constexpr uint32_t CTL_WIRE = 144;    // bytes of a control frame's wire slot
constexpr uint32_t CTL_MAX = 125;     // most payload bytes of a control frame (RFC 6455 5.5)
constexpr uint32_t REASON_MAX = 123;  // most bytes of a close reason (close_reason, rfc6455.hpp)

// begin_msg (stream_impl.hpp:225-252): compress this message?
BPMD_SP_HD bool compress(bool pmd_on, bool opt, uint64_t len, uint64_t threshold)
{
    return pmd_on && opt && len >= threshold;
}

// deflate_upper_bound (zlib/deflate_stream.hpp:402-410), bpmd_deflate_upper_bound
BPMD_SP_HD uint64_t deflate_bound(uint64_t n) { return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 11; }

// bytes of a frame header (frame.hpp:134-175)
BPMD_SP_HD uint32_t hdr_len(uint64_t len, bool masked)
{
    return (len <= 125 ? 2u : len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u);
}

// The frames of one message: `frames` of them, all but the last with `unit`
// payload bytes, the last with `last`.
struct Split {
    uint64_t frames, unit, last;
};

// len: the bytes that go on the wire (the deflated payload of a compressed
// message).  A compressed message goes out in frames of at most frame_max
// bytes whatever auto_fragment says (write.hpp:655-703: one frame per wr_buf
// fill); an uncompressed one does so with auto_fragment (:721-748, :795-829)
// and is one frame without (:706-720, :750-794).  An empty payload is one
// empty frame.  frame_max != 0.
BPMD_SP_HD Split split(uint64_t len, uint32_t frame_max, bool compressed, bool frag)
{
    Split s;
    if (len == 0 || (!compressed && !frag)) {
        s.frames = 1, s.unit = len, s.last = len;
        return s;
    }
    s.frames = (len + frame_max - 1) / frame_max;
    s.unit = frame_max;
    s.last = len - (s.frames - 1) * frame_max;
    return s;
}

BPMD_SP_HD uint64_t frame_len(const Split& s, uint64_t f) { return f + 1 < s.frames ? s.unit : s.last; }
// payload offset and wire offset of frame f inside its message
BPMD_SP_HD uint64_t frame_src(const Split& s, uint64_t f) { return f * s.unit; }
BPMD_SP_HD uint64_t frame_off(const Split& s, bool masked, uint64_t f) { return f * (hdr_len(s.unit, masked) + s.unit); }
BPMD_SP_HD uint64_t wire_size(const Split& s, bool masked)
{
    return frame_off(s, masked, s.frames - 1) + hdr_len(s.last, masked) + s.last;
}

// The header of frame f of `frames` (detail::write): bytes 0-7 in h0, 8-13 in
// h1, little-endian (byte i of the header is byte i of h0, or byte i - 8 of
// h1); returns their count.  FIN on the last frame, RSV1 and the opcode on the
// first and cont after, MASK and the key (little-endian on the wire) when
// masked.
BPMD_SP_HD uint32_t header(uint64_t len, bool first, bool fin, bool rsv1, uint32_t op, bool masked, uint32_t key,
                           uint64_t& h0, uint64_t& h1)
{
    const uint64_t b0 = (fin ? 0x80u : 0u) | (first && rsv1 ? 0x40u : 0u) | (first ? op & 15u : 0u);
    const uint64_t m = masked ? 0x80u : 0u;
    uint32_t hl;
    h1 = 0;
    if (len <= 125) {
        h0 = b0 | (m | len) << 8;
        hl = 2;
    } else if (len <= 65535) {
        h0 = b0 | (m | 126u) << 8 | (len >> 8) << 16 | (len & 0xffu) << 24;
        hl = 4;
    } else {
        // 64-bit big-endian length in bytes 2..9
        h0 = b0 | (m | 127u) << 8;
        for (uint32_t i = 0; i < 6; ++i) h0 |= ((len >> (8 * (7 - i))) & 0xffu) << (8 * (2 + i));
        h1 = ((len >> 8) & 0xffu) | (len & 0xffu) << 8;
        hl = 10;
    }
    if (masked) {
        if (hl == 10) h1 |= (uint64_t)key << 16;
        else h0 |= (uint64_t)key << (8 * hl);
        hl += 4;
    }
    return hl;
}
BPMD_SP_HD uint8_t header_byte(uint64_t h0, uint64_t h1, uint32_t i)
{
    return (uint8_t)((i < 8 ? h0 >> (8 * i) : h1 >> (8 * (i - 8))) & 0xffu);
}

// What a caller can know from a message's input length alone: the most
// frames and the most wire bytes any decision and any deflate result of at
// most deflate_bound(len) bytes can give (wire_size grows with the payload).
// may_compress: the message may be compressed (pmd_on and its opt).
BPMD_SP_HD uint64_t frame_bound(uint64_t len, uint32_t frame_max, bool may_compress, bool frag)
{
    const uint64_t plain = split(len, frame_max, false, frag).frames;
    if (!may_compress) return plain;
    const uint64_t z = split(deflate_bound(len), frame_max, true, frag).frames;
    return z > plain ? z : plain;
}
BPMD_SP_HD uint64_t wire_bound(uint64_t len, uint32_t frame_max, bool masked, bool may_compress, bool frag)
{
    const uint64_t plain = wire_size(split(len, frame_max, false, frag), masked);
    if (!may_compress) return plain;
    const uint64_t z = wire_size(split(deflate_bound(len), frame_max, true, frag), masked);
    return z > plain ? z : plain;
}

// A control frame (write_ping, write_close: stream_impl.hpp:915-996): FIN, no
// RSV bits, one frame.  slot_len: the bytes of the entry's payload slot; code:
// the close code.  Ping and pong carry the slot (at most 125 bytes); a close
// with a code carries the code big-endian and then the slot as the reason (at
// most 123 bytes); a close with code 0 is empty whatever the slot holds.
// Returns 0 and the payload length, or the error.
BPMD_SP_HD int32_t control_plan(uint32_t op, uint32_t slot_len, uint32_t code, uint32_t& payload_len)
{
    payload_len = 0;
    if (op == OP_PING || op == OP_PONG) {
        if (slot_len > CTL_MAX) return E_BAD_CONTROL_SIZE;
        payload_len = slot_len;
        return 0;
    }
    if (op != OP_CLOSE) return E_BAD_OPCODE;
    if (code == 0) return 0;
    if (slot_len > REASON_MAX) return E_BAD_CONTROL_SIZE;
    payload_len = 2 + slot_len;
    return 0;
}
BPMD_SP_HD uint32_t control_size(uint32_t payload_len, bool masked) { return 2u + (masked ? 4u : 0u) + payload_len; }
// byte t of the frame control_plan accepted; slot is read below slot_len only
BPMD_SP_HD uint8_t control_byte(uint32_t t, uint32_t op, uint32_t payload_len, uint32_t code, const uint8_t* slot,
                                bool masked, uint32_t key)
{
    if (t == 0) return (uint8_t)(0x80u | op);
    if (t == 1) return (uint8_t)((masked ? 0x80u : 0u) | payload_len);
    const uint32_t hl = masked ? 6u : 2u;
    if (t < hl) return (uint8_t)(key >> (8 * (t - 2)));
    const uint32_t j = t - hl;
    uint8_t b;
    if (op == OP_CLOSE) b = j == 0 ? (uint8_t)(code >> 8) : j == 1 ? (uint8_t)code : slot[j - 2];
    else b = slot[j];
    return masked ? (uint8_t)(b ^ (uint8_t)(key >> (8 * (j & 3u)))) : b;
}

}  // namespace sp
}  // namespace bpmd
