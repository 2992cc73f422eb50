/*
 * beast_pmd.h -- C ABI of the MI355X permessage-deflate engine.
 *
 * Drop-in boundary for Boost.Beast's WebSocket permessage-deflate path.  In
 * Beast the only caller of the codec is websocket::stream<..., true> through
 * impl_base<true> (include/boost/beast/websocket/detail/impl_base.hpp:85-202),
 * which calls exactly:
 *     zo.reset(level, wbits, memLevel, Strategy::normal)   impl_base.hpp:295-307
 *     zo.write(zs, Flush::{none,block,sync}, ec)            impl_base.hpp:104-141
 *     zo.reset()                                            impl_base.hpp:156-166
 *     zi.reset(wbits)  zi.write(zs, Flush::sync, ec)        impl_base.hpp:168-190, 295-305
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes only.  All functions are noexcept and
 * return 0 on success or a negative bpmd_result; per-message outcomes are
 * Beast's zlib::error values (include/boost/beast/zlib/error.hpp:48-138) in
 * the status array.  Device pointers refer to memory of the current HIP
 * device; `stream` is a hipStream_t (0 = default stream).  Batch calls are
 * asynchronous on `stream`: they enqueue their kernels and return without
 * waiting for the device (bpmd_inflate_batch / bpmd_read_batch of every size,
 * the block-parallel path of long payloads included; deflate of messages of
 * at most 4 KiB), with two exceptions, both waits on `stream`:
 *   - bpmd_deflate_batch / bpmd_write_batch with a message longer than
 *     4 KiB (or any context-takeover deflate) read back a 4-byte chunk count
 *     that sizes their chunk workspace, so they return only once the work
 *     queued on `stream` before them has run (the short messages' kernel is
 *     enqueued before the wait and runs meanwhile);
 *   - a call that needs more device workspace than its stream's pool holds
 *     (work queues, chunk scratch, block-parallel decode workspace) grows
 *     the pool, and freeing the smaller block waits for `stream` to drain;
 *     a stream that repeats one batch shape grows it only on the first calls;
 *   - the first inflate call on a stream that decodes long payloads
 *     block-parallel reads back that batch's workspace totals once (so the
 *     first call already runs the fast path), unless bpmd_inflate_reserve()
 *     sized the stream before.  That read-back waits for the work queued on
 *     the stream before the call, so a stream that is being captured into a
 *     graph (hipStreamBeginCapture) must be reserved first.
 * Concurrent calls from several host threads on one stream are serialised
 * per stream.
 */
#ifndef BEAST_PMD_H
#define BEAST_PMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* zlib::error (zlib/error.hpp:48-138) */
enum bpmd_status {
    BPMD_OK = 0,
    BPMD_NEED_BUFFERS = 1,
    BPMD_END_OF_STREAM = 2,
    BPMD_NEED_DICT = 3,
    BPMD_STREAM_ERROR = 4,
    BPMD_INVALID_BLOCK_TYPE = 5,
    BPMD_INVALID_STORED_LENGTH = 6,
    BPMD_TOO_MANY_SYMBOLS = 7,
    BPMD_INVALID_CODE_LENGTHS = 8,
    BPMD_INVALID_BIT_LENGTH_REPEAT = 9,
    BPMD_MISSING_EOB = 10,
    BPMD_INVALID_LITERAL_LENGTH = 11,
    BPMD_INVALID_DISTANCE_CODE = 12,
    BPMD_INVALID_DISTANCE = 13,
    BPMD_OVER_SUBSCRIBED_LENGTH = 14,
    BPMD_INCOMPLETE_LENGTH_SET = 15,
    BPMD_GENERAL = 16
};

/* call-level results (negative) */
enum bpmd_result {
    BPMD_R_OK = 0,
    BPMD_R_INVALID_ARGUMENT = -1,   /* reference throws std::invalid_argument */
    BPMD_R_DOMAIN_ERROR = -2,       /* reference throws std::domain_error */
    BPMD_R_HIP_ERROR = -3,
    BPMD_R_NO_DEVICE = -4
};

/* zlib::Strategy (zlib/zlib.hpp:209-246) */
enum bpmd_strategy {
    BPMD_STRATEGY_NORMAL = 0, BPMD_STRATEGY_FILTERED = 1, BPMD_STRATEGY_HUFFMAN = 2,
    BPMD_STRATEGY_RLE = 3, BPMD_STRATEGY_FIXED = 4
};

/* flags */
#define BPMD_F_RAW 1u   /* inflate: plain inflate_stream::write() semantics, no 00 00 FF FF tail */
#define BPMD_F_EXACT 2u /* deflate: payloads bit-identical to Beast's deflate_stream (the
                           reference's parse, block splits and trees; slower). Not with
                           context takeover. */

/* Codec configuration: the subset of websocket::permessage_deflate
 * (websocket/option.hpp:34-67) that reaches the codec after negotiation
 * (impl_base.hpp:277-309). */
typedef struct bpmd_cfg {
    int level;        /* compLevel 0..9 (-1 = 6) */
    int window_bits;  /* 9..15 for deflate (8 is bumped to 9), 8..15 for inflate */
    int mem_level;    /* 1..9 */
    int strategy;     /* bpmd_strategy */
    uint32_t flags;
} bpmd_cfg;

/* Library / device bring-up.  Idempotent.  Returns BPMD_R_NO_DEVICE when no
 * HIP device is visible (the engine has no CPU fallback). */
int bpmd_init(void);
/* Library version string. */
const char* bpmd_version(void);

/* Batched inflate of independent permessage-deflate payloads (replaces one
 * zi.reset(wbits) + zi.write(zs, Flush::sync) + inflate_with_eb() sequence
 * per message: impl_base.hpp:168-190, websocket/impl/read.hpp:1284-1356).
 *   d_in + d_in_off[i], d_in_len[i]   payload i without the 00 00 FF FF tail
 *   d_out + d_out_off[i], d_out_cap[i] output slot i
 *   d_out_len[i]  bytes produced;  d_status[i]  zlib::error of message i
 *                 (need_buffers = output exceeded d_out_cap[i])
 * No byte outside [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written. */
int bpmd_inflate_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                       const uint32_t* d_in_len, uint32_t n_msgs, uint8_t* d_out,
                       const uint64_t* d_out_off, const uint32_t* d_out_cap,
                       uint32_t* d_out_len, int32_t* d_status, void* stream);

/* Workspace for the block-parallel decode of long payloads on `stream`
 * (no Beast counterpart: the reference decodes on the caller's thread).  Sizes
 * the stream's capacity for batches whose long payloads total at most
 * in_bytes of compressed input, out_bytes of output capacity and n_long
 * payloads, so that no later call on the stream waits to size it; a long
 * payload that does not fit a stream's capacity is still decoded exactly, by
 * the slower wave kernel.  The capacity never exceeds half the device's free
 * memory.  Optional: without it the stream's first such call sizes it. */
int bpmd_inflate_reserve(void* stream, uint64_t in_bytes, uint64_t out_bytes, uint32_t n_long);

/* Batched deflate of independent messages into permessage-deflate payloads
 * (replaces one zo.write(zs, Flush::none) ... zo.write(zs, Flush::block),
 * zo.write(zs, Flush::sync), strip 00 00 FF FF, zo.reset() sequence per
 * message under no_context_takeover: impl_base.hpp:85-166,
 * websocket/impl/write.hpp:655-703).  cfg->level / window_bits / mem_level
 * are validated as deflate_stream::reset (deflate_stream.ipp:227-265);
 * strategy selects the parser as zlib::Strategy does.  The payload is a
 * valid raw-DEFLATE stream whose blocks all have BFINAL = 0, ending with
 * the header bits of an empty stored block padded to a byte, exactly the
 * framing Beast produces; the block contents are this engine's own parse
 * (byte-identical round trip, compressed size within the tolerance stated
 * in DESIGN.md).
 *   d_in + d_in_off[i], d_in_len[i]     message i
 *   d_out + d_out_off[i], d_out_cap[i]  output slot i (bpmd_deflate_upper_bound(len) always suffices)
 *   d_out_len[i]  payload bytes;  d_status[i]  0, or need_buffers if the
 *                 slot was too small (d_out_len[i] = 0, slot contents undefined)
 * A slot one byte larger than the payload is always accepted.  A slot of
 * exactly the payload's size is accepted for a message of at most 4 KiB;
 * for a longer one (and for every message of a context-takeover batch) it is
 * refused when the last block is Huffman-coded and ends 1-5 bits into a byte.
 * No byte outside [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written. */
int bpmd_deflate_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                       const uint32_t* d_in_len, uint32_t n_msgs, uint8_t* d_out,
                       const uint64_t* d_out_off, const uint32_t* d_out_cap,
                       uint32_t* d_out_len, int32_t* d_status, void* stream);

/* Inflate kernel selection (no reference counterpart; tuning and tests):
 * 0 automatic (one lane per message for batches of >= 2048 messages, one
 * wave per message below), 1 always lane-per-message, 2 always
 * wave-per-message.  Both produce identical results.  Initial value from
 * the BPMD_INFLATE environment variable ("lane" / "wave"). */
int bpmd_set_inflate_kernel(int mode);

/* deflate_upper_bound (zlib/deflate_stream.hpp:402-410): size a d_out slot. */
size_t bpmd_deflate_upper_bound(size_t n);

/* ---------------------------------------------------------------------
 * One process, several GPUs.  Messages are
 * independent streams, so a batch splits into contiguous, byte-balanced
 * message ranges, one per device; every shard's buffers live on its own
 * device and no payload crosses GPUs.
 * ------------------------------------------------------------------- */

/* Byte-balanced contiguous ranges (beast_amd/shard.py): shard p is messages
 * [starts[p], starts[p+1]), starts has n_parts + 1 entries; shard r ends at
 * the first message whose byte prefix sum reaches (r + 1) / n_parts of the
 * total.  Host only. */
int bpmd_shard_ranges(const uint32_t* lens, uint32_t n, int n_parts, uint32_t* starts);

/* One shard: device pointers of `device`, launched on `stream` (a
 * hipStream_t of that device, 0 = its default stream). */
typedef struct bpmd_shard {
    int device;
    void* stream;
    const uint8_t* d_in;
    const uint64_t* d_in_off;
    const uint32_t* d_in_len;
    uint32_t n_msgs;
    uint8_t* d_out;
    const uint64_t* d_out_off;
    const uint32_t* d_out_cap;
    uint32_t* d_out_len;
    int32_t* d_status;
} bpmd_shard;

/* bpmd_inflate_batch / bpmd_deflate_batch on every shard, each on its own
 * device and stream, asynchronously; each shard is launched from a host
 * thread of its own, so a shard whose call waits on its stream (deflate of
 * messages over 4 KiB) does not hold back the others.  out_bytes (n_shards entries, or NULL):
 * each shard's total output bytes (sum of its d_out_len), gathered to the
 * host -- the call then waits for every shard -- so each shard's offset in
 * one global output is the exclusive prefix sum.  The current device is
 * restored. */
int bpmd_inflate_batch_multi(const bpmd_cfg* cfg, const bpmd_shard* shards, int n_shards, uint64_t* out_bytes);
int bpmd_deflate_batch_multi(const bpmd_cfg* cfg, const bpmd_shard* shards, int n_shards, uint64_t* out_bytes);

/* ---------------------------------------------------------------------
 * Frame-adjacent byte passes.  Masking keys are the
 * frame header's 32-bit key as Beast reads it, little-endian from the wire
 * (stream_impl.hpp:866-870): payload byte j is XORed with byte (j + phase) % 4
 * of the key (prepare_key / mask_inplace, websocket/detail/mask.ipp:20-59).
 * ------------------------------------------------------------------- */

/* Batched mask_inplace (mask.ipp:38-59), in place.  d_phase[i] is the key
 * rotation a prepared_key carries after masking the frame's earlier bytes
 * (rol, mask.ipp:29-36), i.e. their count mod 4; NULL = 0.  Masking is an
 * involution: the same call masks (write.hpp:679-685) and unmasks
 * (read.hpp:1324-1327). */
int bpmd_mask_batch(uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t n_msgs,
                    const uint32_t* d_key, const uint8_t* d_phase, void* stream);

/* utf8_checker verdicts (websocket/detail/utf8_checker.ipp) */
enum bpmd_utf8 {
    BPMD_UTF8_VALID = 0,       /* write() and finish() succeed */
    BPMD_UTF8_INCOMPLETE = 1,  /* write() succeeds, finish() fails: ends inside a code point */
    BPMD_UTF8_INVALID = 2      /* write() fails */
};

/* Batched check_utf8 (utf8_checker.ipp:317-324) keeping the verdict of one
 * utf8_checker::write() over each whole message: d_result[i] = bpmd_utf8.
 * Feeding a message in pieces gives the same verdicts: the fail-fast rule
 * (utf8_checker.ipp:86-157) rejects exactly the invalid prefixes. */
int bpmd_utf8_check_batch(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t n_msgs,
                          int32_t* d_result, void* stream);

/* websocket::error::bad_frame_payload (websocket/error.hpp): the per-message
 * status bpmd_read_batch reports for a text message that is not UTF-8. */
#define BPMD_BAD_FRAME_PAYLOAD 256

/* Receive side of a batch of permessage-deflate messages, fused
 * (read.hpp:1284-1385): unmask the payload inside inflate's input loads
 * (server role, read.hpp:1324-1327; d_key NULL = unmasked), inflate as
 * bpmd_inflate_batch, then check the inflated bytes of text messages
 * (d_text[i] != 0; NULL = all binary) as read.hpp:1372-1384 does.
 * d_status[i]: inflate's zlib::error if nonzero, else BPMD_BAD_FRAME_PAYLOAD
 * for a text message that is not valid UTF-8, else 0.  d_in is not
 * modified. */
int bpmd_read_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                    const uint32_t* d_key, const uint8_t* d_text, uint32_t n_msgs, uint8_t* d_out,
                    const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                    void* stream);

/* Send side, fused (write.hpp:655-703): deflate as bpmd_deflate_batch and
 * mask each payload with d_key[i] inside the kernel's output stores (client
 * role, write.hpp:679-685; d_key NULL = unmasked). */
int bpmd_write_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                     const uint32_t* d_key, uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                     const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status, void* stream);

/* Frames of a batch of messages on the send side, as write_some sends a
 * compressed message (websocket/impl/write.hpp:463-545) with headers written
 * by detail::write (websocket/detail/frame.hpp:134-175): message i's payload
 * d_in + d_in_off[i] (d_in_len[i] bytes, e.g. bpmd_deflate_batch's output)
 * goes out in frames of at most frame_max bytes (Beast's wr_buf_size; one
 * empty frame for an empty payload).  Frame f: FIN on the last, RSV1 on the
 * first when d_flags[i] & 1 (compressed; NULL = all compressed), opcode
 * d_op[i] on the first (NULL = binary, 2) and cont (0) after; with d_keys
 * (client role) the MASK bit, key d_keys[d_key_base[i] + f] in the header
 * (little-endian) and the frame's payload masked with it (a fresh
 * prepare_key per frame).  The wire bytes go to d_wire + d_wire_off[i];
 * bpmd_frame_wire_size gives their count.  Any split is a valid RFC 6455
 * message; Beast's own split also depends on when its deflater flushes. */
uint64_t bpmd_frame_wire_size(uint64_t payload_len, uint32_t frame_max, int masked);
int bpmd_frame_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const uint8_t* d_op,
                     const uint8_t* d_flags, const uint32_t* d_keys, const uint32_t* d_key_base, uint32_t frame_max,
                     uint32_t n_msgs, uint8_t* d_wire, const uint64_t* d_wire_off, void* stream);

/* ---------------------------------------------------------------------
 * Receive side: from wire bytes to message payloads.  What read_some does
 * per connection (websocket/impl/read.hpp:1063-1283) around parse_fh
 * (websocket/impl/stream_impl.hpp:701-913), over a batch of connections.
 * ------------------------------------------------------------------- */

/* The message state parse_fh keeps between frames (stream_impl.hpp:78-87
 * rd_size, rd_op, rd_cont; impl_base.hpp:61-78 rd_set), one per entry.  All
 * zero = between messages. */
typedef struct bpmd_rd_state {
    uint64_t rd_size;    /* payload bytes of the current message gathered so far */
    uint8_t rd_cont;     /* a continuation frame is expected */
    uint8_t rd_op;       /* opcode of the current message: 1 text, 2 binary */
    uint8_t rd_deflated; /* the current message's first frame had RSV1 */
    uint8_t reserved[5]; /* zero */
} bpmd_rd_state;

/* role_type (websocket/rfc6455.hpp) of the reading end */
enum bpmd_role {
    BPMD_ROLE_SERVER = 0, /* frames must be masked (stream_impl.hpp:805-810) */
    BPMD_ROLE_CLIENT = 1  /* frames must not be masked (stream_impl.hpp:811-816) */
};

/* What stopped an entry's walk (d_event) */
enum bpmd_event {
    BPMD_EV_NEED_MORE = 0, /* the buffer ended, or d_status[i] holds a parse error */
    BPMD_EV_MESSAGE = 1,   /* a FIN data frame: the message is complete (read.hpp:1281-1283) */
    BPMD_EV_PING = 2,      /* read.hpp:1130-1150 */
    BPMD_EV_PONG = 3,      /* read.hpp:1151-1160 */
    BPMD_EV_CLOSE = 4      /* read.hpp:1161-1199 */
};

/* websocket::error (websocket/error.hpp:22-226) values of d_status, beside
 * BPMD_BAD_FRAME_PAYLOAD; all above every zlib::error value. */
enum bpmd_ws_error {
    BPMD_WS_BUFFER_OVERFLOW = 257,      /* error::buffer_overflow: the message does not fit d_out_cap[i] */
    BPMD_WS_MESSAGE_TOO_BIG = 258,      /* error::message_too_big (stream_impl.hpp:886-906) */
    BPMD_WS_BAD_OPCODE = 259,           /* error::bad_opcode (:779-784) */
    BPMD_WS_BAD_DATA_FRAME = 260,       /* error::bad_data_frame (:748-753) */
    BPMD_WS_BAD_CONTINUATION = 261,     /* error::bad_continuation (:764-769) */
    BPMD_WS_BAD_RESERVED_BITS = 262,    /* error::bad_reserved_bits (:754-760, :770-775, :797-802) */
    BPMD_WS_BAD_CONTROL_FRAGMENT = 263, /* error::bad_control_fragment (:785-790) */
    BPMD_WS_BAD_CONTROL_SIZE = 264,     /* error::bad_control_size (:791-796) */
    BPMD_WS_BAD_UNMASKED_FRAME = 265,   /* error::bad_unmasked_frame (:805-810) */
    BPMD_WS_BAD_MASKED_FRAME = 266,     /* error::bad_masked_frame (:811-816) */
    BPMD_WS_BAD_SIZE = 267,             /* error::bad_size (:833-838, :848-859) */
    BPMD_WS_BAD_CLOSE_CODE = 268,       /* error::bad_close_code (frame.hpp:225-230) */
    BPMD_WS_BAD_CLOSE_SIZE = 269,       /* error::bad_close_size (frame.hpp:209-214) */
    BPMD_WS_BAD_CLOSE_PAYLOAD = 270     /* error::bad_close_payload (frame.hpp:232-238) */
};

/* Frames of a batch of connections on the receive side (replaces the
 * parse_fh loop of read_some, read.hpp:1085-1283, with detail::read_ping,
 * read_close and is_valid_close_code, websocket/detail/frame.hpp:94-126,
 * 181-240; bpmd_frame_batch's inverse).  Entry i holds d_wire_len[i] bytes
 * at d_wire + d_wire_off[i], read in `role`; pmd_on != 0 means
 * permessage-deflate was negotiated, so RSV1 is legal on a message's first
 * frame (impl_base.hpp:61-78; :381-390 without it); msg_max is rd_msg_max
 * (0 = no limit), applied to uncompressed messages at header time as
 * stream_impl.hpp:894-906 does.
 *
 * The entry's frames are walked from the start.  A data frame's payload is
 * unmasked with the frame's key and appended to the out slot at
 * d_out + d_out_off[i] + rd_size.  The walk stops at the first of:
 *   BPMD_EV_MESSAGE  a FIN data frame was consumed: d_out_len[i] is the
 *       message's payload length, d_op[i] its opcode (1 text, 2 binary),
 *       d_compressed[i] its RSV1; the state is reset.
 *   BPMD_EV_PING / _PONG / _CLOSE  a control frame was consumed (it may
 *       come between a message's fragments; those before it are appended
 *       and the state is kept): its unmasked payload is at d_ctl + 128 * i,
 *       d_ctl_len[i] bytes.  For a close, d_close_code[i] is the code (0 for
 *       an empty payload) and d_status[i] is 0 or bad_close_size /
 *       bad_close_code / bad_close_payload as read_close decides; the frame
 *       counts as consumed either way, as in Beast.
 *   BPMD_EV_NEED_MORE  the buffer ended, or a header was refused and
 *       d_status[i] holds the parse_fh error; the refused frame is not
 *       consumed and the frames before it keep their effect.
 * Except after BPMD_EV_MESSAGE, d_out_len / d_op / d_compressed describe
 * the message in progress (zero between messages).  d_consumed[i] is the
 * number of wire bytes consumed; the caller drops them, keeps the rest and
 * calls again, with more bytes after NEED_MORE.  d_state carries each
 * entry's message state from call to call, together with the gathered bytes
 * in its out slot; NULL = every entry starts between messages and no state
 * is stored.
 *
 * One deliberate difference from Beast: only whole frames are consumed.  A
 * frame whose header or payload the buffer cuts stays unconsumed, where
 * Beast hands over the part of a data frame's payload that has arrived
 * (rd_remain, read.hpp:1201-1280); bpmd_receive_pieces_batch (below) is the
 * call that does.  So that a frame which can never fit is
 * refused at once, not waited for, a data frame whose rd_size + length
 * exceeds d_out_cap[i] is refused at header time with buffer_overflow, after
 * parse_fh's own checks.
 *
 * d_wire is not modified and must not overlap d_out; no byte outside
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written, and none beyond
 * the gathered length.  Asynchronous on `stream`.  n == 0 is a no-op;
 * BPMD_R_INVALID_ARGUMENT for a role that is neither, or for a NULL pointer
 * other than d_state; BPMD_R_NO_DEVICE without a GPU. */
int bpmd_unframe_batch(int role, int pmd_on, uint64_t msg_max, const uint8_t* d_wire, const uint64_t* d_wire_off,
                       const uint32_t* d_wire_len, uint32_t n, bpmd_rd_state* d_state, uint8_t* d_out,
                       const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op,
                       uint8_t* d_compressed, uint8_t* d_event, int32_t* d_status, uint32_t* d_consumed,
                       uint8_t* d_ctl, uint8_t* d_ctl_len, uint16_t* d_close_code, void* stream);

/* Unframe, inflate and check a batch of connections in one chained call
 * (bpmd_send_batch's counterpart): what read_some delivers per connection
 * (read.hpp:1063-1385), the inflater with rd_msg_max applied to the inflated
 * size (:1357-1367) and the UTF-8 check of text (:1372-1384) included.
 *
 * The arguments from d_wire to d_close_code are exactly bpmd_unframe_batch's
 * and every output of the frame pass keeps the meaning documented there,
 * d_out_len included (the gathered, still compressed length); only d_status
 * can change afterwards, and only for an entry with BPMD_EV_MESSAGE and frame
 * status 0.  Such an entry holds a complete message:
 *   - d_compressed[i] != 0: the gathered payload is inflated as
 *     bpmd_inflate_batch does under cfg->window_bits (cfg->flags must not
 *     carry BPMD_F_RAW) into the message slot d_msg + d_msg_off[i], of which
 *     the inflater may use min(d_msg_cap[i], msg_max + 1) bytes (all of
 *     d_msg_cap[i] when msg_max == 0): the effective capacity.
 *     d_msg_len[i] is the number of bytes produced, at most that capacity.
 *     d_status[i]: a zlib::error other than need_buffers as the inflater
 *     reports it, in stream order, so an error that precedes the limit wins;
 *     BPMD_WS_MESSAGE_TOO_BIG for a message that inflates to more than
 *     msg_max bytes when msg_max <= d_msg_cap[i]; BPMD_WS_BUFFER_OVERFLOW for
 *     one that outgrows d_msg_cap[i] when that is the smaller; else as below.
 *   - d_compressed[i] == 0: the message stays in its gathered slot in d_out
 *     and d_msg_len[i] = d_out_len[i].
 *   A text message (d_op[i] == 1) with status 0 so far is checked where it
 *   lies, as bpmd_utf8_check_batch does; any verdict but valid gives
 *   BPMD_BAD_FRAME_PAYLOAD.
 * Every other entry keeps the frame pass's event and status and gets
 * d_msg_len[i] = 0.  After the call d_compressed[i] tells which slot holds
 * message i.
 *
 * No byte of d_msg outside [d_msg_off[i], d_msg_off[i] + effective capacity)
 * is written and none of an entry that was not inflated; d_wire is not
 * modified, d_out only by the frame pass.  pmd_on == 0 runs no inflater: cfg,
 * d_msg, d_msg_off, d_msg_cap, d_msg_len and d_work may be NULL.
 *
 * d_work: bpmd_receive_work_bytes(n) (host only) bytes of device memory the
 * call may overwrite: per entry the inflater's input length, its effective
 * capacity, the text flag of its output and its status.  The caller owns it
 * because the inflater takes the stream's launch lock itself, so nothing of
 * this call may live in the stream's scratch across it; one workspace serves
 * one call at a time.
 *
 * Everything is enqueued on `stream` and no step added here reads anything
 * back; the one wait bpmd_inflate_batch has on a stream's first
 * block-parallel call (above) is inherited, and bpmd_inflate_reserve removes
 * it.  Deliberately out of scope: context-takeover receives
 * (bpmd_receive_takeover_batch, below, is this call over connection buffers),
 * more than one event per entry and call, and partial frames
 * (bpmd_unframe_batch, above; bpmd_receive_pieces_batch, below, takes them).
 * n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT for a role that is neither
 * value, a NULL required pointer, BPMD_F_RAW or (pmd_on) a NULL cfg;
 * BPMD_R_DOMAIN_ERROR for window bits outside 8..15; BPMD_R_NO_DEVICE
 * without a GPU. */
size_t bpmd_receive_work_bytes(uint32_t n);
int bpmd_receive_batch(const bpmd_cfg* cfg, int role, int pmd_on, uint64_t msg_max, const uint8_t* d_wire,
                       const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n, bpmd_rd_state* d_state,
                       uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                       uint8_t* d_op, uint8_t* d_compressed, uint8_t* d_event, int32_t* d_status,
                       uint32_t* d_consumed, uint8_t* d_ctl, uint8_t* d_ctl_len, uint16_t* d_close_code,
                       uint8_t* d_msg, const uint64_t* d_msg_off, const uint32_t* d_msg_cap, uint32_t* d_msg_len,
                       void* d_work, void* stream);

/* ---------------------------------------------------------------------
 * Send side: from messages to packed wire bytes.  What write_some does per
 * connection (websocket/impl/write.hpp:625-831) after begin_msg
 * (websocket/impl/stream_impl.hpp:225-252), over a batch of messages, and the
 * control frames of write_ping / write_close (stream_impl.hpp:915-996).
 * ------------------------------------------------------------------- */

/* Decide, deflate and frame a batch of messages in one chained call
 * (bpmd_unframe_batch + bpmd_read_batch's counterpart).  `role` is the
 * bpmd_role of the *sending* end: a client masks its frames.
 *
 * Message i (d_in + d_in_off[i], d_in_len[i] bytes, opcode d_op[i]: 1 text,
 * 2 binary; NULL = all binary) is compressed iff pmd_on && d_opt[i] &&
 * d_in_len[i] >= threshold (begin_msg; d_opt is wr_compress_opt per message,
 * NULL = on; threshold is msg_size_threshold); d_compressed[i] tells.
 *   - A compressed message is deflated as bpmd_deflate_batch does under cfg
 *     (cfg->flags honoured) into its staging slot d_z + d_z_off[i] (d_z_cap[i]
 *     bytes, d_z_len[i] produced: exactly bpmd_deflate_batch's out arrays,
 *     caller-owned; bpmd_deflate_upper_bound sizes a slot) and goes out with
 *     RSV1 in frames of at most frame_max payload bytes whatever `frag` says,
 *     as Beast's deflate branch emits one frame per wr_buf fill
 *     (write.hpp:655-703).  Messages that are not compressed reach the
 *     deflater with length 0: each costs one byte of its staging slot, which
 *     is ignored (a slot of 0 bytes is fine).
 *   - An uncompressed message is framed straight from d_in: in frames of at
 *     most frame_max bytes when frag != 0 (auto_fragment, :721-748, :795-829),
 *     as one frame when frag == 0 (:706-720, :750-794).
 *   An empty payload is one empty frame.  In client role frame f of message i
 *   carries the key d_keys[d_key_base[i] + f] and is masked with it from the
 *   key's first byte.  pmd_on == 0 runs no deflater: cfg and the staging
 *   arrays may be NULL.
 *
 * The wire is packed: message i's frames start at d_wire + d_wire_off[i],
 * the exclusive sum of the sizes before it, back to back in batch order with
 * no padding; d_wire_len[i] is its size and *d_total the sum of all sizes.
 * A message is written iff d_wire_off[i] + size <= wire_cap (bytes of
 * d_wire); one that is not gets BPMD_WS_BUFFER_OVERFLOW and d_wire_len[i] = 0
 * while *d_total still counts it, so the caller can grow the buffer and call
 * again.  d_status[i], by precedence: BPMD_WS_BAD_OPCODE (d_op[i] not 1 or 2),
 * the deflater's BPMD_NEED_BUFFERS, BPMD_WS_BUFFER_OVERFLOW (also for a
 * message whose wire size exceeds 2^32 - 1), 0.  A message with one of the
 * first two has size 0: it takes no room and its neighbours are packed as if
 * it were absent.  No byte of d_wire at or beyond min(*d_total, wire_cap) is
 * written, and none of a refused message's range.
 *
 * bpmd_send_frame_bound / bpmd_send_wire_bound (host only) give the most
 * frames and the most wire bytes of a message of `len` input bytes over any
 * decision (may_compress: pmd_on and the message's opt) and any deflate result
 * within bpmd_deflate_upper_bound(len), so keys and wire are sized from input
 * lengths alone; 0 for frame_max == 0.
 *
 * Everything is enqueued on `stream` and no step added here reads anything
 * back; the one wait bpmd_deflate_batch has for messages over 4 KiB (its
 * chunk count, above) is inherited when such a message is compressed.
 * Until the call returns, d_wire_len holds the deflater's input lengths.
 * Context-takeover sends have their own chained call,
 * bpmd_send_takeover_batch (below), and a message that arrives in several
 * write_some pieces goes through bpmd_send_pieces_batch (below).
 * n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT for frame_max == 0, a role that
 * is neither value, client role without d_keys / d_key_base, a NULL required
 * pointer, or (pmd_on) a cfg bpmd_deflate_batch refuses; BPMD_R_NO_DEVICE
 * without a GPU. */
uint64_t bpmd_send_frame_bound(uint64_t len, uint32_t frame_max, int may_compress, int frag);
uint64_t bpmd_send_wire_bound(uint64_t len, uint32_t frame_max, int masked, int may_compress, int frag);
int bpmd_send_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                    uint32_t n, int role, int pmd_on, uint64_t threshold, int frag, uint32_t frame_max,
                    const uint8_t* d_op, const uint8_t* d_opt, uint8_t* d_z, const uint64_t* d_z_off,
                    const uint32_t* d_z_cap, uint32_t* d_z_len, const uint32_t* d_keys, const uint32_t* d_key_base,
                    uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off, uint32_t* d_wire_len,
                    uint8_t* d_compressed, int32_t* d_status, uint64_t* d_total, void* stream);

/* Control frames (write_ping, write_close: stream_impl.hpp:915-996) over n
 * entries: d_op[i] is 8 close, 9 ping or 10 pong; the payload is the
 * d_ctl_len[i] bytes at d_ctl + 128 * i, the layout bpmd_unframe_batch
 * writes, so a received ping's slot goes back out as a pong unchanged.  Ping
 * and pong carry at most 125 bytes.  A close with d_close_code[i] != 0
 * carries the code big-endian and then the slot's bytes as the reason, at
 * most 123; a close with code 0 is empty whatever the slot holds.  Frames
 * have FIN set and no RSV bits; with d_key (client role; NULL = server)
 * entry i is masked with d_key[i] from the key's first byte.  One frame at
 * d_wire + 144 * i, d_wire_len[i] bytes.  d_status[i]: 0,
 * BPMD_WS_BAD_CONTROL_SIZE for an oversize entry, BPMD_WS_BAD_OPCODE for
 * another opcode; both give length 0 and write nothing.  Asynchronous on
 * `stream`; n == 0 is a no-op, BPMD_R_INVALID_ARGUMENT for a NULL pointer
 * other than d_key. */
int bpmd_control_batch(const uint8_t* d_op, const uint8_t* d_ctl, const uint8_t* d_ctl_len,
                       const uint16_t* d_close_code, const uint32_t* d_key, uint32_t n, uint8_t* d_wire,
                       uint32_t* d_wire_len, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------
 * Context takeover: when no_context_takeover is not
 * negotiated, Beast's inflater keeps its window from message to message
 * (do_context_takeover_read -> inflate_stream::clear() is a no-op,
 * impl_base.hpp:192-202, inflate_stream.ipp:49-53), so a message may copy
 * from the connection's earlier output.  Each connection keeps its output in
 * one device buffer; message i is decoded into d_out + d_out_off[i], right
 * after that connection's earlier output, whose last d_hist_len[i] bytes
 * (clamped to 2^windowBits) are the window.  One message per connection per
 * batch; connections run in parallel.  Statuses as bpmd_inflate_batch
 * (invalid_distance for a distance past the window).  No byte outside
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written, so a slot
 * may end where the next connection's buffer begins.  A message that fails
 * leaves its slot's contents past d_out_len[i] undefined.
 * ------------------------------------------------------------------- */
int bpmd_inflate_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                const uint32_t* d_in_len, const uint32_t* d_hist_len, uint32_t n_msgs,
                                uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                uint32_t* d_out_len, int32_t* d_status, void* stream);

/* Send side of the same connections: Beast's deflater is not reset between
 * messages (do_context_takeover_write resets only under no_context_takeover,
 * impl_base.hpp:156-166), so its payloads may copy from earlier messages.
 * Message i's bytes at d_in + d_in_off[i] are preceded in d_in by
 * d_hist_len[i] bytes of that connection's earlier plaintext; a match reaches
 * at most BPMD_CHUNK_HIST bytes (beast_amd/csrc/lz_core.h) before the 4 KiB
 * chunk it is in and never more than 2^window_bits back, so the stream is
 * valid for any inflater whose windowBits >= cfg->window_bits.  Otherwise as
 * bpmd_deflate_batch. */
int bpmd_deflate_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                                const uint32_t* d_in_len, const uint32_t* d_hist_len, uint32_t n_msgs,
                                uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                uint32_t* d_out_len, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------
 * Cross-connection micro-batcher.  Beast runs one codec
 * call per message inside each connection's async operation
 * (write_some_op, write.hpp:463-545; read.hpp:522-610 via impl_base.hpp:85-190);
 * the batcher coalesces those calls across connections: any thread submits
 * one message (host bytes, copied at submit) with a completion callback;
 * batches launch when max_msgs or the staging bytes fill up, or when the
 * oldest message has waited max_delay_us.  Two pinned staging slots
 * alternate, so submissions continue while the GPU works.
 * ------------------------------------------------------------------- */
enum bpmd_op { BPMD_OP_INFLATE = 0, BPMD_OP_DEFLATE = 1 };
typedef struct bpmd_batcher bpmd_batcher;
/* One message done (on the batcher's completion thread; it must not call
 * bpmd_batcher_flush or _destroy).  status: the message's zlib::error
 * (need_buffers: out_cap too small), or a negative bpmd_result when its batch
 * failed; out_len: bytes written to the submitter's out buffer. */
typedef void (*bpmd_done_fn)(void* user, int32_t status, size_t out_len);
/* cfg as for bpmd_inflate_batch / bpmd_deflate_batch (validated the same
 * way); max_in_bytes / max_out_bytes size each staging slot (input bytes; for
 * inflate the sum of out_cap, for deflate of deflate_upper_bound(n)). */
int bpmd_batcher_create(const bpmd_cfg* cfg, int op, uint32_t max_msgs, size_t max_in_bytes, size_t max_out_bytes,
                        uint32_t max_delay_us, bpmd_batcher** out);
/* Queue one message.  `out` must stay valid until fn runs. */
int bpmd_batcher_submit(bpmd_batcher* b, const void* in, size_t n, void* out, size_t out_cap, bpmd_done_fn fn,
                        void* user);
/* Launch what is queued and wait until every message submitted so far has
 * completed. */
int bpmd_batcher_flush(bpmd_batcher* b);
/* Completes everything queued, then frees the batcher. */
void bpmd_batcher_destroy(bpmd_batcher* b);

/* ---------------------------------------------------------------------
 * permessage-deflate negotiation (wire format only), for
 * a facade that owns the handshake: the Sec-WebSocket-Extensions logic of
 * websocket/detail/pmd_extension.hpp/.ipp.  Host code, no device use.
 * ------------------------------------------------------------------- */
/* detail::pmd_offer (pmd_extension.hpp:27-42) */
typedef struct bpmd_pmd_offer {
    int accept;
    int server_max_window_bits;      /* 0 absent, or 8..15 (-1 present without value when writing) */
    int client_max_window_bits;      /* -1 present without value, 0 absent, or 8..15 */
    int server_no_context_takeover;
    int client_no_context_takeover;
} bpmd_pmd_offer;
/* websocket::permessage_deflate (option.hpp:34-67); the codec fields
 * (compLevel, memLevel, msg_size_threshold) live in bpmd_cfg */
typedef struct bpmd_pmd_options {
    int server_enable, client_enable;
    int server_max_window_bits, client_max_window_bits;
    int server_no_context_takeover, client_no_context_takeover;
} bpmd_pmd_options;
/* pmd_read (pmd_extension.ipp:45-166): the first permessage-deflate offer of
 * a Sec-WebSocket-Extensions value; offer->accept = 0 when it must be declined */
int bpmd_pmd_read(const char* ext, size_t n, bpmd_pmd_offer* offer);
/* pmd_write (pmd_extension.ipp:168-208): the header value of an offer into
 * out (NUL-terminated); returns its length */
int bpmd_pmd_write(const bpmd_pmd_offer* offer, char* out, size_t cap);
/* pmd_negotiate (pmd_extension.hpp:95-111, .ipp:210-290): the server's
 * configuration and response value for a client offer (empty when declined);
 * returns the response length */
int bpmd_pmd_negotiate(const bpmd_pmd_options* o, const bpmd_pmd_offer* offer, bpmd_pmd_offer* config, char* out,
                       size_t cap);
/* pmd_normalize (pmd_extension.ipp:292-305) */
void bpmd_pmd_normalize(bpmd_pmd_offer* offer);

/* Window maintenance for the buffers above: move the d_keep[i] bytes before
 * d_pos[i] of the buffer at d_buf + d_base[i] to its front (the caller slides
 * only when d_pos[i] >= 2 * d_keep[i], so the ranges never overlap). */
int bpmd_slide_batch(uint8_t* d_buf, const uint64_t* d_base, const uint32_t* d_pos, const uint32_t* d_keep,
                     uint32_t n, void* stream);

/* Unframe, inflate with context takeover and check a batch of connections in
 * one chained call: bpmd_receive_batch for connections whose inflater keeps
 * its window (above), which is what Beast negotiates by default.  Entry i is
 * connection i, as d_state[i] already is; a connection takes part in a call
 * once.  pmd_on is implied.
 *
 * The arguments from d_wire to d_close_code are exactly bpmd_unframe_batch's
 * and every output of the frame pass keeps the meaning documented there;
 * afterwards only d_status can change, as in bpmd_receive_batch.
 *
 * Connection i owns the slot_bytes bytes at d_buf + d_base[i], of which the
 * first d_pos[i] hold its latest output: the last min(d_pos[i], W) of them,
 * W = 2^cfg->window_bits, are its window.  d_pos is in/out; a new connection
 * starts at 0 and d_pos[i] never exceeds slot_bytes.  slot_bytes > 2 * W.
 * "The message capacity" of entry i is min(d_msg_cap[i], slot_bytes - 2 * W)
 * everywhere below, and the effective capacity is that limited to msg_max + 1
 * bytes (all of it when msg_max == 0), as in bpmd_receive_batch.
 *   - An entry that completed a compressed message (BPMD_EV_MESSAGE, frame
 *     status 0, d_compressed[i] != 0) is inflated right behind the
 *     connection's earlier output.  If d_pos[i] + effective capacity >
 *     slot_bytes, the W bytes before d_pos[i] are first moved to the buffer's
 *     front and d_pos[i] becomes W (then d_pos[i] was more than 2 * W, so the
 *     move never overlaps itself).  d_msg_off[i] (an output) = d_base[i] +
 *     that position: where message i lies in d_buf.  d_msg_len[i] is the
 *     number of bytes produced, at most the effective capacity.  d_status[i]:
 *     bpmd_receive_batch's rule with the message capacity above -- a
 *     zlib::error as the inflater reports it, in stream order (invalid_distance
 *     for a distance past the window), BPMD_WS_MESSAGE_TOO_BIG,
 *     BPMD_WS_BUFFER_OVERFLOW, BPMD_BAD_FRAME_PAYLOAD for text that is not
 *     UTF-8 (checked in the connection's buffer), or 0.
 *     d_pos[i] advances by d_msg_len[i] iff the inflater's own status is 0:
 *     also when the merged status is BPMD_WS_MESSAGE_TOO_BIG or
 *     BPMD_BAD_FRAME_PAYLOAD, since Beast's window has taken those bytes too
 *     (and the connection fails anyway).  After a zlib::error or an outgrown
 *     capacity d_pos[i] stays, the window is undefined from then on and the
 *     caller drops the connection, as with pmd.py's TakeoverInflater.
 *   - Every other entry leaves its connection alone: no slide, d_pos[i]
 *     unchanged, d_msg_off[i] = d_base[i] + d_pos[i].  A complete uncompressed
 *     message stays in its gathered slot in d_out (d_msg_len[i] =
 *     d_out_len[i], text checked there); any other entry gets d_msg_len[i] = 0.
 *
 * The only bytes of d_buf written are, per entry, [d_base[i], d_base[i] + W)
 * of a connection that slid and [d_msg_off[i], d_msg_off[i] + effective
 * capacity) of an inflated entry (what lies past d_msg_len[i] in there is
 * undefined), so a buffer may end where the next begins, at any alignment.
 * d_pos changes only by the two rules above.  d_wire is not modified, d_out
 * only by the frame pass.
 *
 * d_work: bpmd_receive_takeover_work_bytes(n) (host only) bytes of device
 * memory the call may overwrite: bpmd_receive_batch's arrays, then per entry
 * the window length and the 64-bit output offset.  One workspace serves one
 * call at a time.
 *
 * Everything is enqueued on `stream` and no step reads anything back: which
 * connections slide is decided on the device.  Out of scope as for
 * bpmd_receive_batch: more than one event per entry and call, partial frames
 * (bpmd_receive_pieces_batch, below, takes them).
 * n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT for a role that is neither
 * value, a NULL pointer other than d_state, BPMD_F_RAW, a NULL cfg or
 * slot_bytes <= 2 * W; BPMD_R_DOMAIN_ERROR for window bits outside 8..15;
 * BPMD_R_NO_DEVICE without a GPU. */
size_t bpmd_receive_takeover_work_bytes(uint32_t n);
int bpmd_receive_takeover_batch(const bpmd_cfg* cfg, int role, uint64_t msg_max, const uint8_t* d_wire,
                                const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n,
                                bpmd_rd_state* d_state, uint8_t* d_out, const uint64_t* d_out_off,
                                const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op, uint8_t* d_compressed,
                                uint8_t* d_event, int32_t* d_status, uint32_t* d_consumed, uint8_t* d_ctl,
                                uint8_t* d_ctl_len, uint16_t* d_close_code, uint8_t* d_buf, const uint64_t* d_base,
                                uint32_t slot_bytes, uint32_t* d_pos, const uint32_t* d_msg_cap, uint64_t* d_msg_off,
                                uint32_t* d_msg_len, void* d_work, void* stream);

/* Decide, deflate with context takeover and frame a batch of connections in
 * one chained call: bpmd_send_batch for connections whose deflater keeps its
 * history (above), which is what Beast negotiates by default.  Entry i is
 * connection i; a connection takes part in a call once.  pmd_on is implied.
 *
 * Everything not named here means what it means in bpmd_send_batch: d_in,
 * d_in_off, d_in_len, role, threshold, frag, frame_max, d_opt, the staging
 * slots d_z / d_z_off / d_z_cap / d_z_len, d_keys[d_key_base[i] + f], the
 * packed wire with d_wire_off, d_wire_len and *d_total, d_compressed, and the
 * guarantees about which wire bytes are written.  d_op[i] is 0 idle (nothing
 * to send: status 0, size 0, the connection untouched, whatever the entry's
 * other arrays hold), 1 text or 2 binary; NULL = all binary.
 *
 * K = 4096 is the plaintext a connection's buffer keeps; a match reaches at
 * most BPMD_CHUNK_HIST (4096 at levels 7-9) bytes back, never more than K.
 * Connection i owns the slot_bytes bytes at d_buf + d_base[i], of which the
 * first d_pos[i] hold the messages it compressed last; d_pos is in/out, a new
 * connection starts at 0 and d_pos[i] never exceeds slot_bytes.
 * slot_bytes > 2 * K.  L = min(max_len, slot_bytes - 2 * K) is the longest
 * message that can be compressed.
 *   - Entry i is compressed iff d_op[i] is 1 or 2, d_opt[i] and d_in_len[i] >=
 *     threshold (begin_msg); d_compressed[i] tells.  Such a message longer
 *     than L gets BPMD_WS_MESSAGE_TOO_BIG and is not sent.  Otherwise, if
 *     d_pos[i] + d_in_len[i] > slot_bytes, the K bytes before d_pos[i] are
 *     first moved to the buffer's front and d_pos[i] becomes K (then d_pos[i]
 *     was more than 2 * K, so the move never overlaps itself); the message is
 *     copied to d_buf + d_base[i] + d_pos[i] and deflated there as
 *     bpmd_deflate_takeover_batch does, with min(d_pos[i], K) bytes of
 *     history, into its staging slot, and framed from there.
 *     d_pos[i] advances by d_in_len[i] iff the final d_status[i] is 0, that
 *     is, iff the message's frames are on the wire.  After BPMD_NEED_BUFFERS
 *     or BPMD_WS_BUFFER_OVERFLOW the peer never saw the message, so the
 *     history does not contain it: call again with the same message and a
 *     larger staging slot or wire, and with d_op = 0 for the connections that
 *     succeeded; the payload produced then is one the peer's window decodes.
 *   - Every other entry leaves its connection alone: no slide, d_pos[i]
 *     unchanged, no byte of its buffer written.  An uncompressed message is
 *     framed straight from d_in and never enters the history, as it never
 *     passes the peer's inflater; it may be longer than L.  Such entries reach
 *     the deflater with length 0, which costs one byte of their staging slot
 *     (a slot of 0 bytes is fine).
 * d_status[i], by precedence: BPMD_WS_BAD_OPCODE (d_op[i] not 0, 1 or 2),
 * BPMD_WS_MESSAGE_TOO_BIG, the deflater's BPMD_NEED_BUFFERS,
 * BPMD_WS_BUFFER_OVERFLOW for the wire, 0.  An entry with one of the first
 * three has size 0, like an idle one.
 *
 * The only bytes of d_buf written are, per entry, [d_base[i], d_base[i] + K)
 * of a connection that slid and the message's own
 * [d_base[i] + d_pos[i], ... + d_in_len[i]) of an entry that is deflated, so a
 * buffer may end where the next begins, at any alignment.  d_pos changes only
 * by the two rules above.  The frame step never reads d_buf.
 *
 * d_work: bpmd_send_takeover_work_bytes(n) (host only) bytes of device memory
 * the call may overwrite: per entry the deflater's input length, its history,
 * the status before it and the 64-bit input offset.  One workspace serves one
 * call at a time.
 *
 * Everything is enqueued on `stream` and no step reads anything back: the
 * deflater's chunk workspace (in the stream's scratch pool) is sized on the
 * host for n * ceil(L / 4096) chunks instead of the batch's own count, so a
 * caller whose messages are mostly short pays workspace for max_len; keep
 * max_len near the longest message that is really compressed.  The only wait
 * left is the stream's scratch pool growing on a stream's first calls.
 * n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT for frame_max == 0, a role that
 * is neither value, a NULL required pointer (d_op, d_opt and, in server role,
 * d_keys / d_key_base may be NULL), client role without d_keys / d_key_base,
 * BPMD_F_EXACT or BPMD_F_RAW, slot_bytes <= 2 * K, max_len == 0,
 * n * ceil(L / 4096) > 2^32 - 1, or a cfg bpmd_deflate_batch refuses;
 * BPMD_R_NO_DEVICE without a GPU. */
size_t bpmd_send_takeover_work_bytes(uint32_t n);
int bpmd_send_takeover_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                             const uint32_t* d_in_len, uint32_t n, int role, uint64_t threshold, int frag,
                             uint32_t frame_max, uint32_t max_len, const uint8_t* d_op, const uint8_t* d_opt,
                             uint8_t* d_buf, const uint64_t* d_base, uint32_t slot_bytes, uint32_t* d_pos, uint8_t* d_z,
                             const uint64_t* d_z_off, const uint32_t* d_z_cap, uint32_t* d_z_len,
                             const uint32_t* d_keys, const uint32_t* d_key_base, uint8_t* d_wire, uint64_t wire_cap,
                             uint64_t* d_wire_off, uint32_t* d_wire_len, uint8_t* d_compressed, int32_t* d_status,
                             uint64_t* d_total, void* d_work, void* stream);

/* A message in pieces: bpmd_send_takeover_batch with Beast's
 * write_some(fin, buffers) state (websocket/impl/write.hpp:625-831) kept per
 * connection, so an application streams a message as write_some(false, ...)
 * ... write_some(true, ...), one piece per connection per call, and with a
 * per-connection no_context_takeover flag, so connections that negotiated it
 * and connections that did not share one call.  bpmd_rd_state's counterpart.
 *
 * d_state[i] (in/out, required) is connection i's wr_cont_, wr_compress_ and
 * opcode; all zero = no message open, which is how a connection starts.
 * d_fin[i] != 0 marks a message's final piece (NULL = every piece is final:
 * whole messages).  d_no_takeover[i] != 0 marks a connection that negotiated
 * no_context_takeover for this direction (NULL = none).  Everything not named
 * here means what it means in bpmd_send_takeover_batch, with "message" read
 * as "piece": d_in, d_in_off, d_in_len, role, frag, frame_max, the buffers
 * d_buf / d_base / slot_bytes / d_pos with K and L, the staging slots, the
 * keys d_keys[d_key_base[i] + f] with f counted from 0 in every piece, the
 * packed wire, d_work and the guarantees about d_buf and d_wire.
 *   - A piece with d_state[i].wr_cont == 0 begins a message: begin_msg
 *     decides from this piece alone, compressed iff d_op[i] is 1 or 2,
 *     d_opt[i] and d_in_len[i] >= threshold (Beast passes this write_some's
 *     buffer_bytes, write.hpp:640-652; stream_impl.hpp:225-252), and its
 *     first frame carries d_op[i], with RSV1 iff compressed.  A piece with
 *     wr_cont != 0 continues the open message under the stored decision and
 *     opcode: d_opt[i] is ignored, d_op[i] must be 1 or 2 (0 = idle, as ever)
 *     and is otherwise ignored, and all its frames are continuation frames.
 *     FIN is set on the piece's last frame iff d_fin[i].  A piece always
 *     yields at least one frame, an empty one for an empty uncompressed piece.
 *     d_compressed[i] is the message's decision on every piece (0 for an idle
 *     entry or a bad opcode).
 *   - A piece of a compressed message enters the connection's buffer and is
 *     deflated as a message is in bpmd_send_takeover_batch, with the earlier
 *     pieces as its history like any earlier plaintext.  The deflater's
 *     payload ends with an empty stored block whose 00 00 FF FF is stripped,
 *     and none of its blocks has BFINAL set; the final piece goes out like
 *     that.  A non-final piece gets the four bytes back: they are written at
 *     d_z + d_z_off[i] + d_z_len[i] and d_z_len[i] grows by 4, so the next
 *     piece's blocks follow at a byte boundary (RFC 7692 7.2.1) and a
 *     message's piece payloads concatenated are one valid permessage-deflate
 *     payload.  Size a staging slot bpmd_deflate_upper_bound(len) + 4.  If the
 *     four bytes do not fit d_z_cap[i] the piece gets BPMD_NEED_BUFFERS and
 *     none of them is written.  (Beast sends a non-final piece with
 *     Flush::none and may emit nothing, write.hpp:669-678; the payload bytes
 *     differ, the inflated message does not.)  L bounds a piece, not a
 *     message: a compressed piece longer than L gets BPMD_WS_MESSAGE_TOO_BIG
 *     and can be sent again as shorter pieces.
 *   - A piece of an uncompressed message is framed straight from d_in (frag
 *     as in bpmd_send_batch) and never enters the history.
 *   - After a piece with final status 0: d_pos[i] has advanced by d_in_len[i]
 *     if the piece was deflated; wr_cont = !d_fin[i], wr_compress and the
 *     opcode are the message's; and if the piece was final, the message
 *     compressed and d_no_takeover[i] set, d_pos[i] = 0: the next message
 *     starts without history (do_context_takeover_write,
 *     impl_base.hpp:156-166).
 *   - d_status[i], by precedence: BPMD_WS_BAD_OPCODE (d_op[i] not 0, 1 or 2),
 *     BPMD_WS_MESSAGE_TOO_BIG, BPMD_NEED_BUFFERS (the deflater's, or the
 *     marker's), BPMD_WS_BUFFER_OVERFLOW for the wire, 0.  An entry with any
 *     non-zero status, like an idle one, has d_state[i] and the connection's
 *     history exactly as they were, and d_pos[i] too but for a slide, which
 *     keeps the history's bytes (d_pos[i] = K): the caller sends the same
 *     piece again with more room, or a shorter one after
 *     BPMD_WS_MESSAGE_TOO_BIG.
 * Besides bpmd_send_takeover_batch's bytes the only staging bytes written are
 * the four marker bytes of a non-final compressed piece whose slot has room.
 * d_state[i] and d_pos[i] are written only when their value changes.
 *
 * bpmd_send_piece_frame_bound / bpmd_send_piece_wire_bound (host only) are
 * bpmd_send_frame_bound / bpmd_send_wire_bound for a piece of `len` input
 * bytes: with fin == 0 they count the marker.  may_compress: the message may
 * be compressed (for a continuation piece, the stored decision if known).
 *
 * d_work: bpmd_send_pieces_work_bytes(n) (host only) bytes.  Everything is
 * enqueued on `stream` and nothing is read back, as in
 * bpmd_send_takeover_batch.  n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT as
 * there, and for a NULL d_state (d_fin and d_no_takeover may be NULL).
 * Out of scope: BPMD_F_EXACT, and more than one piece of a connection in one
 * call. */
typedef struct bpmd_wr_state {
    uint8_t wr_cont;       /* a message is open */
    uint8_t wr_compress;   /* its begin_msg decision */
    uint8_t wr_op;         /* its opcode */
    uint8_t reserved;
} bpmd_wr_state;           /* zero = no message open */
uint64_t bpmd_send_piece_frame_bound(uint64_t len, uint32_t frame_max, int may_compress, int frag, int fin);
uint64_t bpmd_send_piece_wire_bound(uint64_t len, uint32_t frame_max, int masked, int may_compress, int frag, int fin);
size_t bpmd_send_pieces_work_bytes(uint32_t n);
int bpmd_send_pieces_batch(const bpmd_cfg* cfg, const uint8_t* d_in, const uint64_t* d_in_off,
                           const uint32_t* d_in_len, uint32_t n, int role, uint64_t threshold, int frag,
                           uint32_t frame_max, uint32_t max_len, const uint8_t* d_op, const uint8_t* d_opt,
                           const uint8_t* d_fin, const uint8_t* d_no_takeover, bpmd_wr_state* d_state, uint8_t* d_buf,
                           const uint64_t* d_base, uint32_t slot_bytes, uint32_t* d_pos, uint8_t* d_z,
                           const uint64_t* d_z_off, const uint32_t* d_z_cap, uint32_t* d_z_len, const uint32_t* d_keys,
                           const uint32_t* d_key_base, uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off,
                           uint32_t* d_wire_len, uint8_t* d_compressed, int32_t* d_status, uint64_t* d_total,
                           void* d_work, void* stream);

/* Receive messages in pieces: read_some as Beast runs it (read.hpp:1063-1385),
 * one piece per connection per call.  bpmd_send_pieces_batch's counterpart,
 * and bpmd_receive_batch / bpmd_receive_takeover_batch for peers whose frames
 * or messages are larger than the buffers a connection should hold: a data
 * frame is taken as far as its bytes have arrived, unmasked with the key as
 * rotated so far, inflated by the per-stream state machine that keeps its
 * window and its half-decoded symbol on the device, checked as UTF-8 with the
 * cut code point carried, and delivered.  Entry i is connection i, once per
 * call.  pmd_on == 0: cfg, d_zstate, d_msg, d_msg_off, d_msg_cap and d_work
 * may be NULL.
 *
 * State.  d_state[i] (required) is read_some's state between calls, all zero
 * between messages.  d_zstate holds n consecutive inflater states of
 * bpmd_receive_pieces_zstate_bytes() bytes each (a multiple of 16; d_zstate
 * 16-byte aligned) that the caller zeroes once: all zero is a new connection,
 * whose window bits the call sets from cfg->window_bits on first use.  The
 * state keeps its window, so context takeover needs nothing, and a
 * no_context_takeover connection uses the same call with the same state
 * (Beast's zi.clear() is a no-op, impl_base.hpp:193-202).
 *
 * Frame walk.  bpmd_unframe_batch's walk with the same header checks, events
 * and control slots, except:
 *   - the bytes gathered in this call start at offset 0 of the out slot
 *     d_out + d_out_off[i], which is reused from call to call; d_out_len[i] is
 *     the piece's gathered length.  At most d_out_cap[i] - 4 payload bytes are
 *     gathered per call; an entry with d_out_cap[i] < 8 gathers nothing and
 *     gets BPMD_WS_BUFFER_OVERFLOW.  No frame is refused for its size.
 *   - a data frame whose payload the buffer or the slot cuts is consumed as
 *     far as it goes: its header and the bytes taken count in d_consumed[i],
 *     and rd_remain, the rotated rd_key and rd_fin carry the rest; a call that
 *     starts with rd_remain > 0 takes payload bytes first.  Control frames and
 *     cut headers stay whole and unconsumed (stream_impl.hpp:817-823).
 *   - the walk also stops when the slot is full: BPMD_EV_NEED_MORE with status
 *     0, and the caller calls again with the unconsumed rest.
 * BPMD_EV_MESSAGE means the FIN frame's last payload byte was taken: this
 * piece is its message's last.  A control frame between fragments stops the
 * walk and the data gathered before it is still this call's piece, as are the
 * bytes gathered before a refused header.  d_op / d_compressed describe the
 * message the piece belongs to.
 *
 * Piece.
 *   - d_compressed[i] == 0: the piece stays in the out slot, d_msg_len[i] =
 *     d_out_len[i]; msg_max is applied at header time.
 *   - d_compressed[i] != 0: behind a message's last piece the walk appends
 *     00 00 FF FF in the slot, and one inflate_stream::write(Flush::sync) runs
 *     over piece (+ tail) from connection i's state into d_msg + d_msg_off[i]
 *     with the room eff = min(d_msg_cap[i], msg_max - rd_size + 1) (all of
 *     d_msg_cap[i] when msg_max == 0).  An empty last piece still inflates the
 *     tail; an empty piece inside a message runs nothing.  d_msg_len[i] = the
 *     bytes produced (0 after a zlib::error, which hands nothing over, as in
 *     Beast).  d_status[i], in stream order: the zlib::error other
 *     than need_buffers; else BPMD_WS_MESSAGE_TOO_BIG when rd_size + produced
 *     > msg_max; else BPMD_WS_BUFFER_OVERFLOW when input was left, i.e. the
 *     room ran out: the connection is dropped.  A piece inside a message that
 *     consumes its input with output still pending in the decoder is no
 *     error: the rest comes with the next piece.
 *   - text (d_op[i] == 1), status 0 so far: utf8_b[0..utf8_n) followed by the
 *     piece are checked where the piece lies: BPMD_BAD_FRAME_PAYLOAD when they
 *     are no prefix of well-formed UTF-8, or when the message ends inside a
 *     code point; else the bytes of a cut code point are the new carry.
 *   - a frame error reported behind a piece that was fine stays in d_status[i].
 * At a message's end the state is all zero again.  Any error leaves the
 * connection to be dropped; its states are unspecified from then on.
 *
 * No byte of d_out outside [d_out_off[i], d_out_off[i] + d_out_cap[i]) is
 * written, none of d_msg outside [d_msg_off[i], d_msg_off[i] + eff) and none
 * of an entry that ran no inflater; d_zstate only inside connection i's state;
 * d_wire is not modified.  The inflater loads its input 16 bytes at a time
 * from the slot's start: the memory behind d_out must be readable for 15 bytes
 * past every slot.  An entry with d_wire_len[i] == 0 changes no state and no
 * slot.  d_work: bpmd_receive_pieces_work_bytes(n) (host only) bytes, per
 * entry the inflater's call record and its result; one workspace serves one
 * call at a time.  Everything is enqueued on `stream` and nothing is read
 * back.
 *
 * n == 0 is a no-op; BPMD_R_INVALID_ARGUMENT for a role that is neither value,
 * a NULL required pointer, BPMD_F_RAW or (pmd_on) a NULL cfg;
 * BPMD_R_DOMAIN_ERROR for window bits outside 8..15; BPMD_R_NO_DEVICE without a
 * GPU.  Out of scope: more than one message per entry and call, and resuming a
 * piece whose output room ran out with input left. */
typedef struct bpmd_rd_piece_state {
    uint64_t rd_size;     /* Beast's rd_size: bytes of the current message delivered so far
                             (gathered bytes of a plain message, inflated bytes of a compressed one) */
    uint64_t rd_remain;   /* payload bytes of the current data frame that have not arrived yet */
    uint32_t rd_key;      /* that frame's key, rotated so that byte 0 applies to its next payload byte (mask.ipp:29-36) */
    uint8_t  rd_cont, rd_op, rd_deflated;
    uint8_t  rd_fin;      /* FIN of the frame rd_remain belongs to */
    uint8_t  utf8_n;      /* 0..3: bytes of a code point the text delivered so far ends inside */
    uint8_t  utf8_b[3];
    uint8_t  reserved[4]; /* zero */
} bpmd_rd_piece_state;    /* 32 bytes; all zero = between messages */
size_t bpmd_receive_pieces_zstate_bytes(void);
size_t bpmd_receive_pieces_work_bytes(uint32_t n);
int bpmd_receive_pieces_batch(const bpmd_cfg* cfg, int role, int pmd_on, uint64_t msg_max, const uint8_t* d_wire,
                              const uint64_t* d_wire_off, const uint32_t* d_wire_len, uint32_t n,
                              bpmd_rd_piece_state* d_state, void* d_zstate, uint8_t* d_out, const uint64_t* d_out_off,
                              const uint32_t* d_out_cap, uint32_t* d_out_len, uint8_t* d_op, uint8_t* d_compressed,
                              uint8_t* d_event, int32_t* d_status, uint32_t* d_consumed, uint8_t* d_ctl,
                              uint8_t* d_ctl_len, uint16_t* d_close_code, uint8_t* d_msg, const uint64_t* d_msg_off,
                              const uint32_t* d_msg_cap, uint32_t* d_msg_len, void* d_work, void* stream);

/* ---------------------------------------------------------------------
 * Per-stream API behind the C++ compatibility facade
 * (include/boost/beast/zlib/ headers).  Host buffers; each call runs on the
 * current device (deflate: the batch kernels on one message; inflate: the
 * per-stream kernel) and synchronises.
 * Throughput comes from the batch API above; these calls exist so code
 * written against zlib::deflate_stream / zlib::inflate_stream (the calls
 * impl_base<true> makes, impl_base.hpp:85-190) runs unchanged.
 * ------------------------------------------------------------------- */

/* z_params (zlib/zlib.hpp:78-144) */
typedef struct bpmd_zparams {
    const void* next_in;
    size_t avail_in;
    size_t total_in;
    void* next_out;
    size_t avail_out;
    size_t total_out;
    int data_type;
} bpmd_zparams;

/* zlib::Flush (zlib/zlib.hpp:159-183); the order matters */
enum bpmd_flush {
    BPMD_FLUSH_NONE = 0, BPMD_FLUSH_BLOCK, BPMD_FLUSH_PARTIAL, BPMD_FLUSH_SYNC, BPMD_FLUSH_FULL,
    BPMD_FLUSH_FINISH, BPMD_FLUSH_TREES
};

typedef struct bpmd_stream bpmd_stream;

/* deflate_stream::reset(level, windowBits, memLevel, strategy)
 * (deflate_stream.ipp:227-265); BPMD_R_INVALID_ARGUMENT where it throws */
int bpmd_deflate_stream_create(int level, int window_bits, int mem_level, int strategy, bpmd_stream** out);
/* deflate_stream::reset() (deflate_stream.hpp:123-127) */
int bpmd_deflate_stream_reset(bpmd_stream* s);
/* deflate_stream::write(zs, flush, ec) (deflate_stream.ipp:357-499): returns
 * the zlib::error value (0 = none) or BPMD_R_INVALID_ARGUMENT where it throws.
 * What each Flush value emits and which guarantees hold: DESIGN.md 8. */
int bpmd_deflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush);
/* deflate_stream::params(zs, level, strategy, ec) (deflate_stream.ipp:307-338) */
int bpmd_deflate_stream_params(bpmd_stream* s, bpmd_zparams* zs, int level, int strategy);
/* deflate_stream::tune(good_length, max_lazy, nice_length, max_chain)
 * (deflate_stream.hpp:163-181, deflate_stream.ipp:307-317): replaces the
 * level's good/lazy/nice/chain limits for the following writes (the GPU
 * parser still caps the chain walk); like the reference, a
 * tune before the stream's first write or prime is undone by its lazy init. */
int bpmd_deflate_stream_tune(bpmd_stream* s, int good_length, int max_lazy, int nice_length, int max_chain);
/* deflate_stream::pending(value, bits) (deflate_stream.hpp:344-348) */
int bpmd_deflate_stream_pending(bpmd_stream* s, unsigned* value, int* bits);
/* deflate_stream::prime(bits, value, ec) (deflate_stream.ipp:340-355) */
int bpmd_deflate_stream_prime(bpmd_stream* s, int bits, int value);
/* inflate_stream::reset(windowBits) (inflate_stream.ipp:55-72);
 * BPMD_R_DOMAIN_ERROR where it throws */
int bpmd_inflate_stream_create(int window_bits, bpmd_stream** out);
int bpmd_inflate_stream_reset(bpmd_stream* s, int window_bits);
/* inflate_stream::clear() -- a no-op in the reference (inflate_stream.ipp:49-53) */
int bpmd_inflate_stream_clear(bpmd_stream* s);
/* inflate_stream::write(zs, flush, ec) (inflate_stream.ipp:74-535).  The
 * reference's decoder state (mode, bit reservoir, tables, 2^windowBits
 * window) lives on the device and each call runs its state machine there
 * (beast_amd/csrc/pmd_zstream.hip), so the status, the output bytes and
 * every z_params field -- next_in/avail_in/total_in included: input the
 * reference leaves unconsumed stays with the caller -- equal Beast's after
 * every call.  A data error returns without advancing z_params, as the
 * reference's err() does (inflate_stream.ipp:120-125). */
int bpmd_inflate_stream_write(bpmd_stream* s, bpmd_zparams* zs, int flush);
/* Memory an inflate stream holds (device: state + window, and with the
 * batcher off the block its calls are laid out in; host: that block's pinned
 * mirror, no decoder state -- 0 with the batcher on, when calls use the
 * batch leader's block); no reference counterpart, for bounded-memory tests. */
int bpmd_inflate_stream_footprint(const bpmd_stream* s, size_t* host_bytes, size_t* device_bytes);
void bpmd_stream_destroy(bpmd_stream* s);

/* The micro-batcher behind the two write() calls above (no reference
 * counterpart; SURVEY §8(f) N2, for the call sites impl_base.hpp:85-190 and
 * write.hpp:463-545): calls of different streams made at the same time run
 * as one launch, each with exactly its single-call result (status, output
 * bytes, every z_params field).  A call that finds no batch running takes
 * up to max_calls queued calls (one per stream) and runs them; calls that
 * arrive meanwhile form the next batch, so a lone stream waits for nothing
 * (its batch is one call; with the batcher on, streams keep no HIP stream or staging buffers of their own).  max_delay_us > 0: a batch's
 * first call also waits up to that long for more.  max_calls < 2 turns it
 * off.  Default: 256 calls, no delay (environment: BPMD_STREAM_BATCH,
 * BPMD_STREAM_BATCH_DELAY_US). */
int bpmd_stream_batching(int max_calls, int max_delay_us);
/* The setting in force (either pointer may be NULL), e.g. to put it back. */
int bpmd_stream_batching_get(int* max_calls, int* max_delay_us);
/* out[0] inflate write() calls through the batcher, out[1] their launches,
 * out[2] deflate flushes, out[3] their deflater calls; reset != 0 zeroes them. */
int bpmd_stream_batch_stats(unsigned long long* out, int reset);

#ifdef __cplusplus
}
#endif
#endif
