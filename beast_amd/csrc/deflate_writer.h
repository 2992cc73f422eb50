// deflate_writer.h -- the per-stream deflater's call protocol:
// zlib::deflate_stream's write() / params() / tune() / prime() / pending() /
// reset() bookkeeping, without the device.  Plain C++ (no HIP): the one step
// that needs the GPU -- compress these bytes behind this history with these
// parameters -- is a function the owner supplies (pmd_stream.hip: the deflate
// transport; tests/cpp/deflate_writer_backend.cpp: a stand-in on the CPU).
//
// Input is buffered until a flush; each flush compresses the buffered bytes
// (blocks with BFINAL = 0, exact bit length returned by the step) and appends
// the flush's own bits the way the reference's doWrite does
// (deflate_stream.ipp:357-499): Flush::block leaves the last partial byte
// pending, partial adds tr_align's empty static block, sync/full/trees add
// the empty stored block 000 + pad + 00 00 FF FF (full also drops the
// history, as clear_hash() does), finish adds a final empty block and reports
// end_of_stream.  Pending output, duplicate-flush need_buffers, stream_error
// and invalid_argument follow doWrite.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/beast_pmd.h"
#include "lz_core.h"

namespace bpmd {

// One flush's compression: what goes in, and what the step hands back.
struct DeflateStep {
    const uint8_t* in;     // the buffered input
    size_t n;
    const uint8_t* hist;   // the plaintext compressed before it (its matches may reach into it)
    size_t hist_len;
    size_t out_cap;        // output room
    int level, wbits, strategy;
    const int* tune;       // good_length, max_lazy, nice_length, max_chain in force, or null
    std::vector<uint8_t> out;
    int32_t status = 0;    // BPMD_OK, or need_buffers when out_cap was too small
    uint32_t bits = 0;     // exact length of `out` in bits
};
// returns 0 or a negative bpmd_result
using DeflateFn = int (*)(void* ctx, DeflateStep& step);

struct DeflateWriter {
    DeflateFn compress = nullptr;
    void* ctx = nullptr;
    int level = 6, wbits = 15, mem_level = 9, strategy = 0;
    // buffered message bytes; the plaintext already compressed since the last
    // reset (its last BPMD_CHUNK_HIST bytes: the history the next flush's
    // matches may reach into, as Beast's window does across flushes and,
    // under context takeover, across messages)
    std::vector<uint8_t> in;
    std::vector<uint8_t> hist;
    // output not yet handed out, plus < 8 pending bits
    std::vector<uint8_t> pend;
    size_t pend_pos = 0;
    uint32_t bits = 0;
    unsigned nbits = 0;
    int last_flush = -1;        // boost::none
    bool finished = false;      // finish_state
    bool inited = false;        // inited_ (deflate_stream.hpp:252): set by the first write or prime after a reset
    bool tuned = false;         // tune() values in force (until reset / a level change)
    int tune4[4] = {0, 0, 0, 0};

    // the bytes of history kept: the most any level uses (lz::chunk_hist)
    static constexpr size_t HIST_KEEP = lz::CHUNK_HIST_DEEP > BPMD_CHUNK_HIST ? lz::CHUNK_HIST_DEEP : BPMD_CHUNK_HIST;

    // the flushed bytes become history; only the last lz::chunk_hist(level) are used
    void add_history(const uint8_t* p, size_t n)
    {
        if (n >= HIST_KEEP) {
            hist.assign(p + n - HIST_KEEP, p + n);
            return;
        }
        hist.insert(hist.end(), p, p + n);
        if (hist.size() > HIST_KEEP) hist.erase(hist.begin(), hist.end() - (ptrdiff_t)HIST_KEEP);
    }

    void put_bits(uint32_t v, unsigned n)
    {
        bits |= v << nbits;
        nbits += n;
        while (nbits >= 8) {
            pend.push_back((uint8_t)bits);
            bits >>= 8;
            nbits -= 8;
        }
    }

    // append `nb` bits of the little-endian bit string p
    void put_bitstring(const uint8_t* p, uint64_t nb)
    {
        uint64_t i = 0;
        if (nbits == 0) {
            const size_t whole = (size_t)(nb >> 3);
            pend.insert(pend.end(), p, p + whole);
            i = (uint64_t)whole * 8;
        }
        for (; i + 8 <= nb; i += 8) put_bits(p[i >> 3], 8);
        if (i < nb) put_bits(p[i >> 3] & ((1u << (nb - i)) - 1), (unsigned)(nb - i));
    }

    void align_bits()
    {
        if (nbits) put_bits(0, 8 - nbits);
    }

    // tr_stored_block(nullptr, 0): 000, pad to a byte, 00 00 FF FF
    void put_empty_stored()
    {
        put_bits(0, 3);
        align_bits();
        put_bits(0x0000, 16);
        put_bits(0xFFFF, 16);
    }

    void drain(bpmd_zparams* zs)
    {
        const size_t avail = pend.size() - pend_pos;
        const size_t k = std::min(avail, zs->avail_out);
        if (k) {
            std::memcpy(zs->next_out, pend.data() + pend_pos, k);
            zs->next_out = (uint8_t*)zs->next_out + k;
            zs->avail_out -= k;
            zs->total_out += k;
            pend_pos += k;
        }
        if (pend_pos == pend.size()) {
            pend.clear();
            pend_pos = 0;
        }
    }

    bool has_pending() const { return pend_pos < pend.size(); }

    // maybe_init() -> init() (deflate_stream.hpp:593, deflate_stream.ipp:597-691): the first write() or
    // prime() after a reset; init() leaves last_flush_ = Flush::none (:685), so
    // a first write(Flush::none) without input is need_buffers
    void init_deflate()
    {
        if (inited) return;
        inited = true;
        last_flush = BPMD_FLUSH_NONE;
    }

    // the constructor's arguments (deflate_stream.ipp:235-253)
    int create(int level_, int window_bits, int mem_level_, int strategy_)
    {
        if (level_ == -1) level_ = 6;
        if (window_bits == 8) window_bits = 9;
        if (level_ < 0 || level_ > 9 || window_bits < 8 || window_bits > 15 || mem_level_ < 1 || mem_level_ > 9 ||
            strategy_ < BPMD_STRATEGY_NORMAL || strategy_ > BPMD_STRATEGY_FIXED)
            return BPMD_R_INVALID_ARGUMENT;
        level = level_;
        wbits = window_bits;
        mem_level = mem_level_;
        strategy = strategy_;
        return BPMD_R_OK;
    }

    int reset()
    {
        in.clear();
        hist.clear();
        pend.clear();
        pend_pos = 0;
        bits = 0;
        nbits = 0;
        last_flush = -1;
        finished = false;
        inited = false;   // the next write's init() -> lm_init() restores the level's table row
        tuned = false;
        return BPMD_R_OK;
    }

    int write(bpmd_zparams* zs, int flush)
    {
        if (flush < BPMD_FLUSH_NONE || flush > BPMD_FLUSH_TREES) return BPMD_R_INVALID_ARGUMENT;
        if (!zs->next_in && zs->avail_in) return BPMD_R_INVALID_ARGUMENT;   // throws invalid_argument
        if (!zs->next_out || (finished && flush != BPMD_FLUSH_FINISH)) return BPMD_STREAM_ERROR;
        if (zs->avail_out == 0) return BPMD_NEED_BUFFERS;
        init_deflate();   // maybe_init() (deflate_stream.ipp:361)
        const int old = last_flush;
        last_flush = flush;
        if (has_pending()) {
            drain(zs);
            if (zs->avail_out == 0) {
                last_flush = -1;
                return BPMD_OK;
            }
        } else if (zs->avail_in == 0 && old >= 0 && flush <= old && flush != BPMD_FLUSH_FINISH) {
            return BPMD_NEED_BUFFERS;
        }
        if (finished && zs->avail_in) return BPMD_NEED_BUFFERS;
        if (zs->avail_in) {
            const uint8_t* p = (const uint8_t*)zs->next_in;
            in.insert(in.end(), p, p + zs->avail_in);
            zs->next_in = p + zs->avail_in;
            zs->total_in += zs->avail_in;
            zs->avail_in = 0;
        }
        if (flush != BPMD_FLUSH_NONE && !finished) {
            if (!in.empty()) {
                DeflateStep st;
                st.in = in.data();
                st.n = in.size();
                st.hist = hist.data();
                st.hist_len = hist.size();
                st.out_cap = bpmd_deflate_upper_bound(in.size()) + 16;
                st.level = level;
                st.wbits = wbits;
                st.strategy = strategy;
                st.tune = tuned ? tune4 : nullptr;
                int r = compress(ctx, st);
                if (r) return r;
                if (st.status != BPMD_OK) return BPMD_STREAM_ERROR;
                // The kernels' blocks start at bit 0 of their output, and the
                // stored blocks and chunk markers among them are padded to a byte
                // from there.  After Flush::block, Flush::partial or a prime() the
                // stream is inside a byte: an empty stored block (what Flush::sync
                // emits) brings it to a byte boundary first.
                if (nbits) put_empty_stored();
                put_bitstring(st.out.data(), st.bits);
                add_history(in.data(), in.size());
                in.clear();
            }
            switch (flush) {
            case BPMD_FLUSH_PARTIAL:     // tr_align: empty static block
                put_bits(1u << 1, 3);
                put_bits(0, 7);
                break;
            case BPMD_FLUSH_SYNC:
            case BPMD_FLUSH_FULL:
            case BPMD_FLUSH_TREES:       // `flush != Flush::block` (deflate_stream.ipp:467-470):
                put_empty_stored();
                // clear_hash() (deflate_stream.ipp:474-483): nothing after a full
                // flush refers to anything before it
                if (flush == BPMD_FLUSH_FULL) hist.clear();
                break;
            case BPMD_FLUSH_FINISH:      // last block: empty fixed block with BFINAL = 1
                put_bits(1u | (1u << 1), 3);
                put_bits(0, 7);
                align_bits();
                finished = true;
                break;
            default:                     // block: the block is complete, bits stay pending
                break;
            }
            drain(zs);
            if (zs->avail_out == 0) last_flush = -1;
        }
        if (flush == BPMD_FLUSH_FINISH) return has_pending() ? BPMD_OK : BPMD_END_OF_STREAM;
        return BPMD_OK;
    }

    // deflate_stream::params (deflate_stream.ipp:307-338): buffered input is
    // compressed with the old parameters first, as a Flush::block
    int params(bpmd_zparams* zs, int level_, int strategy_)
    {
        if (level_ == -1) level_ = 6;
        if (level_ < 0 || level_ > 9 || strategy_ < BPMD_STRATEGY_NORMAL || strategy_ > BPMD_STRATEGY_FIXED)
            return BPMD_STREAM_ERROR;
        int r = BPMD_OK;
        // doParams calls doWrite(Flush::block) when the strategy or the level's
        // parser changes after any input (deflate_stream.ipp:334-341), buffered
        // input or not: the call is also what the next write's duplicate-flush
        // test sees as the previous flush.  Here a flush compresses all it has
        // buffered with one level, so any change of level flushes as well.
        const bool new_parser = lz::level_params(level_).parser != lz::level_params(level).parser;
        const bool ref_flush = (strategy_ != strategy || new_parser) && zs->total_in != 0;
        if (ref_flush || (!in.empty() && level_ != level)) {
            r = write(zs, BPMD_FLUSH_BLOCK);
            if (r == BPMD_NEED_BUFFERS && !has_pending()) r = BPMD_OK;   // `&& pending_ == 0` (:339)
        }
        // the new values hold whatever doWrite returned (deflate_stream.ipp:342-350); with no
        // room for output the input stays buffered and is compressed with them, as Beast's
        // unparsed lookahead is
        if (level_ != level) tuned = false;   // doParams reloads the level's table row
        level = level_;
        strategy = strategy_;
        return r;
    }

    // deflate_stream::tune (deflate_stream.hpp:163-181, deflate_stream.ipp:307-317).
    // Before the stream's first write the values are overwritten by the lazy
    // init()'s lm_init() (deflate_stream.ipp:688, 697-710), so they only take
    // effect on an initialised stream, until the next reset.
    int tune(int good_length, int max_lazy, int nice_length, int max_chain)
    {
        if (!inited) return BPMD_R_OK;
        tune4[0] = good_length;
        tune4[1] = max_lazy;
        tune4[2] = nice_length;
        tune4[3] = max_chain;
        tuned = true;
        return BPMD_R_OK;
    }

    // deflate_stream::pending (deflate_stream.hpp:344-348)
    int pending(unsigned* value, int* bits_) const
    {
        if (value) *value = (unsigned)(pend.size() - pend_pos);
        if (bits_) *bits_ = (int)nbits;
        return BPMD_OK;
    }

    // deflate_stream::prime (deflate_stream.ipp:340-355): insert up to 16 bits
    int prime(int bits_, int value)
    {
        if (bits_ < 0 || bits_ > 16) return BPMD_NEED_BUFFERS;
        init_deflate();   // maybe_init() (deflate_stream.ipp:560): a tune() after prime() is kept
        if (bits_) put_bits((uint32_t)value & ((1u << bits_) - 1u), (unsigned)bits_);
        return BPMD_OK;
    }
};

}  // namespace bpmd
