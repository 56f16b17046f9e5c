// call_layout.h -- where the words of a batch call lie in its staged table (devmem.h, Staged): one device buffer with pinned staging of the
// same layout. A layout is a struct of Fields handed out by one cursor, in the order the table holds them; the cursor is the one place that
// adds up offsets, and it starts every field at a multiple of its type's alignment. No HIP include: a host compiler checks the layouts
// (tests/cpp/call_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rows.h"

namespace rwkvmi {

// `count` elements of T at byte offset `off` of both buffers
template <typename T> struct Field {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return off + bytes(); }
    Field first(size_t k) const { return Field{off, k}; }   // its first k elements
};

struct LayoutCursor {
    size_t at = 0;
    template <typename T> Field<T> take(size_t count) {
        at = (at + alignof(T) - 1) / alignof(T) * alignof(T);
        const Field<T> f{at, count};
        at = f.end();
        return f;
    }
    size_t bytes() const { return at; }
};

// A ragged pass of n segments over T tokens (rwkv_mi_batch_eval_ragged*): the segments, the n_short short ones again (the long ones stay on
// the host: each is a launch of its own), the segment of every token, the last token of every segment. All of it goes up in one copy.
struct SegLayout {
    Field<SegState> segs, shorts;
    Field<int32_t> seg_of, last;
    size_t bytes;
    SegLayout(size_t n, size_t n_short, size_t T) {
        LayoutCursor c;
        segs = c.take<SegState>(n); shorts = c.take<SegState>(n_short); seg_of = c.take<int32_t>(T); last = c.take<int32_t>(n);
        bytes = c.bytes();
    }
};

// The stop words of a call of n rows with n_seqs sequences of n_toks tokens in all (rwkv_mi_batch_decode_until): the rows, their live words,
// lengths and reasons, the live count, the sequences' lengths and tokens. All of it goes up; lens and reasons, which are adjacent, come back.
struct StopLayout {
    Field<StopRow> rows;
    Field<uint32_t> live, lens, reasons, count, seq_lens, seq_tokens;
    size_t bytes;
    StopLayout(size_t n, size_t n_seqs, size_t n_toks) {
        LayoutCursor c;
        rows = c.take<StopRow>(n); live = c.take<uint32_t>(n); lens = c.take<uint32_t>(n); reasons = c.take<uint32_t>(n); count = c.take<uint32_t>(1);
        seq_lens = c.take<uint32_t>(n_seqs); seq_tokens = c.take<uint32_t>(n_toks);
        bytes = c.bytes();
    }
};

// The words of a serve call of n lanes and R requests (rwkv_mi_batch_serve*). What goes up: the request table, the prompts and the sequences,
// the lane words in their start values, the head of the queue and the work count. From `down` on, what comes back as well: the lanes' last
// requests, the requests' lengths, reasons, lanes and start passes, and their emitted tokens out[R][stride] (filled on the device: the upload
// ends at out). guided (a call of rwkv_mi_batch_serve_ex with a guided request; count 0 otherwise): the lanes' guide state and miss words go
// up, the requests' -- the start state and 0 on the way up, the final words on the way back -- do both.
struct ServeLayout {
    Field<ServeReq> reqs;
    Field<uint32_t> prompts, seq_lens, seq_tokens, lane_slot, req, pos, draw, admit, g_state, g_misses, next, work;
    size_t down;
    Field<uint32_t> last, lens, reasons, lane, start, req_g_state, req_g_misses, out;
    size_t bytes;
    ServeLayout(size_t n, size_t R, size_t n_prompt, size_t n_seqs, size_t n_toks, size_t stride, bool guided) {
        LayoutCursor c;
        const auto words = [&c](size_t count) { return c.take<uint32_t>(count); };
        const size_t g = guided ? 1 : 0;
        reqs = c.take<ServeReq>(R);
        prompts = words(n_prompt); seq_lens = words(n_seqs); seq_tokens = words(n_toks);
        lane_slot = words(n); req = words(n); pos = words(n); draw = words(n); admit = words(n);
        g_state = words(n * g); g_misses = words(n * g);
        next = words(1); work = words(1);
        down = c.bytes();
        last = words(n); lens = words(R); reasons = words(R); lane = words(R); start = words(R);
        req_g_state = words(R * g); req_g_misses = words(R * g);
        out = words(R * stride);
        bytes = c.bytes();
    }
};

// The words of a serve session of n lanes over a ring of `capacity` requests (rwkv_mi_batch_serve_open ..). A RING ENTRY has a fixed size:
// the request's ServeReq in the dense table reqs[capacity] (k_serve_reset indexes it as it does a call's), and entry_words words in `ring`
// -- max_prompt prompt tokens, max_seqs sequence lengths, max_seq_tokens sequence tokens, the start state of its guide. Request id q lives
// in entry q % capacity, and a submit goes up as the bytes of its entry alone, one copy for each of the two tables (reqs_range,
// words_range). word(e, w) is word w of entry e as a word of the ring, which is what a ServeReq's prompt0, stop.seq0 and stop.tok0 hold.
// Behind the ring: the cancel words, TWICE -- block b uploads and reads half b & 1, so a copy that is still pending never sees the next
// block's words -- and the lane words in their start values, which go up once, at open. From `down` on, what a block fetches (all of it,
// one copy, into the half b & 1 of pinned staging of its own): the queue's head and the work count, the lanes' last ids, then per entry the
// id it was admitted for, done, length, reason, lane, start pass, end pass, revived, the two guide words (guided sessions) and the emitted
// tokens out[capacity][stride].
struct SessionLayout {
    size_t capacity = 0, entry_words = 0;
    size_t w_prompt = 0, w_seq_lens = 0, w_seq_tokens = 0, w_guide = 0;   // words of an entry, from its start
    Field<ServeReq> reqs;
    Field<uint32_t> ring, cancel, lane_slot, req, pos, draw, admit, g_state, g_misses;
    size_t down = 0;
    Field<uint32_t> next, work, last, ids, done, lens, reasons, lane, start, end, revived, req_g_state, req_g_misses, out;
    size_t bytes = 0;
    SessionLayout() = default;
    SessionLayout(size_t n, size_t capacity_, size_t max_prompt, size_t max_seqs, size_t max_seq_tokens, size_t stride, bool guided) : capacity(capacity_) {
        w_prompt = 0; w_seq_lens = max_prompt; w_seq_tokens = w_seq_lens + max_seqs; w_guide = w_seq_tokens + max_seq_tokens;
        entry_words = w_guide + 1;
        LayoutCursor c;
        const auto words = [&c](size_t count) { return c.take<uint32_t>(count); };
        const size_t g = guided ? 1 : 0, C = capacity;
        reqs = c.take<ServeReq>(C);
        ring = words(C * entry_words);
        cancel = words(2 * C);
        lane_slot = words(n); req = words(n); pos = words(n); draw = words(n); admit = words(n);
        g_state = words(n * g); g_misses = words(n * g);
        down = c.bytes();
        next = words(1); work = words(1); last = words(n);
        ids = words(C); done = words(C); lens = words(C); reasons = words(C); lane = words(C); start = words(C); end = words(C); revived = words(C);
        req_g_state = words(C * g); req_g_misses = words(C * g);
        out = words(C * stride);
        bytes = c.bytes();
    }
    size_t entry_of(uint32_t id) const { return (size_t) id % capacity; }
    size_t word(size_t e, size_t w) const { return e * entry_words + w; }                       // words, of the ring
    // the bytes the entries [e0, e1) go up as: their ServeReqs, their words; and half `half` of the cancel words
    void reqs_range(size_t e0, size_t e1, size_t * from, size_t * to) const { *from = reqs.off + e0 * sizeof(ServeReq); *to = reqs.off + e1 * sizeof(ServeReq); }
    void words_range(size_t e0, size_t e1, size_t * from, size_t * to) const { *from = ring.off + word(e0, 0) * sizeof(uint32_t); *to = ring.off + word(e1, 0) * sizeof(uint32_t); }
    Field<uint32_t> cancel_half(size_t half) const { return Field<uint32_t>{cancel.off + half * capacity * sizeof(uint32_t), capacity}; }
};

// The beam words of `rows` rows (rwkv_mi_batch_decode_beam): scores, finished words, lengths, the live count with its pad word -- up to
// `upload`, the part a call uploads; what lies in front of count comes back -- then the candidates' ids and log-probs
// [rows][RWKV_MI_TOP_MAX] and the body's unused word per row, which never leave the device.
struct BeamLayout {
    Field<double> score;
    Field<uint32_t> finished, lens, count;
    size_t upload;
    Field<uint32_t> ids;
    Field<float> lp, chosen;
    size_t bytes;
    explicit BeamLayout(size_t rows) {
        LayoutCursor c;
        score = c.take<double>(rows); finished = c.take<uint32_t>(rows); lens = c.take<uint32_t>(rows); count = c.take<uint32_t>(2);
        upload = c.bytes();
        ids = c.take<uint32_t>(rows * RWKV_MI_TOP_MAX); lp = c.take<float>(rows * RWKV_MI_TOP_MAX); chosen = c.take<float>(rows);
        bytes = c.bytes();
    }
};

// The words a draft pass leaves (rwkv_mi_batch_eval_draft), for n_slots rows: how much of each row's draft stands, and the tokens the row
// emitted, out[n_slots][1 + RWKV_MI_DRAFT_MAX]. Nothing goes up; the first rows of both come back.
struct DraftLayout {
    Field<uint32_t> keep, out;
    size_t bytes;
    explicit DraftLayout(size_t n_slots) {
        LayoutCursor c;
        keep = c.take<uint32_t>(n_slots); out = c.take<uint32_t>(n_slots * (1 + RWKV_MI_DRAFT_MAX));
        bytes = c.bytes();
    }
};

}  // namespace rwkvmi
