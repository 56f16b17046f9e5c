// Host-side check of the staged-table layouts of the batch calls (rwkv.cpp_amd/csrc/call_layout.h), compiled and run by
// tests/test_call_layout.py. Over a grid of shapes, for all five layouts: every field starts at a multiple of its type's alignment, the fields
// are disjoint and in declaration order, the cursor never padded, every offset equals the formula the hand-made layouts used before the
// cursor existed (written out below: the device sees the addresses it saw), and what a call copies up or down lies inside the range it
// copies. One deliberately wrong declaration shows the cursor pads a field that would be misaligned. No GPU, no HIP headers.
#include "call_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rwkvmi;

static int fails = 0;
#define CHECK(COND, ...) do { if (!(COND)) { fails++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); if (fails > 20) exit(1); } } while (0)

// a field as the checks see it, and the offset the earlier formula gives it
struct Seen { const char * name; size_t off, bytes, align, old_off; };
template <typename T> static Seen seen(const char * name, const Field<T> & f, size_t old_off) { return Seen{name, f.off, f.bytes(), alignof(T), old_off}; }

// alignment, declaration order without gap or overlap from 0 to `bytes`, and the earlier offsets
static void check_fields(const char * layout, const std::vector<Seen> & fs, size_t bytes, size_t old_bytes) {
    size_t at = 0, sum = 0;
    for (const Seen & f : fs) {
        CHECK(f.off % f.align == 0, "%s.%s: offset %zu is no multiple of %zu", layout, f.name, f.off, f.align);
        CHECK(f.off == at, "%s.%s: offset %zu, the field before it ends at %zu", layout, f.name, f.off, at);
        CHECK(f.off == f.old_off, "%s.%s: offset %zu, %zu before", layout, f.name, f.off, f.old_off);
        at = f.off + f.bytes;
        sum += f.bytes;
    }
    CHECK(bytes == sum && bytes == at, "%s: %zu bytes, the fields add up to %zu and end at %zu", layout, bytes, sum, at);
    CHECK(bytes == old_bytes, "%s: %zu bytes, %zu before", layout, bytes, old_bytes);
}

template <typename T> static bool within(const Field<T> & f, size_t from, size_t to) { return f.off >= from && f.end() <= to; }

static void check_seg(size_t n, size_t n_short, size_t T) {
    const SegLayout L(n, n_short, T);
    // (batch_upload_ragged's three inline offsets)
    const size_t off_short = n * sizeof(SegState), off_seg_of = off_short + n_short * sizeof(SegState), off_last = off_seg_of + T * sizeof(int32_t);
    const size_t bytes = off_last + n * sizeof(int32_t);
    check_fields("seg", {seen("segs", L.segs, 0), seen("shorts", L.shorts, off_short), seen("seg_of", L.seg_of, off_seg_of), seen("last", L.last, off_last)}, L.bytes, bytes);
    CHECK(L.segs.count == n && L.shorts.count == n_short && L.seg_of.count == T && L.last.count == n, "seg: counts");
}

static void check_stop(size_t n, size_t n_seqs, size_t n_toks) {
    const StopLayout L(n, n_seqs, n_toks);
    size_t o = 0;
    auto take = [&o](size_t b) { const size_t at = o; o += b; return at; };
    const size_t rows = take(n * sizeof(StopRow)), live = take(n * 4), lens = take(n * 4), reasons = take(n * 4), count = take(4);
    const size_t seq_lens = take(n_seqs * 4), seq_tokens = take(n_toks * 4);
    check_fields("stop", {seen("rows", L.rows, rows), seen("live", L.live, live), seen("lens", L.lens, lens), seen("reasons", L.reasons, reasons), seen("count", L.count, count),
                          seen("seq_lens", L.seq_lens, seq_lens), seen("seq_tokens", L.seq_tokens, seq_tokens)}, L.bytes, o);
    // what comes back is one copy of lens[n], reasons[n]
    CHECK(L.reasons.off == L.lens.end() && L.reasons.end() - L.lens.off == 2 * n * 4, "stop: lens and reasons are not 2 n adjacent words");
}

static void check_serve(size_t n, size_t R, size_t n_prompt, size_t n_seqs, size_t n_toks, size_t stride, bool guided) {
    const ServeLayout L(n, R, n_prompt, n_seqs, n_toks, stride, guided);
    size_t o = 0;
    auto take = [&o](size_t b) { const size_t at = o; o += b; return at; };
    const size_t g = guided ? 4 : 0;
    const size_t reqs = take(R * sizeof(ServeReq));
    const size_t prompts = take(n_prompt * 4), seq_lens = take(n_seqs * 4), seq_tokens = take(n_toks * 4);
    const size_t lane_slot = take(n * 4), req = take(n * 4), pos = take(n * 4), draw = take(n * 4), admit = take(n * 4);
    const size_t g_state = take(n * g), g_misses = take(n * g);
    const size_t next = take(4), work = take(4);
    const size_t down = o;
    const size_t last = take(n * 4), lens = take(R * 4), reasons = take(R * 4), lane = take(R * 4), start = take(R * 4);
    const size_t req_g_state = take(R * g), req_g_misses = take(R * g);
    const size_t out = take(R * stride * 4);
    check_fields("serve", {seen("reqs", L.reqs, reqs), seen("prompts", L.prompts, prompts), seen("seq_lens", L.seq_lens, seq_lens), seen("seq_tokens", L.seq_tokens, seq_tokens),
                           seen("lane_slot", L.lane_slot, lane_slot), seen("req", L.req, req), seen("pos", L.pos, pos), seen("draw", L.draw, draw), seen("admit", L.admit, admit),
                           seen("g_state", L.g_state, g_state), seen("g_misses", L.g_misses, g_misses), seen("next", L.next, next), seen("work", L.work, work),
                           seen("last", L.last, last), seen("lens", L.lens, lens), seen("reasons", L.reasons, reasons), seen("lane", L.lane, lane), seen("start", L.start, start),
                           seen("req_g_state", L.req_g_state, req_g_state), seen("req_g_misses", L.req_g_misses, req_g_misses), seen("out", L.out, out)}, L.bytes, o);
    CHECK(L.down == down && L.down == L.work.end() && L.down == L.last.off, "serve: down is %zu, %zu before", L.down, down);
    const size_t gc = guided ? 1 : 0;
    CHECK(L.g_state.count == n * gc && L.g_misses.count == n * gc && L.req_g_state.count == R * gc && L.req_g_misses.count == R * gc, "serve: the guide fields' counts");
    // the upload is [0, out): every field the host initialises lies in it
    const size_t up = L.out.off;
    CHECK(within(L.reqs, 0, up) && within(L.prompts, 0, up) && within(L.seq_lens, 0, up) && within(L.seq_tokens, 0, up) && within(L.lane_slot, 0, up) && within(L.req, 0, up) &&
          within(L.pos, 0, up) && within(L.draw, 0, up) && within(L.admit, 0, up) && within(L.g_state, 0, up) && within(L.g_misses, 0, up) && within(L.next, 0, up) &&
          within(L.work, 0, up) && within(L.last, 0, up) && within(L.lens, 0, up) && within(L.reasons, 0, up) && within(L.lane, 0, up) && within(L.start, 0, up) &&
          within(L.req_g_state, 0, up) && within(L.req_g_misses, 0, up), "serve: a field the host initialises is outside the upload");
    // the copy back is [down, bytes): every field the host reads after the loop lies in it
    CHECK(within(L.last, L.down, L.bytes) && within(L.lens, L.down, L.bytes) && within(L.reasons, L.down, L.bytes) && within(L.lane, L.down, L.bytes) &&
          within(L.start, L.down, L.bytes) && within(L.req_g_state, L.down, L.bytes) && within(L.req_g_misses, L.down, L.bytes) && within(L.out, L.down, L.bytes),
          "serve: a field that is read back is outside the copy back");
}

static void check_beam(size_t rows) {
    const BeamLayout L(rows);
    const size_t finished = rows * sizeof(double), lens = finished + rows * 4, count = lens + rows * 4, upload = count + 8;
    const size_t ids = upload, lp = ids + rows * RWKV_MI_TOP_MAX * 4, chosen = lp + rows * RWKV_MI_TOP_MAX * 4, bytes = chosen + rows * 4;
    check_fields("beam", {seen("score", L.score, 0), seen("finished", L.finished, finished), seen("lens", L.lens, lens), seen("count", L.count, count), seen("ids", L.ids, ids),
                          seen("lp", L.lp, lp), seen("chosen", L.chosen, chosen)}, L.bytes, bytes);
    CHECK(L.count.bytes() == 8, "beam: the count field is %zu bytes", L.count.bytes());
    CHECK(L.upload == upload && L.upload == L.count.end(), "beam: upload is %zu, %zu before", L.upload, upload);
    // up: [0, upload); back: [0, count)
    CHECK(within(L.score, 0, L.upload) && within(L.finished, 0, L.upload) && within(L.lens, 0, L.upload) && within(L.count, 0, L.upload), "beam: an uploaded field is outside the upload");
    CHECK(within(L.score, 0, L.count.off) && within(L.finished, 0, L.count.off) && within(L.lens, 0, L.count.off), "beam: a field that is read back is outside the copy back");
}

static void check_draft(size_t n_slots) {
    const DraftLayout L(n_slots);
    // (keep at word 0, out at word n_slots, 2 + RWKV_MI_DRAFT_MAX words per slot in all)
    check_fields("draft", {seen("keep", L.keep, 0), seen("out", L.out, n_slots * 4)}, L.bytes, n_slots * (2 + RWKV_MI_DRAFT_MAX) * 4);
    CHECK(L.keep.count == n_slots && L.out.count == n_slots * (1 + RWKV_MI_DRAFT_MAX), "draft: counts");
    // what comes back: the first rows of both
    CHECK(L.out.first(1 + RWKV_MI_DRAFT_MAX).off == L.out.off && L.out.first(1 + RWKV_MI_DRAFT_MAX).end() == L.out.off + (1 + RWKV_MI_DRAFT_MAX) * 4 && L.keep.first(1).end() == L.keep.off + 4,
          "draft: the first row of a field is not its first bytes");
}

// the declaration no layout may make by hand: a 4-byte field in front of an 8-byte one. The cursor pads it.
static void check_cursor_pads() {
    for (size_t n : {(size_t) 1, (size_t) 3, (size_t) 64}) {
        LayoutCursor c;
        const Field<uint32_t> words = c.take<uint32_t>(n);
        const Field<double> scores = c.take<double>(n);
        const size_t want = (n * 4 + 7) / 8 * 8;
        CHECK(words.off == 0 && scores.off == want && scores.off % alignof(double) == 0, "cursor: a double after %zu words starts at %zu, not at %zu", n, scores.off, want);
        CHECK(c.bytes() == want + n * 8, "cursor: %zu bytes, expected %zu", c.bytes(), want + n * 8);
        if (n % 2) CHECK(scores.off != words.end(), "cursor: %zu words were not padded", n);
    }
    LayoutCursor c;
    (void) c.take<uint32_t>(1);
    CHECK(c.take<ServeReq>(1).off == alignof(ServeReq) && c.take<uint8_t>(3).end() % 2 == 1 && c.take<SegState>(0).off % alignof(SegState) == 0, "cursor: struct fields are not aligned");
}

int main() {
    size_t shapes = 0;
    for (size_t n : {(size_t) 1, (size_t) 3, (size_t) 64}) {
        for (size_t T : {n, n + 32, (size_t) 150})
            for (size_t n_short : {(size_t) 0, n}) { check_seg(n, n_short, T); shapes++; }
        for (size_t R : {n, n + 1, 4 * n})
            for (size_t n_seqs : {(size_t) 0, (size_t) 1, 2 * R})
                for (size_t n_toks : {(size_t) 0, n_seqs, 3 * n_seqs}) {
                    check_stop(n, n_seqs, n_toks); shapes++;
                    for (size_t n_prompt : {R, 5 * R})
                        for (size_t stride : {(size_t) 0, (size_t) 1, (size_t) 7})
                            for (bool guided : {false, true}) { check_serve(n, R, n_prompt, n_seqs, n_toks, stride, guided); shapes++; }
                }
    }
    for (size_t rows : {(size_t) 1, (size_t) 4, (size_t) 64}) { check_beam(rows); shapes++; }
    for (size_t n_slots : {(size_t) 1, (size_t) 4}) { check_draft(n_slots); shapes++; }
    check_cursor_pads();
    if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
    printf("call layouts OK (%zu shapes)\n", shapes);
    return 0;
}
