// Host-side check of the staged table of a serve session (rwkv.cpp_amd/csrc/call_layout.h, SessionLayout), compiled and run by
// tests/test_cpu_batch_session.py. Over a grid of shapes: every field starts at a multiple of its type's alignment, the fields are disjoint
// and in declaration order from 0 to `bytes`; the parts of a ring entry lie inside its words, in order, without overlap; request id q
// addresses entry q % capacity in both tables of the ring; what a block copies up (a run of entries, one half of the cancel words) and
// down ([down, bytes)) lies inside the range it copies and holds what the host reads. No GPU, no HIP headers.
#include "call_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rwkvmi;

static int fails = 0;
#define CHECK(COND, ...) do { if (!(COND)) { fails++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); if (fails > 20) exit(1); } } while (0)

struct Seen { const char * name; size_t off, bytes, align; };
template <typename T> static Seen seen(const char * name, const Field<T> & f) { return Seen{name, f.off, f.bytes(), alignof(T)}; }
template <typename T> static bool within(const Field<T> & f, size_t from, size_t to) { return f.off >= from && f.end() <= to; }

static void check(size_t n, size_t C, size_t max_prompt, size_t max_seqs, size_t max_seq_tokens, size_t stride, bool guided) {
    const SessionLayout L(n, C, max_prompt, max_seqs, max_seq_tokens, stride, guided);
    const std::vector<Seen> fs = {seen("reqs", L.reqs), seen("ring", L.ring), seen("cancel", L.cancel), seen("lane_slot", L.lane_slot), seen("req", L.req), seen("pos", L.pos), seen("draw", L.draw),
                                  seen("admit", L.admit), seen("g_state", L.g_state), seen("g_misses", L.g_misses), seen("next", L.next), seen("work", L.work), seen("last", L.last),
                                  seen("ids", L.ids), seen("done", L.done), seen("lens", L.lens), seen("reasons", L.reasons), seen("lane", L.lane), seen("start", L.start),
                                  seen("end", L.end), seen("revived", L.revived), seen("req_g_state", L.req_g_state), seen("req_g_misses", L.req_g_misses), seen("out", L.out)};
    size_t at = 0;
    for (const Seen & f : fs) {
        CHECK(f.off % f.align == 0, "%s: offset %zu is no multiple of %zu", f.name, f.off, f.align);
        CHECK(f.off == at, "%s: offset %zu, the field before it ends at %zu", f.name, f.off, at);
        at = f.off + f.bytes;
    }
    CHECK(at == L.bytes, "%zu bytes, the fields end at %zu", L.bytes, at);
    CHECK(L.down == L.next.off && L.down == L.g_misses.end(), "down is %zu", L.down);
    // the entry's words: prompt, sequence lengths, sequence tokens, guide word
    CHECK(L.w_prompt == 0 && L.w_seq_lens == max_prompt && L.w_seq_tokens == L.w_seq_lens + max_seqs && L.w_guide == L.w_seq_tokens + max_seq_tokens && L.entry_words == L.w_guide + 1,
          "the words of an entry: %zu %zu %zu %zu of %zu", L.w_prompt, L.w_seq_lens, L.w_seq_tokens, L.w_guide, L.entry_words);
    CHECK(L.reqs.count == C && L.ring.count == C * L.entry_words && L.reqs.off % alignof(ServeReq) == 0, "the ring: %zu requests, %zu words", L.reqs.count, L.ring.count);
    // id -> entry -> address: ids count up across several times the capacity
    for (uint32_t id = 0; id < 3 * C + 2; id++) {
        const size_t e = L.entry_of(id);
        CHECK(e == id % C && e < C, "id %u lives in entry %zu", id, e);
        CHECK(L.word(e, 0) == e * L.entry_words && L.word(e, L.w_guide) < L.ring.count && L.word(e, L.w_guide) + 1 == L.word(e + 1, 0), "entry %zu: its words [%zu, %zu]", e,
              L.word(e, 0), L.word(e, L.w_guide));
    }
    // up: a run of entries [e0, e1) is exactly their bytes of both tables
    for (size_t e0 = 0; e0 < C; e0++)
        for (size_t e1 = e0 + 1; e1 <= C; e1++) {
            size_t from = 0, to = 0;
            L.reqs_range(e0, e1, &from, &to);
            CHECK(from == L.reqs.off + e0 * sizeof(ServeReq) && to - from == (e1 - e0) * sizeof(ServeReq) && to <= L.reqs.end(), "requests [%zu, %zu) go up as [%zu, %zu)", e0, e1, from, to);
            L.words_range(e0, e1, &from, &to);
            CHECK(from == L.ring.off + e0 * L.entry_words * 4 && to - from == (e1 - e0) * L.entry_words * 4 && to <= L.ring.end(), "words [%zu, %zu) go up as [%zu, %zu)", e0, e1, from, to);
        }
    // the two halves of the cancel words: C words each, disjoint, inside the field
    const Field<uint32_t> h0 = L.cancel_half(0), h1 = L.cancel_half(1);
    CHECK(h0.count == C && h1.count == C && h0.off == L.cancel.off && h1.off == h0.end() && h1.end() == L.cancel.end(), "the cancel halves");
    // what goes up once, at open, is the whole table; what a block fetches is [down, bytes): every word the host reads lies in it, and
    // nothing the host writes between blocks does
    CHECK(within(L.next, L.down, L.bytes) && within(L.work, L.down, L.bytes) && within(L.last, L.down, L.bytes) && within(L.ids, L.down, L.bytes) &&
          within(L.done, L.down, L.bytes) && within(L.lens, L.down, L.bytes) && within(L.reasons, L.down, L.bytes) && within(L.lane, L.down, L.bytes) &&
          within(L.start, L.down, L.bytes) && within(L.end, L.down, L.bytes) && within(L.revived, L.down, L.bytes) && within(L.req_g_state, L.down, L.bytes) &&
          within(L.req_g_misses, L.down, L.bytes) && within(L.out, L.down, L.bytes), "a field that is read back is outside the fetch");
    CHECK(within(L.reqs, 0, L.down) && within(L.ring, 0, L.down) && within(L.cancel, 0, L.down) && within(L.lane_slot, 0, L.down) && within(L.req, 0, L.down), "a field the host writes is inside the fetch");
    const size_t g = guided ? 1 : 0;
    CHECK(L.g_state.count == n * g && L.g_misses.count == n * g && L.req_g_state.count == C * g && L.req_g_misses.count == C * g, "the guide fields' counts");
    CHECK(L.out.count == C * stride && L.ids.count == C && L.last.count == n, "counts");
}

int main() {
    size_t shapes = 0;
    for (size_t n : {(size_t) 1, (size_t) 3, (size_t) 64})
        for (size_t C : {(size_t) 1, (size_t) 4, (size_t) 7, (size_t) 65})
            for (size_t max_prompt : {(size_t) 1, (size_t) 5, (size_t) 64})
                for (size_t max_seqs : {(size_t) 0, (size_t) 3, (size_t) 16})
                    for (size_t stride : {(size_t) 1, (size_t) 9})
                        for (bool guided : {false, true}) { check(n, C, max_prompt, max_seqs, max_seqs * 3, stride, guided); shapes++; }
    if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
    printf("session layout OK (%zu shapes)\n", shapes);
    return 0;
}
