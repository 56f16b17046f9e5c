// Host-side check of the bookkeeping of a serve session (rwkv.cpp_amd/csrc/session_book.h), compiled with the address and undefined-behaviour
// sanitizers and run by tests/test_cpu_batch_session.py. A few words stand in for the device: the script below writes what a block would have
// brought back and the book reads it. Checked: ids and entries across several times the capacity, room and in-flight, delivery with
// max_events and max_tokens of 1 (nothing lost, nothing twice), the busy rule over a scripted sequence of submit / enqueue / consume, and
// the per-lane sums the parities at close come from. No GPU, no HIP headers.
#include "session_book.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rwkvmi;

static int fails = 0;
#define CHECK(COND, ...) do { if (!(COND)) { fails++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); if (fails > 20) exit(1); } } while (0)

// the words a block brings back, as vectors
struct Words {
    size_t C, stride;
    uint32_t next = 0, work = 0;
    std::vector<uint32_t> ids, done, lens, reasons, lane, start, end, revived, gs, gm, out;
    Words(size_t C_, size_t stride_) : C(C_), stride(stride_), ids(C_, RWKV_MI_NO_TOKEN), done(C_, 0), lens(C_, 0), reasons(C_, RWKV_MI_NO_TOKEN), lane(C_, 0), start(C_, 0), end(C_, 0),
                                       revived(C_, 0), gs(C_, 0), gm(C_, 0), out(C_ * stride_, RWKV_MI_NO_TOKEN) {}
    SessionWords view(bool guided) const {
        return SessionWords{&next, &work, ids.data(), done.data(), lens.data(), reasons.data(), lane.data(), start.data(), end.data(), revived.data(),
                            guided ? gs.data() : nullptr, guided ? gm.data() : nullptr, out.data()};
    }
    void admit(uint32_t id, uint32_t lane_, uint32_t start_, uint32_t revived_) {
        const size_t e = id % C;
        ids[e] = id; done[e] = 0; lens[e] = 0; reasons[e] = RWKV_MI_NO_TOKEN; lane[e] = lane_; start[e] = start_; revived[e] = revived_;
    }
    void emit(uint32_t id, uint32_t token) { const size_t e = id % C; out[e * stride + lens[e]] = token; lens[e]++; }
    void retire(uint32_t id, uint32_t reason, uint32_t end_) { const size_t e = id % C; done[e] = 1; reasons[e] = reason; end[e] = end_; }
};

static uint32_t tok(uint32_t id, uint32_t j) { return 1000u * id + j; }

// ids, entries, room: 5 times the capacity through a ring of 3, one lane, every request two tokens
static void check_wrap() {
    const size_t C = 3, stride = 4, K = 2;
    SessionBook b;
    b.init(C, 1, stride, K);
    Words w(C, stride);
    CHECK(!b.busy() && b.room() == C && b.in_flight == 0, "a fresh book");
    std::vector<rwkv_mi_serve_event> ev(C);
    std::vector<uint32_t> toks(C * stride);
    uint32_t next_to_run = 0, pass = 0;
    std::vector<uint32_t> seen_tokens;
    for (int round = 0; next_to_run < 5 * C; round++) {
        while (b.room() > 0 && b.submitted < 5 * C) {
            const uint32_t before = b.room();
            const uint32_t id = b.submit();
            CHECK(id == b.submitted - 1 && b.entry_of(id) == id % C && b.room() == before - 1, "submit %u", id);
        }
        CHECK(b.submitted - b.oldest <= C && b.busy(), "round %d: %u in the ring", round, b.submitted - b.oldest);
        const SessionBook::Block blk = b.begin_block();
        CHECK(blk.first_pass == pass && blk.tail == b.submitted && blk.upload_to == b.submitted && blk.upload_from <= blk.upload_to, "block %d", round);
        // the device: the one lane runs the next request, two passes, two tokens
        const uint32_t id = next_to_run++;
        CHECK(id < blk.tail, "the device ran a request the host had not uploaded");
        w.admit(id, 0, pass, round == 0 ? 1u : 0u);
        w.emit(id, tok(id, 0)); w.emit(id, tok(id, 1));
        w.retire(id, RWKV_MI_NO_TOKEN, pass + 1);
        w.next = id + 1; w.work = 0;
        pass += (uint32_t) K;
        b.consume(w.view(false));
        size_t ne = 0, nt = 0;
        b.deliver(ev.data(), ev.size(), toks.data(), toks.size(), &ne, &nt);
        CHECK(ne == 1 && nt == 2 && ev[0].id == id && ev[0].first == 0 && ev[0].n_new == 2 && ev[0].finished == 1 && ev[0].stopped_by == RWKV_MI_NO_TOKEN &&
              ev[0].lane == 0 && ev[0].start_pass == blk.first_pass, "round %d: %zu events, %zu tokens", round, ne, nt);
        CHECK(toks[0] == tok(id, 0) && toks[1] == tok(id, 1), "round %d: tokens", round);
        CHECK(b.oldest == id + 1 && !b.is_live(id) && !b.cancel_request(id), "round %d: a delivered request is not in flight", round);
    }
    CHECK(b.in_flight == 0 && b.room() == C && !b.busy(), "the end: %u in flight", b.in_flight);
    CHECK(b.lane_passes[0] == 2 * 5 * C && b.lane_revivals[0] == 1 && b.lane_last[0] == 5 * C - 1, "lane sums: %llu passes", (unsigned long long) b.lane_passes[0]);
    CHECK(b.parity_flip(0) == (int) ((2 * 5 * C - 1) & 1), "parity");
    CHECK(!b.cancel_request(5 * C) && !b.cancel_request(RWKV_MI_NO_TOKEN), "an id never issued");
}

// delivery one event and one token at a time: two requests, out of order ends, nothing lost or repeated
static void check_trickle() {
    const size_t C = 4, stride = 5;
    SessionBook b;
    b.init(C, 2, stride, 3);
    Words w(C, stride);
    const uint32_t a = b.submit(), c = b.submit();
    (void) b.begin_block();
    w.admit(a, 0, 0, 1); w.admit(c, 1, 0, 1);
    for (uint32_t j = 0; j < 3; j++) { w.emit(a, tok(a, j)); w.emit(c, tok(c, j)); }
    w.retire(c, 1u, 2);   // (the younger one ends first, by its stop sequence 1)
    w.next = 2; w.work = 1;
    b.consume(w.view(true));
    std::vector<std::vector<uint32_t>> got(2);
    std::vector<int> finished(2, 0);
    rwkv_mi_serve_event ev;
    uint32_t t = 0;
    int polls = 0;
    for (;; polls++) {
        size_t ne = 0, nt = 0;
        b.deliver(&ev, 1, &t, 1, &ne, &nt);
        if (ne == 0) break;
        CHECK(ne == 1 && nt == ev.n_new && ev.n_new <= 1 && ev.id < 2, "a trickled event");
        CHECK(ev.first == got[ev.id].size(), "request %u: first %u after %zu tokens", ev.id, ev.first, got[ev.id].size());
        if (nt) got[ev.id].push_back(t);
        if (ev.finished) { finished[ev.id]++; CHECK(ev.id == c && ev.stopped_by == 1u, "who finished"); }
        CHECK(polls < 20, "delivery does not end");
    }
    CHECK(got[a].size() == 3 && got[c].size() == 3 && finished[c] == 1 && finished[a] == 0, "after the first block: %zu %zu", got[a].size(), got[c].size());
    for (uint32_t j = 0; j < 3; j++) CHECK(got[a][j] == tok(a, j) && got[c][j] == tok(c, j), "token %u", j);
    // the older one is still in flight: the ring has room for capacity - 2 (its entry and the younger one's slot behind it count)
    CHECK(b.in_flight == 1 && b.oldest == a && b.room() == C - 2 && b.is_live(a) && !b.is_live(c), "in flight %u, room %u", b.in_flight, b.room());
    // a cancel, one more token in the pass of the block that carried it, then the end
    CHECK(b.cancel_request(a) && b.cancel[b.entry_of(a)] == 1u, "cancel");
    (void) b.begin_block();
    w.emit(a, tok(a, 3)); w.retire(a, RWKV_MI_STOP_CANCELLED, 3); w.work = 0;
    b.consume(w.view(true));
    size_t ne = 0, nt = 0;
    uint32_t two[2];
    b.deliver(&ev, 1, two, 2, &ne, &nt);
    CHECK(ne == 1 && nt == 1 && ev.id == a && ev.first == 3 && ev.finished == 1 && ev.stopped_by == RWKV_MI_STOP_CANCELLED && two[0] == tok(a, 3), "the cancelled end");
    CHECK(b.in_flight == 0 && b.room() == C && b.oldest == 2, "all delivered");
    // lane 0: passes 0 .. 3, revived once; lane 1: passes 0 .. 2, revived once
    CHECK(b.lane_passes[0] == 4 && b.lane_passes[1] == 3 && b.parity_flip(0) == 1 && b.parity_flip(1) == 0, "the parity sums: %llu %llu", (unsigned long long) b.lane_passes[0],
          (unsigned long long) b.lane_passes[1]);
    // a new request in the cancelled one's entry starts with a cleared cancel word
    for (size_t i = 0; i < C - 1; i++) (void) b.submit();
    (void) b.submit();
    for (size_t i = 0; i < C; i++) CHECK(b.cancel[i] == 0u, "cancel word %zu survives its request", i);
    CHECK(b.room() == 0, "a full ring has no room");
}

// the busy rule over a script
static void check_busy() {
    const size_t C = 2, stride = 2;
    SessionBook b;
    b.init(C, 1, stride, 4);
    Words w(C, stride);
    CHECK(!b.busy(), "nothing submitted");
    const uint32_t id = b.submit();
    CHECK(b.busy(), "a submit the device has not seen: the head (0) is below the number submitted (1)");
    (void) b.begin_block();                                    // block 0
    CHECK(b.busy() && b.enqueued == 1 && b.consumed == 0 && b.passes == 4, "a block enqueued and unconsumed");
    (void) b.begin_block();                                    // block 1
    // block 0: admitted, one token, still running
    w.admit(id, 0, 0, 1); w.emit(id, 7); w.next = 1; w.work = 1;
    b.consume(w.view(false));
    CHECK(b.busy() && b.consumed == 1, "block 1 is unconsumed");
    // block 1: it ends
    w.emit(id, 8); w.retire(id, RWKV_MI_NO_TOKEN, 1); w.work = 0;
    b.consume(w.view(false));
    CHECK(!b.busy() && b.enqueued == 2 && b.consumed == 2, "everything consumed, no work, the head at the number submitted");
    // busy is about the device, not about delivery: the end is still undelivered
    CHECK(b.in_flight == 1, "undelivered");
    // a consumed block that left work: busy though nothing is enqueued
    const uint32_t id2 = b.submit();
    (void) b.begin_block();
    w.admit(id2, 0, 8, 1); w.next = 2; w.work = 1;
    b.consume(w.view(false));
    CHECK(b.busy() && b.enqueued == b.consumed, "the last consumed block left a work count above 0");
    // an entry the device has not admitted for the new id is not read: the old occupant's words stay out
    rwkv_mi_serve_event ev[2];
    uint32_t toks[4];
    size_t ne = 0, nt = 0;
    b.deliver(ev, 2, toks, 4, &ne, &nt);
    CHECK(ne == 1 && ev[0].id == id && ev[0].n_new == 2 && ev[0].finished == 1 && toks[0] == 7 && toks[1] == 8, "the first request, whole");
    const uint32_t id3 = b.submit();   // (entry 0 again; the words still say `id`)
    CHECK(b.entry_of(id3) == b.entry_of(id), "the ring reuses the entry");
    (void) b.begin_block();
    b.consume(w.view(false));
    b.deliver(ev, 2, toks, 4, &ne, &nt);
    CHECK(ne == 0 && nt == 0, "words of the entry's earlier request were taken for the new one");
}

// The enqueue decision of a poll, over the polls of a caller that never drains: enqueue when busy and wants_block, then read every block
// but the newest -- all of them when nothing was enqueued. One request that ends in block 1: the caller comes to rest, with one dead block.
static void check_rest() {
    const size_t C = 2, stride = 4, K = 4;
    SessionBook b;
    b.init(C, 1, stride, K);
    Words w(C, stride);
    std::vector<Words> device;   // what block i leaves, written when it is "enqueued"
    const auto poll = [&]() {
        const bool enqueue = b.busy() && b.wants_block();
        if (enqueue) {
            const SessionBook::Block blk = b.begin_block();
            if (blk.index == 0) { w.admit(0, 0, 0, 1); w.emit(0, 5); w.next = 1; w.work = 1; }
            if (blk.index == 1) { w.emit(0, 6); w.retire(0, RWKV_MI_NO_TOKEN, 5); w.work = 0; }
            device.push_back(w);   // (later blocks: dead passes, the words stay)
        }
        for (const uint64_t upto = enqueue ? b.enqueued - 1 : b.enqueued; b.consumed < upto;) b.consume(device[b.consumed].view(false));
        return enqueue;
    };
    CHECK(!poll() && b.enqueued == 0, "a poll of a session with nothing submitted enqueues nothing");
    (void) b.submit();
    CHECK(b.wants_block(), "before any block has been read, a submit asks for one");
    CHECK(poll() && b.enqueued == 1 && b.consumed == 0, "poll 1: block 0 goes out, nothing to read");
    CHECK(poll() && b.enqueued == 2 && b.consumed == 1 && b.work == 1, "poll 2: block 1 goes out behind block 0, which left work");
    CHECK(poll() && b.enqueued == 3 && b.consumed == 2 && b.work == 0, "poll 3: block 0's work count still says work: block 2 goes out, block 1 is read");
    CHECK(b.busy() && !b.wants_block(), "block 1 left no work and the head at the number submitted: block 2 is dead, and is only read");
    CHECK(!poll() && b.enqueued == 3 && b.consumed == 3 && !b.busy(), "poll 4 enqueues nothing, reads block 2, and the session is at rest");
    CHECK(!poll() && !poll() && b.enqueued == 3 && b.passes == 3 * K, "further polls move nothing");
    // the work ended in block 1: one dead block behind it (two at the most, when the end falls on a block's last pass and is seen a poll later)
    CHECK(b.enqueued - 2 <= 2, "dead blocks");
    // a submit wakes it: the head (1) is below the number submitted (2)
    (void) b.submit();
    CHECK(b.busy() && b.wants_block() && poll() && b.enqueued == 4, "a submit after the rest");
}

int main() {
    check_rest();
    check_wrap();
    check_trickle();
    check_busy();
    if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
    printf("session book OK\n");
    return 0;
}
