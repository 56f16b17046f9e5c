// session_book.h -- the host's bookkeeping of a serve session (rwkv_mi_batch_serve_open ..; batch.cpp enqueues and copies, this decides):
// which id lives in which ring entry, what is in flight and how much room the ring has, how far each request has been read and delivered,
// which blocks are enqueued and which consumed, whether the session is busy, and the passes each lane's requests ran, for the parities at
// close. No HIP include and no device pointer: a host compiler exercises it (tests/cpp/session_book_check.cpp). What the session does is a
// function of the calls made on this book, never of timing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rwkv_mi355x.h"

namespace rwkvmi {

// The words one block brought back (SessionLayout from `down` on), wherever the caller keeps them. g_state / g_misses: NULL in a session
// without guides.
struct SessionWords {
    const uint32_t * next, * work, * ids, * done, * lens, * reasons, * lane, * start, * end, * revived, * g_state, * g_misses, * out;
};

struct SessionBook {
    struct Entry {
        uint32_t id = 0;
        bool live = false;        // submitted, its end not delivered
        bool admitted = false;    // a consumed block showed the entry admitted for this id
        bool done = false;        // ... and retired
        uint32_t seen = 0, delivered = 0;   // tokens read from consumed blocks; tokens handed to the caller
        uint32_t reason = RWKV_MI_NO_TOKEN, lane = RWKV_MI_NO_TOKEN, start = 0, end = 0, revived = 0, g_state = 0, g_misses = 0;
    };
    // what the next block carries
    struct Block { uint64_t index; uint32_t first_pass, tail, upload_from, upload_to; };

    size_t capacity = 0, n_lanes = 0, stride = 0, K = 0;
    std::vector<Entry> entries;            // [capacity]
    std::vector<uint32_t> tokens;          // [capacity][stride]: what has been read and not yet delivered lies here, not in the staging
    std::vector<uint32_t> cancel;          // [capacity]: 1: the entry's request is to retire
    uint32_t submitted = 0, uploaded = 0;  // ids issued; ids whose entries a block has carried up
    uint32_t oldest = 0;                   // the lowest id whose end has not been delivered (== submitted: none)
    uint32_t in_flight = 0;
    uint64_t enqueued = 0, consumed = 0;   // blocks
    uint64_t passes = 0;
    uint32_t head = 0, work = 0;           // of the last consumed block
    std::vector<uint64_t> lane_passes;     // the passes the lane's delivered requests ran
    std::vector<uint32_t> lane_revivals, lane_last;   // how many of them found the lane idle; the last id the lane was given

    void init(size_t capacity_, size_t n_lanes_, size_t stride_, size_t K_) {
        capacity = capacity_; n_lanes = n_lanes_; stride = stride_; K = K_;
        entries.assign(capacity, Entry()); tokens.assign(capacity * stride, RWKV_MI_NO_TOKEN); cancel.assign(capacity, 0u);
        lane_passes.assign(n_lanes, 0); lane_revivals.assign(n_lanes, 0u); lane_last.assign(n_lanes, RWKV_MI_NO_TOKEN);
    }
    size_t entry_of(uint32_t id) const { return (size_t) id % capacity; }
    // submits the ring takes now: entry q % capacity is free once request q - capacity has been delivered
    uint32_t room() const { return (uint32_t) capacity - (submitted - oldest); }
    bool busy() const { return enqueued > consumed || work > 0u || head < submitted; }
    // Whether a busy session's poll enqueues a block: there is work on a lane or in the queue as far as the last consumed block says
    // (before any has been consumed: as soon as something is submitted). When that block left no work and its head is the number
    // submitted, a block that is still unconsumed was enqueued with a tail the head had already reached: it ran dead passes, nothing in
    // it can start work, and the poll reads it instead of putting another one behind it. This is what lets a caller that never drains
    // come to rest, and what bounds the dead passes behind the end of the work by two blocks.
    bool wants_block() const { return work > 0u || head < submitted; }

    // the id of a new request (room() > 0): its entry is the caller's to fill before the next block
    uint32_t submit() {
        const uint32_t id = submitted++;
        Entry & e = entries[entry_of(id)];
        e = Entry(); e.id = id; e.live = true;
        cancel[entry_of(id)] = 0u;
        in_flight++;
        return id;
    }
    bool is_live(uint32_t id) const { return id < submitted && entries[entry_of(id)].live && entries[entry_of(id)].id == id; }
    bool cancel_request(uint32_t id) {
        if (!is_live(id)) return false;
        cancel[entry_of(id)] = 1u;
        return true;
    }

    // the next block: its passes, the tail its launches carry, the ids whose entries go up with it
    Block begin_block() {
        const Block b{enqueued, (uint32_t) passes, submitted, uploaded, submitted};
        uploaded = submitted; passes += K; enqueued++;
        return b;
    }
    // the words of the oldest unconsumed block: the head and the work count, and for every live entry the device has admitted for its
    // id, what is new
    void consume(const SessionWords & w) {
        consumed++;
        head = *w.next; work = *w.work;
        for (size_t i = 0; i < capacity; i++) {
            Entry & e = entries[i];
            if (!e.live || e.done || w.ids[i] != e.id) continue;
            e.admitted = true; e.lane = w.lane[i]; e.start = w.start[i];
            const uint32_t len = w.lens[i] < stride ? w.lens[i] : (uint32_t) stride;
            for (uint32_t j = e.seen; j < len; j++) tokens[i * stride + j] = w.out[i * stride + j];
            if (len > e.seen) e.seen = len;
            if (w.done[i]) {
                e.done = true; e.reason = w.reasons[i]; e.end = w.end[i]; e.revived = w.revived[i];
                if (w.g_state) { e.g_state = w.g_state[i]; e.g_misses = w.g_misses[i]; }
            }
        }
    }
    // Events for what has been read and not delivered, oldest request first: one per request with new tokens or a newly known end. A
    // request's `finished` event frees its entry and adds its passes to its lane's.
    void deliver(rwkv_mi_serve_event * events, size_t max_events, uint32_t * tokens_out, size_t max_tokens, size_t * n_events, size_t * n_tokens) {
        size_t ne = 0, nt = 0;
        for (uint32_t id = oldest; id != submitted; id++) {
            const size_t i = entry_of(id);
            Entry & e = entries[i];
            if (!e.live || e.id != id) continue;   // (delivered out of order, before an older one)
            const uint32_t avail = e.seen - e.delivered;
            if (avail == 0u && !e.done) continue;
            if (ne == max_events) break;
            const uint32_t take = (uint32_t) (avail < max_tokens - nt ? avail : max_tokens - nt);
            if (take == 0u && avail > 0u) break;
            const bool fin = e.done && take == avail;
            events[ne++] = rwkv_mi_serve_event{id, e.delivered, take, fin ? 1u : 0u, fin ? e.reason : RWKV_MI_NO_TOKEN, e.lane, e.start,
                                               fin ? e.g_state : 0u, fin ? e.g_misses : 0u};
            for (uint32_t j = 0; j < take; j++) tokens_out[nt++] = tokens[i * stride + e.delivered + j];
            e.delivered += take;
            if (fin) finish(e);
        }
        while (oldest != submitted && !(entries[entry_of(oldest)].live && entries[entry_of(oldest)].id == oldest)) oldest++;
        *n_events = ne; *n_tokens = nt;
    }
    // A lane's buffers change places with every pass one of its requests runs, except that the first pass after an idle stretch writes
    // the buffer the last pass before it wrote: 1 when the lane slot's state lies in the other buffer than at open.
    int parity_flip(size_t lane) const { return (int) ((lane_passes[lane] - lane_revivals[lane]) & 1u); }

private:
    void finish(Entry & e) {
        e.live = false; in_flight--;
        if (e.lane < n_lanes) {
            lane_passes[e.lane] += (uint32_t) (e.end - e.start + 1u);
            lane_revivals[e.lane] += e.revived;
            if (lane_last[e.lane] == RWKV_MI_NO_TOKEN || (int32_t) (e.id - lane_last[e.lane]) > 0) lane_last[e.lane] = e.id;
        }
    }
};

}  // namespace rwkvmi
