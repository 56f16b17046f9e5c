// model.h -- weights resident in HBM + the per-context execution state of librwkv.so.
#pragma once
#include <string>

#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>

#include "common.h"
#include "devmem.h"
#include "kernels.h"
#include "rows.h"
#include "persist_host.h"
#include "rwkv_mi355x.h"

struct rwkv_context;

namespace rwkvmi {

// Parameter slots of one layer; names follow the reference's key table (rwkv_model_loading.inc:132-282).
struct LayerW {
    const DevTensor *ln1_w = nullptr, *ln1_b = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
    // v4 / v5
    const DevTensor *att_time_mix_k = nullptr, *att_time_mix_v = nullptr, *att_time_mix_r = nullptr, *att_time_mix_g = nullptr;
    const DevTensor *att_time_first = nullptr, *att_time_decay = nullptr, *att_time_faaaa = nullptr;
    const DevTensor *att_key = nullptr, *att_value = nullptr, *att_receptance = nullptr, *att_output = nullptr, *att_gate = nullptr;
    const DevTensor *att_ln_x_w = nullptr, *att_ln_x_b = nullptr;
    // v6
    const DevTensor *att_time_maa_x = nullptr, *att_time_maa_w = nullptr, *att_time_maa_k = nullptr, *att_time_maa_v = nullptr,
                    *att_time_maa_r = nullptr, *att_time_maa_g = nullptr, *att_time_maa_w1 = nullptr, *att_time_maa_w2 = nullptr,
                    *att_time_decay_w1 = nullptr, *att_time_decay_w2 = nullptr;
    // v7
    const DevTensor *att_x_rwkvag = nullptr, *att_w0 = nullptr, *att_w1 = nullptr, *att_w2 = nullptr, *att_a0 = nullptr, *att_a1 = nullptr,
                    *att_a2 = nullptr, *att_g1 = nullptr, *att_g2 = nullptr, *att_v0 = nullptr, *att_v1 = nullptr, *att_v2 = nullptr,
                    *att_r_k = nullptr, *att_k_k = nullptr, *att_k_a = nullptr;
    // channel mixing
    const DevTensor *ffn_time_mix_k = nullptr, *ffn_time_mix_r = nullptr, *ffn_time_maa_k = nullptr, *ffn_time_maa_r = nullptr, *ffn_x_k = nullptr;
    const DevTensor *ffn_key = nullptr, *ffn_value = nullptr, *ffn_receptance = nullptr;
};

struct Model {
    FileHeader header{};
    int arch_major = 4, arch_minor = 0;
    int64_t head_count = 0, head_size = 0, ffn_size = 0;
    int64_t max_lowrank = 0;  // widest intermediate of a low-rank pair (v6 5*r, decay rank; v7 ranks)
    // Single-token path the first context of this model measured as fastest on its device (engine.hip, calibrate_decode_path): a
    // persistent kernel (RWKV-6: Regs or Ring; RWKV-4 / RWKV-7: K47) or the fused per-layer launches. Clones reuse it instead of
    // timing every path again.
    mutable std::atomic<DecodePath> decode_choice{DecodePath::Unmeasured};

    // Device images a decode path derives from the weights alone (ring_v6.hip: the per-workgroup weight streams, the blocked W2, the
    // layer table): built by the first context that needs them, shared by every context of the model, freed with the last holder.
    mutable std::mutex derived_mu;
    mutable void * ring_shared = nullptr;

    std::vector<std::unique_ptr<DevTensor>> tensors;
    std::unordered_map<std::string, DevTensor *> by_name;

    const DevTensor *emb = nullptr, *ln0_w = nullptr, *ln0_b = nullptr, *ln_out_w = nullptr, *ln_out_b = nullptr, *head = nullptr;
    std::vector<LayerW> layers;  // indexed by absolute layer id; only [layer_begin, layer_end) are populated

    // pipeline stage owned by this process (whole model by default)
    uint32_t layer_begin = 0, layer_end = 0;
    bool has_embed = true, has_head = true;

    void * arena = nullptr;       // one HBM allocation holding every parameter plane
    size_t arena_bytes = 0;
    int device = 0;
    uint64_t bytes_per_token = 0; // algorithmic bytes of one decoded token on this stage
    uint64_t weight_bytes = 0;
    double load_seconds = 0.0;    // file payload -> HBM (pass 2 of load_model: reads, copies, re-pack kernels)

    std::atomic<int> refcount{0};

    int64_t n_embed() const { return header.n_embed; }
    int64_t n_vocab() const { return header.n_vocab; }
    int64_t n_layer() const { return header.n_layer; }
    int64_t state_per_layer() const { return arch_major >= 5 ? n_embed() * (2 + head_size) : n_embed() * 5; }
    int64_t state_len() const { return state_per_layer() * n_layer(); }
};

// ---- sequence mode on the matrix cores (prefill.hip) ----
struct TileAct {   // quantised activations of T tokens in the tile-major image (see prefill.hip)
    int8_t * q = nullptr; float * d = nullptr; float * s = nullptr; float * o = nullptr;
    int64_t T_pad = 0;
};
size_t  tile_act_bytes(int64_t T, int64_t K);
TileAct tile_act_at(void * base, int64_t T, int64_t K);
void launch_quantize_act_tiles(const float * x, int64_t T, int64_t K, int wtype, const TileAct & out, hipStream_t st);
// up to 5 inputs of the same shape in one launch
void launch_quantize_act_tiles_batched(int n, const float * const * xs, int64_t T, int64_t K, int wtype, const TileAct * outs, hipStream_t st);
// sequence-mode mixes writing their outputs as tile images (prefill.hip); `outs` = one image per output
bool launch_v6_mix2_seq(const V6Mix2Args & a, int64_t T, int64_t D, int64_t R, hipStream_t st, const TileAct * outs = nullptr, int wtype = 0);
bool launch_mix_seq_q(const MixArgs & a, int64_t T, int64_t D, hipStream_t st, const TileAct * outs, int wtype);
bool launch_groupnorm_seq_q(const float * x, const float * lw, const float * lb, float eps, const float * gate, int64_t T, int64_t H, int64_t S,
                            const TileAct & out, int wtype, hipStream_t st);
// workspace of the split walk (GEMMs with too few output tiles for the chip): partial sums + one zeroed counter per tile
struct MmqWs { float * part = nullptr; size_t part_bytes = 0; int * counters = nullptr; int n_counters = 0; };
bool launch_mmq_mfma(const DevTensor & W, const TileAct & x, int64_t T, float * y, int64_t ldy, const Epi & epi, hipStream_t st, const MmqWs * ws = nullptr);
bool launch_mmq_mfma_q(const DevTensor & W, const TileAct & x, int64_t T, const Epi & epi, const TileAct & out, int out_wtype, hipStream_t st);   // output only as the next product's quantised image
// up to 4 products of the same shape and type in one launch (y_i = epi_i(W_i . x_i))
bool launch_mmq_mfma_batched(int n, const DevTensor * const * Ws, const TileAct * xs, float * const * ys, const Epi * epis, int64_t T, int64_t ldy,
                             const MmqWs * ws, hipStream_t st);
bool ensure_pf(const DevTensor & W, hipStream_t st);
void prefill_prepare_current_device();   // per-device kernel attributes of the sequence-mode kernels (multi-device processes)
void free_pf(const DevTensor & W);
bool launch_wkv6_seq(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                     const float * state_in, float * state_out, float * out, int64_t T, int64_t H, hipStream_t st);
constexpr int64_t k_mfma_min_tokens = 32;   // sequence calls of at least this many tokens per pass take the GEMM path

// ---- the device sampler (sampling.hip): temperature / top-k / top-p / min-p draws on logits in HBM ----
// (rows.h, DrawRow: everything the draw of one row can read)
constexpr uint16_t GUIDE_DEAD = 0xFFFF;   // a dead transition of a guide's table
// the two settings as a sequence keeps them (DrawState's host words)
struct CutRow { uint32_t top_k; float min_p; };
struct RepRow { float decay; float repetition; };
// What the kernel of a call is specialised on, decided ONCE per call from the sequences it names (DrawState::form): which choice is made --
// the greedy argmax (none: no draw kernel runs), the sampler or the penalised sampler -- and which of the row's optional fields its kernel
// reads. A call that uses none of a feature launches the kernel of before that feature:
//   guided   a named sequence has a guide;   rep   the call is penalised and a named sequence has a repetition setting;
//   cut      a named sequence has a truncation setting -- or guided, or rep: those kernels exist in the truncating form only.
enum class Draw { none, sample, penalized };
enum : int { SRC_PLAIN = 0, SRC_PEN = 1, SRC_REP = 2 };   // what a draw kernel reads (sampling.hip): logits, penalised, penalised with repetition
struct DrawForm {
    Draw draw = Draw::none; bool cut = false, guided = false, rep = false;
    static DrawForm of(Draw draw, bool has_cut, bool has_guide, bool has_rep) {
        DrawForm f;
        f.draw = draw; f.guided = draw != Draw::none && has_guide; f.rep = draw == Draw::penalized && has_rep; f.cut = draw != Draw::none && (has_cut || f.guided || f.rep);
        return f;
    }
    // the form of a context's draw of `row`: its truncating kernel runs whenever a word of the setting is set (top_k >= n too, which truncates nothing)
    static DrawForm of_row(Draw draw, const DrawRow & row) {
        return of(draw, row.top_k != 0u || row.min_p != 0.0f, false, row.decay != 1.0f || row.repetition != 1.0f);
    }
};
// probs: scratch of sample_scratch_floats(n) floats (the vocabulary rounded up to whole chunks of the 1024 threads: the kernel keeps it transposed).
inline size_t sample_scratch_floats(int64_t n) { return (size_t) ((n + 1023) / 1024) * 1024; }
// One draw of a context: one workgroup on logits[n] with `row`. The token is written to out_token (and to hist[hist_pos] when hist is given).
void launch_draw(const float * logits, int n, const DrawRow & row, const DrawForm & form, float * probs, uint32_t * out_token, uint32_t * hist, int hist_pos,
                 hipStream_t st);
// The row form (batched decode): one workgroup per row of logits[rows][n], row r with table[r]. probs: [rows][sample_scratch_floats(n)] scratch.
// Row r's token goes to tokens[r] (the word its next embedding lookup reads) and, when hist is given, to hist[r].
// live (NULL: every row draws): rwkv_mi_batch_decode_until's per-row live words -- a row with live[r] == 0 returns before it reads anything: no
// draw, no counter advance, no count, no guide step, no token or history word.
void launch_draw_rows(const float * logits, int64_t rows, int n, const DrawRow * table, const DrawForm & form, float * probs, uint32_t * tokens, uint32_t * hist,
                      const uint32_t * live, hipStream_t st);
void launch_sample_seek_rows(const DrawRow * table, int64_t rows, unsigned long long value, hipStream_t st);   // *table[r].counter = value
// next[n_states][n_vocab] from the edges in CSR form on the device (checked by the caller: tokens < n_vocab and distinct per state, next < n_states)
void launch_guide_expand(uint16_t * next, uint32_t n_states, int n_vocab, const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next,
                         hipStream_t st);
// draw_state.cpp: the rules of rwkv_mi_batch_guide_create on a guide's edges (nullptr: they hold; else which one does not), and the table built on
// the device from edges that passed: allocated, expanded, the stream drained. A failure leaves `table` as it was
const char * guide_edges_fault(size_t n_vocab, uint32_t n_states, const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next);
hipError_t guide_table_build(DevBuf<uint16_t> & table, size_t n_vocab, uint32_t n_states, const uint32_t * edge_begin, const uint32_t * edge_tokens,
                             const uint32_t * edge_next, hipStream_t st, bool * alloc_failed);
// The device words of a call (rows.h, StopRow: a row's parameters): per row its live word (1 until it retires), its length and its reason (the index of the matching sequence, or
// RWKV_MI_NO_TOKEN for the budget) once it has; live_count: the rows still live.
struct StopTables { const StopRow * rows; const uint32_t * seq_lens, * seq_tokens; uint32_t * live, * lens, * reasons, * live_count; };
// After the draw of pass `step` (hist: [step][rows], this call's tokens): retires the live rows whose tokens end with one of their sequences or
// whose budget is step + 1. A retired row gets {in = what pass `step` wrote, out = its other buffer} in both row tables (used: the table of
// pass `step`, other: the one of pass step + 1).
void launch_stop_rows(const StopTables & t, int64_t rows, const uint32_t * hist, uint32_t step, RowState * used, RowState * other, hipStream_t st);
// rwkv_mi_batch_serve (sampling.hip, k_serve_rows / k_serve_reset): a queue of requests behind the n lanes of a call (rows.h, ServeReq: a
// request as the device reads it). The device words of a call. Per request: its emitted tokens out[q][stride], its length (it grows with every token), its reason, its lane and
// the pass that fed its first prompt token. Per lane: the request it serves (SERVE_FREE: it waits for one -- only between the two halves of
// k_serve_rows, and before the first pass; RWKV_MI_NO_TOKEN: dead), the prompt tokens it has been fed, its DRAW WORD (1: the logits of the
// coming pass are drawn from -- the `live` argument of the draw kernels), its admit word (1: k_serve_reset has a state to copy), the last
// request it was given, and its slot. rows: the draw table of the lanes (NULL: the greedy family); counters / counts: the batch's, indexed by
// slot (counts NULL: the batch has no occurrence tables). next_request: the head of the queue, written by k_serve_rows alone; work: the lanes
// that are not dead, which the host polls. A call with guided requests (rwkv_mi_batch_serve_ex; NULL otherwise, all four): guide_state /
// guide_misses, one pair of guide words per LANE -- the call's own, not the lane slots' -- which a guided request's draw row points at from
// its admission on, and req_guide_state / req_guide_misses per REQUEST: the host leaves the request's start state and 0 there, the scheduler
// the lane's two words when the request retires. A request is guided when its row has a table (row.next).
constexpr uint32_t SERVE_FREE = 0xFFFFFFFEu;
struct ServeTables {
    const ServeReq * reqs; const uint32_t * prompts, * seq_lens, * seq_tokens;
    uint32_t * out; uint32_t stride;
    uint32_t * lens, * reasons, * lane, * start_pass;
    uint32_t * req, * pos, * draw, * admit, * last; const uint32_t * lane_slot;
    DrawRow * rows; unsigned long long * counters; uint32_t * counts;
    uint32_t * next_request, * work;
    uint32_t n_requests, n_vocab;
    uint32_t * guide_state, * guide_misses, * req_guide_state, * req_guide_misses;
};
// After the draw of pass `step` over the n lanes (tokens: the lanes' token words; used: the row table of that pass, other: the one of pass
// step + 1): every lane emits, advances its prompt, retires, admits or goes dead. step == UINT32_MAX with used = the table of pass 1: the
// admission in front of pass 0.
void launch_serve_rows(const ServeTables & t, int64_t n, uint32_t * tokens, uint32_t step, RowState * used, RowState * other, hipStream_t st);
// Behind it: lanes x chunks workgroups; those of an admitted lane copy the request's start state into used[lane].out -- the buffer the lane's
// next pass reads -- and zero its occurrence row
void launch_serve_reset(const ServeTables & t, int64_t n, unsigned chunks, const RowState * used, int64_t state_len, hipStream_t st);
// A serve session (rwkv_mi_batch_serve_open ..; sampling.hip, k_session_rows): the same tables with the queue a RING of `capacity` entries
// (call_layout.h, SessionLayout). Request id q lives in entry q % capacity; t.req[r] holds the lane's ENTRY (SESSION_IDLE: the lane has no
// request and waits for one), t.last[r] the ID of the last request it was given; the per-request words of t are indexed by entry, and
// t.prompts == t.seq_lens == t.seq_tokens is the ring as words (a ServeReq's prompt0 / seq0 / tok0 are word offsets into it). tail: the ids
// below it have been uploaded -- a kernel argument, so a request is visible from the block whose launches carry it. cancel[entry]: the
// request is to retire (the half of the cancel words this block's upload wrote). Per entry, beside t's: the id the entry was admitted for
// (the host trusts an entry's words when it is the id it submitted there), done (1 from its retirement on), the pass after which it
// retired, and revived (1: its lane was idle when it took it). entry_words / guide_word: the words of a ring entry and where a guided
// request's start state lies in it. admit_only: the launch stands in front of a block's first pass and only hands requests to idle lanes.
constexpr uint32_t SESSION_IDLE = 0xFFFFFFFFu;
struct SessionTables {
    ServeTables t;
    uint32_t capacity, tail;
    const uint32_t * cancel;
    uint32_t * ids, * done, * end_pass, * revived;
    uint32_t entry_words, guide_word;
    uint32_t admit_only;
};
// As launch_serve_rows; launch_serve_reset follows it unchanged (t.reqs[t.req[r]] is the ring entry).
void launch_session_rows(const SessionTables & s, int64_t n, uint32_t * tokens, uint32_t step, RowState * used, RowState * other, hipStream_t st);
// rwkv_mi_batch_decode_beam (score.hip): the device words of a call of G groups of `width` hypotheses, row g * width + j = hypothesis j of group g.
// Per row its cumulative score (double), its finished word, its length; the candidates of the step -- cand_ids / cand_lp [rows][width], the
// report's top-`width` of the row's logits -- and the word the shared body writes its unused `chosen` to; the history [steps][rows] of emitted
// token (RWKV_MI_NO_TOKEN: none), parent (the index within the group) and the token's f32 log-prob; live_count (may be NULL): the unfinished
// hypotheses of all groups; the ids that finish a hypothesis, by value.
struct BeamTables {
    double * score; uint32_t * finished, * len;
    uint32_t * cand_ids; float * cand_lp; float * chosen;
    uint32_t * hist_tok, * hist_parent; float * hist_lp;
    uint32_t * live_count;
    uint32_t width, n_end;
    uint32_t end_tokens[8];
};
// The two kernels of a step, after the head of a pass over `rows` = groups * width rows: the candidates of every row that is unfinished and has a
// finite score, then per group the selection, which rewrites the rows' words in place, appends row `step` of the history, puts each row's next
// token into tokens[row] and re-parents the next pass: other[row].in = used[row of its parent].out (used: the row table of this pass, other:
// the one of the next; both NULL: no table is touched).
void launch_beam_rows(const float * logits, int64_t rows, int n, const BeamTables & t, hipStream_t st);
void launch_beam_select(const BeamTables & t, int64_t groups, uint32_t * tokens, uint32_t step, const RowState * used, RowState * other, hipStream_t st);
void launch_count_add(uint32_t * count, const uint32_t * tokens, int64_t n, int n_vocab, hipStream_t st);                        // count[tokens[i]] += 1
// the same on a decaying sequence's row: per token of the list, in its order, every entry * decay, then the token's entry + 1.0f
void launch_count_add_decay(float * occ, const uint32_t * tokens, int64_t n, int n_vocab, float decay, hipStream_t st);
void launch_bias_scatter(float * bias, const uint32_t * ids, const float * values, int64_t n, int n_vocab, hipStream_t st);     // bias[ids[i]] = values[i]

// The draw state of `slots` sequences of a model, owned in one place (draw_state.cpp): per slot the draw counter, the sampler's scratch vector, the
// occurrence table and the bias table of the penalised draw, and whether a bias is set. A context holds one of 1 slot, a batch one of n_slots.
// Nothing is allocated by init(): the counters come with ensure_counters (a batch calls it when it is created, so its counters exist and are
// zero from then on; a context gets its counter with its first draw or seek), the scratch with ensure_sampler, the two tables -- zeroed; a
// table that could not be zeroed is not kept -- with the first call of the penalised family, the guide words with the first attach. Every growth is one grow(want(...)) decision: a
// call that fails leaves every buffer as it was. No stream is kept (rwkv_mi_set_stream can change a context's): each operation takes the
// stream it works on and the context its errors are reported on -- RWKV_ERROR_ALLOC for memory, RWKV_ERROR_GRAPH for any other HIP error.
// The operations on a slot's tables drain the stream before they return.
struct DrawState {
    size_t slots = 0, n_vocab = 0;
    DevBuf<unsigned long long> counters;   // [slots]
    DevBuf<float>    probs;                // [slots][sample_scratch_floats(n_vocab)]
    DevBuf<uint32_t> counts;               // [slots][n_vocab]
    DevBuf<float>    bias;                 // [slots][n_vocab]
    std::vector<uint8_t> has_bias;         // [slots]: a bias has been set and not cleared
    // the guide words (rwkv_mi_batch_guide_*): the guide attached to each slot (the host's: RWKV_MI_NO_GUIDE for none) and, on the device, the
    // slot's current state and miss counter -- zeroed, allocated by the first attach
    std::vector<uint32_t> guide_of;        // [slots]
    DevBuf<uint32_t> guide_state;          // [slots]
    DevBuf<uint32_t> guide_misses;         // [slots]
    // the truncation settings (rwkv_mi_*truncation_set): host words only, {0, 0} -- none -- from init() on; every draw of the slot reads them
    std::vector<CutRow> cuts;              // [slots]
    // the repetition settings (rwkv_mi_*repetition_set): host words only, {1, 1} -- none -- from init() on; every PENALISED draw of the slot reads
    // them. A slot with decay != 1 is decaying: the words of its row of `counts` are floats (the row is zeroed when a set changes that)
    std::vector<RepRow> reps;              // [slots]

    void init(size_t n_slots, size_t vocab) {
        slots = n_slots; n_vocab = vocab; has_bias.assign(n_slots, 0); guide_of.assign(n_slots, RWKV_MI_NO_GUIDE); cuts.assign(n_slots, CutRow{0u, 0.0f});
        reps.assign(n_slots, RepRow{1.0f, 1.0f});
    }
    unsigned long long * counter(size_t slot) const { return counters.p + slot; }
    uint32_t * counts_of(size_t slot) const { return counts.p + slot * n_vocab; }
    const float * bias_of(size_t slot) const { return has_bias[slot] ? bias.p + slot * n_vocab : nullptr; }   // NULL: none is set
    // whether the slot's setting truncates anything (top_k == 0 or >= n_vocab: no top-k; min_p == 0: no min-p)
    bool has_cut(size_t slot) const { return (cuts[slot].top_k != 0u && cuts[slot].top_k < n_vocab) || cuts[slot].min_p != 0.0f; }
    bool decaying(size_t slot) const { return reps[slot].decay != 1.0f; }
    bool has_rep(size_t slot) const { return decaying(slot) || reps[slot].repetition != 1.0f; }
    // The row of a draw of `slot` -- the one place that knows where a sequence's counter, tables, guide words and settings live. pen (NULL: the
    // plain draw, which reads neither table) with `record` in place of its own; guides (NULL: a context, which has none): the batch's tables,
    // indexed by guide_of
    DrawRow row(size_t slot, const rwkv_mi_sample_params & p, const rwkv_mi_penalty_params * pen, uint32_t record, const DevBuf<uint16_t> * guides = nullptr) const {
        const uint32_t g = guide_of[slot];
        const bool guided = guides && g != RWKV_MI_NO_GUIDE;
        return DrawRow{p, counter(slot), pen ? pen->presence : 0.0f, pen ? pen->frequency : 0.0f, pen ? record : 0u, pen ? counts_of(slot) : nullptr,
                       pen ? bias_of(slot) : nullptr, guided ? guides[g].p : nullptr, guided ? guide_state.p + slot : nullptr,
                       guided ? guide_misses.p + slot : nullptr, cuts[slot].top_k, cuts[slot].min_p, reps[slot].decay, reps[slot].repetition};
    }
    // the form of a call that draws for the n named slots
    DrawForm form(Draw draw, const uint32_t * named, size_t n) const {
        bool cut = false, guided = false, rep = false;
        for (size_t i = 0; i < n; i++) { cut |= has_cut(named[i]); guided |= guide_of[named[i]] != RWKV_MI_NO_GUIDE; rep |= has_rep(named[i]); }
        return DrawForm::of(draw, cut, guided, rep);
    }

    bool ensure_counters(rwkv_context * ctx, hipStream_t st);
    bool ensure_sampler(rwkv_context * ctx, hipStream_t st);   // the counters and the scratch
    bool ensure_penalty(rwkv_context * ctx, hipStream_t st);   // the two tables
    bool seek(rwkv_context * ctx, size_t slot, unsigned long long value, hipStream_t st);
    bool counts_reset(rwkv_context * ctx, size_t slot, hipStream_t st);
    bool counts_add(rwkv_context * ctx, size_t slot, const uint32_t * tokens, size_t n, hipStream_t st);   // (arguments checked: check_count_tokens)
    bool counts_store(rwkv_context * ctx, size_t slot, uint32_t * counts_out, hipStream_t st);   // RWKV_ERROR_ARGS on a decaying slot
    bool bias_set(rwkv_context * ctx, size_t slot, const uint32_t * ids, const float * values, size_t n, hipStream_t st);   // n == 0: cleared (check_bias)
    bool ensure_guides(rwkv_context * ctx, hipStream_t st);    // the two guide words per slot
    // attaches `guide` in `state` (checked by the caller) or, with RWKV_MI_NO_GUIDE, detaches; the slot's miss counter starts from 0 either way
    bool guide_attach(rwkv_context * ctx, size_t slot, uint32_t guide, uint32_t state, hipStream_t st);
    bool guide_words(rwkv_context * ctx, size_t slot, uint32_t * state_out, uint32_t * misses_out, hipStream_t st);   // (0, 0 without a guide)
    bool cut_set(rwkv_context * ctx, size_t slot, uint32_t top_k, float min_p);   // min_p in [0, 1], or RWKV_ERROR_ARGS and nothing changed
    // decay in [0, 1], repetition finite and > 0, or RWKV_ERROR_ARGS and nothing changed; a set that changes whether the slot is decaying zeroes its row
    bool rep_set(rwkv_context * ctx, size_t slot, float decay, float repetition, hipStream_t st);
    bool counts_store_f32(rwkv_context * ctx, size_t slot, float * out, hipStream_t st);   // either kind of row, as floats
};
// the arguments of counts_add / logit_bias_set / a penalty (checked before anything changes; errors are reported on ctx)
bool check_count_tokens(rwkv_context * ctx, const uint32_t * tokens, size_t n);
bool check_bias(rwkv_context * ctx, const uint32_t * ids, const float * values, size_t n);
bool check_penalty(rwkv_context * ctx, float presence, float frequency, size_t index);

// Loads [layer_begin, layer_end) of the file (layer_end == UINT32_MAX: all layers) onto the current HIP device.
// Returns nullptr with the thread-local error set, like the reference loader (rwkv_model_loading.inc:288-419).
Model * load_model(const char * path, uint32_t layer_begin, uint32_t layer_end);
void    release_model(Model * m);
bool    scan_stage_costs(const char * path, std::vector<uint64_t> & per_layer, uint64_t & head_bytes);

}  // namespace rwkvmi

// ---------------------------------------------------------------------------------------------------------------
// The context (opaque to callers).
// ---------------------------------------------------------------------------------------------------------------

namespace rwkvmi {
enum class FusedLayer { none, v4, v6, v7 };   // which fused per-layer decode path a context runs (at most one exists for a model)

// The report of a context's or a batch's emitting calls (rwkv_mi_*set_logprobs): whether it is on and with how many alternatives; the device
// buffers, laid out like the loops' history -- chosen[steps][rows], ids / vals [steps][rows][top_n] -- allocated by the first reporting call
// and grown to the largest since; and what the last reporting call left in them (valid: there is one). lens[r]: the steps row r wrote.
// `valid` implies `enabled`: set() alone changes `enabled` and clears `valid`; done() alone sets `valid`, for an enabled report. The
// operations (logprob_report.cpp) take the context their errors go to, and the stream where they use one.
struct RowReport { float * chosen; uint32_t * ids; float * vals; uint32_t top_n; };   // the buffers as a pass writes them (RowSampler, below)
struct LogprobReport {
    bool enabled = false;
    uint32_t top_n = 0;
    DevBuf<float> d_chosen;        // .count: the entries the buffers were sized for ...
    DevBuf<uint32_t> d_ids;        // ... and entries * top_n of d_ids and d_vals
    DevBuf<float> d_vals;
    bool valid = false;
    size_t rows = 0, steps = 0;
    uint32_t last_top_n = 0;
    std::vector<uint32_t> lens;

    RowReport buffers() const { return RowReport{d_chosen.p, d_ids.p, d_vals.p, top_n}; }   // (begin has sized them for the call)
    bool set(rwkv_context * ctx, bool enabled, uint32_t top_n);
    bool ensure(rwkv_context * ctx, size_t entries);
    // what every emitting call of `entries` = steps * rows records starts with (nothing when the report is off): the stream drained, the
    // buffers sized, the previous report ended
    bool begin(rwkv_context * ctx, hipStream_t st, size_t entries);
    void done(size_t rows, size_t steps, const uint32_t * lens);
    bool shape(rwkv_context * ctx, size_t * rows, size_t * steps, uint32_t * top_n) const;
    bool store(rwkv_context * ctx, hipStream_t st, size_t stride, float * chosen_out, uint32_t * top_ids_out, float * top_logprobs_out) const;
};
}  // namespace rwkvmi

struct rwkv_context {
    rwkvmi::Model * model = nullptr;
    uint32_t n_threads = 0;
    int  last_error = 0;
    bool print_errors = false;  // a fresh reference context starts silent (rwkv.cpp:74 value-initialises it)

    hipStream_t stream = nullptr;
    bool owns_stream = true;   // false after rwkv_mi_set_stream (the caller's stream, e.g. torch's current stream)

    // Device-resident recurrent state, ping-pong (kernels read [cur], write [cur ^ 1]).
    rwkvmi::DevBuf<float> state[2];
    int cur = 0;

    // Scratch for T tokens (grown on demand).
    int64_t scratch_T = 0;
    rwkvmi::DevBuf<uint8_t> scratch;   // (.count: its bytes)
    struct Buf {
        float *x, *xn, *sx, *m[6], *r, *k, *v, *g, *w, *a, *t0, *t1, *t2, *out, *ffk, *lr1, *lr2, *v_first, *xlast;
        rwkvmi::QAct qa;
        void * tile = nullptr;   // tile-major quantised activations (T >= k_mfma_min_tokens)
        void * tiles[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the same for inputs quantised ahead, several per launch (row length D)
        rwkvmi::MmqWs ws;         // workspace of the split walk (prefill.hip)
    } b{};

    rwkvmi::DevBuf<uint32_t> d_tokens;            // the token words of a pass and their pinned staging, grown together (.count: the capacity)
    rwkvmi::PinBuf<uint32_t> h_tokens;
    rwkvmi::DevBuf<float>    d_logits;
    rwkvmi::DevBuf<uint32_t> d_next_token;
    rwkvmi::DrawState draw;                       // the context's draw state, 1 slot: counter, sampler scratch, occurrence and bias table
    // scoring (rwkv_mi_score_resident / rwkv_mi_batch_score_ragged; engine.hip ensure_score), allocated by the first scoring call: the chunk
    // of the all-position head, [score_R][n_vocab] logits, and the per-row words of a pass for score_cap rows -- targets in (with their
    // pinned staging), log-probs and argmax out
    rwkvmi::DevBuf<float>    d_score;
    int64_t    score_R = 0;
    rwkvmi::DevBuf<uint32_t> d_score_targets;
    rwkvmi::PinBuf<uint32_t> h_score_targets;
    rwkvmi::DevBuf<float>    d_score_logprobs;
    rwkvmi::DevBuf<uint32_t> d_score_argmax;
    int64_t    score_cap = 0;
    rwkvmi::LogprobReport lp;                     // the report of the context's draws (rwkv_mi_set_logprobs)

    // captured single-token graphs: [cur][with_logits]
    hipGraphExec_t graph_exec[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    bool use_graph = true;

    // Layer pipeline inside ONE process (RWKV_MI_DEVICES, pipeline.cpp): this context is then only the front of a chain of stage
    // contexts, one per listed device; every rwkv.h entry point walks the chain.
    std::vector<rwkv_context *> stages;
    hipEvent_t handoff_ev = nullptr;   // (stage contexts) residual stream handed to the next stage
    hipEvent_t consumed_ev = nullptr;  // (stage contexts) this stage is done with the pass whose input it was handed

    void * abi_streamer = nullptr;   // copy streams + download thread of the streamed rwkv_eval (engine.hip), created on first use

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t mega_done = nullptr;   // completion of this context's latest persistent-kernel launch (engine.hip: launches are chained per device)
    uint32_t * ntok_out = nullptr;        // (runner.cpp) where a launch that folds the argmax leaves the chosen token instead of d_tokens / d_next_token:
                                          // the first stage's token word, through the peer mapping (the token feedback without a copy)
    hipEvent_t chain_covered = nullptr;   // (runner.cpp) an event this context's stream already waits on for the coming step: when it is the device's latest
                                          // persistent launch, the per-device chain does not wait on it a second time
    std::string persist_note;         // why this context runs the single-token path it runs (rwkv_mi_persist_info: chosen kernel, calibration, fall-backs)

    // fused single-token layer when the model qualifies: RWKV-6 (fused_v6.hip), RWKV-7 or RWKV-4 / RWKV-5 (both in fused_v7.hip)
    rwkvmi::FusedLayer fused = rwkvmi::FusedLayer::none;
    rwkvmi::DevBuf<uint8_t> fused_scratch;
    // persistent whole-stage decode kernel (persist_host.h) when the model and the device qualify; takes precedence
    std::unique_ptr<rwkvmi::PersistentDecoder> mega;

    using Prof = rwkvmi::DecodeProf;
    Prof prof;
};

#define RW_NO_PIPELINE(CTX, RET) RW_CTX_CHECK((CTX), RWKV_ERROR_ARGS | RWKV_ERROR_UNSUPPORTED, RET, (CTX)->stages.empty(), \
    "this rwkv_mi_* extension works on a single-device context; with RWKV_MI_DEVICES use the rwkv.h entry points")

namespace rwkvmi {

inline bool on_device(rwkv_context * ctx) { HIP_CTX_OK(ctx, hipSetDevice(ctx->model->device)); return true; }

rwkv_context * create_context(Model * m, uint32_t n_threads);
void destroy_context(rwkv_context * ctx);

extern std::atomic<int> g_test_fail_state_init;   // test hook (rwkv_mi_test_fail_state_init): the next n state initialisations fail
// state upload / download / init on the device-resident state
bool state_from_host(rwkv_context * ctx, const float * state_in /* NULL = fresh */);
bool state_to_host(rwkv_context * ctx, float * state_out);

// Runs T tokens (already in ctx->d_tokens) through the layers of this stage. Reads state[cur], writes state[cur^1], flips cur.
// x_in / x_out: residual stream hand-off for pipeline stages (nullptr on a full model). Logits land in ctx->d_logits.
// score: the head runs on EVERY row of the pass instead of the last one (see ScorePass); T >= 2 (a single token goes through forward_decode
// and is scored from ctx->d_logits by the caller).
struct ScorePass;
bool forward(rwkv_context * ctx, int64_t T, bool want_logits, const ScorePass * score = nullptr);

// Score mode of a pass (forward, forward_segs): ln_out and the head over all T rows in chunks of ctx->score_R rows into ctx->d_score, each
// chunk followed by k_score_rows (score.hip) on the per-row words of the context -- row t of the pass reads ctx->d_score_targets[t] and writes
// ctx->d_score_logprobs[t] / ctx->d_score_argmax[t] -- and, when h_logits_all is given, by a copy of the chunk's logits to the host. The
// product kernel is chosen on the chunk's row count, as row mode's head chooses it on T: on the default arms both sides of the 32-row
// threshold are bit-identical per row, so the chunking cannot be seen in the result. keep_last: the last row's logits also go to
// ctx->d_logits, where the sampler and rwkv_mi_logits_store read them. ensure_score(ctx, T) must have succeeded.
struct ScorePass {
    bool targets = false, logprobs = false, argmax = false;   // which of the per-row words are read / written
    float * h_logits_all = nullptr;                           // host [T][n_vocab], or nullptr
    bool keep_last = false;
};
// the chunk buffer (first call: score_R = clamp(64 MiB / (4 n_vocab), 32, 1024) rows, or RWKV_MI_SCORE_ROWS >= 1) and per-row words for
// `rows` rows; false with RWKV_ERROR_ALLOC, nothing changed, when they cannot be allocated
bool ensure_score(rwkv_context * ctx, int64_t rows);
// api.cpp: the targets of a scoring call (checked with the other arguments, before anything changes)
bool check_targets(rwkv_context * ctx, const uint32_t * targets, size_t n, const float * logprobs_out);

// batched decode (engine.hip): the batch's own context (model, stream, scratch, tokens, [max_rows][n_vocab] logits; a member of the per-device
// chain of persistent launches) and one pass of T rows, row t from state d_rows[t].in into d_rows[t].out
rwkv_context * batch_context_create(Model * m, int64_t max_rows);
void batch_context_destroy(rwkv_context * c);
// What follows the head of a batch pass over `rows` rows (launch_row_sampler), described once: row r's token goes to ctx->d_tokens.p[r].
//   form, rows, probs   which choice is made -- the greedy argmax (Draw::none) or launch_draw_rows in the call's form -- on the call's row table
//           (one DrawRow per row of the pass) with the samplers' scratch
//   hist, report, step   the call's WHOLE history [steps][rows] and report buffers (chosen [steps][rows], ids / vals [steps][rows][top_n]), either
//           may be NULL, and the step of the call this pass is: the step's slot of each is written. A single pass is step 0
//   used, other   in a device loop, whose kernels rewrite the row tables between two passes: the row table of this pass and the one of the next
//   stop    the pass is a step of rwkv_mi_batch_decode_until: the choice and the report run behind the live words and launch_stop_rows follows them
//   beam    the pass is a step of rwkv_mi_batch_decode_beam: instead of a choice, launch_beam_rows and launch_beam_select follow the head;
//           of the rest only `step`, `used` and `other` are read
//   serve   the pass is a step of rwkv_mi_batch_serve: the choice runs behind the lanes' draw words and writes no history; launch_serve_rows and
//           launch_serve_reset (`chunks` workgroups per lane over state_len floats) follow it
//   session the pass is a step of a serve session: as serve, without a report, launch_session_rows in the scheduler's place
// Order within a step: the choice, then the report of what it wrote, then the stop test.
struct RowServe { ServeTables t; int64_t state_len; unsigned chunks; };
struct RowSession { SessionTables s; int64_t state_len; unsigned chunks; };
struct RowSampler {
    DrawForm form;
    const DrawRow * rows = nullptr;
    float * probs = nullptr;
    uint32_t * hist = nullptr;
    const RowReport * report = nullptr;
    uint32_t step = 0;
    RowState * used = nullptr, * other = nullptr;
    const StopTables * stop = nullptr;
    const BeamTables * beam = nullptr;
    const RowServe * serve = nullptr;
    const RowSession * session = nullptr;
};
void launch_row_sampler(rwkv_context * ctx, const RowSampler & s, int64_t rows);
// sample: when given, launch_row_sampler follows the head inside the pass's place in the chain
bool forward_rows(rwkv_context * ctx, const RowState * d_rows, int64_t T, bool want_logits, const RowSampler * sample = nullptr);

// Ragged batch pass: row i of the call is a SEGMENT, tokens [t0, t1) of the pass, consecutive tokens of one slot's sequence.
struct SegPass {
    const SegState * d_segs = nullptr;    // device: the n segments in call order (what d_seg_of indexes: the token-shift mixes)
    const int32_t *  d_seg_of = nullptr;  // device: [T], the segment of each token
    const int32_t *  d_last = nullptr;    // device: [n], the last token of each segment (the head's rows)
    const SegState * d_short = nullptr;   // device: the n_short segments the _segs recurrences run ...
    const SegState * h_long = nullptr;    // ... host: the n_long others, each on a sequence kernel over its token range (seg_takes_seq_kernel)
    int64_t n = 0, n_short = 0, n_long = 0;
};
bool seg_takes_seq_kernel(const Model & m, int64_t len);
bool forward_segs(rwkv_context * ctx, const SegPass & p, int64_t T, bool want_logits, const RowSampler * sample = nullptr, const ScorePass * score = nullptr);

// Speculative decoding (rwkv_mi_batch_eval_draft): a ragged pass whose n segments are x0 d1 .. dk of at most 1 + RWKV_MI_DRAFT_MAX tokens each
// (all of them on the _segs recurrences), with three additions that run in this call only:
//   the stash    every layer copies the inputs of its recurrences into `stash` (kernels.h, DraftStash) while the pass runs;
//   the head     on ALL T tokens into logits_all[T][n_vocab], addressable together: a row's positions are read in sequence;
//   the choice   k_draft_accept_rows (sampling.hip) walks each row's positions with the draw of the call's family -- form / rows / probs as
//                in RowSampler -- and leaves out[n][out_stride] (the emitted tokens, RWKV_MI_NO_TOKEN behind them), keep[n] (their
//                number) and, in ctx->d_logits row r, the logits the row's last emitted token was chosen from;
//   the replay   launch_draft_replay re-runs the recurrences of every row whose draft did not stand in full over its first keep tokens.
// keep never leaves the device in between. lw: the layers' vectors on the device (kernels.h, DraftLayer).
struct DraftPass {
    DraftStash stash;
    const DraftLayer * lw = nullptr;
    float * logits_all = nullptr;
    DrawForm form;                      // as in RowSampler; a row's settings are read at every position walked
    const DrawRow * rows = nullptr;
    float * probs = nullptr;
    uint32_t * out = nullptr;
    int out_stride = 0;
    uint32_t * keep = nullptr;
};
void launch_draft_accept_rows(const float * logits, int64_t rows, int n, const SegState * segs, const uint32_t * tokens, const DrawRow * table, const DrawForm & form,
                              float * probs, uint32_t * out, int out_stride, uint32_t * keep, float * logits_row, hipStream_t st);
// inputs of a layer's WKV body a pass stashes (DraftStash::n_in): 3, 3, 4, 6 for RWKV-4, 5, 6, 7
inline int draft_stash_inputs(const Model & m) { return m.arch_major == 7 ? 6 : (m.arch_major == 6 ? 4 : 3); }
bool forward_draft(rwkv_context * ctx, const SegPass & p, int64_t T, const DraftPass & d);

// fused RWKV-6 decode layer (fused_v6.hip)
bool   fused_v6_supported(const Model & m);
size_t fused_v6_scratch_bytes(const Model & m);
void   fused_v6_layer(const Model & m, const LayerW & L, float * x, const float * sin, float * sout, void * scratch, hipStream_t st, rwkv_context::Prof * pf);
// fused RWKV-7 decode layer (fused_v7.hip): five launches per layer
bool   fused_v7_supported(const Model & m);
size_t fused_v7_scratch_bytes(const Model & m);
void   fused_v7_layer(const Model & m, const LayerW & L, int layer, float * x, float * v_first, const float * sin, float * sout, void * scratch, hipStream_t st, rwkv_context::Prof * pf);
// fused RWKV-4 decode layer (fused_v7.hip): four launches per layer
bool   fused_v4_supported(const Model & m);
size_t fused_v4_scratch_bytes(const Model & m);
void   fused_v4_layer(const Model & m, const LayerW & L, float * x, const float * sin, float * sout, void * scratch, hipStream_t st, rwkv_context::Prof * pf);
// the persistent decode kernels (persist_host.h), one creator each. nullptr: the model / device does not qualify
PersistentDecoder * mega_v6_create(const Model & m);   // RWKV-6, register prefetch (mega_v6.hip)
PersistentDecoder * ring_v6_create(const Model & m);   // RWKV-6, LDS-DMA weight ring (ring_v6.hip)
// tests/ only (csrc/testhooks_rowsum.cpp): ring_v6.hip's two row-sum reductions on n x 64 device floats, n in 1..16 (false: n out of range);
// ring_rowsum_lanes(n): the lanes one value occupies in the scattered result (ScatP<n>::W)
bool launch_ring_rowsum_test(int n, const float * in, float * out_n, float * out_s, hipStream_t st);
int ring_rowsum_lanes(int n);
PersistentDecoder * p47_create(const Model & m);       // RWKV-4 / RWKV-7 (persist_v47.hip)
const char * persist_unavailable_reason(const Model & m);   // nullptr: a persistent kernel exists for this model on this device
// ---- layer pipeline in one process (pipeline.cpp) ----
bool upload_tokens(rwkv_context * ctx, const uint32_t * tokens, size_t n);   // api.cpp: pinned staging + async copy into ctx->d_tokens
rwkv_context * pipeline_create(const char * path, uint32_t n_threads, const char * devices);
void pipeline_destroy(rwkv_context * front);
bool pipeline_eval(rwkv_context * front, const uint32_t * tokens, size_t n, size_t chunk, const float * state_in, float * state_out, float * logits_out);
rwkv_context * pipeline_clone(rwkv_context * front, uint32_t n_threads);
// runner.cpp: resident state of a chain; greedy decode of n_streams contexts (chains of the same stages, or one-device contexts) interleaved
bool pipeline_state_load(rwkv_context * front, const float * state_in);
bool pipeline_state_store(rwkv_context * front, float * state_out);
bool pipeline_decode_greedy(rwkv_context * const * fronts, size_t n_streams, const uint32_t * first_tokens, size_t n_tokens, uint32_t * tokens_out, float * elapsed_ms);
// after a poll time-out of the persistent kernel: drain, clear, drop the persistent path (see engine.hip)
void recover_from_abort(rwkv_context * ctx);
// rwkv_eval with the caller's state streamed group by group under the layers (engine.hip)
bool forward_streamed_eligible(const rwkv_context * ctx);
bool forward_streamed(rwkv_context * ctx, bool want_logits, const float * h_in, float * h_out, float * h_logits, bool * aborted);
void abi_streamer_free(void * p);
// single-token forward through the captured hipGraph (falls back to forward() when capture is disabled)
bool forward_decode(rwkv_context * ctx, bool want_logits);
bool single_launch_step(const rwkv_context * ctx, bool want_logits);
hipEvent_t mega_chain_marker(rwkv_context * ctx);   // the event recorded behind ctx's persistent launch if that launch is the latest of its device (else nullptr)   // the step is one directly issued persistent launch (no graph replay)
void drop_graphs(rwkv_context * ctx);   // the captured single-token graphs hold pointers: dropped when a buffer they name moves
// grows the per-context activation scratch to hold T tokens
bool ensure_scratch(rwkv_context * ctx, int64_t T);
uint32_t * folded_argmax_target(const rwkv_context * ctx);
// hand-off buffer size in floats: D, or 2 D for RWKV-7 (x and v_first travel together)
int64_t handoff_len(const Model & m);

}  // namespace rwkvmi
