/*
 * rwkv_mi355x.h -- opt-in extensions of librwkv.so for MI355X. None of these change the behaviour of the rwkv.h entry
 * points; they expose what the device-resident engine can do beyond the reference ABI:
 *
 *  - the recurrent state can stay in HBM between calls (the reference ABI hands the whole state in and out through host
 *    memory on every call, rwkv_eval.inc:2-22 -- 34.6 MB each way for RWKV-6 7B, i.e. as long as the token itself);
 *  - a greedy decode loop that never leaves the device (argmax on the GPU feeds the next embedding lookup);
 *  - the numbers the benchmark needs (algorithmic bytes per token).
 */
#ifndef RWKV_MI355X_H
#define RWKV_MI355X_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Copies a host state (or a fresh state when NULL) into the context's device-resident state (on a RWKV_MI_DEVICES chain: every stage
 * takes the slice of its layers; rwkv_mi_state_store and rwkv_mi_decode_greedy work on chains as well). */
RWKV_API bool rwkv_mi_state_load(struct rwkv_context * ctx, const float * state_in);
/* Copies the device-resident state to host memory (FP32[rwkv_get_state_len]). */
RWKV_API bool rwkv_mi_state_store(struct rwkv_context * ctx, float * state_out);

/* Like rwkv_eval_sequence, but continues from and updates the device-resident state; no state traffic over PCIe.
 * logits_out (of the last token) may be NULL. */
RWKV_API bool rwkv_mi_eval_resident(struct rwkv_context * ctx, const uint32_t * tokens, size_t n_tokens, float * logits_out);

/* Greedy single-stream decode entirely on the device: feeds first_token, then n_tokens - 1 times the argmax of the
 * previous logits. tokens_out[i] = argmax after step i (may be NULL). elapsed_ms (may be NULL) receives the HIP-event
 * time of the whole loop measured on the context's stream. */
RWKV_API bool rwkv_mi_decode_greedy(struct rwkv_context * ctx, uint32_t first_token, size_t n_tokens, uint32_t * tokens_out, float * elapsed_ms);

/* Temperature / top-p sampling ON THE DEVICE from the logits of the last evaluation (the reference samples on the host:
 * python/sampling.py:10-52 -- same statements: softmax, top-p cut-off, p^(1/temperature), renormalise, draw). temperature == 0: argmax;
 * top_p == 0 means 1. u in [0, 1): the caller's uniform random number; u < 0: the context's counter-based generator with `seed`.
 * top-k and min-p are not arguments but a setting of the sequence (rwkv_mi_truncation_set, below): every draw reads it. */
RWKV_API bool rwkv_mi_sample(struct rwkv_context * ctx, float temperature, float top_p, float u, uint64_t seed, uint32_t * token_out);
/* Sampling decode loop entirely on the device (like rwkv_mi_decode_greedy, the sampled token feeds the next embedding lookup). */
RWKV_API bool rwkv_mi_decode_sample(struct rwkv_context * ctx, uint32_t first_token, size_t n_tokens, float temperature, float top_p, uint64_t seed,
                                    uint32_t * tokens_out, float * elapsed_ms);

/* Measurement aid: eager greedy decode with a HIP-event pair (on the context's stream) around every launch of the dominant
 * kernel -- the single-token projection of the model's quantised format. out[0] = summed kernel ms, out[1] = launches,
 * out[2] = summed algorithmic bytes (weight rows + quantised activation + outputs), out[3] = wall ms of the loop. */
RWKV_API bool rwkv_mi_profile_decode(struct rwkv_context * ctx, uint32_t first_token, size_t n_tokens, double * out);

/* The same for sequence mode: one pass over `tokens` (at most 1024) from the resident state, HIP events around every launch of the int8
 * MFMA GEMM. out[0] = summed kernel ms, out[1] = launches, out[2] = summed integer operations (2 T N K per launch), out[3] = wall ms of the pass. */
RWKV_API bool rwkv_mi_profile_prefill(struct rwkv_context * ctx, const uint32_t * tokens, size_t n_tokens, double * out);

/* Algorithmic HBM bytes one decoded token must move on this context's layers: every parameter once (file dtype), one
 * embedding row, state read + write, logits write. */
RWKV_API uint64_t rwkv_mi_bytes_per_token(const struct rwkv_context * ctx);
RWKV_API uint64_t rwkv_mi_weight_bytes(const struct rwkv_context * ctx);
/* Arithmetic of one rwkv_eval_sequence pass over n_tokens: 2 * n_tokens * (elements of every 2-D layer matrix) + 2 * n_vocab * n_embed. */
RWKV_API uint64_t rwkv_mi_prefill_flops(const struct rwkv_context * ctx, size_t n_tokens);

/* Detected architecture (4, 5.1, 5.2, 6, 7) and head geometry. Any pointer may be NULL. */
RWKV_API void rwkv_mi_get_arch(const struct rwkv_context * ctx, uint32_t * major, uint32_t * minor, uint32_t * head_count, uint32_t * head_size);

/* Single-token steps are replayed from a captured hipGraph by default; disable for debugging / profiling per kernel. */
RWKV_API void rwkv_mi_set_graph_enabled(struct rwkv_context * ctx, bool enabled);

/* Which single-token path this context runs: 0 = one kernel per graph op, 1 = fused RWKV-6 layer (seven launches per layer),
 * 2 = persistent whole-stage kernel (one launch per token; needs the device to itself). The choice is made
 * at context creation from the model geometry, the weight format and the environment (RWKV_MI_NO_FUSED / RWKV_MI_NO_MEGA). */
RWKV_API int rwkv_mi_decode_path(const struct rwkv_context * ctx);

/* Which persistent kernel serves decode path 2: 2 = weights streamed through an LDS ring by a loader wave (LDS-DMA; the default where the
 * model qualifies), 1 = weights prefetched into the registers of the waves that use them (RWKV_MI_PERSIST=regs), 0 = path 2 not active. */
RWKV_API int rwkv_mi_persist_kind(const struct rwkv_context * ctx);
/* "persist: ring|regs|k47|none; <why>" -- the kernel above by name and what decided it: the device (the persistent kernels need all 256 CUs of an
 * unpartitioned MI355X; rwkv_get_system_info_string() carries PERSISTENT_DECODE=available|unavailable for the current device), the model's
 * format / geometry, the environment, the calibration's two figures, or a fall-back after a poll time-out at run time (a second process on the
 * GPU). The string is valid until the next call on this thread. */
RWKV_API const char * rwkv_mi_persist_info(struct rwkv_context * ctx);

/* How long the payload of the model file took to reach HBM at rwkv_init_from_file (parallel reads into pinned staging buffers,
 * asynchronous copies, re-pack kernels; the reference reads one tensor at a time, rwkv_file_format.inc:302-313), and its bytes. */
RWKV_API void rwkv_mi_load_stats(const struct rwkv_context * ctx, double * seconds, uint64_t * bytes);

/* Waits for the context's stream and reports whether every persistent-kernel step so far completed (false: a poll timed out
 * because not all workgroups could be resident -- the device is shared, or other kernels held CUs for seconds; results since
 * then are invalid and the context should be re-created with RWKV_MI_NO_MEGA=1). Always true on paths 0 and 1. */
RWKV_API bool rwkv_mi_decode_healthy(struct rwkv_context * ctx);

/* Diagnostic for decode path 2: runs `n` eager single-token steps of `token` and returns the shader-clock stamps the
 * persistent kernel took in layer `layer`: out[(workgroup * 8 + wave) * 32 + k], 256 workgroups, k < 30 (k < 17 shader-clock stamps, 17..29 stamps of the 100 MHz real-time counter; wave 0: the
 * polling wave's phases, waves 1..7: the row workers' phases; tools/trace.py prints them). false if path 2 is not active. */
RWKV_API bool rwkv_mi_trace_phases(struct rwkv_context * ctx, uint32_t token, int layer, int n, long long * out);

/* ---- layer pipeline: one process per GPU, each owning layers [layer_begin, layer_end) and their slice of the state ----
 * (supersedes the reference's n_gpu_layers CPU/GPU split, rwkv_model_loading.inc:129-142). The hand-off of the residual
 * stream between stages is the caller's job (RCCL send/recv over xGMI, see rwkv.cpp_amd/pipeline.py). */

/* Loads only the tensors of layers [layer_begin, layer_end) (plus emb + ln0 on the first stage, ln_out + head on the last). */
RWKV_API struct rwkv_context * rwkv_mi_init_stage(const char * model_file_path, uint32_t n_threads, uint32_t layer_begin, uint32_t layer_end);
/* Runs every later call of this context on the given hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
RWKV_API bool rwkv_mi_set_stream(struct rwkv_context * ctx, void * hip_stream);
/* Floats in one hand-off message: n_embed, or 2 * n_embed for RWKV-7 (x and v_first). */
RWKV_API size_t rwkv_mi_handoff_len(const struct rwkv_context * ctx);
RWKV_API void rwkv_mi_stage_range(const struct rwkv_context * ctx, uint32_t * layer_begin, uint32_t * layer_end);
/* One single-token step of the stage on its stream, not synchronised. First stage: token id read from device memory
 * (d_token). Other stages: residual stream from x_in (device). Not last: writes x_out (device). Last: ln_out + head,
 * argmax into d_next_token (device, may be NULL). State stays resident (use rwkv_mi_state_load(ctx, NULL) to reset). */
RWKV_API bool rwkv_mi_stage_step(struct rwkv_context * ctx, const uint32_t * d_token, const float * x_in, float * x_out, uint32_t * d_next_token);
/* The greedy decode loop of a whole pipeline, enqueued from C++ (runner.cpp) -- no host language between tokens.
 * rwkv_mi_decode_greedy_streams: n_streams contexts of ONE process (a RWKV_MI_DEVICES chain and its clones, or a one-device context
 * and its clones), interleaved stream by stream so that every stage of the chain has work; per-stage launches replay per-device
 * hipGraphs, the residual stream travels device to device. tokens_out: [n_streams][n_tokens] (may be NULL); elapsed_ms: host wall time
 * of the loop including the final drain (may be NULL). State: resident (rwkv_mi_state_load works on chains too). */
RWKV_API bool rwkv_mi_decode_greedy_streams(struct rwkv_context * const * ctxs, size_t n_streams, const uint32_t * first_tokens, size_t n_tokens,
                                            uint32_t * tokens_out, float * elapsed_ms);
/* One process per GPU: this rank's stage (rwkv_mi_init_stage + clones, one per decode stream, all bound to one stream) runs its share
 * of the same loop with ncclSend / ncclRecv of librccl.so on the stage's stream. librccl.so is dlopen'ed by the first rwkv_mi_comm_*
 * call (librwkv.so itself does not depend on it). comm_fwd: residual stream rank -> rank + 1; comm_fb: the chosen token from the last
 * rank to rank 0 -- two communicators of the same ranks (a single one would dead-lock, see runner.cpp). The 128-byte id of
 * rwkv_mi_comm_unique_id (rank 0) is distributed by the caller (e.g. torch.distributed.broadcast). tokens_out is filled on the last rank. */
RWKV_API bool rwkv_mi_comm_available(void);
RWKV_API bool rwkv_mi_comm_unique_id(void * id_out, size_t capacity);
RWKV_API void * rwkv_mi_comm_init(const void * id128, int rank, int world);
RWKV_API void rwkv_mi_comm_free(void * comm);
/* The same kind of handle WITHOUT RCCL, for ranks that share one GPU (RCCL refuses that; tests of the multi-process loop): mailboxes in
 * device memory shared through HIP IPC, hand-shakes through a POSIX shared-memory segment `name` ("/...", the same on every rank, unique
 * per communicator and run). A hop synchronises the stream on both sides: correct and slow, not a production transport. */
RWKV_API void * rwkv_mi_comm_init_ipc(const char * name, int rank, int world);
RWKV_API bool rwkv_mi_stage_run(struct rwkv_context * const * handles, size_t n_streams, const uint32_t * first_tokens, size_t n_tokens,
                                int rank, int world, void * comm_fwd, void * comm_fb, uint32_t * tokens_out, float * elapsed_ms);
/* Copies the context's logits (n_vocab floats, from the last step that produced any) to host memory. */
RWKV_API bool rwkv_mi_logits_store(struct rwkv_context * ctx, float * logits_out);
/* Device pointer of the context's logits (n_vocab floats), valid after a step that produced logits. */
RWKV_API const float * rwkv_mi_logits_device_ptr(const struct rwkv_context * ctx);

/* The hand-over generation of decode path 2 (the persistent kernel compares its low 16 bits; it advances by 8 per layer and launch).
 * Diagnostic, read-only: bench.py places its parity run across the 16-bit wrap with it. 0 if path 2 is off. */
RWKV_API uint32_t rwkv_mi_decode_generation(struct rwkv_context * ctx);

/* ---- Batched decode: n independent sequences per pass over the weights ----
 * A batch owns n_slots device-resident states ([2][n_slots][state_len], double-buffered with a parity per slot) for ctx's model, and
 * its own stream, scratch and [n_slots][n_vocab] logits buffer. Single-device contexts only (not a RWKV_MI_DEVICES chain). It must be
 * freed before ctx; errors are reported on ctx (rwkv_get_last_error). One batch object is not thread-safe.
 * Each row of a call is bit-identical to rwkv_eval of that sequence alone. A call reads each named slot's current buffer, writes the
 * other one and flips the slot's parity only when the pass succeeded; slots not named are untouched. A call returns false with
 * RWKV_ERROR_ARGS and changes no slot when n == 0, n > n_slots, a slot index is out of range or repeated, or a token is >= n_vocab.
 * On a device that also runs a persistent decode kernel, batch passes and persistent launches are ordered on the device, never concurrent. */
struct rwkv_mi_batch;
RWKV_API struct rwkv_mi_batch * rwkv_mi_batch_create(struct rwkv_context * ctx, size_t n_slots);
RWKV_API void rwkv_mi_batch_free(struct rwkv_mi_batch * batch);
/* host state (or a fresh state when NULL) into a slot / a slot into host memory (FP32[rwkv_get_state_len]) */
RWKV_API bool rwkv_mi_batch_state_load(struct rwkv_mi_batch * batch, size_t slot, const float * state_in);
RWKV_API bool rwkv_mi_batch_state_store(struct rwkv_mi_batch * batch, size_t slot, float * state_out);
/* device-to-device: a context's resident state into a slot, and a slot into a context's resident state (prefill on a context, then join
 * the batch; rwkv_mi_batch_eval_ragged below takes a prompt in without the extra pass). ctx must be a single-device context of the same
 * device and state size. */
RWKV_API bool rwkv_mi_batch_state_from_context(struct rwkv_mi_batch * batch, size_t slot, struct rwkv_context * ctx);
RWKV_API bool rwkv_mi_batch_state_to_context(struct rwkv_mi_batch * batch, size_t slot, struct rwkv_context * ctx);
/* One token for each of n slots in ONE pass over the weights: row i = slots[i] fed tokens[i].
 * logits_out: [n][n_vocab] in call order, or NULL to skip the head. */
RWKV_API bool rwkv_mi_batch_eval(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * tokens, size_t n, float * logits_out);
/* Greedy loop on the device: as rwkv_mi_decode_greedy on each slot, all n advancing together (the argmax of each row feeds that row's
 * next embedding lookup, no host round trip). tokens_out: [n][n_tokens] (may be NULL); elapsed_ms as rwkv_mi_decode_greedy. A failure
 * after the first pass leaves the named slots' states unspecified. */
RWKV_API bool rwkv_mi_batch_decode_greedy(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                          size_t n_tokens, uint32_t * tokens_out, float * elapsed_ms);

/* Sampling in the batch, on the device: one row of parameters per row of the call, with the meaning of rwkv_mi_sample's arguments
 * (temperature == 0: argmax; top_p == 0 means 1; u in [0, 1): the caller's uniform number; u < 0: the generator uniform01(seed, counter));
 * top-k and min-p are a setting of the slot (rwkv_mi_batch_truncation_set, below).
 * The batch owns ONE DRAW COUNTER PER SLOT (zero at rwkv_mi_batch_create): a row's draw reads and advances the counter of its slot, not of
 * its position in the call, by one per draw that is not an argmax -- a sequence's random stream does not depend on who else is in the pass
 * or in which order the slots are named. rwkv_mi_batch_eval and rwkv_mi_batch_decode_greedy never touch the counters.
 * Besides what every batch call rejects, the two sampling calls return false with RWKV_ERROR_ARGS and change no slot, parity or counter when
 * params (or sampled_out) is NULL, a temperature is < 0, a top_p is outside [0, 1], a u is >= 1, or any of the three is NaN. */
struct rwkv_mi_sample_params { float temperature; float top_p; float u; uint64_t seed; };   /* 24 bytes */
/* One token for each of n slots in one pass (as rwkv_mi_batch_eval), then one sampled token per row from that row's logits, on the
 * device. sampled_out: [n]. logits_out: [n][n_vocab] or NULL (the head runs either way). Only 4 n bytes have to cross PCIe. */
RWKV_API bool rwkv_mi_batch_eval_sample(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * tokens, size_t n,
                                        const struct rwkv_mi_sample_params * params /* [n] */, uint32_t * sampled_out, float * logits_out);
/* Sampling loop on the device: as rwkv_mi_decode_sample on each slot, all n advancing together. Resets the named slots' draw
 * counters to 0 first (as rwkv_mi_decode_sample resets its context's). params[i].u is ignored: the generator draws.
 * tokens_out: [n][n_tokens] (may be NULL); elapsed_ms, parity and failure rules as rwkv_mi_batch_decode_greedy. */
RWKV_API bool rwkv_mi_batch_decode_sample(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                          size_t n_tokens, const struct rwkv_mi_sample_params * params /* [n] */,
                                          uint32_t * tokens_out, float * elapsed_ms);
/* Sets a slot's draw counter (a new request in a reused slot: 0; resuming a recorded sequence: its count). */
RWKV_API bool rwkv_mi_batch_rng_seek(struct rwkv_mi_batch * batch, size_t slot, uint64_t counter);

/* ---- Ragged passes: prompts and decode rows in one pass over the weights ----
 * Row i of a call names slot slots[i] and feeds it lens[i] >= 1 CONSECUTIVE tokens; the pass runs all T = sum(lens) tokens in one walk over
 * the weights. A row with lens[i] == 1 is a decode row of rwkv_mi_batch_eval; a longer one is a prompt, or a chunk of one, taken in
 * without a separate context. tokens: the rows' tokens back to back, T words.
 * Each named slot ends with the state rwkv_eval_sequence gives on that slot's tokens alone from its current state -- the state of repeated
 * rwkv_eval, bit for bit -- and its logits (those of the row's LAST token) are bit-identical as well, however a prompt is cut into chunks
 * and whoever else is in the pass. The matrix-core product path is chosen on T, not on n: 31 prompts of 2 tokens are one 62-token pass.
 * Under the opt-in arms RWKV_MI_SEQ_Q=fast and RWKV_MI_SEQ_F16=mfma a ragged pass of T >= 32 tokens has the stated tolerance of sequence
 * mode instead; it is not bit-identical there.
 * Parity, untouched slots and ordering against a persistent kernel: as every batch call. Besides what rwkv_mi_batch_eval rejects, a call
 * returns false with RWKV_ERROR_ARGS and changes no slot, parity or counter when lens is NULL, a lens[i] is 0, any of the T tokens is
 * >= n_vocab, or the lengths add up to more than INT32_MAX. When the scratch (or the token words) for T tokens cannot be allocated it
 * returns false with RWKV_ERROR_ALLOC and changes no slot.
 * logits_out: [n][n_vocab] in call order, or NULL to skip the head. */
RWKV_API bool rwkv_mi_batch_eval_ragged(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens,
                                        size_t n, float * logits_out);
/* The same, then one sampled token per row from that row's last-token logits, with the per-slot draw counters and the argument rules of
 * rwkv_mi_batch_eval_sample. EVERY row is sampled: give a row that is a non-final chunk of a prompt temperature == 0 -- it is then an
 * argmax, and an argmax does not advance its slot's draw counter, so the slot's random stream is that of its decode steps alone. */
RWKV_API bool rwkv_mi_batch_eval_ragged_sample(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens,
                                               size_t n, const struct rwkv_mi_sample_params * params /* [n] */, uint32_t * sampled_out,
                                               float * logits_out);

/* ---- Scoring: the model's prediction at EVERY position of given text, in one pass ----
 * rwkv_eval_sequence and rwkv_mi_eval_resident report the logits of the last token only. Perplexity (the reference's
 * python/measure_pexplexity.py calls rwkv_eval once per token) and the log-probability of given text (multiple choice, the log-probs of a
 * prompt, checking a draft) need the prediction after each token. These calls run the tokens through the sequence path once and put the
 * head on all positions, in chunks of R rows (R = 64 MiB of logits: 256 rows at 65536 tokens, at least 32, at most 1024; RWKV_MI_SCORE_ROWS
 * overrides it, read when a context's or batch's first scoring call allocates the chunk); a kernel reduces every row on the device to
 *   argmax[t]  = the index of the largest logit after tokens[t], the lowest index among equals (the rule of the greedy loops), and
 *   logprob[t] = (float) ((double) l[target] - (m + log(sum_j exp((double) l[j] - m)))),  l = the logits after tokens[t], m = their maximum,
 * the sum accumulated in float64 in a fixed order (no atomics) and the result rounded to f32 once: a log-prob depends on its row's logits
 * and its target only, bit for bit, not on the chunking, the other rows or the run. Against float64 arithmetic on the same logits it is off
 * by at most one f32 ulp of the result plus 2^-32. A target of RWKV_MI_NO_TARGET gives 0.
 * Each position's logits equal rwkv_eval's at that token bit for bit, the state afterwards equals rwkv_eval_sequence's, however the call is
 * cut -- on the default arms. Under the opt-in arms RWKV_MI_SEQ_Q=fast and RWKV_MI_SEQ_F16=mfma, the per-position logits (and what is
 * derived from them) have sequence mode's stated tolerance instead.
 * The buffers are allocated by the first scoring call of a context / batch (RWKV_ERROR_ALLOC, nothing changed, when they cannot be) and
 * released by rwkv_free / rwkv_mi_batch_free. */
#define RWKV_MI_NO_TARGET UINT32_MAX
/* Feeds n_tokens tokens from the resident state (as rwkv_mi_eval_resident: state updated, pieces of 1024) and reports the model's
 * prediction AFTER EACH of them. targets[t] (< n_vocab, or RWKV_MI_NO_TARGET) is scored against the logits after tokens[t].
 * logprobs_out [n_tokens], argmax_out [n_tokens], logits_all_out [n_tokens][n_vocab]: each may be NULL; targets may be NULL iff logprobs_out is
 * (targets without logprobs_out are checked and otherwise ignored). With every output NULL the call is rwkv_mi_eval_resident(.., NULL).
 * Afterwards the context's own logits are those of the last token: rwkv_mi_sample and rwkv_mi_logits_store work as after rwkv_mi_eval_resident.
 * Returns false with RWKV_ERROR_ARGS, nothing changed, for what rwkv_mi_eval_resident rejects (a RWKV_MI_DEVICES chain included), for a
 * target >= n_vocab that is not RWKV_MI_NO_TARGET, and for logprobs_out without targets. */
RWKV_API bool rwkv_mi_score_resident(struct rwkv_context * ctx, const uint32_t * tokens, size_t n_tokens, const uint32_t * targets,
                                     float * logprobs_out, uint32_t * argmax_out, float * logits_all_out);
/* The ragged form: row i feeds lens[i] tokens to slot slots[i] (rules, parity and rejections of rwkv_mi_batch_eval_ragged, plus the two
 * target rules above); targets / logprobs_out / argmax_out are [T = sum(lens)] in token order. Each slot's values equal
 * rwkv_mi_score_resident of its tokens alone, bit for bit. With both outputs NULL the call is rwkv_mi_batch_eval_ragged(.., NULL). */
RWKV_API bool rwkv_mi_batch_score_ragged(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens,
                                         const uint32_t * targets, size_t n, float * logprobs_out, uint32_t * argmax_out);

/* ---- Presence / frequency penalties and logit bias in the device sampler ----
 * What the reference's chat program does before every draw (chat_with_bot.py:243-258: for each token n generated so far in this response,
 * logits[n] -= PRESENCE_PENALTY + token_counts[n] * FREQUENCY_PENALTY, defaults 0.2 / 0.2) and what sample_logits' logit_bias adds
 * (sampling.py:27-36; chat_with_bot.py:78,233 forbids a newline with it), on the device, between the head and the next embedding lookup.
 * Per sequence -- per slot of a batch, or per context -- the device keeps two tables:
 *   count[n_vocab]  uint32, the OCCURRENCE TABLE, zero at creation;
 *   bias[n_vocab]   float, the BIAS TABLE, absent until set.
 * A penalised draw reads, instead of the logit l[j],
 *   adj[j] = (l[j] - (presence + (float) count[j] * frequency)) + bias[j]
 * every operation rounded to f32 in that order, no contraction (the reference's order: the penalty is taken from the logits, then
 * sample_probs adds the bias). As the reference's loop runs over the tokens that HAVE occurred, the penalty is taken where count[j] > 0
 * only: a token that has not occurred keeps l[j] (+ bias[j]); the presence penalty is what separates the two. The bias add is skipped
 * for a sequence without a bias. A count is exact as a float below 2^24.
 * Everything after that is the sampler of rwkv_mi_sample: softmax, top-p cut-off, temperature power, draw, and the draw-counter rule.
 * When the row's `record` is non-zero the chosen token's count goes up by one AFTER the draw, argmax or not: the draw of step i sees the
 * counts of the steps before it. A row with record == 0 updates nothing -- give a non-final prompt chunk of a ragged pass
 * temperature == 0 AND record == 0. The logits are never modified: logits_out and rwkv_mi_logits_store return the model's logits.
 * With presence == frequency == 0 and no bias, adj[j] == l[j] bit for bit and the token is the one the plain call picks.
 * The calls above (rwkv_mi_sample, rwkv_mi_batch_eval_sample, ...) never read or touch counts or bias.
 * THE TWO PENALISED LOOPS CONTINUE: they reset neither the counts nor the draw counters, and every step records (penalties[i].record is
 * not read there). A new request calls counts_reset and rng_seek(.., 0) first; decoding 16 + 16 tokens equals decoding 32, bit for bit.
 * Batches allocate their tables ([n_slots][n_vocab] each) on the first call of this family (RWKV_ERROR_ALLOC when they cannot be),
 * contexts likewise; rwkv_mi_batch_free / rwkv_free release them. Not on RWKV_MI_DEVICES chains.
 * Besides what their plain counterparts reject, these calls return false with RWKV_ERROR_ARGS and change no slot, parity, draw counter,
 * count or bias when penalties is NULL, a presence or frequency is not finite, a bias id is >= n_vocab or repeated, a bias value is NaN
 * or +inf (-inf and large negatives such as the chat program's -999999999 are allowed), a token of counts_add is >= n_vocab, or a slot
 * is out of range. */
struct rwkv_mi_penalty_params { float presence; float frequency; uint32_t record; };   /* 12 bytes */
RWKV_API bool rwkv_mi_batch_counts_reset(struct rwkv_mi_batch * batch, size_t slot);
/* count[tokens[i]] += 1 for each of the n tokens (resuming a recorded response); n == 0 changes nothing */
RWKV_API bool rwkv_mi_batch_counts_add(struct rwkv_mi_batch * batch, size_t slot, const uint32_t * tokens, size_t n);
RWKV_API bool rwkv_mi_batch_counts_store(struct rwkv_mi_batch * batch, size_t slot, uint32_t * counts_out /* [n_vocab] */);
/* REPLACES the slot's bias by bias[ids[i]] = values[i], zero elsewhere; n == 0 clears it (the slot has no bias again) */
RWKV_API bool rwkv_mi_batch_logit_bias_set(struct rwkv_mi_batch * batch, size_t slot, const uint32_t * ids, const float * values, size_t n);
/* rwkv_mi_batch_eval_sample / _eval_ragged_sample / _decode_sample with the penalised draw; penalties: [n], one row per row of the call */
RWKV_API bool rwkv_mi_batch_eval_sample_penalized(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * tokens, size_t n,
                                                  const struct rwkv_mi_sample_params * params /* [n] */, const struct rwkv_mi_penalty_params * penalties /* [n] */,
                                                  uint32_t * sampled_out, float * logits_out);
RWKV_API bool rwkv_mi_batch_eval_ragged_sample_penalized(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens,
                                                         size_t n, const struct rwkv_mi_sample_params * params /* [n] */,
                                                         const struct rwkv_mi_penalty_params * penalties /* [n] */, uint32_t * sampled_out, float * logits_out);
RWKV_API bool rwkv_mi_batch_decode_sample_penalized(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                                    size_t n_tokens, const struct rwkv_mi_sample_params * params /* [n] */,
                                                    const struct rwkv_mi_penalty_params * penalties /* [n] */, uint32_t * tokens_out, float * elapsed_ms);
/* The single context: one occurrence table and one bias table per context (a clone has its own), the same rules. */
RWKV_API bool rwkv_mi_counts_reset(struct rwkv_context * ctx);
RWKV_API bool rwkv_mi_counts_add(struct rwkv_context * ctx, const uint32_t * tokens, size_t n);
RWKV_API bool rwkv_mi_counts_store(struct rwkv_context * ctx, uint32_t * counts_out /* [n_vocab] */);
RWKV_API bool rwkv_mi_logit_bias_set(struct rwkv_context * ctx, const uint32_t * ids, const float * values, size_t n);
/* Sets the context's draw counter (rwkv_mi_decode_sample resets it to 0 itself; the penalised loop does not). */
RWKV_API bool rwkv_mi_rng_seek(struct rwkv_context * ctx, uint64_t counter);
RWKV_API bool rwkv_mi_sample_penalized(struct rwkv_context * ctx, float temperature, float top_p, float u, uint64_t seed,
                                       float presence, float frequency, uint32_t record, uint32_t * token_out);
RWKV_API bool rwkv_mi_decode_sample_penalized(struct rwkv_context * ctx, uint32_t first_token, size_t n_tokens, float temperature, float top_p, uint64_t seed,
                                              float presence, float frequency, uint32_t * tokens_out, float * elapsed_ms);

/* ---- Stop sequences and per-row token budgets in the batch decode loops ----
 * The three device loops above advance every row by exactly n_tokens passes. A request ends at a step of its own: at end of text, at a stop
 * string such as the chat program's '\n\n' (chat_with_bot.py:245-276), or at its length limit. rwkv_mi_batch_decode_until is the loop of the
 * same family -- params == NULL: the greedy loop; params without penalties: rwkv_mi_batch_decode_sample (the named slots' draw counters start
 * from 0); both: rwkv_mi_batch_decode_sample_penalized (it continues, every step records) -- in which each row ends by itself.
 * Row r emits tokens as its plain loop does: tokens_out[r][i] is the token chosen after pass i. It RETIRES after the first pass i at which
 * its emitted tokens tokens_out[r][0..i] end with one of its stop sequences, or i + 1 == stops[r].max_tokens. Then lens_out[r] = i + 1 and
 * stopped_by_out[r] = the index of the matching sequence among the row's own (the lowest when several match; a match at the budget's last step
 * reports the match), or RWKV_MI_NO_TOKEN when the budget ended the row. Only tokens emitted by this call are matched: first_tokens[r] is not
 * part of the window and a sequence cannot straddle two calls. n_seqs == 0: a budget only. A one-token sequence is a stop token ({0}: end of
 * text). tokens_out[r][j] = RWKV_MI_NO_TOKEN for lens_out[r] <= j < stride.
 * The rows' sequences are given back to back: seq_lens holds sum(n_seqs) lengths, row 0's first; seq_tokens their sum(seq_lens) tokens.
 * THE GUARANTEE: after the call everything that belongs to slots[r] -- its state, the batch's parity for it, its draw counter, its occurrence
 * table and the first lens_out[r] emitted tokens -- is, bit for bit and word for word, what the plain loop of the same family with
 * n_tokens = lens_out[r] leaves when it runs that slot, whoever else was in the call and however long they ran. The stop token is emitted
 * (and, penalised, recorded) but not fed: continue a slot by feeding tokens_out[r][lens_out[r] - 1], as after a plain loop. A retired row
 * draws nothing, records nothing and advances no counter.
 * The call ends when every row has retired, not at the largest budget: passes are enqueued in blocks of K (16; RWKV_MI_LOOP_BLOCK in
 * 1 .. 1024 overrides it, read at the call) and the number of live rows of block b - 1 is read after block b has been enqueued, so at most 2 K
 * passes run past the step at which the last row retired -- invisible in the results, counted by rwkv_mi_batch_last_loop_passes, covered by
 * elapsed_ms. The buffers are allocated by the first call (RWKV_ERROR_ALLOC when they cannot be) and released by rwkv_mi_batch_free.
 * Besides what the plain loop of its family rejects, the call returns false with RWKV_ERROR_ARGS and changes no slot, parity, counter, count or
 * bias when stops or lens_out is NULL, penalties is given without params, a max_tokens is 0, stride is less than the largest max_tokens, an
 * n_seqs is above RWKV_MI_STOP_MAX_SEQS, seq_lens is NULL with any n_seqs > 0 (or seq_tokens with any sequence), a sequence's length is 0 or
 * above RWKV_MI_STOP_MAX_LEN, or a sequence token is >= n_vocab. A failure after the first pass leaves the named slots unspecified. */
#define RWKV_MI_STOP_MAX_SEQS 16          /* stop sequences per row */
#define RWKV_MI_STOP_MAX_LEN  8           /* tokens per stop sequence */
#define RWKV_MI_NO_TOKEN      UINT32_MAX
struct rwkv_mi_stop_params { uint32_t max_tokens; uint32_t n_seqs; };   /* 8 bytes */
RWKV_API bool rwkv_mi_batch_decode_until(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                         const struct rwkv_mi_sample_params * params       /* [n], NULL: greedy */,
                                         const struct rwkv_mi_penalty_params * penalties   /* [n], NULL: the plain draw; needs params */,
                                         const struct rwkv_mi_stop_params * stops          /* [n] */,
                                         const uint32_t * seq_lens                         /* the rows' sequences back to back: sum(n_seqs) lengths ... */,
                                         const uint32_t * seq_tokens                       /* ... and their tokens back to back: sum(seq_lens) words */,
                                         size_t stride, uint32_t * tokens_out /* [n][stride], may be NULL */, uint32_t * lens_out /* [n] */,
                                         uint32_t * stopped_by_out /* [n], may be NULL */, float * elapsed_ms /* may be NULL */);
/* passes the last device loop of the batch enqueued (0 before the first) */
RWKV_API size_t rwkv_mi_batch_last_loop_passes(const struct rwkv_mi_batch * batch);

/* ---- Slot-to-slot copy and beam search: sequences that continue ANOTHER slot's state ----
 * rwkv_mi_batch_state_copy: slot src's state into slot dst, device to device on the batch's stream -- what n parallel samples of one prompt
 * need (prefill once, copy n - 1 times), and how a beam caller keeps its prompt state. `what` is a bit set: the state is copied always
 * (RWKV_MI_COPY_STATE names it); _COUNTER adds the slot's draw counter, _COUNTS its occurrence table, _BIAS its bias table and whether a bias
 * is set (a batch that has never used the penalised family has neither table: every count is 0, no bias is set, and the two bits copy
 * nothing). dst == src is a no-op that returns true. An out-of-range slot or an unknown bit is RWKV_ERROR_ARGS and changes nothing.
 * There is no bit for the truncation setting (rwkv_mi_batch_truncation_set): it is two words the caller holds, and sets on dst themselves. */
#define RWKV_MI_COPY_STATE   1u
#define RWKV_MI_COPY_COUNTER 2u
#define RWKV_MI_COPY_COUNTS  4u
#define RWKV_MI_COPY_BIAS    8u
RWKV_API bool rwkv_mi_batch_state_copy(struct rwkv_mi_batch * batch, size_t dst_slot, size_t src_slot, uint32_t what);

/* rwkv_mi_batch_decode_beam: beam search on the device. n_groups independent groups of W = params->width hypotheses in n_groups * W rows; row
 * g * W + j is slot slots[g * W + j] (all distinct). Group g starts from the state of slots[g * W] and from first_tokens[g], which is not yet
 * evaluated (the convention of rwkv_mi_batch_decode_greedy), with scores {0, -inf, ...}. THE STATE slots[g * W] HELD IS CONSUMED, as are the
 * other named slots': keep a prompt state with rwkv_mi_batch_state_copy into a slot the call does not name.
 * One step, after each pass: every unfinished hypothesis offers the W best tokens of its logits -- the report's top-N rule above (value
 * descending, then index ascending; NaN never ranks) with the report's log-prob expression, bit for bit -- each with the cumulative score
 * (double) score + (double) logprob, kept as double; not a token whose log-prob is not above -inf. A finished hypothesis offers itself once,
 * score unchanged. A score of -inf offers nothing. The W best of a group's candidates, by score descending, then parent index ascending, then
 * rank within the parent ascending -- a total order, so the result depends on the logits alone -- become hypotheses 0 .. W - 1 (0 the best).
 * A hypothesis finishes when its token is one of end_tokens (at most 8; the end token is part of its text and its score). Where fewer than W
 * candidates exist (a group whose logits are all NaN) the remaining hypotheses are dead: score -inf, length 0, finished.
 * The call ends when every hypothesis of every group has finished, or after n_tokens steps; the passes go out in blocks as in
 * rwkv_mi_batch_decode_until (rwkv_mi_batch_last_loop_passes: the passes enqueued). No state moves during the loop: a step re-parents the rows of
 * the next pass on the device. Afterwards slots[g * W + j] holds the state of hypothesis j before its last token, if j is unfinished, exactly
 * as a greedy loop leaves a slot: rwkv_mi_batch_eval of that token continues the text. The state of a finished hypothesis is unspecified.
 * Slots the call does not name, all draw counters, occurrence and bias tables are untouched. The report (rwkv_mi_batch_set_logprobs) is not
 * filled: logprobs_out carries the numbers, each equal, bit for bit, to rwkv_mi_batch_score_ragged's for that token.
 * tokens_out [G][W][n_tokens] (RWKV_MI_NO_TOKEN past a hypothesis' length), lens_out [G][W], scores_out [G][W], logprobs_out [G][W][n_tokens]
 * (0 past the length), elapsed_ms: each may be NULL. With W = 1 and no end tokens the call is rwkv_mi_batch_decode_greedy.
 * OUT OF SCOPE: penalties and bias, length normalisation, continuing a beam from given scores.
 * RWKV_ERROR_ARGS, nothing changed: a slot out of range or named twice; width not in 1 .. RWKV_MI_TOP_MAX or above n_vocab; n_end > 8 or an
 * end id >= n_vocab; a first token >= n_vocab; n_tokens or n_groups 0; n_groups * width > n_slots. The call's device words are allocated by
 * the first beam call of a batch (RWKV_ERROR_ALLOC, nothing changed, when they cannot be). */
struct rwkv_mi_beam_params { uint32_t width; uint32_t n_end; const uint32_t * end_tokens; };   /* 16 bytes */
RWKV_API bool rwkv_mi_batch_decode_beam(struct rwkv_mi_batch * batch, const uint32_t * slots /* [G][W] */, const uint32_t * first_tokens /* [G] */,
                                        size_t n_groups, const struct rwkv_mi_beam_params * params, size_t n_tokens, uint32_t * tokens_out,
                                        uint32_t * lens_out, double * scores_out, float * logprobs_out, float * elapsed_ms);

/* ---- The report: log-probs and top-N alternatives of every emitted token ----
 * What serving APIs call logprobs / top_logprobs. A caller of the device loops could so far learn how likely an emitted token was only by leaving
 * the loop (n_vocab floats per row and step to the host) or by a second pass with rwkv_mi_batch_score_ragged over what was emitted, and the
 * alternatives not at all. The REPORT is an opt-in property of a batch, or of a context, beside a call's input, draw and repeat; off by default.
 * While it is on, every call that EMITS a token -- a draw, or the greedy argmax of a loop -- records, for each emitted token of each row,
 * from the MODEL'S logits l of that step (the unmodified logits logits_out returns: not the penalised or biased adj, not shaped by temperature
 * or top_p):
 *   chosen       = (float) ((double) l[token] - (m + log(S))),  m and S exactly those of the scoring calls above: the value is, bit for bit,
 *                  the logprob rwkv_mi_batch_score_ragged / rwkv_mi_score_resident gives for the same logits with target = token (the two
 *                  kernels share one body);
 *   top_ids[k], top_logprobs[k], k < top_n <= RWKV_MI_TOP_MAX: the top_n logits that are not NaN, by value descending, then by index
 *                  ascending, each with the same log-prob expression. A NaN never ranks; -inf ranks last among the rest; where fewer than
 *                  top_n logits rank the remaining entries are RWKV_MI_NO_TOKEN / -INFINITY. Whenever some logit exceeds -inf, top_ids[0] is
 *                  the token the greedy loops pick. The selection is exact and depends on the row's logits alone -- not on the other rows,
 *                  the chunking or the run.
 * A PENALISED OR BIASED ROW REPORTS THE MODEL'S DISTRIBUTION, not the one it was drawn from: its chosen token need not be among the top_n, and
 * a token a bias forbids may be.
 * With the report on, the emitted tokens, states, parities, draw counters and occurrence tables are bit for bit those of the same call with it
 * off; with it off, no launch, allocation or copy is added.
 * Covered: rwkv_mi_batch_eval_sample, _eval_ragged_sample and their _penalized forms (steps = 1, from each row's last-token logits); the three
 * device loops, rwkv_mi_batch_decode_greedy included (steps = n_tokens); rwkv_mi_batch_decode_until (steps = the passes it enqueued,
 * rwkv_mi_batch_last_loop_passes: row r's entries at j >= lens_out[r] are 0.0f / RWKV_MI_NO_TOKEN / -INFINITY; the step at which a row retires IS
 * reported -- the stop token's log-prob -- and a retired row writes nothing afterwards); on a context rwkv_mi_sample, rwkv_mi_sample_penalized
 * (rows = steps = 1), rwkv_mi_decode_sample and rwkv_mi_decode_sample_penalized (rows = 1, steps = n_tokens). rwkv_mi_decode_greedy picks its
 * token inside the persistent launch and is NOT covered: greedy with a report is rwkv_mi_decode_sample at temperature 0.
 * The report of a call stays readable until the next emitting call, the next set_logprobs, or free; calls that emit nothing (rwkv_mi_batch_eval,
 * the scoring calls, ...) leave it alone, and so does a call that is rejected for its arguments. The device buffers are allocated by the
 * first reporting call and grown to the largest since (RWKV_ERROR_ALLOC, nothing changed, when they cannot be); rwkv_mi_batch_free / rwkv_free
 * release them.
 * The calls below return false with RWKV_ERROR_ARGS and change nothing when top_n > RWKV_MI_TOP_MAX or top_n > n_vocab, when _shape or _store
 * runs before any reporting call (or after a set_logprobs), when stride < steps, or when the context is a RWKV_MI_DEVICES chain. */
#define RWKV_MI_TOP_MAX 20
/* Turns the report on (with top_n alternatives per token; 0: the chosen token's log-prob only) or off. Ends the current report either way. */
RWKV_API bool rwkv_mi_batch_set_logprobs(struct rwkv_mi_batch * batch, bool enabled, uint32_t top_n);
/* The shape of the last reporting call: its rows, its steps, the top_n it ran with. Any pointer may be NULL. */
RWKV_API bool rwkv_mi_batch_logprobs_shape(struct rwkv_mi_batch * batch, size_t * rows, size_t * steps, uint32_t * top_n);
/* Copies the report to the host, rows in the last call's order, transposed like the loops' tokens_out. Each output may be NULL. */
RWKV_API bool rwkv_mi_batch_logprobs_store(struct rwkv_mi_batch * batch, size_t stride, float * chosen_out /* [rows][stride] */,
                                           uint32_t * top_ids_out /* [rows][stride][top_n] */, float * top_logprobs_out /* [rows][stride][top_n] */);
/* The single context: the same three (rows = 1). */
RWKV_API bool rwkv_mi_set_logprobs(struct rwkv_context * ctx, bool enabled, uint32_t top_n);
RWKV_API bool rwkv_mi_logprobs_shape(struct rwkv_context * ctx, size_t * rows, size_t * steps, uint32_t * top_n);
RWKV_API bool rwkv_mi_logprobs_store(struct rwkv_context * ctx, size_t stride, float * chosen_out /* [stride] */,
                                     uint32_t * top_ids_out /* [stride][top_n] */, float * top_logprobs_out /* [stride][top_n] */);

/* ---- Guided decoding: token automata that mask the device sampler per slot ----
 * What serving APIs call JSON mode, a regex, a choice among fixed answers, a tool-call grammar: constraining WHICH tokens a row may emit. A GUIDE
 * is a deterministic automaton over token ids: n_states states and a transition next(state, token) that is a state or DEAD. A batch holds up
 * to RWKV_MI_GUIDE_MAX guides, shared by its slots (one schema serves many requests); each slot may have one attached, with a current state.
 * Compiling a regex or a schema into such an automaton is the caller's business.
 * THE SEMANTICS, one statement: a row whose slot has a guide attached, in state s, reads instead of its logit for token j
 *     the value its draw would read anyway -- l[j] for the plain sampler, adj[j] for the penalised one -- where next(s, j) is a state,
 *     -inf                                                                                               where next(s, j) is dead;
 * everything after that is the sampler unchanged: softmax, top-p cut-off, temperature power, draw, the draw-counter rule, temperature == 0 ->
 * argmax. After the draw the slot's state becomes next(s, token). If the picked token is dead -- possible only with all-NaN logits, or when
 * the caller's own -inf bias removes every allowed token -- the state stays s and the slot's MISS COUNTER goes up by one.
 * The logits are never written, and the report keeps reporting the model's logits, as it does under penalties.
 * HONOURED by the sampled and penalised batch calls, for whatever is attached to the slots they name: rwkv_mi_batch_eval_sample,
 * _eval_ragged_sample, _decode_sample, their _penalized forms, and rwkv_mi_batch_decode_until with params. The loops CONTINUE a guide as the
 * penalised loops continue their counts: nothing resets a guide state except rwkv_mi_batch_guide_attach. In a ragged pass EVERY row draws and
 * so advances its guide: a caller that feeds non-final prompt chunks attaches the guide before the pass whose draw is the first constrained
 * token, not earlier. A retired row of rwkv_mi_batch_decode_until does not advance its guide, and THE GUARANTEE of that call extends to the
 * guide words: afterwards a slot's guide state and miss counter are those of the plain loop of lens_out[r] steps.
 * An unguided slot in a call that also names guided ones draws, bit for bit, what it draws in a call without any; a call that names no guided
 * slot performs no launch, allocation or copy it did not perform before, and a batch that never creates a guide allocates nothing.
 * REJECTED with RWKV_ERROR_ARGS, nothing changed, when a named slot has a guide attached: rwkv_mi_batch_decode_greedy, rwkv_mi_batch_decode_until
 * with params == NULL and rwkv_mi_batch_decode_beam -- the greedy family has no sampler to mask; guided greedy is temperature == 0 on the
 * sampled family. rwkv_mi_batch_eval, rwkv_mi_batch_score_ragged and rwkv_mi_batch_state_copy (no copy bit names them) leave guide words alone.
 * ON THE DEVICE a guide is the dense table uint16_t next[n_states][n_vocab], 0xFFFF for dead: 2 n_vocab bytes per state (128 KiB at 65 536
 * tokens). The edges cross to the device in the CSR form below and are expanded there.
 * rwkv_mi_batch_guide_create: the edges of state s are edge_tokens / edge_next [edge_begin[s] .. edge_begin[s + 1]), tokens strictly ascending.
 * *guide_out is the new guide's id (0 .. RWKV_MI_GUIDE_MAX - 1). False with RWKV_ERROR_ARGS, nothing changed, when a pointer is NULL, n_states is 0
 * or above RWKV_MI_GUIDE_MAX_STATES, RWKV_MI_GUIDE_MAX guides exist, edge_begin does not start at 0 or decreases, a state has no edge (every state
 * allows at least one token: a mask is never empty), a token is >= n_vocab, a state's tokens are not strictly ascending, or a next is >=
 * n_states; with RWKV_ERROR_ALLOC, nothing changed, when the table cannot be allocated.
 * rwkv_mi_batch_guide_free: RWKV_ERROR_ARGS, nothing changed, for an id that names no guide and for a guide still attached to a slot.
 * rwkv_mi_batch_guide_attach: attaches `guide` to the slot in `state` and sets the slot's miss counter to 0; RWKV_MI_NO_GUIDE detaches (state is
 * ignored). RWKV_ERROR_ARGS, nothing changed, for a slot out of range, an id that names no guide, a state >= the guide's n_states. The slots'
 * guide words are allocated by the first attach (RWKV_ERROR_ALLOC, nothing changed, when they cannot be).
 * rwkv_mi_batch_guide_state: the slot's guide (RWKV_MI_NO_GUIDE, state 0, misses 0 for a slot without one), its current state and its miss
 * counter; each output may be NULL. rwkv_mi_batch_free releases the guides and the guide words. */
#define RWKV_MI_GUIDE_MAX        16        /* guides per batch */
#define RWKV_MI_GUIDE_MAX_STATES 65535     /* states per guide (0xFFFF is the dead word) */
#define RWKV_MI_NO_GUIDE         UINT32_MAX
RWKV_API bool rwkv_mi_batch_guide_create(struct rwkv_mi_batch * batch, uint32_t n_states, const uint32_t * edge_begin /* [n_states + 1] */,
                                         const uint32_t * edge_tokens, const uint32_t * edge_next, uint32_t * guide_out);
RWKV_API bool rwkv_mi_batch_guide_free(struct rwkv_mi_batch * batch, uint32_t guide);
RWKV_API bool rwkv_mi_batch_guide_attach(struct rwkv_mi_batch * batch, size_t slot, uint32_t guide /* RWKV_MI_NO_GUIDE: detach */, uint32_t state);
RWKV_API bool rwkv_mi_batch_guide_state(struct rwkv_mi_batch * batch, size_t slot, uint32_t * guide_out, uint32_t * state_out, uint32_t * misses_out);

/* ---- Speculative decoding: verify a draft in one pass, keep its prefix ----
 * A decode pass is bound by the walk over the weights, not by arithmetic: a pass that feeds a row 5 tokens walks them once, as a pass that feeds
 * it 1 does. Where a cheap drafter (prompt lookup, an n-gram table, a small model in another context) guesses a row's next few tokens, one pass
 * can therefore emit several. What a recurrent model adds to the problem: THE STATE CANNOT BE TRUNCATED. After a pass over x0 d1 .. dk the slot
 * holds the state after dk, which is useless when only d1 .. da were right. This call verifies and repairs in ONE walk over the weights: the pass
 * stashes the inputs of its recurrences per token, the device decides how much of each draft stands, and the recurrences of the rows whose
 * draft did not stand in full are replayed over what did.
 * Row r names slot slots[r] and feeds it x0 -- the token not yet fed, by the convention of the device loops -- followed by a draft d1 .. dk,
 * k = lens[r] - 1, 0 <= k <= RWKV_MI_DRAFT_MAX; tokens holds the rows back to back, T = sum(lens) words.
 * THE SEMANTICS. Let e0, e1, ... be the tokens the PLAIN LOOP OF THE SAME FAMILY would emit for that slot from its current state, draw counter
 * and occurrence table:
 *     params == NULL              greedy      rwkv_mi_batch_decode_greedy
 *     params given                sampled     successive rwkv_mi_batch_eval_sample steps with u < 0 (the generator draws), the slot's draw
 *                                             counter CONTINUING, not reset
 *     params and penalties given  penalised   rwkv_mi_batch_decode_sample_penalized: it continues and every step records
 * (params[r].u and penalties[r].record are not read.) The number of accepted draft tokens a is the largest a <= k with e0 .. e(a-1) == d1 .. da.
 * The call emits lens_out[r] = a + 1 and tokens_out[r][0 .. a] = e0 .. ea -- the accepted draft, then the correction or bonus token -- and
 * tokens_out[r][j] = RWKV_MI_NO_TOKEN for a < j < stride.
 * THE GUARANTEE: speculation never changes what is emitted, only how many passes it takes. After the call everything that belongs to slots[r]
 * -- its state as rwkv_mi_batch_state_store shows it, its draw counter (advanced once per draw that is not an argmax: a + 1 times at a
 * temperature > 0), its occurrence table (a + 1 tokens recorded in the penalised family) -- is, bit for bit and word for word, what that plain
 * loop with n_tokens = a + 1 leaves, whoever else is in the call and whatever their drafts were. ea is emitted (and, penalised, recorded) but
 * not fed: the next call feeds it as its x0. logits_out[r] holds the model's logits from which ea was chosen. A row with lens[r] == 1 is a
 * plain step. Slots not named are untouched.
 * The guarantee holds on the default arms; under the opt-in arms RWKV_MI_SEQ_Q=fast and RWKV_MI_SEQ_F16=mfma a pass of T >= 32 tokens has the
 * stated tolerance of sequence mode instead, as the ragged calls have.
 * OUT OF SCOPE: the report -- like beam search the call does not fill it and leaves the current one alone; slots with a guide attached, which
 * are rejected; a device loop with a drafter on the device; stochastic acceptance against a draft distribution, which would change the
 * emitted stream, and this call must not.
 * Besides what rwkv_mi_batch_eval_ragged rejects, the call returns false with RWKV_ERROR_ARGS and changes no slot, parity, counter or count
 * when a lens[r] is above 1 + RWKV_MI_DRAFT_MAX, tokens_out or lens_out is NULL, stride is less than the largest lens[r], penalties is given
 * without params, params or penalties hold what the sampled and penalised calls reject, or a named slot has a guide attached.
 * The call's buffers -- the logits of all T tokens, and per layer and token the inputs of the recurrences: (5, 5, 6, 8) x n_embed floats for
 * RWKV-4, 5, 6, 7, plus one plane the replay writes -- are allocated by the first call and grown to the largest since (RWKV_ERROR_ALLOC,
 * nothing changed, when they cannot be); rwkv_mi_batch_free releases them. Every other call performs no launch, allocation or copy it did not
 * perform before. */
#define RWKV_MI_DRAFT_MAX 8      /* draft tokens per row */
RWKV_API bool rwkv_mi_batch_eval_draft(struct rwkv_mi_batch * batch, const uint32_t * slots, const uint32_t * lens /* [n]: 1 + the row's draft length */,
                                       const uint32_t * tokens /* T = sum(lens): per row x0, d1 .. dk */, size_t n,
                                       const struct rwkv_mi_sample_params * params      /* [n], NULL: greedy */,
                                       const struct rwkv_mi_penalty_params * penalties  /* [n], NULL: the plain draw; needs params */,
                                       size_t stride, uint32_t * tokens_out /* [n][stride] */, uint32_t * lens_out /* [n] */,
                                       float * logits_out /* [n][n_vocab], may be NULL */);

/* ---- Top-k and min-p in the device sampler: per-sequence truncation settings ----
 * A sequence -- a slot of a batch, or a context -- carries an optional TRUNCATION SETTING {top_k, min_p}. It is kept like the slot's bias
 * table and its guide: it stays until it is changed, and EVERY draw of that sequence reads it -- rwkv_mi_sample, rwkv_mi_decode_sample and
 * their _penalized forms on a context; rwkv_mi_batch_eval_sample, _eval_ragged_sample, the three _penalized forms, _decode_sample, the
 * sampled and penalised families of _decode_until and of _eval_draft (which emits what the plain loop with the same setting would), on
 * guided slots as on others. top_k == 0 or top_k >= n_vocab: no top-k; min_p == 0: no min-p; {0, 0} is "none", the state at creation (a
 * context made by rwkv_clone_context starts with none as well).
 * THE ORDER: mask -> softmax -> top-p and min-p, intersected -> temperature.
 *   top-k is a MASK on the values the draw reads. Let a[j] be what the row's draw reads today: the logit l[j]; penalised, the adjusted
 *   adj[j]; guided, either with the guide's -inf applied. The tokens are ranked by (a descending, index ascending) -- the total order of the
 *   report's top-N; a NaN never ranks, -inf ranks last -- and every token outside the first top_k of that order reads -inf. The sampler then
 *   runs unchanged on these values: softmax, the top-p cut-off, the temperature power, the scan, the draw. top-p is therefore taken on the
 *   distribution of the k survivors (the order of llama.cpp, vLLM and HF; RWKV's own pipeline cuts top-p on the FULL distribution and
 *   applies top-k afterwards, which keeps fewer tokens). By construction the token is, bit for bit, what the sampler without a setting
 *   picks from logits the caller had masked to -inf themselves.
 *   min-p runs on the sampler's f32 probabilities p, beside the top-p cut-off: a token survives where p[j] >= min_p * p_max (the product
 *   rounded to f32, p_max the largest p) AND it passes the top-p cut-off as before. Both thresholds are taken on the same distribution:
 *   the surviving set is their intersection.
 *   A row with temperature == 0 is an argmax; the maximum at its lowest index survives both truncations, so the setting changes nothing
 *   there. The draw counter's rule is unchanged: one advance per draw that is not an argmax.
 * With the setting "none" a draw is exactly the draw described above -- token, counter, counts, guide state -- and no call performs a launch,
 * allocation or copy it did not perform before. The logits are never written; the report (rwkv_mi_*set_logprobs) still reads the model's
 * logits; the greedy loops and beam search do not read the setting. rwkv_mi_batch_state_copy has no bit for it.
 * set returns false with RWKV_ERROR_ARGS and changes nothing when the slot is out of range, when min_p is NaN, below 0 or above 1, or (the
 * context forms, as the penalised context calls) on a RWKV_MI_DEVICES chain. get: either pointer may be NULL.
 * OUT OF SCOPE: typical-p and tail-free sampling. */
RWKV_API bool rwkv_mi_batch_truncation_set(struct rwkv_mi_batch * batch, size_t slot, uint32_t top_k, float min_p);
RWKV_API bool rwkv_mi_batch_truncation_get(struct rwkv_mi_batch * batch, size_t slot, uint32_t * top_k_out, float * min_p_out);
RWKV_API bool rwkv_mi_truncation_set(struct rwkv_context * ctx, uint32_t top_k, float min_p);
RWKV_API bool rwkv_mi_truncation_get(struct rwkv_context * ctx, uint32_t * top_k_out, float * min_p_out);

/* ---- Penalty decay and repetition penalty in the device sampler: per-sequence repetition settings ----
 * A sequence -- a slot of a batch, or a context -- carries an optional REPETITION SETTING {decay, repetition}. It is kept like the truncation
 * setting: it stays until it is changed, a context made by rwkv_clone_context starts with none, and EVERY PENALISED DRAW of that sequence reads
 * it -- rwkv_mi_sample_penalized and rwkv_mi_decode_sample_penalized on a context; rwkv_mi_batch_eval_sample_penalized,
 * _eval_ragged_sample_penalized, _decode_sample_penalized, the penalised families of _decode_until and of _eval_draft, on guided slots and on
 * slots with a truncation setting as on others. {1, 1} is "none", the state at creation.
 *   repetition  the multiplicative penalty of HF, vLLM and llama.cpp on the tokens that have occurred.
 *   decay       RWKV's own recipe: the occurrence table decays before the new token is counted (the demos' alpha_decay, 0.996), so the
 *               frequency penalty of a long answer stays bounded. A sequence with decay != 1 is DECAYING: the 4-byte words of its occurrence
 *               row hold float instead of uint32.
 * THE ARITHMETIC. With o[j] the row's occurrence entry -- the float, or (float) count[j] on a sequence that is not decaying -- a penalised draw
 * reads, every operation rounded to f32 in this order, no contraction, IEEE division:
 *     a = l[j]
 *     if (o[j] > 0) { a = a > 0 ? a / repetition : a * repetition;       (HF's rule: 0, -0, NaN and -inf take the multiply)
 *                     a = a - (presence + o[j] * frequency); }
 *     if (bias)       a = a + bias[j]
 * With the setting none this is adj[j] above, statement for statement. Everything after that is the sampler, with the guide's mask and the
 * truncation setting applied to these values as they are to adj[j].
 * After the draw, where the row records (its record is non-zero; in rwkv_mi_batch_decode_until, the row is live; every position walked by
 * rwkv_mi_batch_eval_draft), a decaying sequence does, in this order,
 *     for every j:  o[j] = o[j] * decay           (f32, subnormals kept)
 *     o[token] = o[token] + 1.0f
 * and a sequence that is not decaying count[token] += 1 as before. A row that does not record neither decays nor counts. The draw of step i
 * sees the table of the steps before it. An entry that has underflowed to 0 is a token that has not occurred.
 * On a decaying sequence rwkv_mi_*counts_add applies the two statements once per token, in the order given (resuming a recorded response leaves
 * the table the draws would have left); counts_reset zeroes the row; counts_store (uint32) returns false with RWKV_ERROR_ARGS and writes
 * nothing; counts_store_f32 works on both kinds of sequence (the counts of one that is not decaying are exact as floats below 2^24).
 * A set that changes WHETHER the sequence is decaying zeroes its occurrence row (a new request calls counts_reset anyway; a caller resuming a
 * response calls counts_add afterwards); a set that does not leaves the row alone.
 * rwkv_mi_batch_state_copy with RWKV_MI_COPY_COUNTS copies the row as it is between two slots of one kind; between a decaying slot and one that
 * is not it returns false with RWKV_ERROR_ARGS and changes nothing. It has no bit for the setting itself.
 * With the setting none a penalised draw is exactly the draw described above, and no call performs a launch, allocation or copy it did not
 * perform before. A pass that names slots with and without a setting draws them all with the kernels of this section; a row with {1, 1} then
 * reads uint32 counts and picks what it always picked. The plain sampled calls, the greedy loops, beam search and the report never read or
 * touch the setting.
 * set returns false with RWKV_ERROR_ARGS and changes nothing when the slot is out of range, when decay is NaN, below 0 or above 1, when
 * repetition is NaN, infinite or not above 0, or (the context forms, as the penalised context calls) on a RWKV_MI_DEVICES chain. get: either
 * pointer may be NULL.
 * OUT OF SCOPE: per-token count weights (the demos' zero weight for digits and punctuation), a last-n window for the repetition penalty. */
RWKV_API bool rwkv_mi_batch_repetition_set(struct rwkv_mi_batch * batch, size_t slot, float decay, float repetition);
RWKV_API bool rwkv_mi_batch_repetition_get(struct rwkv_mi_batch * batch, size_t slot, float * decay_out, float * repetition_out);
RWKV_API bool rwkv_mi_batch_counts_store_f32(struct rwkv_mi_batch * batch, size_t slot, float * out /* [n_vocab] */);
RWKV_API bool rwkv_mi_repetition_set(struct rwkv_context * ctx, float decay, float repetition);
RWKV_API bool rwkv_mi_repetition_get(struct rwkv_context * ctx, float * decay_out, float * repetition_out);
RWKV_API bool rwkv_mi_counts_store_f32(struct rwkv_context * ctx, float * out /* [n_vocab] */);

/* ---- Continuous batching: a queue of requests behind the lanes of one device loop ----
 * rwkv_mi_batch_decode_until runs n rows until the slowest has ended; a row that has retired recomputes a dead step on every pass.
 * rwkv_mi_batch_serve takes n LANES (distinct slots of the batch) and a queue of n_requests >= n REQUESTS, all known at the call; when the
 * request of a lane retires, the next request not yet taken has the lane from the next pass on, decided on the device.
 * A request q carries: its prompt, prompt_len >= 1 tokens, the requests' prompts back to back in prompt_tokens; from_slot, a slot of the batch
 * that is NOT a lane of the call, whose current state the request starts from (RWKV_MI_NO_SLOT: the fresh state; from_slot is only read: many
 * requests may share a system prompt evaluated once); its draw settings -- `sample` (family sample and penalised; u is not read: the
 * generator draws), `penalty` (penalised; record is not read: every draw records), top_k / min_p (rwkv_mi_batch_truncation_set's, {0, 0}:
 * none) and decay / repetition (rwkv_mi_batch_repetition_set's, read by the penalised family, {1, 1}: none); its budget and stop sequences,
 * `stop`, the requests' sequences back to back in seq_lens / seq_tokens as for rwkv_mi_batch_decode_until. The family is the call's.
 * SCHEDULE: lane r starts with request r. A lane whose request retires after pass i serves the next request not yet taken from pass i + 1 on;
 * lanes that retire in the same pass take requests in ascending lane order. The assignment is a function of the requests' lengths alone. A
 * lane feeds its prompt one token per pass and draws nothing until the pass that fed the last prompt token; from then on it is a row of
 * rwkv_mi_batch_decode_until. Prompt tokens are not counted in the occurrence table. At an admission the lane's draw counter becomes 0 and its
 * occurrence row zero. With the queue empty a retiring lane goes dead; the call ends when no lane has work (blocks of RWKV_MI_LOOP_BLOCK
 * passes, as rwkv_mi_batch_decode_until), and never enqueues more than sum(prompt_len - 1 + max_tokens) passes.
 * THE GUARANTEE: for every request q, tokens_out[q][0 .. lens_out[q]), lens_out[q] and stopped_by_out[q] are, bit for bit, what these calls
 * give on a batch of one slot: load the fresh state or from_slot's; rwkv_mi_batch_rng_seek 0 and _counts_reset; set the request's truncation and
 * repetition settings; rwkv_mi_batch_eval of prompt[0 .. prompt_len - 1); rwkv_mi_batch_decode_until of the family with first_token =
 * prompt[prompt_len - 1] and the request's parameters -- whoever else was in the queue. After the call lane r holds, bit for bit, what those
 * calls leave for request last_request_out[r]: state (and the batch's parity for it), draw counter and occurrence row. The lane slots' own
 * truncation / repetition settings are neither read nor changed: to continue a request on its lane, set them to the request's (a lane slot
 * that is to continue a decaying request must have been decaying before the call: a set that changes that zeroes the row).
 * Outputs: tokens_out [n_requests][stride] (RWKV_MI_NO_TOKEN past a request's length), lens_out, stopped_by_out (as rwkv_mi_batch_decode_until),
 * lane_out[q] the lane (index into lanes) that served q, start_pass_out[q] the pass that fed its first prompt token, last_request_out[r] the
 * last request lane r was given; rwkv_mi_batch_last_loop_passes: the passes enqueued.
 * REJECTED with RWKV_ERROR_ARGS, nothing changed: lanes, requests, prompt_tokens or lens_out NULL; n not in 1 .. n_slots, a lane out of range
 * or named twice; n_requests < n; an unknown family; a prompt_len of 0; a prompt token >= n_vocab; a from_slot that is a lane or out of
 * range; a lane with a guide attached or a bias set; a batch with the log-prob report on; and everything rwkv_mi_batch_decode_until,
 * rwkv_mi_batch_truncation_set and rwkv_mi_batch_repetition_set reject for the same fields. The buffers are allocated by the first call
 * (RWKV_ERROR_ALLOC when they cannot be) and released by rwkv_mi_batch_free. A failure after the first pass leaves the lanes unspecified.
 * Guides, bias and the report for served requests are rwkv_mi_batch_serve_ex's, below.
 * OUT OF SCOPE: chunked prompt ingestion inside the loop (take a long prompt in with rwkv_mi_batch_eval_ragged into a from_slot); requests
 * that arrive during the call; compacting dead lanes. */
#define RWKV_MI_NO_SLOT          UINT32_MAX
#define RWKV_MI_SERVE_GREEDY     0
#define RWKV_MI_SERVE_SAMPLE     1
#define RWKV_MI_SERVE_PENALIZED  2
struct rwkv_mi_serve_request {            /* 72 bytes */
    uint32_t prompt_len; uint32_t from_slot;
    struct rwkv_mi_sample_params sample;
    struct rwkv_mi_penalty_params penalty;
    uint32_t top_k; float min_p; float decay; float repetition;
    struct rwkv_mi_stop_params stop;
    uint32_t reserved;                    /* 0 */
};
RWKV_API bool rwkv_mi_batch_serve(struct rwkv_mi_batch * batch, const uint32_t * lanes /* [n] slots */, size_t n, int family,
                                  const struct rwkv_mi_serve_request * requests /* [n_requests] */, size_t n_requests,
                                  const uint32_t * prompt_tokens /* sum(prompt_len) words */, const uint32_t * seq_lens, const uint32_t * seq_tokens,
                                  size_t stride, uint32_t * tokens_out /* [n_requests][stride], may be NULL */, uint32_t * lens_out /* [n_requests] */,
                                  uint32_t * stopped_by_out /* [n_requests], may be NULL */, uint32_t * lane_out /* [n_requests], may be NULL */,
                                  uint32_t * start_pass_out /* [n_requests], may be NULL */, uint32_t * last_request_out /* [n], may be NULL */,
                                  float * elapsed_ms /* may be NULL */);

/* ---- Served requests with a guide, a logit bias and the log-prob report ----
 * rwkv_mi_batch_serve_ex is rwkv_mi_batch_serve -- its 17 arguments, its schedule, its outputs -- with what belongs to a REQUEST rather than to
 * a lane: two requests that follow each other on a lane may have different schemas, different biases, or one of them none.
 * extras[q] (extras NULL: no request has any):
 *   guide, guide_state   the request's draws are masked by `guide` (a guide of the batch; RWKV_MI_NO_GUIDE: none) from guide_state on, as after
 *       rwkv_mi_batch_guide_attach(guide, guide_state): the state moves along every token the request draws, prompt tokens do not move it, a
 *       dead pick counts a miss. The state and miss words are the CALL's, one pair per lane, set at every admission: the lane slots' own guide
 *       words are neither read nor written. guide_state_out[q] / guide_misses_out[q]: the request's final state and miss count (0 and 0 for
 *       an unguided request). One guided request puts the whole call on the guided draw kernel; an unguided request draws unmasked on it.
 *       rwkv_mi_batch_guide_free is not guarded against a running call; the call drains before it returns.
 *   bias_slot   the request reads the bias table of this slot of the batch (RWKV_MI_NO_SLOT: none), set beforehand with
 *       rwkv_mi_batch_logit_bias_set. Like from_slot it is only read: many requests may share one table, none is copied. The penalised
 *       family reads the bias; the plain sampler never does.
 * THE REPORT: on a batch with the report on (rwkv_mi_batch_set_logprobs) the call fills it per request, every family: rows = n_requests, steps =
 * stride, so rwkv_mi_batch_logprobs_shape / _store read [n_requests][stride]. The entry at position j of request q is what
 * rwkv_mi_batch_decode_until reports for that step -- from the model's logits, `chosen` equal to rwkv_mi_batch_score_ragged on the emitted
 * text bit for bit, an exact top-N of the batch's top_n; entries at j >= lens_out[q] are 0.0f / RWKV_MI_NO_TOKEN / -inf.
 * THE GUARANTEE extends rwkv_mi_batch_serve's: tokens, length, reason, guide state, miss count and report rows of request q are, bit for bit, what
 * a batch of one slot gives after: the state load; rwkv_mi_batch_rng_seek 0 and _counts_reset; the two settings;
 * rwkv_mi_batch_guide_attach(guide, guide_state); rwkv_mi_batch_logit_bias_set of the same ids and values; rwkv_mi_batch_set_logprobs(top_n);
 * rwkv_mi_batch_eval of prompt[0 .. prompt_len - 1); rwkv_mi_batch_decode_until from prompt[prompt_len - 1] -- whoever else is in the queue and
 * whatever the lane served before. An unguided, unbiased request draws what it draws through rwkv_mi_batch_serve. With extras NULL and the
 * report off the call performs the launches, allocations and copies of rwkv_mi_batch_serve and returns the same outputs. The schedule is
 * still a function of the requests' lengths alone.
 * REJECTED with RWKV_ERROR_ARGS, nothing changed: everything rwkv_mi_batch_serve rejects except a reporting batch (a lane whose SLOT has a guide
 * attached or a bias set is still rejected: settings come with requests); a guide that names no guide; a guide_state >= its n_states; a
 * bias_slot out of range, one that is a lane, or one with no bias set; a guided request in the greedy family (guided greedy is temperature 0
 * of the sampled family); a bias_slot in a family other than the penalised one; reserved != 0; the report on with a stride of 0.
 * OUT OF SCOPE: as rwkv_mi_batch_serve; guided greedy; a top_n per request (it is the batch's). */
struct rwkv_mi_serve_extra {              /* 16 bytes */
    uint32_t guide;                       /* a guide of the batch; RWKV_MI_NO_GUIDE: none */
    uint32_t guide_state;                 /* the state the request's first draw is masked from */
    uint32_t bias_slot;                   /* a slot of the batch whose bias table the request reads; RWKV_MI_NO_SLOT: none */
    uint32_t reserved;                    /* 0 */
};
RWKV_API bool rwkv_mi_batch_serve_ex(struct rwkv_mi_batch * batch, const uint32_t * lanes /* [n] slots */, size_t n, int family,
                                     const struct rwkv_mi_serve_request * requests /* [n_requests] */, size_t n_requests,
                                     const uint32_t * prompt_tokens /* sum(prompt_len) words */, const uint32_t * seq_lens, const uint32_t * seq_tokens,
                                     size_t stride, uint32_t * tokens_out /* [n_requests][stride], may be NULL */, uint32_t * lens_out /* [n_requests] */,
                                     uint32_t * stopped_by_out /* [n_requests], may be NULL */, uint32_t * lane_out /* [n_requests], may be NULL */,
                                     uint32_t * start_pass_out /* [n_requests], may be NULL */, uint32_t * last_request_out /* [n], may be NULL */,
                                     float * elapsed_ms /* may be NULL */, const struct rwkv_mi_serve_extra * extras /* [n_requests], may be NULL */,
                                     uint32_t * guide_state_out /* [n_requests], may be NULL */, uint32_t * guide_misses_out /* [n_requests], may be NULL */);

/* ---- Serve sessions: submit, stream and cancel requests while the loop runs ----
 * rwkv_mi_batch_serve blocks until the last request of a queue that was complete at the call has ended. A SESSION is the same device loop cut
 * at its block boundaries (RWKV_MI_LOOP_BLOCK passes, read at open) and owned by a handle: between two blocks the host adds requests to the
 * queue, takes the tokens emitted so far and drops requests. No kernel ever waits for the host.
 * THE GUARANTEE is rwkv_mi_batch_serve_ex's, whenever a request was submitted: its tokens, length, stop reason and guide words are, bit for
 * bit, what it gives alone on a batch of one slot. A cancelled request gives a prefix of those tokens.
 * rwkv_mi_batch_serve_open(batch, lanes, n, family, limits): one session per batch at a time; nothing is enqueued. limits:
 *   capacity        the entries of the request ring, >= 1 (it may be below n). Request id q lives in entry q % capacity, and an entry is free
 *                   again once its request's `finished` event has been delivered: at most `capacity` requests are in flight, and a
 *                   request that outlives capacity - 1 younger ones holds the ring until its end is delivered;
 *   max_prompt, stride, max_seqs, max_seq_tokens   per request: prompt_len <= max_prompt, stop.max_tokens <= stride, stop.n_seqs <= max_seqs,
 *                   the tokens of its sequences <= max_seq_tokens -- a ring entry has a fixed size;
 *   features        RWKV_MI_SERVE_CUT | _REP | _GUIDED: what a request may ask for (top_k / min_p; decay / repetition; a guide). It fixes
 *                   the draw kernel for the life of the session (_GUIDED and _REP bring _CUT with them, as the draw kernels do); a request
 *                   with no setting draws the same tokens on the wider kernels;
 *   reserved        0.
 * rwkv_mi_batch_serve_submit(session, request, prompt_tokens, seq_lens, seq_tokens, extra, id_out): one request, by the rules of
 *   rwkv_mi_batch_serve_ex for one request; ids count up from 0 in submit order. from_slot and bias_slot must not be lanes, and their
 *   contents must stay untouched until the request's end has been delivered (not checked). A rejected submit changes nothing.
 * rwkv_mi_batch_serve_cancel(session, id): true for a request in flight (submitted, its end not yet delivered); false, nothing changed, for
 *   an id never issued or one whose end has been delivered. The request retires at the scheduler step after the first pass of the next
 *   block enqueued -- a token drawn in that pass is still appended, and an end it brings about by itself wins -- with stopped_by
 *   RWKV_MI_STOP_CANCELLED; in its prompt phase with length 0. A request cancelled while queued is admitted and retires after one pass.
 *   True says that the request was in flight, not that the cancel decides its end: a request that has ended by itself on the device,
 *   its end not yet delivered, still reports its own stopped_by.
 * rwkv_mi_batch_serve_poll(session, flags, events_out, max_events, tokens_out, max_tokens, n_events, n_tokens): in this order,
 *   1. if the session is BUSY and the last block read left work -- a lane with a request, or a queue head below the number submitted
 *      (before any block has been read: if anything has been submitted): uploads what was submitted and cancelled since the last block and enqueues one block of passes, an
 *      admission in front of its first pass (idle lanes take what has arrived at that pass), the fetch of the session's words and an
 *      event behind it;
 *   2. waits for the event of every enqueued block but the newest (RWKV_MI_POLL_DRAIN, or a poll that enqueued nothing: the newest too)
 *      and reads their words;
 *   3. delivers: one event per request with new tokens or a newly known end, oldest request first, the events' new tokens back to back
 *      in tokens_out. What does not fit max_events / max_tokens is delivered by the next poll; no token is delivered twice.
 *   BUSY: a block is enqueued and unread, or the last block read left a lane with a request, or its queue head is below the number
 *   submitted. A poll of a session that is not busy enqueues nothing and returns at once. When the last block read left no work, a block
 *   still unread was enqueued with nothing to do: the poll reads it and enqueues no other, so a caller that polls in a loop, with or
 *   without RWKV_MI_POLL_DRAIN, comes to rest (rwkv_mi_batch_serve_stats stops moving) with at most two blocks of dead passes behind the
 *   end of the work. What the session does is a function of the sequence of calls, never of timing.
 *   An event: id; first, the position of its first token; n_new; finished; stopped_by (valid when finished: the sequence index,
 *   RWKV_MI_NO_TOKEN for the budget, RWKV_MI_STOP_CANCELLED); lane, start_pass (the pass, counted from open, that fed the first prompt
 *   token); guide_state, guide_misses (valid when finished; 0 and 0 for an unguided request).
 * rwkv_mi_batch_serve_stats: passes and blocks enqueued so far, requests in flight, submits the ring has room for.
 * rwkv_mi_batch_serve_close(session, last_request_out): cancels what is in flight, drains, sets each lane slot's parity from the passes its
 *   requests ran and frees the session; last_request_out[r]: the id lane r served last (RWKV_MI_NO_TOKEN: none -- the slot is as it was). A
 *   lane holds what its last request left, as after rwkv_mi_batch_serve. rwkv_mi_batch_free closes an open session first.
 * WHILE A SESSION IS OPEN every batch call that runs a pass (eval*, decode*, score*, serve*), rwkv_mi_batch_set_logprobs and a second open are
 * rejected with RWKV_ERROR_ARGS, nothing changed. Calls that run no pass stay legal on slots that are not lanes: state_load / _store / _copy,
 * logit_bias_set, guide_create.
 * REJECTED with RWKV_ERROR_ARGS, nothing changed -- open: what rwkv_mi_batch_serve rejects for lanes and family (a lane with a guide attached
 * or a bias set, a RWKV_MI_DEVICES chain); a batch with the log-prob report on; limits NULL, capacity or max_prompt or stride 0, max_seqs
 * above RWKV_MI_STOP_MAX_SEQS, unknown feature bits, RWKV_MI_SERVE_GUIDED in the greedy family, reserved != 0; an open session. submit: what
 * rwkv_mi_batch_serve_ex rejects for one request; a request over a limit; one that needs a feature the session did not declare; a full
 * ring (the message says "full"). poll: events_out or tokens_out NULL with a non-zero maximum.
 * OUT OF SCOPE: the log-prob report inside a session; chunked prompt ingestion (a long prompt goes in through a from_slot prepared before
 * open, or one pass per token); priorities or reordering of the queue; compacting idle lanes. */
#define RWKV_MI_STOP_CANCELLED   (UINT32_MAX - 1u)
#define RWKV_MI_SERVE_CUT        1u
#define RWKV_MI_SERVE_REP        2u
#define RWKV_MI_SERVE_GUIDED     4u
#define RWKV_MI_POLL_DRAIN       1u
struct rwkv_mi_serve_limits {             /* 28 bytes */
    uint32_t capacity; uint32_t max_prompt; uint32_t stride; uint32_t max_seqs; uint32_t max_seq_tokens;
    uint32_t features;                    /* RWKV_MI_SERVE_CUT | _REP | _GUIDED */
    uint32_t reserved;                    /* 0 */
};
struct rwkv_mi_serve_event {              /* 36 bytes */
    uint32_t id; uint32_t first; uint32_t n_new; uint32_t finished; uint32_t stopped_by;
    uint32_t lane; uint32_t start_pass; uint32_t guide_state; uint32_t guide_misses;
};
struct rwkv_mi_serve_session;
RWKV_API struct rwkv_mi_serve_session * rwkv_mi_batch_serve_open(struct rwkv_mi_batch * batch, const uint32_t * lanes /* [n] slots */, size_t n, int family,
                                                                 const struct rwkv_mi_serve_limits * limits);
RWKV_API bool rwkv_mi_batch_serve_submit(struct rwkv_mi_serve_session * session, const struct rwkv_mi_serve_request * request,
                                         const uint32_t * prompt_tokens /* [prompt_len] */, const uint32_t * seq_lens, const uint32_t * seq_tokens,
                                         const struct rwkv_mi_serve_extra * extra /* may be NULL */, uint32_t * id_out);
RWKV_API bool rwkv_mi_batch_serve_cancel(struct rwkv_mi_serve_session * session, uint32_t id);
RWKV_API bool rwkv_mi_batch_serve_poll(struct rwkv_mi_serve_session * session, uint32_t flags, struct rwkv_mi_serve_event * events_out, size_t max_events,
                                       uint32_t * tokens_out, size_t max_tokens, size_t * n_events, size_t * n_tokens);
RWKV_API bool rwkv_mi_batch_serve_stats(struct rwkv_mi_serve_session * session, uint64_t * passes, uint64_t * blocks, uint32_t * in_flight, uint32_t * room);
RWKV_API bool rwkv_mi_batch_serve_close(struct rwkv_mi_serve_session * session, uint32_t * last_request_out /* [n], may be NULL */);

#if defined(__cplusplus)
}
#endif

#endif
