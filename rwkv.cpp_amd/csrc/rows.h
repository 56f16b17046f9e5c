// rows.h -- the plain rows of the device tables: what a kernel reads per row, segment or request, and what the host lays out in a call's
// staged tables (call_layout.h). Scalars and pointers only, no HIP type: a host compiler can take their sizes.
#pragma once
#include <stdint.h>

#include "rwkv_mi355x.h"

namespace rwkvmi {

// Where the state of a row (batched decode) or of a segment -- tokens [t0, t1) of a ragged pass -- goes in -> out (kernels.h, StateRef)
struct RowState { const float * in; float * out; };
struct SegState { const float * in; float * out; int32_t t0, t1; };

// Everything the draw of one row can read, in one struct: a context's draw builds one on the host, a batch call uploads one table of them.
//   p, counter   the sampler's parameters and the draw counter of the row's sequence. p.u < 0: the draw comes from the counter-based generator
//                (p.seed, *counter), and thread 0 advances the counter on the device
//   presence, frequency, record, count, bias   the penalised draw (rwkv_mi_*_penalized) reads, instead of the logit,
//                adj[j] = (logits[j] - (presence + (float) count[j] * frequency)) + bias[j]   (the penalty where count[j] > 0 only; bias == NULL:
//                no bias) and, when record is set, counts the token: count[token] += 1. count: the sequence's occurrence table ([n] words),
//                bias: its bias table ([n] floats)
//   next, state, misses   the guide of the row's slot (rwkv_mi_batch_guide_*): its dense table next[n_states][n], GUIDE_DEAD where the transition
//                is dead -- NULL: the row has no guide and draws as the unguided kernel does -- and the slot's state and miss words. A guided
//                row in state s reads -inf for token j where next[s][j] is dead, the value of its draw elsewhere; thread 0 then moves the state
//                to next[s][token], or counts a miss when that is dead
//   top_k, min_p   the truncation setting of the row's sequence (rwkv_mi_*truncation_set; {0, 0}: none). top_k (0 or >= n: off): of the values
//                the draw would read -- logits, adjusted logits, a guide's mask applied -- the first top_k in the order (value descending, index
//                ascending; a NaN never ranks) are read as they are, every other one as -inf. min_p (0: off): of the probabilities the body
//                computes from these, those below (float) (min_p * the largest) are cut, beside the top-p cut-off. A row with temperature 0
//                is an argmax, which survives both: it ignores the setting
//   decay, repetition   the repetition setting of the row's sequence (rwkv_mi_*repetition_set; {1, 1}: none), read by the penalised draw.
//                repetition: where the token has occurred, the logit is divided by it when positive and multiplied by it otherwise, in front
//                of the penalty. decay != 1: the sequence is DECAYING -- the words of `count` hold floats, and a draw that records multiplies
//                every one of them by decay before it adds 1.0f to the pick's. The arithmetic is spelled out in include/rwkv_mi355x.h
struct DrawRow {
    rwkv_mi_sample_params p; unsigned long long * counter;
    float presence; float frequency; uint32_t record;
    uint32_t * count; const float * bias;
    const uint16_t * next; uint32_t * state; uint32_t * misses;
    uint32_t top_k; float min_p;
    float decay; float repetition;
};
// A row's stop parameters and where its sequences start in the call's flat tables: its lengths at seq_lens[seq0 ..], its tokens at seq_tokens[tok0 ..].
struct StopRow { uint32_t max_tokens, n_seqs, seq0, tok0; };
// rwkv_mi_batch_serve (sampling.hip, k_serve_rows / k_serve_reset): a queue of requests behind the n lanes of a call. A request as the device
// reads it: its draw row -- the request's settings, with (rwkv_mi_batch_serve_ex) its guide's table and its bias slot's table, both only read;
// the counter, the occurrence row and the guide words are the LANE's, patched in at admission -- its stop row, its prompt (prompt_len tokens at
// prompts[prompt0 ..]) and the buffer its start state is copied from.
struct ServeReq { DrawRow row; StopRow stop; uint32_t prompt_len, prompt0; const float * start; };

}  // namespace rwkvmi
