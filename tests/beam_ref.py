"""The reference of the beam search's selection rule (include/rwkv_mi355x.h, rwkv_mi_batch_decode_beam), in NumPy, working from the per-row lists
of (ids, float32 log-probs) the report kernel gives at top_n = W. tests/test_cpu_beam_ref.py holds it to a hand-written table; tests/test_gpu_beam.py
holds the device to it, bit for bit.

One step of one group of W hypotheses:
  * a live hypothesis i with a finite score offers its W candidates (ids[i][k], lps[i][k]), k = its rank, with the cumulative score
    float64(score[i]) + float64(lps[i][k]); not a candidate without a token (NO_TOKEN) or whose log-prob is not above -inf (-inf, NaN);
  * a finished hypothesis with a finite score offers itself once (rank 0): the same score, no token;
  * a score of -inf offers nothing;
  * the W best by score descending, then parent ascending, then rank ascending become hypotheses 0 .. W - 1; a selected token that is one of
    end_tokens finishes its hypothesis;
  * where fewer than W candidates exist the remaining hypotheses are dead: score -inf, parent = itself, finished, no token, length 0.
A step without a token records the log-prob 0."""
import numpy as np

NO_TOKEN = 0xFFFFFFFF


def step(ids, lps, scores, finished, lens, end_tokens=()):
    """ids uint32 [W][W], lps float32 [W][W], scores float64 [W], finished [W], lens [W] of one group ->
    (tokens uint32 [W], parents uint32 [W], logprobs float32 [W], scores float64 [W], finished uint32 [W], lens uint32 [W])."""
    ids = np.asarray(ids, dtype=np.uint32)
    lps = np.asarray(lps, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float64)
    W = scores.size
    cands = []   # (score, parent, rank, token or NO_TOKEN, lp)
    for i in range(W):
        if not scores[i] > -np.inf:
            continue
        if finished[i]:
            cands.append((scores[i], i, 0, NO_TOKEN, np.float32(0.0)))
            continue
        for k in range(W):
            if int(ids[i, k]) != NO_TOKEN and lps[i, k] > -np.inf:
                cands.append((np.float64(scores[i]) + np.float64(lps[i, k]), i, k, int(ids[i, k]), lps[i, k]))
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    tok = np.full(W, NO_TOKEN, dtype=np.uint32)
    par = np.arange(W, dtype=np.uint32)
    lp = np.zeros(W, dtype=np.float32)
    sc = np.full(W, -np.inf, dtype=np.float64)
    fin = np.ones(W, dtype=np.uint32)
    ln = np.zeros(W, dtype=np.uint32)
    ends = {int(e) for e in end_tokens}
    for j, (s, i, k, t, l) in enumerate(cands[:W]):
        par[j], sc[j] = i, s
        if t == NO_TOKEN:   # a finished hypothesis, carried
            ln[j] = lens[i]
            continue
        tok[j], lp[j], ln[j] = t, l, int(lens[i]) + 1
        fin[j] = 1 if t in ends else 0
    return tok, par, lp, sc, fin, ln


def start(W):
    """the words a group starts with: scores {0, -inf, ...}, nothing finished, no length"""
    sc = np.full(W, -np.inf, dtype=np.float64)
    sc[0] = 0.0
    return sc, np.zeros(W, dtype=np.uint32), np.zeros(W, dtype=np.uint32)


def backtrace(hist_tok, hist_par, hist_lp, scores, n_tokens):
    """The texts of the W hypotheses of the last selection from the history [steps][W] of one group: (tokens uint32 [W][n_tokens] with NO_TOKEN
    past a hypothesis' length, lens uint32 [W], logprobs float32 [W][n_tokens] with 0 past it). A dead hypothesis (score -inf) has no text."""
    hist_tok, hist_par, hist_lp = np.asarray(hist_tok), np.asarray(hist_par), np.asarray(hist_lp)
    steps, W = hist_tok.shape
    tokens = np.full((W, n_tokens), NO_TOKEN, dtype=np.uint32)
    lps = np.zeros((W, n_tokens), dtype=np.float32)
    lens = np.zeros(W, dtype=np.uint32)
    for j in range(W):
        if not scores[j] > -np.inf:
            continue
        text, at = [], j
        for i in range(steps - 1, -1, -1):
            if int(hist_tok[i, at]) != NO_TOKEN:
                text.append((int(hist_tok[i, at]), hist_lp[i, at]))
            at = int(hist_par[i, at])
        text.reverse()
        lens[j] = len(text)
        for i, (t, l) in enumerate(text):
            tokens[j, i], lps[j, i] = t, l
    return tokens, lens, lps


def search(candidates, first_token, W, n_tokens, end_tokens=()):
    """A whole search of one group over a model given as candidates(fed tokens [W], parents [W] or None at the start, live [W]) -> (ids [W][W],
    lps [W][W]): the per-row lists of the step, row j continuing parent parents[j] with the token fed[j]. Returns (tokens, lens, scores, logprobs,
    steps run, parents of the last step, finished)."""
    sc, fin, ln = start(W)
    fed = np.full(W, first_token, dtype=np.uint32)
    par = None
    ht, hp, hl = [], [], []
    while len(ht) < n_tokens:
        live = [bool(sc[j] > -np.inf and not fin[j]) for j in range(W)]
        ids, lps = candidates(fed, par, live)
        tok, par, lp, sc, fin, ln = step(ids, lps, sc, fin, ln, end_tokens)
        fed = np.where(tok != NO_TOKEN, tok, fed[par])
        ht.append(tok); hp.append(par); hl.append(lp)
        if fin.all():
            break
    tokens, lens, lps_out = backtrace(ht, hp, hl, sc, n_tokens)
    assert np.array_equal(lens, ln)
    return tokens, lens, sc, lps_out, len(ht), par, fin
