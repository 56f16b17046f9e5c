"""Guides on the host (include/rwkv_mi355x.h, guided decoding): a guide is a deterministic automaton over token ids, here a list with one
{token: next_state} dict per state, which is what RWKVBatch.create_guide takes. mask(state) and step(state, tok) restate the two halves of a
guided draw -- which tokens read their own value and not -inf, and where the state goes afterwards (a dead pick: it stays, one miss) -- for
tests/test_gpu_guide.py, which holds the device to them; the builders below make the automata those tests run under."""
import numpy as np

DEAD = None   # step()'s next state after a dead pick is the state itself; this names the transition table's dead entry


class Guide:
    def __init__(self, edges, n_vocab):
        self.edges = [dict((int(k), int(v)) for k, v in e.items()) for e in edges]
        self.n_vocab = int(n_vocab)
        self.n_states = len(self.edges)
        check(self)

    def mask(self, state):
        """bool [n_vocab]: True where next(state, token) is a state"""
        m = np.zeros(self.n_vocab, dtype=bool)
        m[list(self.edges[state].keys())] = True
        return m

    def step(self, state, tok):
        """(next state, misses added) after the draw of `tok` in `state`"""
        nxt = self.edges[state].get(int(tok), DEAD)
        return (state, 1) if nxt is DEAD else (nxt, 0)

    def walk(self, state, tokens):
        """(state, misses) after the draws of `tokens` from `state`"""
        misses = 0
        for t in tokens:
            state, m = self.step(state, t)
            misses += m
        return state, misses

    def csr(self):
        """(edge_begin [n_states + 1], edge_tokens, edge_next) as uint32 arrays, each state's tokens ascending"""
        begin, toks, nxt = [0], [], []
        for e in self.edges:
            for t in sorted(e):
                toks.append(t)
                nxt.append(e[t])
            begin.append(len(toks))
        return tuple(np.asarray(a, dtype=np.uint32) for a in (begin, toks, nxt))

    def dense(self):
        """uint16 [n_states][n_vocab], 0xFFFF for dead: the table the device holds"""
        t = np.full((self.n_states, self.n_vocab), 0xFFFF, dtype=np.uint16)
        for s, e in enumerate(self.edges):
            for k, v in e.items():
                t[s, k] = v
        return t


def check(g):
    """the rules of rwkv_mi_batch_guide_create"""
    assert 1 <= g.n_states <= 65535
    for s, e in enumerate(g.edges):
        assert len(e) >= 1, ("a state without an edge", s)
        for k, v in e.items():
            assert 0 <= k < g.n_vocab and 0 <= v < g.n_states, (s, k, v)


def random_guide(n_vocab, n_states, seed, allow=0.5):
    """every state allows about `allow` of the vocabulary (at least one token), each edge to a random state"""
    rng = np.random.default_rng(seed)
    edges = []
    for _ in range(n_states):
        toks = np.flatnonzero(rng.random(n_vocab) < allow)
        if toks.size == 0:
            toks = rng.integers(0, n_vocab, size=1)
        edges.append({int(t): int(n) for t, n in zip(toks, rng.integers(0, n_states, size=toks.size))})
    return Guide(edges, n_vocab)


def chain_guide(n_vocab, tokens):
    """state i allows tokens[i] alone and leads to state i + 1 (the last one back to 0): the guide forces the string, over and over"""
    n = len(tokens)
    return Guide([{int(t): (i + 1) % n} for i, t in enumerate(tokens)], n_vocab)


def all_allowed_guide(n_vocab, n_states=1):
    """every token allowed in every state; state s leads to (s + token) % n_states"""
    return Guide([{t: (s + t) % n_states for t in range(n_vocab)} for s in range(n_states)], n_vocab)
