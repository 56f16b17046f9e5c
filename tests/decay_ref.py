"""The arithmetic of a penalised draw with a repetition setting (include/rwkv_mi355x.h, "Penalty decay and repetition penalty"), performed
literally in NumPy float32: what the draw reads, and what a recorded draw leaves in the occurrence row. tests/test_gpu_decay.py holds the
device to these statements bit for bit; nothing here is fitted to the device.

An occurrence row travels as uint32 WORDS, as the device keeps it: the bit patterns of floats on a decaying sequence (decay != 1), counts on
any other."""
import numpy as np

F = np.float32


def is_decaying(decay):
    return F(decay) != F(1.0)


def occurrences(words, decay):
    """o[j] as float32: the row's floats on a decaying sequence, (float) count[j] elsewhere."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    return words.view(np.float32).copy() if is_decaying(decay) else words.astype(np.float32)


def words_of(o):
    """float32 occurrences as the words of a decaying row"""
    return np.ascontiguousarray(o, dtype=np.float32).view(np.uint32).copy()


def adjusted(logits, words, presence, frequency, decay, repetition, bias=None):
    """What the draw reads instead of the logits:
        a = l[j]
        if (o[j] > 0) { a = a > 0 ? a / repetition : a * repetition;  a = a - (presence + o[j] * frequency); }
        if (bias)       a = a + bias[j]
    every operation rounded to float32 in this order."""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    o = occurrences(words, decay)
    rep, pres, freq = F(repetition), F(presence), F(frequency)
    with np.errstate(all="ignore"):
        scaled = np.where(l > F(0.0), l / rep, l * rep).astype(np.float32)   # (0, -0, NaN and -inf take the multiply)
        penalty = (pres + (o * freq).astype(np.float32)).astype(np.float32)
        a = np.where(o > F(0.0), (scaled - penalty).astype(np.float32), l).astype(np.float32)
        if bias is not None:
            a = (a + np.ascontiguousarray(bias, dtype=np.float32)).astype(np.float32)
    return a


def recorded(words, decay, pick, record=True):
    """The row after the draw picked `pick`: a row that does not record is left alone; a decaying one does o[j] = o[j] * decay for every j,
    then o[pick] = o[pick] + 1; any other counts count[pick] += 1."""
    words = np.ascontiguousarray(words, dtype=np.uint32).copy()
    if not record:
        return words
    if not is_decaying(decay):
        words[pick] += np.uint32(1)
        return words
    with np.errstate(all="ignore"):
        o = (words.view(np.float32) * F(decay)).astype(np.float32)   # (subnormals kept)
        o[pick] = o[pick] + F(1.0)
    return words_of(o)


def counts_add(words, decay, tokens):
    """counts_add: the two statements of `recorded` once per token, in the order given."""
    for t in tokens:
        words = recorded(words, decay, int(t))
    return np.ascontiguousarray(words, dtype=np.uint32)
