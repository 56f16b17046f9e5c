"""bench.py's command line and its output dump (no GPU: bench.py is imported, nothing is launched). A plain run times the headline only, the
legs beside it wait for --full; --dump-outputs writes what the timed path computed, within 64 MB, the same elements for every build."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(argv):
    saved = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        return b, b.parse_args()
    finally:
        sys.argv = saved


def test_plain_run_leaves_the_side_legs_to_full():
    _, a = _bench(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    _, a = _bench(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_writes_float_arrays_whole_when_they_fit(tmp_path):
    b, _ = _bench([])
    toks = np.arange(5, dtype=np.uint32)
    logits = np.linspace(-1, 1, 11, dtype=np.float32)
    b.dump_outputs(str(tmp_path / "d"), {"tokens": toks, "logits": logits})
    t, lg = np.load(tmp_path / "d" / "tokens.npy"), np.load(tmp_path / "d" / "logits.npy")
    assert t.dtype == np.float64 and np.array_equal(t, toks)
    assert lg.dtype == np.float32 and np.array_equal(lg, logits)


def test_dump_samples_the_same_elements_beyond_the_limit(tmp_path, monkeypatch):
    b, _ = _bench([])
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4000)
    big = np.arange(3000, dtype=np.float32)
    small = np.arange(100, dtype=np.float32)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"state": big, "logits": small})
    sa, sb = np.load(tmp_path / "a" / "state.npy"), np.load(tmp_path / "b" / "state.npy")
    la = np.load(tmp_path / "a" / "logits.npy")
    assert sa.nbytes + la.nbytes <= 4000
    assert np.array_equal(sa, sb) and np.all(np.diff(sa) > 0)
