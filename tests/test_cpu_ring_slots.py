"""The issue slots of k6_ring's row phases are a ratchet, like its register budget (tests/test_cpu_ring_budget.py): per record and per
phase tail, the instructions the compiler emits between the R6REC / R6TAIL markers of rows<> (ring_v6.hip) must not exceed what
profiles/rowsum_slots_new.txt records for the 7B Q4_0 and the 1.6B Q4_0 instantiation -- the recorded values, no slack. A consumer wave
is bound by issue slots, so an instruction more per record is time. tools/ring_slots.py does the counting; the check
compiles ring_v6.hip for gfx950 (device side only, no GPU needed) with the flags of the budget test."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("ring_slots", os.path.join(ROOT, "tools", "ring_slots.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classes_are_read_from_the_mnemonic():
    rs = _tool()
    text = "\n".join([
        "_ZN6rwkvmi7k6_ringILi2ELi8ELi4ELi7ELi3EEEvNS_3R6PE: ; @k",
        "\tv_add_f32_e32 v1, v2, v3", "\t; R6REC 1 0 begin", "\ts_waitcnt lgkmcnt(0)", "\tv_dot4_i32_i8 v1, v2, v3, v1", "\tv_mov_b32_e32 v4, v1",
        ".LBB0_1:", "\tv_add_f32_dpp v1, v1, v1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", "\tds_read_b128 v[0:3], v9", "\ts_cbranch_scc1 .LBB0_1",
        "\t; R6REC 1 0 end", "\tv_readlane_b32 s4, v1, 4", "\t; R6TAIL 1 0 begin", "\tglobal_store_dword v[0:1], v2, off", "\t; R6TAIL 1 0 end", "\ts_endpgm",
        ".Lfunc_end0:", ""])
    c = rs.count(text)[("Q4_0", "7B")]
    assert c["kernel"] == 10
    assert dict(c[("R6REC", 1, 0)]) == {"wait": 1, "arith": 1, "mov": 1, "xlane": 1, "lds": 1, "scalar": 1}
    assert dict(c[("R6TAIL", 1, 0)]) == {"xlane": 1, "vmem": 1}      # (what stands between two brackets of a phase belongs to the second)
    assert rs.parse_table(rs.table(rs.count(text))) == {("7B", "Q4_0", "R6REC", "C", 0): 6, ("7B", "Q4_0", "R6TAIL", "C", 0): 2}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_slots_per_record_and_tail_do_not_exceed_the_recorded_table(tmp_path):
    rs = _tool()
    out = str(tmp_path / "ring.s")
    rs.compile_asm(out)
    now = rs.parse_table(rs.table(rs.count(open(out).read())))
    recorded = rs.parse_table(open(os.path.join(ROOT, "profiles", "rowsum_slots_new.txt")).read())
    assert {k[:2] for k in recorded} == {("7B", "Q4_0"), ("1.6B", "Q4_0")}
    assert set(now) == set(recorded), sorted(set(now) ^ set(recorded))
    over = {k: (now[k], recorded[k]) for k in recorded if now[k] > recorded[k]}
    assert not over, over
