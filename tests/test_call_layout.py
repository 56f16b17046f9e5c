"""The staged-table layouts of the batch calls (csrc/call_layout.h) are host code without a HIP include: their invariants are checked on
the CPU by a small C++ program (tests/cpp/call_layout_check.cpp) -- every field aligned to its type, fields disjoint and in declaration
order, no padding, every offset what the hand-made layouts gave before the cursor existed, what a call copies inside the range it
copies, and a cursor that pads a field declared in the wrong place."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_layout_invariants(tmp_path):
    exe = str(tmp_path / "call_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "call_layout_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "call layouts OK" in r.stdout
