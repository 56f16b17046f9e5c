"""The ring kernel's consumer waves read their share of the geometry from a table the host fills once (csrc/ring_geom.h, rg_wave): the
first record, the record count, the stream offset and the continuation of every (workgroup, consumer wave, phase). A small C++ program
(tests/cpp/ring_wave_check.cpp) checks every entry against the rg_* functions -- D = 2048 / 2560 / 4096, the five formats' block shapes,
several ring sizes -- and the division-free ring offsets the kernel derives from it over 32 layers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_wave_table_equals_the_geometry_functions(tmp_path):
    exe = str(tmp_path / "ring_wave_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ring_wave_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ring wave table OK" in r.stdout
