"""The kernel metadata hipcc emits for a file of rwkv.cpp_amd/csrc, without a GPU: the device side of the file is compiled for gfx950 with the
flags of the product build, once per file per process, and the amdhsa.kernels block of the assembly is read -- nothing else of it.

kernels("sampling.hip") maps a readable key to a Kernel: the kernel's name inside namespace rwkvmi, or (name, template arguments) for an
instantiation whose arguments are integers or booleans -- ("k_draw_rows", (0, 0, 0)). A name that is not of that shape is its own key."""
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD")

Kernel = collections.namedtuple("Kernel", "name wg lds private sgprs vgprs spills sgpr_spills")
_FIELDS = (("wg", "max_flat_workgroup_size"), ("lds", "group_segment_fixed_size"), ("private", "private_segment_fixed_size"), ("sgprs", "sgpr_count"),
           ("vgprs", "vgpr_count"), ("sgpr_spills", "sgpr_spill_count"), ("vgpr_spills", "vgpr_spill_count"))
_cache = {}


def have_hipcc():
    return os.path.exists(HIPCC)


def key_of(mangled):
    """_ZN6rwkvmi8k_sampleEPKf... -> "k_sample";  _ZN6rwkvmi11k_draw_rowsILi0ELb1ELb0EEEvPKf... -> ("k_draw_rows", (0, 1, 0))"""
    m = re.match(r"_ZN6rwkvmi(\d+)", mangled)
    if not m:
        return mangled
    at = m.end()
    name, rest = mangled[at:at + int(m.group(1))], mangled[at + int(m.group(1)):]
    t = re.match(r"I((?:L[a-z]\d+E)+)EE", rest)
    if t:
        return name, tuple(int(a) for a in re.findall(r"L[a-z](\d+)E", t.group(1)))
    return name if rest.startswith("E") else mangled


def kernels(src_name):
    """{key: Kernel} of every kernel of csrc/<src_name>; spills: vgpr_spill_count, registers spilled to memory (sgpr_spills: scalars kept in
    vector lanes, which cost no memory)"""
    if src_name in _cache:
        return _cache[src_name]
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", src_name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src_name + ".s")
        cmd = [HIPCC, *FLAGS, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    found = {}
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:   # (one list item per kernel; its .args items are indented further)
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        v = {f: int(re.search(r"^    \." + word + r":\s+(\d+)", entry, re.M).group(1)) for f, word in _FIELDS}
        key = key_of(name)
        assert key not in found, (key, name, found[key].name)
        found[key] = Kernel(name, v["wg"], v["lds"], v["private"], v["sgprs"], v["vgprs"], v["vgpr_spills"], v["sgpr_spills"])
    _cache[src_name] = found
    return found


def named(src_name, name):
    """every kernel of the file with that name: {template arguments, or () for a plain kernel: Kernel}"""
    out = {}
    for key, k in kernels(src_name).items():
        if key == name:
            out[()] = k
        elif isinstance(key, tuple) and key[0] == name:
            out[key[1]] = k
    return out


def budget(src_name, keys, wg=1024):
    """{key: Kernel} of the listed kernels, each of which exists (once: kernels() has one entry per key) and keeps within the budget of a
    1024-thread workgroup -- no private segment, no spills, at most 128 registers per thread -- at the workgroup size wg"""
    found = kernels(src_name)
    missing = [key for key in keys if key not in found]
    assert not missing, (missing, sorted(found, key=str))
    for key in keys:
        k = found[key]
        print(key, k)
        assert k.private == 0 and k.spills == 0, (key, k)
        assert k.vgprs <= 128, (key, k, "1024 threads per workgroup leave 128 registers per thread")
        assert k.wg == wg, (key, k)
    assert len({found[key].name for key in keys}) == len(keys), keys
    return {key: found[key] for key in keys}


if __name__ == "__main__":
    import sys
    for key, k in sorted(kernels(sys.argv[1] if len(sys.argv) > 1 else "sampling.hip").items(), key=lambda kv: str(kv[0])):
        print(key, "wg", k.wg, "lds", k.lds, "private", k.private, "sgpr", k.sgprs, "vgpr", k.vgprs, "spills", k.spills, "sgpr_spills", k.sgpr_spills)
