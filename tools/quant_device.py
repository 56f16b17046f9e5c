#!/usr/bin/env python3
"""The device weight quantiser (csrc/quant_w.hip) timed on synthetic FP16 files, one JSON line per figure:

  file    rwkv_quantize_model_file (host) against rwkv_mi_quantize_model_file (device), same input, outputs compared byte for byte
  load    a plain load of the quantised file against rwkv_mi_init_from_file_as of the FP16 file, both warm (the files are in the page cache:
          each is loaded once before it is timed), beside a plain load of the FP16 file itself -- it reads the bytes load-as reads
  kernel  k_quant_w alone: this script once more under `rocprofv3 --kernel-trace --stats`, doing only the load-as, and the kernel's rows
          of the statistics next to the bytes it moved (source bytes in, quantised bytes out)

usage: quant_device.py [--models rwkv6-1b6,rwkv6-7b] [--format Q4_0] [--repeat 3] [--dir /tmp] [--out FILE.jsonl] [--no-kernel]"""
import argparse
import csv
import filecmp
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="rwkv6-1b6,rwkv6-7b")
    ap.add_argument("--format", default="Q4_0")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--load-as-only", default=None, help=argparse.SUPPRESS)   # the child under the profiler: the FP16 file to load
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "quant_device.py measures on the GPU: no device is visible"
    torch.cuda.init()
    from gpu_lib import library, synth
    lib = library()
    L = lib.library
    lib.rwkv_set_print_errors(None, False)

    def load(path, fmt=None):
        """seconds of the call, and the payload's seconds and bytes as rwkv_mi_load_stats reports them"""
        import ctypes
        t0 = time.perf_counter()
        ctx = lib.rwkv_init_from_file(path, 1, 0) if fmt is None else lib.rwkv_mi_init_from_file_as(path, 1, 0, fmt)
        wall = time.perf_counter() - t0
        s, b = ctypes.c_double(0), ctypes.c_uint64(0)
        L.rwkv_mi_load_stats(ctx.ptr, ctypes.byref(s), ctypes.byref(b))
        lib.rwkv_free(ctx)
        return wall, s.value, int(b.value)

    if args.load_as_only:
        load(args.load_as_only, args.format)
        return

    sink = open(args.out, "a") if args.out else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for name in args.models.split(","):
        fmt = args.format
        src = os.path.join(args.dir, f"synthetic-{name}-FP16-seed42.bin")
        if not os.path.exists(src):
            synth.write_model(src, synth.CONFIGS[name], "FP16", seed=42)
        host_q, dev_q = src + f".{fmt}.host", src + f".{fmt}.device"
        src_bytes = os.path.getsize(src)
        for r in range(args.repeat):   # host / device / device / host would need two host runs per repeat: the host run is the slow one, once per repeat
            t0 = time.perf_counter(); lib.rwkv_quantize_model_file(src, host_q, fmt); t_host = time.perf_counter() - t0
            t0 = time.perf_counter(); lib.rwkv_mi_quantize_model_file(src, dev_q, fmt); t_dev = time.perf_counter() - t0
            same = filecmp.cmp(host_q, dev_q, shallow=False)
            emit(what="file", model=name, format=fmt, repeat=r, src_bytes=src_bytes, out_bytes=os.path.getsize(dev_q), host_s=round(t_host, 3), device_s=round(t_dev, 3), identical=same)
            assert same, "the device file differs from the host file"
        load(host_q); load(src); load(src, fmt)   # warm: pages in the cache, code objects loaded
        for r in range(args.repeat):
            q, f, a, a2, f2, q2 = load(host_q), load(src), load(src, fmt), load(src, fmt), load(src), load(host_q)
            emit(what="load", model=name, format=fmt, repeat=r, quantised_file_s=[round(q[1], 4), round(q2[1], 4)], fp16_file_s=[round(f[1], 4), round(f2[1], 4)],
                 load_as_s=[round(a[1], 4), round(a2[1], 4)], weight_bytes_quantised=q[2], weight_bytes_load_as=a[2], weight_bytes_fp16=f[2])
        os.remove(dev_q)
        if args.no_kernel:
            continue
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--load-as-only", src, "--format", fmt]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            rows = [row for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for row in csv.DictReader(open(p))]
        for row in rows:
            if "k_quant_w" in row.get("Name", ""):
                emit(what="kernel", model=name, format=fmt, name=row["Name"][:96], calls=int(row["Calls"]), total_ns=int(float(row["TotalDurationNs"])),
                     note="bytes in: the selected tensors' FP16 payload; bytes out: weight_bytes_load_as less the tensors that load as they are")


if __name__ == "__main__":
    main()
