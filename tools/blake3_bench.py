#!/usr/bin/env python3
"""BLAKE3 on the device, measured: one large file, and the files of `bench.py --workload xxh3`
(--files equal files over the same bytes), each beside XXH3-64 of the same bytes in the same
process.  Prints one JSON line.

    python tools/blake3_bench.py [--gib 4] [--files 4096] [--warmup 2] [--reps 5] [--out FILE]

Call times are HIP events around the whole call (tables, launches, the copy of the hashes
back) on the caller's stream; kernel times are the library's own event pairs around each
kernel (set_profiling), taken in passes of their own.  Rates are file bytes over time.

Yardsticks (estimates): the ALU ceiling is 7 rounds x 8 G x 12 VALU operations per
64-byte block plus 1/16 for the tree, over 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz; the copy
rate and k_sig_fast's rate are the project's measured 6.29 and 6.3 TB/s.  What the vector
ALU really sustains on this instruction mix is measured by tools/micro_b3_alu.hip.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ALU_OPS_PER_BYTE = 7 * 8 * 12 / 64 * (1 + 1 / 16)
ALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
ALU_CEILING = ALU_LANE_OPS_PER_S / ALU_OPS_PER_BYTE  # bytes / s
COPY_RATE = 6.29e12
SIG_FAST_RATE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("blake3_bench needs a GPU")
    import sy_amd.device as dev

    n = int(a.gib * (1 << 30))
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev.synth_fill(buf, 0x5E1D0B03)
    fsz = n // a.files
    offs = np.arange(a.files, dtype=np.uint64) * np.uint64(fsz)
    lens = np.full(a.files, fsz, dtype=np.uint64)
    one_off, one_len = np.zeros(1, np.uint64), np.full(1, n, np.uint64)
    work = {
        "blake3_one": (lambda: dev.blake3(buf), n),
        "xxh3_one": (lambda: dev.xxh3_batch(buf, one_off, one_len), n),
        "blake3_files": (lambda: dev.blake3_batch(buf, offs, lens), fsz * a.files),
        "xxh3_files": (lambda: dev.xxh3_batch(buf, offs, lens), fsz * a.files),
    }
    res = {"tool": "blake3_bench", "bytes": n, "files": a.files, "file_bytes": fsz, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    results = {}
    for name, (fn, nbytes) in work.items():
        for _ in range(a.warmup):
            results[name] = fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            results[name] = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        res[name] = {"call_ms_median": round(med, 4), "call_ms_min": round(ms[0], 4), "call_ms_max": round(ms[-1], 4),
                     "call_GBps": round(nbytes / med / 1e6, 1)}
    # the batch and the single file hash the same bytes file by file
    assert bytes(results["blake3_files"][0]) == dev.blake3(buf[:fsz])
    # kernel times, in passes of their own
    dev.set_profiling(True)
    try:
        for name, (fn, nbytes) in work.items():
            dev.profile(reset=True)
            for _ in range(a.reps):
                fn()
            prof = dev.profile(reset=True)
            kern = {k: round(v["ms"] / a.reps, 4) for k, v in prof.items() if not k.startswith("__")}
            res[name]["kernel_ms"] = kern
            res[name]["kernels_GBps"] = round(nbytes / sum(kern.values()) / 1e6, 1)
    finally:
        dev.set_profiling(False)
    chunks_ms = res["blake3_one"]["kernel_ms"]["k_b3_chunks"]
    rate = n / chunks_ms / 1e6 * 1e9
    res["k_b3_chunks_GBps"] = round(rate / 1e9, 1)
    res["yardsticks"] = {
        "alu_ops_per_byte": round(ALU_OPS_PER_BYTE, 3),
        "alu_ceiling_GBps": round(ALU_CEILING / 1e9, 1),
        "k_b3_chunks_over_alu_ceiling": round(rate / ALU_CEILING, 4),
        "k_b3_chunks_over_copy_rate": round(rate / COPY_RATE, 4),
        "k_b3_chunks_over_k_sig_fast": round(rate / SIG_FAST_RATE, 4),
        "blake3_over_xxh3_one_file_call": round(res["xxh3_one"]["call_ms_median"] / res["blake3_one"]["call_ms_median"], 4),
        "blake3_over_xxh3_files_call": round(res["xxh3_files"]["call_ms_median"] / res["blake3_files"]["call_ms_median"], 4),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
