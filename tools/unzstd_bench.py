#!/usr/bin/env python3
"""zstd frames decoded on the device (sydelta_zstd_decompress_device), measured: the Delta JSON
text of a C3b-shaped delta (block Copies at 4 KiB, a whole literal block in 5% of them) and of
a C5-shaped one (consecutive 8 KiB Copies, 300 literal bytes every 97 ops), each as the frame
libzstd writes when streamed at level 3 (the real sender), as our own encoder's frame, and
as libzstd's level-19 frame of a prefix.  Prints one JSON line.

    python tools/unzstd_bench.py [--mib 256] [--prefix-mib 64] [--warmup 2] [--reps 10] [--out FILE]

The texts are written on the device (delta_to_json_device) from synthetic op tables.  Every
frame's output is compared with its text before any timing.  Rates are GiB of regenerated
text over HIP-event time around one call into a preallocated output (median of the timed
calls, with their min and max); `cpu_baseline` is ZSTD_decompress of the same frame on one
host thread in the same run (the better of 2 calls); `text_mib` is what was asked for, every
text is at least that long and its entry has its `text_bytes`; `kernel_ms` the library's own
event pairs around each stage, in passes of their own.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def c3b_ops(np, text_bytes):
    per = 0.05 * (4096 * 3.57 + 12) + 0.95 * 48
    n = int(text_bytes / per) + 1
    rng = np.random.default_rng(3)
    data = rng.random(n) < 0.05
    kind = data.astype(np.uint32)
    a = np.arange(n, dtype=np.uint64) * np.uint64(4096)
    lit_off = np.cumsum(np.where(data, 4096, 0)).astype(np.uint64) - np.where(data, 4096, 0).astype(np.uint64)
    a = np.where(data, lit_off, a)
    b = np.full(n, 4096, dtype=np.uint64)
    return kind, a, b, n * 4096, 4096, int(data.sum()) * 4096


def c5_ops(np, text_bytes):
    n = int(text_bytes / 56) + 1
    k = np.arange(n)
    data = (k % 97) == 0
    kind = data.astype(np.uint32)
    lit_off = (np.cumsum(np.where(data, 300, 0)) - np.where(data, 300, 0)).astype(np.uint64)
    a = np.where(data, lit_off, k.astype(np.uint64) * np.uint64(8192))
    b = np.where(data, 300, 8192).astype(np.uint64)
    return kind, a, b, n * 8192, 8192, int(data.sum()) * 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--prefix-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("unzstd_bench needs a GPU")
    import sy_amd.device as dev
    import zstd_frames as F
    from sy_amd import wire

    z = F._z()
    res = {"tool": "unzstd_bench", "text_mib": a.mib, "prefix_mib": a.prefix_mib, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "libzstd": z.ZSTD_versionNumber()}

    def measure(frame_t, text_t):
        n = text_t.numel()
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        got = wire.zstd_decompress_device(frame_t, out=out)
        assert got.numel() == n and torch.equal(got, text_t), "decoded text differs"
        for _ in range(a.warmup):
            wire.zstd_decompress_device(frame_t, out=out)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            wire.zstd_decompress_device(frame_t, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        r = {"frame_bytes": frame_t.numel(), "text_bytes": n, "call_ms_median": round(med, 3),
             "call_ms_min": round(ms[0], 3), "call_ms_max": round(ms[-1], 3),
             "GiBps": round(n / med / 1e-3 / 2**30, 3)}
        dev.set_profiling(True)
        try:
            dev.profile(reset=True)
            for _ in range(3):
                wire.zstd_decompress_device(frame_t, out=out)
            prof = dev.profile(reset=True)
            r["kernel_ms"] = {k: round(v["ms"] / 3, 3) for k, v in prof.items() if not k.startswith("__")}
        finally:
            dev.set_profiling(False)
        # one host thread on the same frame
        fb = frame_t.cpu().numpy().tobytes()
        dst = ctypes.create_string_buffer(n)
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            rc = z.ZSTD_decompress(dst, n, fb, len(fb))
            dt = time.perf_counter() - t0
            assert rc == n
            best = dt if best is None else min(best, dt)
        r["cpu_baseline"] = {"ms": round(best * 1e3, 3), "GiBps": round(n / best / 2**30, 3)}
        r["device_over_cpu"] = round(best * 1e3 / med, 3)
        return r

    for shape, make in (("c3b", c3b_ops), ("c5", c5_ops)):
        want = a.mib << 20
        ask = want
        while True:  # the op count comes from an estimate of the text per op: ask for more until it reaches
            kind, oa, ob, ss, bs, nlit = make(np, ask)
            lit = torch.empty(max(nlit, 1), dtype=torch.uint8, device="cuda")
            dev.synth_fill(lit, 0x5E1D0C07)
            text = wire.delta_to_json_device(kind, oa, ob, ss, bs, lit)
            del lit
            if text.numel() >= want:
                break
            ask = int(ask * (want / text.numel()) * 1.01) + 4096
            del text
        host_text = text.cpu().numpy().tobytes()
        entry = {"ops": int(len(kind)), "text_bytes": len(host_text)}
        f3 = torch.frombuffer(bytearray(F.stream_compress(host_text, 3)), dtype=torch.uint8).cuda()
        entry["libzstd_stream_l3"] = measure(f3, text)
        own = wire.zstd_compress_device(text).clone()
        entry["own_encoder"] = measure(own, text)
        pre = min(len(host_text), a.prefix_mib << 20)
        f19 = torch.frombuffer(bytearray(F.stream_compress(host_text[:pre], 19)), dtype=torch.uint8).cuda()
        entry["libzstd_stream_l19_prefix"] = measure(f19, text[:pre])
        res[shape] = entry
        del text, f3, own, f19
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
