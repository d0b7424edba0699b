#!/usr/bin/env python3
"""The sender's compressed wire bytes of the many-small-files workload (BASELINE C4: 10 000 x
1 MiB files, block size 4096, one inserted byte and 16 substitutions per file), measured two
ways in one process:

  loop   one sydelta_zstd_compress_device call per text, the only form there was before the
         batched call, timed on the first --loop-files texts and extrapolated to the batch by
         the file count (the texts are alike); labelled as extrapolated in the result;
  batch  one sydelta_zstd_compress_batch_device call (wire.zstd_compress_batch_device).

    python tools/zstd_batch_bench.py [--files 10000] [--size 1048576] [--warmup 2] [--reps 10]
                                     [--loop-files 200] [--loop-reps 3]
                                     [--out profiles/zstd_batch_bench.json]

The deltas come from delta_pairs_handle, the texts from delta_batch_to_json_device.  The loop's
frames are compared with the batch's on the subset once, before any timing.  Times are host
clocks around calls that end in a stream synchronise; the median is reported with min and max.
`text_GiBps` is the text's bytes over the batch call's median.  `kernel_ms` is the union of the
library's event pairs around the call's kernels in a profiled pass of its own, and
`host_ms_outside_kernels` the call's median minus it (the placement scans are not among the
profiled kernels, so their time counts as outside).  `bar_met` says whether the batch's median
is below the loop's fastest extrapolated repetition.  Prints one JSON line and writes it to
--out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats_of(ms):
    ms = sorted(ms)
    if not ms:
        return None
    return {"median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3), "max": round(ms[-1], 3), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10000)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-files", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_batch_bench.json"))
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("zstd_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev
    from sy_amd import wire
    from sy_amd._lib import check, lib

    nf, fsz, bs = a.files, a.size, a.block_size
    basis, new, (boff, blen, soff, slen) = bench.c4_files(dev, basis_bytes=fsz, nfiles=nf, first=0)
    batch = dev.delta_pairs_handle(basis, boff, blen, new, soff, slen, bs)
    del basis
    packed, toffs, tlens = wire.delta_batch_to_json_device(batch, new, soff, slen)
    text = packed.clone()  # trimmed: the bound's arena goes back
    batch.close()
    del packed, new
    torch.cuda.empty_cache()
    text_bytes = int(tlens.sum())
    blocks = int(sum(max(1, -(-int(n) // (128 << 10))) for n in tlens))
    bound = int(lib.sydelta_zstd_batch_bound(tlens.ctypes.data, nf))
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)

    def run_batch():
        t0 = time.perf_counter()
        res = wire.zstd_compress_batch_device(text, toffs, tlens, out=out)
        return (time.perf_counter() - t0) * 1e3, res

    sub = min(a.loop_files, nf)
    tptr = [text.data_ptr() + int(toffs[f]) for f in range(sub)]
    tlen_i = [int(tlens[f]) for f in range(sub)]
    cap = max(int(lib.sydelta_zstd_bound(n)) for n in tlen_i)
    single = torch.empty(sub * cap, dtype=torch.uint8, device="cuda")

    def run_loop():
        n = ctypes.c_uint64()
        lens = []
        base = single.data_ptr()
        t0 = time.perf_counter()
        for f in range(sub):
            check(lib.sydelta_zstd_compress_device(0, tptr[f], tlen_i[f], base + f * cap, cap, ctypes.byref(n), stream))
            lens.append(n.value)
        return (time.perf_counter() - t0) * 1e3, lens

    # the data, once: the loop's frames against the batch's, on the subset
    _, (frames, foffs, flens) = run_batch()
    _, lens = run_loop()
    torch.cuda.synchronize()
    assert lens == [int(x) for x in flens[:sub]], "the loop's frame lengths differ from the batch's"
    for f in range(sub):
        o = int(foffs[f])
        assert torch.equal(single[f * cap:f * cap + lens[f]], frames[o:o + lens[f]]), f"file {f}: frames differ"
    frame_bytes = frames.numel()

    for _ in range(a.warmup):
        run_batch()
    loop_ms, batch_ms = [], []
    for _ in range(a.loop_reps):
        loop_ms.append(run_loop()[0])
    for _ in range(a.reps):
        batch_ms.append(run_batch()[0])
    lo, ba = stats_of(loop_ms), stats_of(batch_ms)
    scale = nf / sub
    lo_x = {k: (round(v * scale, 1) if k != "n" else v) for k, v in lo.items()} if lo else None

    dev.set_profiling(True)
    try:
        dev.profile(reset=True)
        for _ in range(3):
            run_batch()
        prof = dev.profile(reset=True)
    finally:
        dev.set_profiling(False)
    kernel_ms = prof.get("__busy__", {}).get("ms", 0.0) / 3
    launches = sum(v["count"] for k, v in prof.items() if not k.startswith("__")) / 3
    per_kernel = {k: round(v["ms"] / 3, 3) for k, v in prof.items() if not k.startswith("__") and "ms" in v}
    knob = os.environ.get("SYDELTA_ZSTD_BATCH")
    round_blocks = int(knob) if knob and knob.isdigit() and int(knob) else 4096

    res = {"tool": "zstd_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "text_bytes": text_bytes, "frame_bytes": frame_bytes,
           "ratio": round(text_bytes / frame_bytes, 2), "blocks": blocks, "round_blocks": round_blocks,
           "rounds": -(-blocks // round_blocks), "arena_bound_bytes": bound, "batch_ms": ba,
           "loop_files_timed": sub, "loop_subset_ms": lo, "loop_ms_extrapolated": lo_x,
           "loop_ms_per_file": round(lo["median"] / sub, 3) if lo else None,
           "loop_over_batch": round(lo_x["median"] / ba["median"], 1) if lo else None,
           "bar_met": bool(ba["median"] < lo_x["min"]) if lo else None,
           "text_GiBps": round(text_bytes / (ba["median"] * 1e-3) / 2**30, 2), "kernel_ms": round(kernel_ms, 3),
           "kernel_ms_by_name": per_kernel, "kernel_share": round(kernel_ms / ba["median"], 3),
           "kernel_launches_per_call": launches, "host_ms_outside_kernels": round(ba["median"] - kernel_ms, 3),
           "verified_files": sub}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
