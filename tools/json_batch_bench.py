#!/usr/bin/env python3
"""The sender's wire text of the many-small-files workload (BASELINE C4: 10 000 x 1 MiB files,
block size 4096, one inserted byte and 16 substitutions per file), measured two ways in one
process:

  loop   one sydelta_delta_to_json_device call per file, the only form there was before the
         batched call (each call straight on the batch's own delta, into a buffer that holds
         the text: one call per file, no sizing pass);
  batch  one sydelta_delta_batch_to_json_device call (wire.delta_batch_to_json_device).

    python tools/json_batch_bench.py [--files 10000] [--size 1048576] [--warmup 1] [--reps 5]
                                     [--loop-reps 3] [--out profiles/json_batch_bench.json]

The deltas come from delta_pairs_handle.  The batch's texts are compared with the loop's once,
before any timing.  Times are host clocks around calls that end in a stream synchronise; the
repetitions of the two forms are interleaved (each loop repetition is followed by its share
of the batch repetitions) and the median is reported with min and max.  `hbm_frac` is
(literal bytes read + text bytes written) over the batch call's median, as a fraction of
bench.py's HBM peak; it is a whole-call rate, not the kernels' share of peak.  `kernel_ms` is
the union of the library's event pairs around the call's kernels in a profiled pass of its own,
and `host_ms_outside_kernels` the call's median minus it.  `bar_met` says whether the batch's
median is below the loop's minimum.  Prints one JSON line and writes it to --out.
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5, help="batch calls timed per loop repetition")
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_batch_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("json_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev
    from sy_amd import wire
    from sy_amd._lib import check, lib

    nf, fsz, bs = a.files, a.size, a.block_size
    basis, new, (boff, blen, soff, slen) = bench.c4_files(dev, basis_bytes=fsz, nfiles=nf, first=0)
    batch = dev.delta_pairs_handle(basis, boff, blen, new, soff, slen, bs)
    del basis
    ptrs = (ctypes.c_void_p * nf)()
    assert int(lib.sydelta_delta_batch_ptrs(batch.h, ptrs, nf)) == nf
    nops = sum(int(lib.sydelta_delta_num_ops(ptrs[f])) for f in range(nf))
    bound = int(lib.sydelta_delta_batch_to_json_bound(ptrs, nf))
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    stream = int(torch.cuda.current_stream().cuda_stream)
    sptr = [new.data_ptr() + int(soff[f]) for f in range(nf)]
    slen_i = [int(x) for x in slen]

    def run_batch():
        t0 = time.perf_counter()
        res = wire.delta_batch_to_json_device(batch, new, soff, slen, out=out)
        return (time.perf_counter() - t0) * 1e3, res

    def run_loop(toffs, caps):
        """Every text to where the batch put it (toffs; caps: the room up to the next text)."""
        n = ctypes.c_uint64()
        lens = []
        base = out.data_ptr()
        t0 = time.perf_counter()
        for f in range(nf):
            check(lib.sydelta_delta_to_json_device(ptrs[f], sptr[f], slen_i[f], base + toffs[f], caps[f], ctypes.byref(n),
                                                   stream))
            lens.append(n.value)
        return (time.perf_counter() - t0) * 1e3, lens

    # the data, once: the loop's texts against the batch's
    # (neither form touches the pad bytes between texts: they stay zero in both images)
    out.zero_()
    _, (packed, toffs, tlens) = run_batch()
    torch.cuda.synchronize()
    need = packed.numel()
    want = packed.clone()
    toffs_i = [int(x) for x in toffs]
    caps = [(toffs_i[f + 1] if f + 1 < nf else need) - toffs_i[f] for f in range(nf)]
    out.zero_()
    _, lens = run_loop(toffs_i, caps)
    torch.cuda.synchronize()
    assert lens == [int(x) for x in tlens], "the loop's text lengths differ from the batch's"
    assert torch.equal(out[:need], want), "the batch's texts differ from the loop's"
    del want
    literal = 0
    for f in range(nf):
        st = dev._lib.MatchStatsC()
        check(lib.sydelta_delta_stats(ptrs[f], ctypes.byref(st)))
        literal += int(st.literal_bytes)
    text_bytes = int(tlens.sum())

    for _ in range(a.warmup):
        run_batch()
    loop_ms, batch_ms = [], []
    for r in range(max(a.loop_reps, 1)):
        if r < a.loop_reps:  # --loop-reps 0: the batch alone
            loop_ms.append(run_loop(toffs_i, caps)[0])
        for _ in range(a.reps):
            batch_ms.append(run_batch()[0])
    lo, ba = stats_of(loop_ms), stats_of(batch_ms)

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

    gbs = (literal + text_bytes) / (ba["median"] * 1e-3) / 1e9
    res = {"tool": "json_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "ops": nops, "ops_per_file": round(nops / nf, 1), "literal_bytes": literal,
           "text_bytes": text_bytes, "arena_bound_bytes": bound, "loop_ms": lo, "batch_ms": ba,
           "loop_over_batch": round(lo["median"] / ba["median"], 1) if lo else None,
           "bar_met": bool(ba["median"] < lo["min"]) if lo else None,
           "batch_GBps_read_plus_written": round(gbs, 1), "hbm_peak_GBps": bench.HBM_PEAK_GBS,
           "hbm_frac": round(gbs / bench.HBM_PEAK_GBS, 4), "kernel_ms": round(kernel_ms, 3),
           "kernel_ms_by_name": per_kernel, "kernel_share": round(kernel_ms / ba["median"], 3),
           "kernel_launches_per_call": launches,
           "host_ms_outside_kernels": round(ba["median"] - kernel_ms, 3), "verified": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    batch.close()


if __name__ == "__main__":
    main()
