#!/usr/bin/env python3
"""The receiver side of the many-small-files workload (BASELINE C4: 10 000 x 1 MiB files, block
size 4096, one inserted byte and 16 substitutions per file), measured two ways in one process:

  loop   one sydelta_apply_delta_device call per file (device.apply_device), the only form
         there was before the batched call;
  batch  one sydelta_apply_delta_batch_device call (device.apply_batch).

    python tools/apply_batch_bench.py [--files 10000] [--size 1048576] [--warmup 1] [--reps 5]
                                      [--loop-reps 3] [--out profiles/apply_batch_bench.json]

The deltas come from delta_pairs_handle.  Both forms rebuild every source; the batch's output
is compared with the sources once, before any timing.  Times are host clocks around calls
that end in a stream synchronise; the repetitions of the two forms are interleaved (each
loop repetition is followed by its share of the batch repetitions) and the median is reported
with min and max.  `hbm_frac` is 2 x output bytes (read + written) over the batch call's
median, as a fraction of bench.py's HBM peak; it is a whole-call rate, not the kernel's share
of peak.  `kernel_ms` is the union of the library's event pairs around the call's kernels in
a profiled pass of its own, and `host_ms_outside_kernels` the call's median minus it.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merged_runs(np, d):
    """Runs the batched call makes of a delta: ops with b > 0, neighbours of one kind with
    contiguous sources merged."""
    nz = np.asarray(d.b) > 0
    k, a, b = np.asarray(d.kind)[nz], np.asarray(d.a, dtype=np.uint64)[nz], np.asarray(d.b, dtype=np.uint64)[nz]
    if len(k) < 2:
        return len(k)
    return int(len(k) - ((k[1:] == k[:-1]) & (a[:-1] + b[:-1] == a[1:])).sum())


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apply_batch_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("apply_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev

    nf, fsz, bs = a.files, a.size, a.block_size
    basis, new, (boff, blen, soff, slen) = bench.c4_files(dev, basis_bytes=fsz, nfiles=nf, first=0)
    stride = int(soff[1] - soff[0]) if nf > 1 else new.numel()
    batch = dev.delta_pairs_handle(basis, boff, blen, new, soff, slen, bs)
    deltas = batch.deltas()
    nops = sum(len(d.kind) for d in deltas)
    runs = [merged_runs(np, d) for d in deltas]
    out_bytes = int(slen.sum())
    out = torch.zeros_like(new)
    one = torch.empty(fsz + 1 + 16, dtype=torch.uint8, device="cuda")
    bviews = [basis[int(boff[f]):int(boff[f] + blen[f])] for f in range(nf)]
    sviews = [new[int(soff[f]):int(soff[f] + slen[f])] for f in range(nf)]

    def run_batch():
        t0 = time.perf_counter()
        dev.apply_batch(basis, boff, blen, batch, new, soff, slen, out=out, ooffs=soff)
        return (time.perf_counter() - t0) * 1e3

    def run_loop():
        t0 = time.perf_counter()
        for f in range(nf):
            dev.apply_device(bviews[f], deltas[f], sviews[f], out=one)
        return (time.perf_counter() - t0) * 1e3

    # the data, once
    run_batch()
    torch.cuda.synchronize()
    L = fsz + 1
    if nf > 1:
        same = torch.equal(out[:nf * stride].view(nf, stride)[:, :L], new[:nf * stride].view(nf, stride)[:, :L])
    else:
        same = torch.equal(out[:L], new[:L])
    assert same, "the batch's output differs from the sources"
    rebuilt, _ = dev.apply_device(bviews[nf - 1], deltas[nf - 1], sviews[nf - 1], out=one)
    assert torch.equal(rebuilt, sviews[nf - 1]), "the loop's output differs from the source"

    for _ in range(a.warmup):
        run_batch()
    loop_ms, batch_ms = [], []
    for r in range(max(a.loop_reps, 1)):
        if r < a.loop_reps:  # --loop-reps 0: the batch alone
            loop_ms.append(run_loop())
        for _ in range(a.reps):
            batch_ms.append(run_batch())
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

    gbs = 2 * out_bytes / (ba["median"] * 1e-3) / 1e9
    res = {"tool": "apply_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "ops": nops, "ops_per_file": round(nops / nf, 1),
           "merged_runs_per_file": round(sum(runs) / nf, 2), "merged_runs_max": max(runs), "output_bytes": out_bytes,
           "loop_ms": lo, "batch_ms": ba, "loop_over_batch": round(lo["median"] / ba["median"], 1) if lo else None,
           "batch_GBps_read_plus_written": round(gbs, 1), "hbm_peak_GBps": bench.HBM_PEAK_GBS,
           "hbm_frac": round(gbs / bench.HBM_PEAK_GBS, 4), "kernel_ms": round(kernel_ms, 3),
           "kernel_launches_per_call": launches,
           "host_ms_outside_kernels": round(ba["median"] - kernel_ms, 3), "verified": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
