#!/usr/bin/env python3
"""The receiver's first step for the many-small-files workload (BASELINE C4: 10 000 x 1 MiB
files, block size 4096, one inserted byte and 16 substitutions per file): the frames of the
batch's Delta texts decoded two ways in one process:

  loop   one sydelta_zstd_decompress_device call per frame into a preallocated output, the only
         form there was before the batched call, timed on the first --loop-files frames and
         extrapolated to the batch by the file count (the frames are alike); labelled as
         extrapolated in the result;
  batch  one sydelta_zstd_decompress_batch_device call into a preallocated arena.

    python tools/unzstd_batch_bench.py [--files 10000] [--size 1048576] [--warmup 2] [--reps 10]
                                       [--loop-files 200] [--loop-reps 3] [--c3b-mib 256]
                                       [--out profiles/unzstd_batch_bench.json]

The texts come from delta_pairs_handle and delta_batch_to_json_device.  Two sets of frames are
measured: the batched compressor's (`own_encoder`) and libzstd's streamed at level 3, the real
sender (`libzstd_stream_l3`).  Every text of the batch's output is compared with its source
text before any timing.  Times are HIP events around the calls (median of --reps after --warmup,
with min and max).  `kernel_ms` is the union of the library's event pairs around the call's
kernels in a profiled pass of its own, `kernel_ms_by_name` the split, and
`host_ms_outside_kernels` the call's median minus the union.  `c3b_one_frame` decodes one large
frame (a C3b-shaped text of --c3b-mib MiB, libzstd streamed at level 3) as a batch of one and
with the single call, in the same process.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats_of(ms):
    ms = sorted(ms)
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
    ap.add_argument("--c3b-mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unzstd_batch_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("unzstd_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev
    import zstd_frames as F
    from sy_amd import wire
    from sy_amd._lib import check, lib

    nf, fsz, bs = a.files, a.size, a.block_size
    basis, new, (boff, blen, soff, slen) = bench.c4_files(dev, basis_bytes=fsz, nfiles=nf, first=0)
    batch = dev.delta_pairs_handle(basis, boff, blen, new, soff, slen, bs)
    del basis
    packed, toffs, tlens = wire.delta_batch_to_json_device(batch, new, soff, slen)
    text = packed.clone()
    batch.close()
    del packed, new
    torch.cuda.empty_cache()
    text_bytes = int(tlens.sum())
    text_h = text.cpu().numpy()
    stream =int(torch.cuda.current_stream().cuda_stream)

    def timed(fn, warmup, reps):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        st = stats_of(ms)
        st["calls"] = [round(x, 1) for x in ms]  # in the order they ran
        return st

    def profiled(fn):
        dev.set_profiling(True)
        try:
            dev.profile(reset=True)
            for _ in range(3):
                fn()
            prof = dev.profile(reset=True)
        finally:
            dev.set_profiling(False)
        busy = prof.get("__busy__", {}).get("ms", 0.0) / 3
        names = {k: round(v["ms"] / 3, 3) for k, v in prof.items() if not k.startswith("__") and "ms" in v}
        launches = sum(v["count"] for k, v in prof.items() if not k.startswith("__")) / 3
        return busy, names, launches

    def measure(frames, foffs, flens):
        out = torch.empty(text.numel(), dtype=torch.uint8, device="cuda")

        def run_batch():
            return wire.zstd_decompress_batch_device(frames, foffs, flens, out=out)

        got, to, tl = run_batch()
        assert np.array_equal(to, toffs) and np.array_equal(tl, tlens), "the batch's tables differ from the texts'"
        assert got.numel() == text.numel()
        got_h = got.cpu().numpy()
        for f in range(nf):  # the pads are not compared
            o, n = int(toffs[f]), int(tlens[f])
            assert np.array_equal(got_h[o:o + n], text_h[o:o + n]), f"file {f}: decoded text differs"
        out.zero_()
        sub = min(a.loop_files, nf)
        fptr = [frames.data_ptr() + int(foffs[f]) for f in range(sub)]
        flen_i = [int(flens[f]) for f in range(sub)]
        optr = [out.data_ptr() + int(toffs[f]) for f in range(sub)]
        ocap = [int(tlens[f]) for f in range(sub)]

        def run_loop():
            n = ctypes.c_uint64()
            for f in range(sub):
                check(lib.sydelta_zstd_decompress_device(0, fptr[f], flen_i[f], optr[f], ocap[f], ctypes.byref(n), stream))

        run_loop()
        torch.cuda.synchronize()
        got_h = out.cpu().numpy()
        for f in range(sub):
            o, n = int(toffs[f]), int(tlens[f])
            assert np.array_equal(got_h[o:o + n], text_h[o:o + n]), f"file {f}: the loop's text differs"
        ba = timed(run_batch, a.warmup, a.reps)
        lo = timed(run_loop, 1, a.loop_reps)
        scale = nf / sub
        lo_x = {k: (round(v * scale, 1) if k != "n" else v) for k, v in lo.items() if k != "calls"}
        busy, names, launches = profiled(run_batch)
        return {"frame_bytes": int(flens.sum()), "ratio": round(text_bytes / int(flens.sum()), 2), "batch_ms": ba,
                "loop_files_timed": sub, "loop_subset_ms": lo, "loop_ms_extrapolated": lo_x,
                "loop_ms_per_file": round(lo["median"] / sub, 3),
                "loop_over_batch_extrapolated": round(lo_x["median"] / ba["median"], 1),
                "text_GiBps": round(text_bytes / (ba["median"] * 1e-3) / 2**30, 2), "kernel_ms": round(busy, 3),
                "kernel_ms_by_name": names, "kernel_launches_per_call": launches,
                "host_ms_outside_kernels": round(ba["median"] - busy, 3), "verified_files": nf}

    res = {"tool": "unzstd_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "text_bytes": text_bytes, "warmup": a.warmup, "reps": a.reps}
    frames, foffs, flens = wire.zstd_compress_batch_device(text, toffs, tlens)
    res["own_encoder"] = measure(frames.clone(), foffs, flens)
    del frames
    blobs = [F.stream_compress(text_h[int(toffs[f]):int(toffs[f] + tlens[f])].tobytes(), 3) for f in range(nf)]
    flens = np.array([len(b) for b in blobs], dtype=np.uint64)
    foffs = np.concatenate([[0], np.cumsum(flens)[:-1]]).astype(np.uint64)
    frames = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).cuda()
    res["libzstd_stream_l3"] = measure(frames, foffs, flens)
    del frames, blobs

    if a.c3b_mib:
        import unzstd_bench

        del text
        torch.cuda.empty_cache()
        want = ask = a.c3b_mib << 20
        while True:
            kind, oa, ob, ss, cbs, nlit = unzstd_bench.c3b_ops(np, ask)
            lit = torch.empty(max(nlit, 1), dtype=torch.uint8, device="cuda")
            dev.synth_fill(lit, 0x5E1D0C07)
            big = wire.delta_to_json_device(kind, oa, ob, ss, cbs, lit)
            del lit
            if big.numel() >= want:
                break
            ask = int(ask * (want / big.numel()) * 1.01) + 4096
            del big
        frame = torch.frombuffer(bytearray(F.stream_compress(big.cpu().numpy().tobytes(), 3)), dtype=torch.uint8).cuda()
        n = big.numel()
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        fo, fl = np.zeros(1, dtype=np.uint64), np.array([frame.numel()], dtype=np.uint64)

        def as_batch():
            return wire.zstd_decompress_batch_device(frame, fo, fl, out=out)

        def as_single():
            return wire.zstd_decompress_device(frame, out=out)

        out.zero_()
        assert torch.equal(as_batch()[0], big), "the batch of one differs from the text"
        out.zero_()
        assert torch.equal(as_single(), big), "the single call differs from the text"
        entry = {"text_bytes": n, "frame_bytes": frame.numel()}
        for name, fn in (("single_call", as_single), ("batch_of_one", as_batch), ("single_call_again", as_single)):
            st = timed(fn, a.warmup, a.reps)
            _, names, _ = profiled(fn)
            entry[name] = {"ms": st, "GiBps": round(n / (st["median"] * 1e-3) / 2**30, 3), "kernel_ms_by_name": names}
        entry["batch_over_single"] = round(entry["batch_of_one"]["ms"]["median"] / entry["single_call"]["ms"]["median"], 3)
        res["c3b_one_frame"] = entry

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
