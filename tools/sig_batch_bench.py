#!/usr/bin/env python3
"""The signature exchange of the many-small-files workload (BASELINE C4: 10 000 x 1 MiB files,
block size 4096, 256 blocks each): the batch's signature texts written (receiver) and parsed
(sender) two ways in one process:

  loop   one sydelta_checksums_to_json_device / sydelta_checksums_from_json_device call per file
         into preallocated buffers, the only form there was before the batched calls, timed on
         the first --loop-files files and extrapolated to the batch by the file count (the files
         are alike); labelled as extrapolated in the result;
  batch  one sydelta_checksums_batch_to_json_device / sydelta_checksums_batch_from_json_device
         call into preallocated buffers.

    python tools/sig_batch_bench.py [--files 10000] [--size 1048576] [--warmup 2] [--reps 10]
                                    [--loop-files 500] [--loop-reps 3] [--big-entries 2621440]
                                    [--out profiles/sig_batch_bench.json]

The signatures come from signature_batch of bench.c4_files' bases.  Every text and every SoA
value is compared between the two legs, for all files, before any timing.  Times are HIP events
around the calls (median of --reps after --warmup, with min and max).  `kernel_ms` is the union
of the library's event pairs around the call's kernels in a profiled pass of its own,
`kernel_ms_by_name` the split, and `host_ms_outside_kernels` the call's median minus the union.
The parser is measured in both of its forms: the waves reading their tile through LDS (staged,
the default) and from global memory (SYDELTA_SIGB_STAGE=0).  `one_text` parses one text of
--big-entries entries with the single call (k_sigparse) and as a batch of one, in the same
process.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--loop-files", type=int, default=500)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--big-entries", type=int, default=2560 << 10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sig_batch_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("sig_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev
    from sy_amd import wire
    from sy_amd._lib import check, lib

    nf, fsz, bs = a.files, a.size, a.block_size
    basis, new, (boff, blen, _, _) = bench.c4_files(dev, basis_bytes=fsz, nfiles=nf, first=0)
    del new
    w, s = dev.signature_batch(basis, boff, blen, bs)
    w, s = w.clone(), s.clone()
    del basis
    torch.cuda.empty_cache()
    nb = ((blen + np.uint64(bs - 1)) // np.uint64(bs)).astype(np.uint64)
    last = (blen - (nb - np.uint64(1)) * np.uint64(bs)).astype(np.uint64)
    sbase = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.uint64)
    nent = int(nb.sum())
    stream = int(torch.cuda.current_stream().cuda_stream)

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
        st["calls"] = [round(x, 2) for x in ms]  # in the order they ran
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

    def staged(on):
        os.environ["SYDELTA_SIGB_STAGE"] = "1" if on else "0"

    # ---- the batch once, then every file of the loop against it
    text, toffs, tlens = wire.checksums_batch_to_json_device(w, s, nb, last, bs)
    text = text.clone()
    text_bytes = int(tlens.sum())
    need = text.numel()
    wp, sp = w.data_ptr(), s.data_ptr()
    got = ctypes.c_uint64()

    def write_one(f, arena):
        check(lib.sydelta_checksums_to_json_device(wp + 4 * int(sbase[f]), sp + 8 * int(sbase[f]), int(nb[f]), bs,
                                                   int(last[f]), arena.data_ptr() + int(toffs[f]), int(tlens[f]),
                                                   ctypes.byref(got), stream))

    recs = torch.zeros(max(nent, 1) * 5, dtype=torch.int64, device="cuda")  # sydelta_block_checksum: 40 bytes

    def parse_one(f):
        check(lib.sydelta_checksums_from_json_device(text.data_ptr() + int(toffs[f]), int(tlens[f]),
                                                     recs.data_ptr() + 40 * int(sbase[f]), int(nb[f]), ctypes.byref(got),
                                                     stream))

    inside = torch.zeros(need, dtype=torch.bool, device="cuda")
    for f in range(nf):
        inside[int(toffs[f]):int(toffs[f] + tlens[f])] = True
    loop_text = torch.zeros(need, dtype=torch.uint8, device="cuda")
    for f in range(nf):
        write_one(f, loop_text)
        assert got.value == int(tlens[f]), f"file {f}: the single writer's length differs"
    assert torch.equal(loop_text[inside], text[inside]), "the loop's texts differ from the batch's"
    del loop_text
    for f in range(nf):
        parse_one(f)
        assert got.value == int(nb[f]), f"file {f}: the single parser's count differs"
    r = recs.view(-1, 5)
    for form in (True, False):
        staged(form)
        pw, ps, pn, pl = wire.checksums_batch_from_json_device(text, toffs, tlens, bs)
        assert np.array_equal(pn, nb) and np.array_equal(pl, last), "the batch's tables differ"
        assert torch.equal(pw, w) and torch.equal(ps, s), "the batch's SoA differs from the signature"
        assert torch.equal((r[:, 3] & 0xFFFFFFFF).to(torch.int32), pw) and torch.equal(r[:, 4], ps), \
            "the loop's entries differ from the batch's"
    staged(True)
    del pw, ps

    # ---- timing
    arena = torch.empty(need, dtype=torch.uint8, device="cuda")
    ow = torch.empty(nent, dtype=torch.int32, device="cuda")
    os_ = torch.empty(nent, dtype=torch.int64, device="cuda")
    to, tl, so, pn, pl = (np.zeros(nf, dtype=np.uint64) for _ in range(5))

    def batch_write():
        check(lib.sydelta_checksums_batch_to_json_device(0, wp, sp, nb.ctypes.data, last.ctypes.data, nf, bs, arena.data_ptr(),
                                                         need, to.ctypes.data, tl.ctypes.data, ctypes.byref(got), stream))

    def batch_parse():
        check(lib.sydelta_checksums_batch_from_json_device(0, text.data_ptr(), need, toffs.ctypes.data, tlens.ctypes.data, nf,
                                                           bs, ow.data_ptr(), os_.data_ptr(), nent, so.ctypes.data,
                                                           pn.ctypes.data, pl.ctypes.data, None, ctypes.byref(got), stream))

    sub = min(a.loop_files, nf)

    def loop_write():
        for f in range(sub):
            write_one(f, arena)

    def loop_parse():
        for f in range(sub):
            parse_one(f)

    scale = nf / sub

    def leg(batch_fn, loop_fn):
        ba = timed(batch_fn, a.warmup, a.reps)
        lo = timed(loop_fn, 1, a.loop_reps)
        lo_x = {k: (round(v * scale, 1) if k != "n" else v) for k, v in lo.items() if k != "calls"}
        busy, names, launches = profiled(batch_fn)
        return {"batch_ms": ba, "loop_files_timed": sub, "loop_subset_ms": lo, "loop_ms_extrapolated": lo_x,
                "loop_ms_per_file": round(lo["median"] / sub, 4),
                "loop_over_batch_extrapolated": round(lo_x["median"] / ba["median"], 1),
                "batch_median_below_loop_min": ba["median"] < lo_x["min"],
                "text_GiBps": round(text_bytes / (ba["median"] * 1e-3) / 2**30, 2), "kernel_ms": round(busy, 3),
                "kernel_ms_by_name": names, "kernel_launches_per_call": launches,
                "host_ms_outside_kernels": round(ba["median"] - busy, 3)}

    res = {"tool": "sig_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "entries": nent, "text_bytes": text_bytes, "warmup": a.warmup, "reps": a.reps,
           "verified_files": nf}
    res["writer"] = leg(batch_write, loop_write)
    staged(True)
    res["parser_staged"] = leg(batch_parse, loop_parse)
    staged(False)
    res["parser_plain"] = leg(batch_parse, loop_parse)
    staged(True)

    if a.big_entries:
        del text, arena, recs, ow, os_, inside
        torch.cuda.empty_cache()
        n = a.big_entries
        g = torch.Generator(device="cuda").manual_seed(0x5E1D0007)
        bw = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
        bsg = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
        big = wire.checksums_to_json_device(bw, bsg, bs, bs).clone()
        nbytes = big.numel()
        brecs = torch.empty(n * 5, dtype=torch.int64, device="cuda")
        ow = torch.empty(n, dtype=torch.int32, device="cuda")
        os_ = torch.empty(n, dtype=torch.int64, device="cuda")
        to1, tl1 = np.zeros(1, dtype=np.uint64), np.array([nbytes], dtype=np.uint64)
        o1 = [np.zeros(1, dtype=np.uint64) for _ in range(3)]

        def as_single():
            check(lib.sydelta_checksums_from_json_device(big.data_ptr(), nbytes, brecs.data_ptr(), n, ctypes.byref(got), stream))

        def as_batch():
            check(lib.sydelta_checksums_batch_from_json_device(0, big.data_ptr(), nbytes, to1.ctypes.data, tl1.ctypes.data, 1,
                                                               bs, ow.data_ptr(), os_.data_ptr(), n, o1[0].ctypes.data,
                                                               o1[1].ctypes.data, o1[2].ctypes.data, None, ctypes.byref(got),
                                                               stream))

        as_single()
        assert got.value == n
        rr = brecs.view(-1, 5)
        assert torch.equal((rr[:, 3] & 0xFFFFFFFF).to(torch.int32), bw) and torch.equal(rr[:, 4], bsg)
        entry = {"entries": n, "text_bytes": nbytes}
        for name, fn, form in (("single_call", as_single, True), ("batch_of_one_staged", as_batch, True),
                               ("batch_of_one_plain", as_batch, False), ("single_call_again", as_single, True)):
            staged(form)
            if fn is as_batch:
                ow.zero_(), os_.zero_()
                as_batch()
                assert int(o1[1][0]) == n and torch.equal(ow, bw) and torch.equal(os_, bsg), name
            st = timed(fn, a.warmup, a.reps)
            kms = []
            for _ in range(max(3, a.reps // 2)):  # the kernels' time of single calls: its own spread
                dev.set_profiling(True)
                try:
                    dev.profile(reset=True)
                    fn()
                    prof = dev.profile(reset=True)
                finally:
                    dev.set_profiling(False)
                kms.append({k: v["ms"] for k, v in prof.items() if not k.startswith("__") and "ms" in v})
            keys = sorted(kms[0])
            ksum = stats_of([sum(k.values()) for k in kms])
            entry[name] = {"ms": st, "GiBps": round(nbytes / (st["median"] * 1e-3) / 2**30, 3),
                           "kernel_ms_by_name": {k: stats_of([x[k] for x in kms]) for k in keys}, "kernel_ms": ksum,
                           "kernel_ns_per_entry": round(ksum["median"] * 1e6 / n, 3)}
        staged(True)
        entry["staged_kernel_over_single"] = round(entry["batch_of_one_staged"]["kernel_ms"]["median"] /
                                                   entry["single_call"]["kernel_ms"]["median"], 3)
        entry["plain_kernel_over_single"] = round(entry["batch_of_one_plain"]["kernel_ms"]["median"] /
                                                  entry["single_call"]["kernel_ms"]["median"], 3)
        res["one_text"] = entry

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
