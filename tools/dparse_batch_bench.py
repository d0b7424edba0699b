#!/usr/bin/env python3
"""The receiver's middle step for the many-small-files workload (BASELINE C4: 10 000 x 1 MiB
files, block size 4096, one inserted byte and 16 substitutions per file): the batch's Delta
texts parsed two ways in one process:

  loop   one sydelta_delta_from_json_device call per text into a preallocated literal buffer,
         the only form there was before the batched call, timed on the first --loop-files texts
         and extrapolated to the batch by the file count (the texts are alike); labelled as
         extrapolated in the result;
  batch  one sydelta_delta_batch_from_json_device call into a preallocated literal arena.

    python tools/dparse_batch_bench.py [--files 10000] [--size 1048576] [--warmup 2] [--reps 10]
                                       [--loop-files 200] [--loop-reps 3] [--c3b-mib 256]
                                       [--out profiles/dparse_batch_bench.json]

The texts come from delta_pairs_handle and delta_batch_to_json_device.  Every delta and literal
range of the batch's result is compared with the single call's on that text before any timing.
Times are HIP events around the calls (median of --reps after --warmup, with min and max).
`kernel_ms` is the union of the library's event pairs around the call's kernels in a profiled
pass of its own, `kernel_ms_by_name` the split, and `host_ms_outside_kernels` the call's median
minus the union.  `c3b_one_text` parses one large text (C3b-shaped, --c3b-mib MiB) as a batch of
one and with the single call, in the same process.  Prints one JSON line and writes it to --out.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dparse_batch_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("dparse_batch_bench needs a GPU")
    import bench
    import sy_amd.device as dev
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

    def ops_of(h):
        cnt = int(lib.sydelta_delta_num_ops(h))
        p = lib.sydelta_delta_ops(h)
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(cnt, 3)).copy() if cnt else \
            np.zeros((0, 3), dtype=np.uint64)
        return arr, int(lib.sydelta_delta_source_size(h)), int(lib.sydelta_delta_block_size(h))

    def single(ptr, n, lit_ptr, cap, want_out):
        got, h = ctypes.c_uint64(), ctypes.c_void_p()
        check(lib.sydelta_delta_from_json_device(ptr, n, lit_ptr, cap, ctypes.byref(got), ctypes.byref(h) if want_out else None,
                                                 stream))
        if not want_out:
            return got.value, None
        try:
            return got.value, ops_of(h)
        finally:
            lib.sydelta_delta_free(h)

    # the batch into an arena of its own size, then every file against the single call
    parsed, lit, loffs, llens = wire.delta_batch_from_json_device(text, toffs, tlens)
    lit = lit.clone()
    lit_h = lit.cpu().numpy()
    one_lit = torch.empty(max(1, int(llens.max())), dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * nf)()
    assert int(lib.sydelta_delta_batch_ptrs(parsed.h, ptrs, nf)) == nf
    nops = 0
    for f in range(nf):
        n1, d1 = single(text.data_ptr() + int(toffs[f]), int(tlens[f]), one_lit.data_ptr(), one_lit.numel(), True)
        db = ops_of(ptrs[f])
        assert n1 == int(llens[f]) and d1[1:] == db[1:] and np.array_equal(d1[0], db[0]), f"file {f}: delta differs"
        o = int(loffs[f])
        assert np.array_equal(one_lit[:n1].cpu().numpy(), lit_h[o:o + n1]), f"file {f}: literal bytes differ"
        nops += len(db[0])
    parsed.close()

    def run_batch():
        b, *_ = wire.delta_batch_from_json_device(text, toffs, tlens, lit=lit)
        b.close()

    sub = min(a.loop_files, nf)
    tptr = [text.data_ptr() + int(toffs[f]) for f in range(sub)]
    tlen_i = [int(tlens[f]) for f in range(sub)]
    lptr = [lit.data_ptr() + int(loffs[f]) for f in range(sub)]
    lcap = [int(llens[f]) for f in range(sub)]

    def run_loop():
        got, h = ctypes.c_uint64(), ctypes.c_void_p()
        for f in range(sub):
            check(lib.sydelta_delta_from_json_device(tptr[f], tlen_i[f], lptr[f], lcap[f], ctypes.byref(got), ctypes.byref(h),
                                                     stream))
            lib.sydelta_delta_free(h)

    ba = timed(run_batch, a.warmup, a.reps)
    lo = timed(run_loop, 1, a.loop_reps)
    scale = nf / sub
    lo_x = {k: (round(v * scale, 1) if k != "n" else v) for k, v in lo.items() if k != "calls"}
    busy, names, launches = profiled(run_batch)
    res = {"tool": "dparse_batch_bench", "device": torch.cuda.get_device_name(0), "files": nf, "file_bytes": fsz,
           "block_size": bs, "text_bytes": text_bytes, "literal_bytes": int(llens.sum()), "ops": nops, "warmup": a.warmup,
           "reps": a.reps, "batch_ms": ba, "loop_files_timed": sub, "loop_subset_ms": lo, "loop_ms_extrapolated": lo_x,
           "loop_ms_per_file": round(lo["median"] / sub, 4),
           "loop_over_batch_extrapolated": round(lo_x["median"] / ba["median"], 1),
           "text_GiBps": round(text_bytes / (ba["median"] * 1e-3) / 2**30, 2), "kernel_ms": round(busy, 3),
           "kernel_ms_by_name": names, "kernel_launches_per_call": launches,
           "host_ms_outside_kernels": round(ba["median"] - busy, 3), "verified_files": nf}

    if a.c3b_mib:
        import unzstd_bench

        del text, lit
        torch.cuda.empty_cache()
        want = ask = a.c3b_mib << 20
        while True:
            kind, oa, ob, ss, cbs, nlit = unzstd_bench.c3b_ops(np, ask)
            src = torch.empty(max(nlit, 1), dtype=torch.uint8, device="cuda")
            dev.synth_fill(src, 0x5E1D0C07)
            big = wire.delta_to_json_device(kind, oa, ob, ss, cbs, src)
            if big.numel() >= want:
                break
            ask = int(ask * (want / big.numel()) * 1.01) + 4096
            del big, src
        big = big.clone()
        n = big.numel()
        out = torch.empty(max(nlit, 1), dtype=torch.uint8, device="cuda")
        to, tl = np.zeros(1, dtype=np.uint64), np.array([n], dtype=np.uint64)

        def as_batch():
            b, *_ = wire.delta_batch_from_json_device(big, to, tl, lit=out)
            b.close()

        def as_single():
            single(big.data_ptr(), n, out.data_ptr(), out.numel(), True)

        out.zero_()
        b, l1, lo1, ll1 = wire.delta_batch_from_json_device(big, to, tl, lit=out)
        db = ops_of(lib.sydelta_delta_batch_get(b.h, 0))
        b.close()
        assert int(ll1[0]) == nlit and torch.equal(out[:nlit], src[:nlit]), "the batch of one differs from the literals"
        out.zero_()
        n1, d1 = single(big.data_ptr(), n, out.data_ptr(), out.numel(), True)
        assert n1 == nlit and torch.equal(out[:nlit], src[:nlit]), "the single call differs from the literals"
        assert d1[1:] == db[1:] and np.array_equal(d1[0], db[0]), "the batch of one's delta differs from the single call's"
        entry = {"text_bytes": n, "literal_bytes": nlit, "ops": len(db[0])}
        for name, fn in (("single_call", as_single), ("batch_of_one", as_batch), ("single_call_again", as_single)):
            st = timed(fn, a.warmup, a.reps)
            _, knames, _ = profiled(fn)
            entry[name] = {"ms": st, "GiBps": round(n / (st["median"] * 1e-3) / 2**30, 3), "kernel_ms_by_name": knames}
        entry["batch_over_single"] = round(entry["batch_of_one"]["ms"]["median"] / entry["single_call"]["ms"]["median"], 3)
        res["c3b_one_text"] = entry

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
