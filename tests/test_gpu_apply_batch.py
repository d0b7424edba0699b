"""device.apply_batch (sydelta_apply_delta_batch_device, k_applyb): a whole batch of deltas
applied in one call, against oracle.py_apply_delta and the single-file apply_device."""
import re
import threading

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT = 0xEE


def _pack(arrs, align=16, lead=0):
    """Files packed into one device buffer at `align`-byte aligned offsets (after `lead` bytes);
    16 spare bytes at the end."""
    import torch

    offs, pos = [], lead
    for a in arrs:
        pos = -(-pos // align) * align
        offs.append(pos)
        pos += len(a)
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, a in zip(offs, arrs):
        host[o:o + len(a)] = a
    lens = np.array([len(a) for a in arrs], dtype=np.uint64)
    return torch.from_numpy(host).cuda(), np.array(offs, dtype=np.uint64), lens


def _delta(gpu, ops, source_size=0, bs=4096):
    """A hand-made DeviceDelta from (kind, a, b) tuples (kind "C" / "D")."""
    kind = np.array([0 if k == "C" else 1 for k, _, _ in ops], dtype=np.uint32)
    a = np.array([x for _, x, _ in ops], dtype=np.uint64)
    b = np.array([y for _, _, y in ops], dtype=np.uint64)
    return gpu.DeviceDelta(kind, a, b, source_size, bs, {})


def _stats_rows(stats):
    return [(int(r["operations_count"]), int(r["literal_bytes"]), int(r["bytes_written"])) for r in stats]


def _matcher_files(bs, cap_blocks=None):
    """About 40 (basis, source) pairs: every basis length of the list with every kind of source."""
    rng = np.random.default_rng(1000 + bs)
    big = 300 * 1024 if cap_blocks is None else min(300 * 1024, cap_blocks * bs)
    lens = [0, 1, bs - 1, bs, bs + 1, 3 * bs + 17, 40 * bs + 7, big]
    pairs = []
    for n in lens:
        basis = rng.integers(0, 256, n, dtype=np.uint8)
        # one inserted byte and a few substitutions
        p = int(rng.integers(0, n + 1))
        ed = np.concatenate([basis[:p], rng.integers(0, 256, 1, dtype=np.uint8), basis[p:]])
        for q in rng.integers(0, len(ed), min(5, len(ed))):
            ed[q] ^= np.uint8(rng.integers(1, 256))
        pairs += [(basis, ed), (basis, basis.copy()), (basis, rng.integers(0, 256, n // 2 + 50, dtype=np.uint8)),
                  (basis, np.zeros(0, dtype=np.uint8))]
    for n in (2 * bs, 5 * bs + 3, 17, 9 * bs - 1, 2 * bs + 1, 64, 11 * bs, 6 * bs + 5):  # and 8 more: a shifted tail
        basis = rng.integers(0, 256, n, dtype=np.uint8)
        pairs.append((basis, np.concatenate([basis[n // 3:], basis[:n // 3]])))
    return pairs


@pytest.mark.parametrize("bs,path", [(7, "index"), (1000, "index"), (256, "pairs"), (4096, "pairs")])
def test_round_trip_from_the_matcher(gpu, bs, path):
    """The deltas of a batched match rebuild their sources into an arena packed back to back
    (odd lengths: neighbouring files share 16-byte granules), nothing else is written, and the
    per-file stats are the single-file call's.  sydelta_delta_pairs_device takes bases of at
    most 1024 blocks, so its largest basis is min(300 KiB, 1024 blocks)."""
    import torch

    pairs = _matcher_files(bs, cap_blocks=1024 if path == "pairs" else None)
    bbuf, boff, blen = _pack([b for b, _ in pairs])
    sbuf, soff, slen = _pack([s for _, s in pairs])
    if path == "pairs":
        batch = gpu.delta_pairs_handle(bbuf, boff, blen, sbuf, soff, slen, bs)
    else:
        w, s = gpu.signature_batch(bbuf, boff, blen, bs)
        nblk = (blen + np.uint64(bs - 1)) // np.uint64(bs)
        last = np.where(nblk > 0, blen - (np.maximum(nblk, 1) - 1) * np.uint64(bs), 0).astype(np.uint64)
        idx = gpu.BatchIndex(w, s, nblk, last, bs)
        batch = gpu.match_batch_handle(idx, sbuf, soff, slen)
        idx.close()
    ooff = np.concatenate([[0], np.cumsum(slen)[:-1]]).astype(np.uint64) + np.uint64(3)
    total = int(slen.sum()) + 3 + 5
    out = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    got, ooffs, stats = gpu.apply_batch(bbuf, boff, blen, batch, sbuf, soff, slen, out=out, ooffs=ooff)
    torch.cuda.synchronize()
    host = got.cpu().numpy()
    want = np.full(total, SENT, dtype=np.uint8)
    deltas = batch.deltas()
    for f, (basis, src) in enumerate(pairs):
        o = int(ooff[f])
        assert host[o:o + len(src)].tobytes() == src.tobytes(), f
        assert O.py_apply_delta(basis.tobytes(), src.tobytes(), deltas[f].tuples()) == src.tobytes(), f
        want[o:o + len(src)] = src
    assert np.array_equal(host, want)  # every byte outside the ranges is still the sentinel
    scratch = torch.empty(int(slen.max()) + 16, dtype=torch.uint8, device="cuda")
    rows = _stats_rows(stats)
    for f, d in enumerate(deltas):
        _, st = gpu.apply_device(bbuf[int(boff[f]):int(boff[f] + blen[f])], d, sbuf[int(soff[f]):int(soff[f] + slen[f])],
                                 out=scratch)
        assert rows[f] == (st["operations_count"], st["literal_bytes"], st["bytes_written"]), f
    # out=None: an arena of its own, outputs at 16-byte aligned offsets
    got2, ooffs2, stats2 = gpu.apply_batch(bbuf, boff, blen, batch, sbuf, soff, slen)
    assert (ooffs2 % np.uint64(16) == 0).all() and _stats_rows(stats2) == rows
    host2 = got2.cpu().numpy()
    for f, (_, src) in enumerate(pairs):
        assert host2[int(ooffs2[f]):int(ooffs2[f]) + len(src)].tobytes() == src.tobytes(), f
    batch.close()


def _hand_files(rng):
    """(basis, literal, ops) of the hand-made files."""
    files = []

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8)

    files.append((rnd(10), rnd(5000), [("D", 0, 100), ("D", 1000, 3999), ("D", 7, 1)]))               # Data only
    files.append((rnd(9000), rnd(0), [("C", 4096, 4096), ("C", 0, 4096), ("C", 8999, 1)]))            # Copy only
    files.append((rnd(4096), rnd(3), [("C", 1024, 999)] * 50))                                         # one block 50 times
    files.append((rnd(40000), rnd(3), [("C", o, 4000) for o in range(36000, -1, -4000)]))             # descending
    files.append((rnd(300), rnd(300), [("C", 0, 0), ("C", 5, 20), ("D", 9, 0), ("C", 300, 0), ("D", 100, 33),
                                       ("D", 300, 0), ("C", 25, 10), ("D", 0, 0)]))                   # zero lengths
    files.append((rnd(1), rnd(200 * 1024 + 9), [("D", 9, 200 * 1024)]))                                # one large Data
    tiny = []
    for i in range(5000):                                                                              # 5000 tiny ops
        tiny.append(("C" if i % 2 == 0 else "D", int(rng.integers(0, 900)), int(rng.integers(1, 4))))
    files.append((rnd(903), rnd(903), tiny))
    runs = [("C", 77 + 129 * i, 129) for i in range(300)] + [("C", 5, 1000)]                          # merged, then not
    files.append((rnd(77 + 129 * 300), rnd(1), runs))
    return files


@pytest.mark.parametrize("lead", [(1, 3, 5), (15, 0, 9)])
def test_hand_made_deltas(gpu, lead):
    """DeviceDelta arrays, the three arenas starting at odd byte offsets."""
    import torch

    files = _hand_files(np.random.default_rng(77))
    bbuf, boff, blen = _pack([b for b, _, _ in files], align=1, lead=lead[0])
    lbuf, loff, llen = _pack([l for _, l, _ in files], align=1, lead=lead[1])
    bbuf, lbuf = bbuf[lead[0]:], lbuf[lead[1]:]
    boff -= np.uint64(lead[0])
    loff -= np.uint64(lead[1])
    want = [O.py_apply_delta(b.tobytes(), l.tobytes(), ops) for b, l, ops in files]
    sizes = np.array([len(w) for w in want], dtype=np.uint64)
    ooff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    total = int(sizes.sum())
    whole = torch.full((lead[2] + total + 21,), SENT, dtype=torch.uint8, device="cuda")
    out = whole[lead[2]:lead[2] + total]
    assert (bbuf.data_ptr() % 16, lbuf.data_ptr() % 16, out.data_ptr() % 16) == lead
    deltas =[_delta(gpu, ops) for _, _, ops in files]
    _, _, stats = gpu.apply_batch(bbuf, boff, blen, deltas, lbuf, loff, llen, out=out, ooffs=ooff)
    host = whole.cpu().numpy()
    exp = np.full(len(host), SENT, dtype=np.uint8)
    exp[lead[2]:lead[2] + total] = np.frombuffer(b"".join(want), dtype=np.uint8)
    assert np.array_equal(host, exp)
    for f, (_, _, ops) in enumerate(files):  # the ops as given, not the merged runs
        lit = sum(y for k, _, y in ops if k == "D")
        assert _stats_rows(stats)[f] == (len(ops), lit, len(want[f])), f


def test_64_bit_offsets(gpu):
    """A basis at 2^32 + 5 and an output at 2^32 + 11 of arenas of 4 GiB + 1 MiB."""
    import torch

    big = (1 << 32) + (1 << 20)
    rng = np.random.default_rng(64)
    basis = torch.empty(big, dtype=torch.uint8, device="cuda")
    out = torch.empty(big, dtype=torch.uint8, device="cuda")
    blens = np.array([70000, 5000, 333], dtype=np.uint64)
    boff = np.array([(1 << 32) + 5, 1000003, (1 << 31) + 1], dtype=np.uint64)
    ooff = np.array([(1 << 32) + 11, (1 << 31) + 7, 4099], dtype=np.uint64)
    hb = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in blens]
    for o, b in zip(boff, hb):
        basis[int(o):int(o) + len(b)] = torch.from_numpy(b).cuda()
    lit_h = rng.integers(0, 256, 4000, dtype=np.uint8)
    lit = torch.from_numpy(np.concatenate([lit_h, np.zeros(16, np.uint8)])).cuda()
    ops = [[("C", 60000, 10000), ("D", 5, 3000), ("C", 0, 60000), ("C", 1, 4097)],
           [("D", 0, 4000), ("C", 13, 4987)],
           [("C", 0, 333), ("C", 0, 333), ("D", 3999, 1)]]
    want = [O.py_apply_delta(hb[f].tobytes(), lit_h.tobytes(), ops[f]) for f in range(3)]
    for f in range(3):
        o = int(ooff[f])
        out[o - 64:o + len(want[f]) + 64] = SENT
    z = np.zeros(3, dtype=np.uint64)
    _, _, stats = gpu.apply_batch(basis, boff, blens, [_delta(gpu, o) for o in ops], lit, z,
                                  np.full(3, 4000, np.uint64), out=out, ooffs=ooff)
    for f in range(3):
        o, n = int(ooff[f]), len(want[f])
        got = out[o - 64:o + n + 64].cpu().numpy()
        assert (got[:64] == SENT).all() and (got[64 + n:] == SENT).all(), f
        assert got[64:64 + n].tobytes() == want[f], f
        assert int(stats[f]["bytes_written"]) == n


def _error_batch(gpu):
    """20 files of 100 ops; returns the pieces to rebuild the call with one thing changed."""
    rng = np.random.default_rng(13)
    L = 6000
    bases = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(20)]
    lits = [rng.integers(0, 256, L - 3, dtype=np.uint8) for _ in range(20)]
    ops = []
    for f in range(20):
        ops.append([("C" if i % 2 == 0 else "D", int(rng.integers(0, L - 300)), int(rng.integers(1, 100)))
                    for i in range(100)])
    return bases, lits, ops


def _run_error_case(gpu, change):
    import torch

    from sy_amd._lib import SyDeltaError

    bases, lits, ops = _error_batch(gpu)
    bbuf, boff, blen = _pack(bases, align=1)
    lbuf, loff, llen = _pack(lits, align=1)
    bbuf, lbuf = bbuf[:int(blen.sum())], lbuf[:int(llen.sum())]  # the arenas end with their last file
    sizes = np.array([sum(y for _, _, y in o) for o in ops], dtype=np.uint64)
    ooff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    t = dict(ops=ops, boff=boff, blen=blen, loff=loff, llen=llen, ooff=ooff)
    change(t)
    out = torch.full((int(sizes.sum()),), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(SyDeltaError) as e:
        gpu.apply_batch(bbuf, t["boff"], t["blen"], [_delta(gpu, o) for o in t["ops"]], lbuf, t["loff"], t["llen"],
                        out=out, ooffs=t["ooff"])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "an output byte was written before the batch was refused"
    return e.value


def test_copy_past_the_basis_names_file_and_op(gpu):
    def change(t):  # one byte past file 13's basis, still inside the arena
        t["ops"][13][77] = ("C", 6000 - 9, 10)

    err = _run_error_case(gpu, change)
    assert err.code == -5
    msg = str(err)
    assert re.search(r"file 13\b", msg) and re.search(r"op 77\b", msg) and "past the end of the basis" in msg, msg


def _data_outside(t):
    t["ops"][4][50] = ("D", 6000 - 3 - 9, 10)


def _output_above_cap(t):  # file 7 writes one byte more than the slot its neighbour leaves it
    t["ops"][7][98] = (t["ops"][7][98][0], t["ops"][7][98][1], t["ops"][7][98][2] + 1)


def _range_leaves_arena(t):
    t["blen"] = t["blen"].copy()
    t["blen"][19] += np.uint64(1)


def _lit_range_wraps(t):
    t["loff"] = t["loff"].copy()
    t["loff"][3] = np.uint64(2**64 - 2)


def _op_wraps(t):
    t["ops"][11][0] = ("D", 2**64 - 1, 2)


@pytest.mark.parametrize("change,where", [(_data_outside, r"file 4: op 50:"), (_output_above_cap, r"file 7: op \d+:"),
                                          (_range_leaves_arena, r"file 19:"), (_lit_range_wraps, r"file 3:"),
                                          (_op_wraps, r"file 11: op 0:")])
def test_invalid_batches_touch_nothing(gpu, change, where):
    err = _run_error_case(gpu, change)
    assert err.code == -3
    assert re.search(where, str(err)), str(err)


def test_empty_batch(gpu):
    import torch

    e = torch.zeros(16, dtype=torch.uint8, device="cuda")
    z = np.zeros(0, dtype=np.uint64)
    out, ooffs, stats = gpu.apply_batch(e, z, z, [], e, z, z)
    assert len(ooffs) == 0 and len(stats) == 0


def _small_batch(gpu, nfiles, fsz, seed):
    """nfiles files of fsz bytes: hand-made deltas of Copies with a literal in the middle."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 256, fsz, dtype=np.uint8) for _ in range(nfiles)]
    lits = [rng.integers(0, 256, 64, dtype=np.uint8) for _ in range(nfiles)]
    ops = []
    for f in range(nfiles):
        cut = int(rng.integers(1, fsz // 1024)) * 1024
        ops.append([("C", o, 1024) for o in range(0, cut, 1024)] + [("D", 3, 50 + f % 7)] +
                   [("C", o, 1024) for o in range(cut, fsz, 1024)])
    want = [O.py_apply_delta(b.tobytes(), l.tobytes(), o) for b, l, o in zip(bases, lits, ops)]
    bbuf, boff, blen = _pack(bases)
    lbuf, loff, llen = _pack(lits)
    return (bbuf, boff, blen, [_delta(gpu, o) for o in ops], lbuf, loff, llen), want


def _check_outputs(out, ooffs, want):
    host = out.cpu().numpy()
    for f, w in enumerate(want):
        assert host[int(ooffs[f]):int(ooffs[f]) + len(w)].tobytes() == w, f


def test_launches_do_not_grow_with_files(gpu):
    """Slice rule: the merged table goes up in slices of at most 16384 runs and 16384
    segments (a segment: the part of a file's output covered by a slice's runs, so at least
    one per non-empty file), one k_applyb launch per slice.  600 files of three runs each are
    1800 runs and 600 segments: one slice, as for 8 files."""
    counts = {}
    for n in (8, 600):
        args, want = _small_batch(gpu, n, 8192, 5)
        gpu.set_profiling(True)
        gpu.profile(reset=True)
        try:
            out, ooffs, _ = gpu.apply_batch(*args)
            prof = gpu.profile(reset=True)
        finally:
            gpu.set_profiling(False)
        _check_outputs(out, ooffs, want)
        assert any(k.startswith("k_applyb") for k in prof), prof
        counts[n] = sum(v["count"] for k, v in prof.items() if k != "__busy__")
    slices = max(-(-600 * 3 // 16384), -(-600 // 16384))
    assert slices == 1
    assert counts[600] <= 16
    assert counts[600] <= counts[8] + slices, counts


def test_stream_order(gpu):
    """The basis is written by a kernel queued on the caller's stream just before the call and
    the result is read by a copy queued just after it: no synchronise in between."""
    import torch

    args, _ = _small_batch(gpu, 30, 64 * 1024, 9)
    bbuf, boff, blen, deltas, lbuf, loff, llen = args
    stream = torch.cuda.Stream()
    n8 = bbuf.numel() // 8 * 8
    fresh = bbuf.clone()
    gpu.synth_fill(fresh[:n8], 0xABCD)  # what the basis arena holds when the apply runs
    host = torch.empty(30 * 64 * 1024 + 30 * 64, dtype=torch.uint8, pin_memory=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for i in range(20):  # keep the stream busy, then the write the apply must see
            gpu.synth_fill(bbuf[:n8], i, stream=stream)
        gpu.synth_fill(bbuf[:n8], 0xABCD, stream=stream)
        out, ooffs, stats = gpu.apply_batch(bbuf, boff, blen, deltas, lbuf, loff, llen, stream=stream)
        host[:out.numel()].copy_(out, non_blocking=True)
    stream.synchronize()
    fb, lb = fresh.cpu().numpy(), lbuf.cpu().numpy()
    got = host.numpy()
    for f, d in enumerate(deltas):
        w = O.py_apply_delta(fb[int(boff[f]):int(boff[f] + blen[f])].tobytes(),
                             lb[int(loff[f]):int(loff[f] + llen[f])].tobytes(), d.tuples())
        assert got[int(ooffs[f]):int(ooffs[f]) + len(w)].tobytes() == w, f


@pytest.mark.late
def test_concurrent_callers(gpu):
    """Four threads, each applying its own 50-file batch at once."""
    import torch

    jobs = [_small_batch(gpu, 50, 16 * 1024, 100 + t) for t in range(4)]
    torch.cuda.synchronize()
    results, errors = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                out, ooffs, _ = gpu.apply_batch(*jobs[t][0], stream=torch.cuda.Stream())
                results[t] = (out, ooffs)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(4):
        _check_outputs(results[t][0], results[t][1], jobs[t][1])
