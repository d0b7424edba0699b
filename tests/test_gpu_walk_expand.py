"""The op lists written on the device, at the record, lane and unit edges of the two pieces of
code that write them: expand_file (run by a file's last k_walk_files unit) and k_chunk_write
(sydelta_filewalk.hip).  Both turn run-length records into sydelta_ops with a wave scan, a
prefix carried across rounds of 64 records and a binary search per lane.

The inputs come from tests/walk_expand_cases.py; tests/test_walk_expand_cases.py proves on the
CPU that each one has the record, op and unit counts it is named for.  Here every case goes
through the C ABI and is compared op for op with the C oracle and with a
SYDELTA_DEVICE_EXPAND=0 run of the same input; every case names the exact movement of
sydelta_expand_counters it expects -- (files, 0): the device expanded every file; (0, 1): one
file reported `bad` and the host expanded the batch -- and checks the per-delta stats and the
batch totals against the host run and against counts taken from the oracle's ops.

Not reachable, and so not here: a chunk unit whose first record is dropped *and* whose next
record joins the previous op (skip 2).  A unit's records never hold two Data records in a row
(k_walk_files puts a Data record only before a Copy, or as the unit's last), and the previous
unit ends with the Copy that crosses the boundary whenever the first record is dropped or cut.
The nearest reachable plan is in the `skip` case: a unit's only record both cut at its start
and extended by the next unit's leading literal."""
import pytest

import test_gpu_file_walk as FW
import walk_expand_cases as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STATS = ("copy_ops", "data_ops", "literal_bytes", "weak_hits", "verified_hits")
_ORACLE = {}


def _oracle_ops(oracle_c, key, files):
    """The oracle's op lists of a batch's files (computed once per batch)."""
    if key not in _ORACLE:
        _ORACLE[key] = [FW._oracle_ops(oracle_c, c.src, c.basis, c.bs) for c in files]
    return _ORACLE[key]


def _counts(ops):
    nd = sum(1 for o in ops if o[0] == "D")
    return {"copy_ops": len(ops) - nd, "data_ops": nd, "literal_bytes": sum(o[2] for o in ops if o[0] == "D"),
            "verified_hits": len(ops) - nd}  # (every Copy is one verified hit)


def _check(batch, exp, out, tot, out0, tot0):
    for i, (c, e, d, d0) in enumerate(zip(batch.files, exp, out, out0)):
        assert d.tuples() == e, (batch.name, i, c.name)
        assert d0.tuples() == e, (batch.name, i, c.name, "host expansion")
        assert d.source_size == len(c.src) and d.block_size == batch.bs
        assert {k: d.stats[k] for k in STATS} == {k: d0.stats[k] for k in STATS}, (batch.name, c.name)
        for k, v in _counts(e).items():
            assert d.stats[k] == v, (batch.name, c.name, k)
    for k in STATS:
        assert tot[k] == tot0[k] == sum(d.stats[k] for d in out), (batch.name, k)


def _run_batch(gpu, oracle_c, monkeypatch, batch):
    """match_batch of the batch with the ops expanded on the device, then on the host; the
    counters' exact movement; ops, stats and totals."""
    monkeypatch.setenv("SYDELTA_FILE_SEGS", batch.segs)
    monkeypatch.delenv("SYDELTA_ASM_THREADS", raising=False)
    pairs = [(c.src, c.basis) for c in batch.files]
    exp = _oracle_ops(oracle_c, batch.name, batch.files)
    x0 = FW._expanded()
    out, tot, prof = FW._batch(gpu, pairs, batch.bs, "1", monkeypatch, "1")
    x1 = FW._expanded()
    assert "k_walk_files" in prof, prof
    want = (len(pairs), 0) if batch.expect == "dev" else (0, 1)
    assert (x1[0] - x0[0], x1[1] - x0[1]) == want, (batch.name, x0, x1)
    out0, tot0, _ = FW._batch(gpu, pairs, batch.bs, "1", monkeypatch, "0")
    assert FW._expanded() == x1, batch.name
    _check(batch, exp, out, tot, out0, tot0)


@pytest.mark.parametrize("max_nblk", [32, 64, 1024])
def test_expand_capacity(gpu, oracle_c, monkeypatch, max_nblk):
    """Files of cap - 1 and cap records expand (cap: the records the walk's LDS holds, 108 / 140 /
    1100); one file of cap + 1 records sends the whole batch to the host, every file still exact;
    the next all-good batch on the same thread expands again (the slab survives the discarded
    expansion)."""
    good, over = W.capacity_batches(max_nblk)
    assert good.cap == {32: 108, 64: 140, 1024: 1100}[max_nblk]
    _run_batch(gpu, oracle_c, monkeypatch, good)
    _run_batch(gpu, oracle_c, monkeypatch, over)
    _run_batch(gpu, oracle_c, monkeypatch, good)


def test_expand_merged_record_counts(gpu, oracle_c, monkeypatch):
    """0 .. 129 records per file (the op prefix and the Data / literal sums carried across
    rounds of 64), the empty source, the empty basis, sources shorter than a block."""
    _run_batch(gpu, oracle_c, monkeypatch, W.merged_batch())


def test_expand_op_counts_and_runs(gpu, oracle_c, monkeypatch):
    """Files of 63, 64, 65, 128 and 4097 ops; Copy runs of 1, 64, 65, 200 and 1000 blocks
    starting at op 0, 63 and 64; one run of 1024 blocks; a run of 1000 after 70 one-op records."""
    _run_batch(gpu, oracle_c, monkeypatch, W.opcount_batch())


@pytest.mark.parametrize("bs", [256, 320, 8192])
def test_expand_last_block(gpu, oracle_c, monkeypatch, bs):
    """A full-size last block matched mid-file and inside a run; a short one taken by the tail
    rule into the run that ends on block nbf - 2, and after a literal run."""
    _run_batch(gpu, oracle_c, monkeypatch, W.lastblock_batch(bs))


def test_expand_literal_joins_across_units(gpu, oracle_c, monkeypatch):
    """Three units per file: a literal run across one boundary, across a whole unit (three
    units' Data records, one op), and exactly one unit long."""
    _run_batch(gpu, oracle_c, monkeypatch, W.joins_batch())


def test_expand_shifted_units(gpu, oracle_c, monkeypatch):
    """Five units per file, the source shifted by 1 / 255 bytes: every later unit's leading
    literal ends at the previous exit (the record dropped), or passes it (cut there)."""
    _run_batch(gpu, oracle_c, monkeypatch, W.shifted_batch())


def test_expand_unit_that_does_not_chain(gpu, oracle_c, monkeypatch):
    """64 good files and one whose second unit starts with a Copy although the first unit's
    last Copy crosses the boundary: (0, 1), and every file exact."""
    _run_batch(gpu, oracle_c, monkeypatch, W.nochain_batch())


@pytest.mark.parametrize("which", [0, 1], ids=["64units", "65units"])
def test_expand_unit_count(gpu, oracle_c, monkeypatch, which):
    """A file in 64 units expands; one in 65 reports bad."""
    _run_batch(gpu, oracle_c, monkeypatch, W.unitcount_batches()[which])


def test_expand_delta_pairs(gpu, oracle_c, monkeypatch):
    """sydelta_delta_pairs_device on 130 good files (two groups): the device expands all 130."""
    batch = W.pairs_batch()
    monkeypatch.setenv("SYDELTA_FILE_SEGS", batch.segs)
    monkeypatch.delenv("SYDELTA_ASM_THREADS", raising=False)
    exp = _oracle_ops(oracle_c, batch.name, batch.files)
    bbuf, boff, blen = FW._pack([c.basis for c in batch.files])
    sbuf, soff, slen = FW._pack([c.src for c in batch.files])
    res = {}
    for dx in ("1", "0"):
        monkeypatch.setenv("SYDELTA_DEVICE_EXPAND", dx)
        x0 = FW._expanded()
        res[dx] = gpu.delta_pairs(bbuf, boff, blen, sbuf, soff, slen, batch.bs)
        x1 = FW._expanded()
        assert (x1[0] - x0[0], x1[1] - x0[1]) == ((130, 0) if dx == "1" else (0, 0)), (dx, x0, x1)
    _check(batch, exp, res["1"][0], res["1"][1], res["0"][0], res["0"][1])


# ---------------------------------------------------------------------------
# k_chunk_write
# ---------------------------------------------------------------------------
def _chunk_once(gpu, c):
    """The whole source as one final chunk of a single-file index: (the library's delta, the
    kernels launched)."""
    bs, L = c.bs, len(c.src)
    b = FW._to_dev(c.basis)
    w, s = gpu.signature(b[:len(c.basis)], bs)
    nb = w.numel()
    idx = gpu.Index(w, s, bs, len(c.basis) - (nb - 1) * bs)
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    ch = gpu.Chunk(idx, FW._to_dev(c.src), 0, L, 0, L)
    d, ex = ch.walk(0)
    prof = gpu.profile(reset=True)
    gpu.set_profiling(False)
    ch.close()
    idx.close()
    assert ex == L
    return d, prof


CHUNKS = W.chunk_cases()


@pytest.mark.parametrize("c", CHUNKS, ids=[c.name for c in CHUNKS])
def test_chunk_write(gpu, oracle_c, monkeypatch, c):
    """records_seg*: 1 .. 200 records per segment (rounds of 64; one run of 1024 Copies);
    ext: an extended last record at index 63, 64 and 130, and a wholly literal segment;
    skip: a dropped first record (the rounds start off the 64 grid), a cut one, one cut and
    extended; patch: the device-written part joins the host-assembled part's last op;
    rewalk: a unit walked again after the device wrote the ones before it; tail: the short
    last block in the final unit."""
    for k in ("SYDELTA_CHUNK_WALK", "SYDELTA_PROBE", "SYDELTA_CHUNK_PIPE", "SYDELTA_PREROLL", "SYDELTA_SLIM_WALK",
              "SYDELTA_CHUNK_SEG_LAST", "SYDELTA_CHUNK_SEG", "SYDELTA_DEVICE_EXPAND"):
        monkeypatch.delenv(k, raising=False)
    if c.seg != 128:
        monkeypatch.setenv("SYDELTA_CHUNK_SEG", str(c.seg))
    if c.dx:
        monkeypatch.setenv("SYDELTA_DEVICE_EXPAND", c.dx)
    exp = FW._oracle_ops(oracle_c, c.src, c.basis, c.bs)
    d, prof = _chunk_once(gpu, c)
    assert "k_walk_files" in prof and "k_chunk_write" in prof, prof
    if "stop" in c.claims:
        assert prof["k_walk_files"]["count"] >= 3, prof  # the two parts and the re-walk
    assert d.tuples() == exp
    monkeypatch.setenv("SYDELTA_DEVICE_EXPAND", "0")
    d0, prof0 = _chunk_once(gpu, c)
    assert "k_chunk_write" not in prof0, prof0
    assert d0.tuples() == exp
    assert {k: d.stats[k] for k in STATS} == {k: d0.stats[k] for k in STATS}
    for k, v in _counts(exp).items():
        assert d.stats[k] == v, k
    assert d.source_size == len(c.src) and d.block_size == c.bs
