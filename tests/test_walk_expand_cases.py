"""The inputs of tests/test_gpu_walk_expand.py proved on the CPU: every case's expected ops
equal the C oracle's, it has the record, op and unit counts it is named for, and the designed
record (the dropped or cut leading literal, the extended Data record, the Copy that starts a
unit) sits at the unit boundary it claims -- boundaries computed as match_walk_files and
chunk_units do (walk_expand_cases.file_units / chunk_units)."""
import pytest

import walk_expand_cases as W
from oracle import oracle as O


def _oracle_ops(oracle_c, src, basis, bs):
    w, s, z = oracle_c.compute_checksums(basis, bs)
    return O.ops_from_arrays(*oracle_c.generate_delta(src, w, s, z, bs))


def test_lds_cap_worked_values():
    """walk_lds + sydelta_filewalk.hip:680 by hand: 32 blocks: fw 64, (1792 + 512 + 128 - 272) / 20."""
    assert W.lds_cap(32) == 108
    assert W.lds_cap(64) == 140
    assert W.lds_cap(1024) == 1100
    assert W.lds_cap(0) == W.lds_cap(1) == (1792 + 512 + 4 * 4 - 272) // 20
    assert W.lds_cap(33) == (1792 + 8 * 128 + 4 * 36 - 272) // 20


def test_records_of_rule():
    bs = 256
    assert W.records_of([], bs) == 0
    assert W.records_of([("D", 0, 5)], bs) == 1
    # consecutive blocks: one run; the same block twice, or a gap: two
    assert W.records_of([("C", 0, bs), ("C", bs, bs), ("C", 2 * bs, 10)], bs) == 1
    assert W.records_of([("C", 0, bs), ("C", 0, bs)], bs) == 2
    assert W.records_of([("C", 0, bs), ("C", 2 * bs, bs)], bs) == 2
    assert W.records_of([("C", 0, bs), ("D", bs, 1), ("C", bs, bs)], bs) == 3


def test_builder_merges_adjacent_literals():
    src, basis, ops, rec = W.build([("D", 3), ("D", 4), ("X", 1), ("C", 1, 2), ("C", 0, 1), ("C", 3, 1)], 4, 256, ls=9, seed=1)
    assert ops == [("D", 0, 7 + 256), ("C", 256, 256), ("C", 512, 256), ("C", 0, 256), ("C", 768, 9)]
    assert rec == 4 and len(src) == 263 + 3 * 256 + 9 and len(basis) == 3 * 256 + 9


BATCHES = W.file_batches() + [W.pairs_batch()]


@pytest.mark.parametrize("batch", BATCHES, ids=[b.name for b in BATCHES])
def test_file_batch_cases(oracle_c, batch):
    bs, cap, G = batch.bs, batch.cap, int(batch.segs)
    assert 2 <= len(batch.files) <= 130 and batch.max_nblk <= 1024
    bad = []
    for c in batch.files:
        exp = _oracle_ops(oracle_c, c.src, c.basis, bs)
        assert c.ops == exp, (batch.name, c.name)
        assert c.records == W.records_of(exp, bs)
        cl = c.claims
        if "records" in cl:
            assert c.records == cl["records"], c.name
        if "nops" in cl:
            assert len(exp) == cl["nops"], c.name
        if "run" in cl:  # a run of k Copies of consecutive blocks from op index p, not joined to its neighbours
            p, k = cl["run"]
            run = exp[p:p + k]
            assert len(run) == k and all(o[0] == "C" for o in run), c.name
            assert [o[1] for o in run] == [run[0][1] + j * bs for j in range(k)], c.name
            assert p == 0 or exp[p - 1][0] == "D" or exp[p - 1][1] + bs != run[0][1]
            assert W.records_of(exp[:p], bs) == p, c.name  # (one-op records before it)
            assert p + k == len(exp) or exp[p + k][0] == "D"
        if "last" in cl:
            assert exp[-1] == cl["last"], c.name
            if "absorbed" in c.name:  # the run that ends on block nbf - 2 takes the short last block
                assert exp[-2] == ("C", exp[-1][1] - bs, bs) and W.records_of(exp[-3:], bs) == 1, c.name
            else:
                assert exp[-2][0] == "D", c.name
        m = W.expand_model(c.src, c.basis, bs, G, cap)
        if "nu" in cl:
            assert m["nu"] == cl["nu"], c.name
        if "events" in cl:
            assert m["events"] == cl["events"], (c.name, m["events"])
        if G == 1:
            assert m["nu"] == 1 and (m["bad"] == "cap" or m["counts"] == [c.records]), c.name
        if m["bad"]:
            bad.append((c.name, m["bad"]))
        else:
            assert m["ops"] == exp, (batch.name, c.name)
    if batch.expect == "dev":
        assert not bad, bad
    else:
        assert len(bad) == 1, bad


@pytest.mark.parametrize("nb", [32, 64, 1024])
def test_capacity_cases_sit_on_the_capacity(nb):
    good, over = W.capacity_batches(nb)
    cap = W.lds_cap(nb)
    assert good.max_nblk == over.max_nblk == nb and good.cap == cap
    recs = sorted(c.records for c in good.files if "records" in c.claims)
    assert recs == ([cap, cap] if nb == 1024 else [cap - 1, cap - 1, cap, cap])
    assert over.files[:-1] == good.files and over.files[-1].records == cap + 1
    for c in over.files:
        if "records" in c.claims:  # longer than their bases
            assert len(c.src) > len(c.basis) or nb == 1024 and len(c.src) > len(c.basis) // 2


def test_joins_cases_straddle_the_boundaries():
    b = W.joins_batch()
    by = {c.name: c for c in b.files}
    for name, lo, hi in (("lit_crosses", 2048, 2048), ("lit_swallows_unit", 2048, 4096), ("lit_is_unit", 2048, 4096)):
        c = by[name]
        units = W.file_units(len(c.src), len(c.basis) // 256, 256, 3)
        assert [u[0] for u in units] == [0, 2048, 4096]
        d = [o for o in c.ops if o[0] == "D"]
        assert len(d) == 1 and d[0][1] <= lo and d[0][1] + d[0][2] >= hi
    d = [o for o in by["lit_crosses"].ops if o[0] == "D"][0]
    assert d[1] < 2048 < d[1] + d[2] < 4096
    d = [o for o in by["lit_swallows_unit"].ops if o[0] == "D"][0]
    assert d[1] < 2048 and d[1] + d[2] > 4096  # three units' Data records, one op


def test_nochain_case_starts_a_unit_with_a_copy():
    c = next(c for c in W.nochain_batch().files if c.name == "nochain")
    units = W.file_units(len(c.src), len(c.basis) // 256, 256, 5)
    assert units[1][0] == W.NOCHAIN_E
    recs0, exit0 = W.walk_unit(c.src, c.basis, 256, *units[0])
    recs1, _ = W.walk_unit(c.src, c.basis, 256, *units[1])
    assert exit0 == W.NOCHAIN_E + 7 and recs0[-1][0] > 0      # the previous unit's Copy crosses E
    assert recs1[0] == [1, len(c.basis) // 256 - 1, 0]        # the appended block, at E
    assert len(W.nochain_batch().files) >= 65


CHUNKS = W.chunk_cases()


@pytest.mark.parametrize("c", CHUNKS, ids=[c.name for c in CHUNKS])
def test_chunk_cases(oracle_c, c):
    exp = _oracle_ops(oracle_c, c.src, c.basis, c.bs)
    assert c.ops == exp
    m = W.chunk_model(c.src, c.basis, c.bs, c.seg)
    plan, cl = m["plan"], c.claims
    if "stop" in cl:
        assert m["stop"] == cl["stop"] and len(m["ub"]) == 3 and m["ub"][1] < cl["stop"]
        assert m["units"][cl["stop"]][0] % (c.seg * c.bs) == 0
        assert all(p["event"] == "drop" and p["skip"] == 1 for p in plan[1:])
        return
    assert m["stop"] is None and m["ops"] == exp
    if "counts" in cl:  # records per segment, none joined or cut
        assert [p["cnt"] for p in plan[:len(cl["counts"])]] == list(cl["counts"])
        assert all(p["skip"] == 0 and not p["cut"] and not p["ext"] for p in plan)
        if c.seg == 1024:
            assert plan[0]["cnt"] == 1 and plan[0]["nops"] == 1024  # one run of 1024 Copies
    if "owners" in cl:
        for u, cnt in cl["owners"].items():
            assert plan[u]["cnt"] == cnt and plan[u]["skip"] == 0 and plan[u]["ext"] > 0, (u, plan[u])
            assert plan[u + 1]["join"] and plan[u + 1]["skip"] == 1
        s = cl["silent"]
        assert plan[s]["cnt"] == 1 and plan[s]["join"] and plan[s]["nops"] == 0 and plan[s + 1]["join"]
        assert plan[s - 1]["ext"] > c.seg * c.bs  # taken twice: the literal segment and the next one's start
    if c.name == "skip":
        assert (plan[1]["event"], plan[1]["skip"], plan[1]["cnt"]) == ("drop", 1, 102)
        assert (plan[2]["event"], plan[2]["cut"], plan[2]["skip"], plan[2]["cnt"]) == ("cut", 1, 0, 100)
        assert (plan[3]["event"], plan[3]["cut"], plan[3]["cnt"], plan[3]["ext"]) == ("cut", 1, 1, W.CHUNK_SHIFT + 256)
        assert plan[4]["join"] and plan[4]["skip"] == 1
    if "boundary" in cl:
        u = cl["boundary"]
        assert len(m["ub"]) == 3 and m["ub"][1] == u and len(plan) >= 512
        assert plan[u]["join"] and plan[u]["patch"] and plan[u]["skip"] == 1
    if c.name.startswith("tail"):
        assert len(plan) == 3 and exp[-1] == ("C", 299 * c.bs, c.bs // 2 + 3)
        assert (exp[-2][0] == "C") == ("absorbed" in c.name)
