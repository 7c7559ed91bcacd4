"""The store model (tests/store_model.py) against the project's other host
statement, honu_amd/keys.py, over the two histories of the store tests, and the
histories' coverage conditions. No GPU.

After every batch the model's column, its answer to the batch and its reads are
recomputed with keys.sort, seek, merge, delete, compact, scan, filter, fetch,
next and compare over the column before and after. The model is written from
the header's comments without those functions, so what tests/
test_gpu_store_rounds.py compares the GPU with is what two independent
statements agree on. The coverage conditions are asserted here on the model:
they hold before any GPU run.
"""
import pytest

import store_model as sm
from honu_amd import keys as hkeys
from honu_amd.metadata import (CMP_ANCESTOR, CMP_EARLIER, CMP_EQUAL, CMP_LATER, CMP_PEER_HAS, NEXT_ASSIGNED, SEEK_FOUND,
                               SEEK_NONE)
from honu_amd.workload import gen_host_batch

T = sm.TILE  # the GPU test asserts that the library's tiles are this


def gen(seed, n):
    return gen_host_batch(seed, "small", 0, n)


@pytest.fixture(scope="module")
def marshal(oracle_lib):
    return oracle_lib.marshal_batch


def snapshot(model):
    return list(model.column()), list(model.keys())


def check_step(model, before, step, result):
    """The step's answer and the column after it, by honu_amd.keys over the column before it."""
    col0, keys0 = before
    col1, keys1 = snapshot(model)
    assert keys1 == hkeys.sort(model.records[i][0] for i in model.live)
    kind = step["kind"]
    if kind == "write":
        req, status = step["requests"]
        res = hkeys.next(keys0, [bytes(r) for r in req], step["op"], step.get("pid", sm.PID),
                         live=lambda p: not model.records[col0[p]][1], skip=[s != 0 for s in status])
        for i, g in enumerate(res):
            row = result.rows[i]
            assert int(row["flags"]) == g.flags, (i, hex(int(row["flags"])), hex(g.flags))
            assert bytes(result.keys[i]) == g.key
            assert (int(row["pid"]), int(row["vid"])) == ((g.scalar.PID, g.scalar.VID) if g.scalar else (0, 0))
            assert (int(row["parent_pid"]), int(row["parent_vid"])) == ((g.parent.PID, g.parent.VID) if g.parent else (0, 0))
            assert int(row["parent_record"]) == (SEEK_NONE if g.parent_pos is None else col0[g.parent_pos])
            assert (result.status[i] == 0) == bool(g.flags & NEXT_ASSIGNED)
        new = hkeys.sort(g.key for g in res if g.flags & NEXT_ASSIGNED)
        assert keys1 == hkeys.merge(keys0, new)
    elif kind == "put_stored":
        assert keys1 == hkeys.merge(keys0, hkeys.sort(result[1]))
    elif kind == "drop":
        kept, removed = hkeys.delete(keys0, [bytes(p[:17]) for p in step["prefixes"]])
        assert keys1 == kept and [model.records[i][0] for i in result] == removed
    elif kind == "compact":
        kept, removed = hkeys.compact(keys0)
        assert keys1 == kept and [model.records[i][0] for i in result] == removed
    assert sorted(model.order()) == list(range(model.n))


def check_reads(model, probes):
    col, keys = snapshot(model)
    values = [r[2] for r in model.records]
    tomb = lambda r: model.records[r][1]  # noqa: E731
    ranges = [hkeys.seek(keys, bytes(p[:17])) for p in probes]
    retrieve = hkeys.filter(keys, hkeys.scan(keys, ranges, reverse=True, limit=1), tomb, col)
    want = [None] * len(probes)
    for (q, _), rec in zip(retrieve, hkeys.fetch(values, retrieve, col)):
        want[q] = rec
    got = model.retrieve(probes)
    assert [None if i is None else values[i] for i in got] == want
    walk = hkeys.scan(keys, ranges, reverse=True)
    assert model.versions(probes, True) == hkeys.filter(keys, walk, tomb, col, deleted=True)
    assert model.versions(probes, False) == hkeys.filter(keys, walk, tomb, col)
    assert model.latest_of_all() == [p for _, p in hkeys.scan(keys, [(0, len(keys))], latest=True)]
    offs, latest = model.objects()
    assert offs[-1] == len(keys) and [p - 1 for p in offs[1:]] == model.latest_of_all()
    assert latest == [col[p] for p in model.latest_of_all()]
    return got


def check_compare(a, b, digest=None):
    cmp = a.compare(b, digest)
    want = hkeys.compare(a.keys(), b.keys() if digest is None else digest)
    assert cmp.rows == [(c.pos, c.end, c.flags, c.peer) for c in want]
    f = [c.flags for c in want]
    has = [x for x in f if x & CMP_PEER_HAS]
    assert cmp.counts == [len(f), len(f) - len(has), sum(1 for x in has if x & CMP_LATER),
                          sum(1 for x in f if x & CMP_EARLIER), sum(1 for x in f if x & CMP_EQUAL),
                          sum(1 for x in has if not x & CMP_ANCESTOR), 0, 0]
    assert all(bool(x & SEEK_FOUND) == (r[0] < r[1]) for x, r in zip(f, cmp.rows))
    return cmp


def check_ship(a, b, cap, digest=None):
    col, keys = snapshot(a)
    before = snapshot(b)
    cmp = check_compare(a, b, digest)
    visits, idx = a.ship(b, cap, digest)
    assert visits == hkeys.scan(keys, [(r[0], r[1]) for r in cmp.rows])
    assert [a.records[i][2] for i in idx] == hkeys.fetch([r[2] for r in a.records], visits, col)
    assert b.keys() == hkeys.merge(before[1], hkeys.sort(keys[p] for _, p in visits))
    return visits, idx


def test_rounds_on_the_model(marshal):
    rounds = sm.Rounds(T)
    model, cover = sm.StoreModel(marshal), sm.Coverage(rounds)
    bytes_before = None
    for step in rounds.steps:
        before = snapshot(model)
        result = sm.apply_step(model, step, gen)
        check_step(model, before, step, result)
        got = check_reads(model, rounds.probes)
        cover.after(model, step, result)
        vd, vt = model.versions(rounds.probes, True), model.versions(rounds.probes, False)
        if step["name"] >= "3":
            assert vd != vt
        if step["kind"] == "put_stored":  # the later arrival's bytes win
            hb, keys, first = result
            tops = {model.records[i][0]: i for i in got if i is not None}
            hit = [k for k in keys if k in tops]
            assert len(hit) >= 10 and all(tops[k] >= first for k in hit)
            bytes_before = [None if i is None else model.records[i][2] for i in got]
        if step["kind"] == "compact":  # and compaction frees exactly the older records
            assert len(result) >= 50 and len(set(model.keys())) == model.valid
            assert [None if i is None else model.records[i][2] for i in got] == bytes_before
    cover.check(model)


def test_replicas_on_the_model(marshal):
    h = sm.Replicas()
    a, b = sm.StoreModel(marshal), sm.StoreModel(marshal)
    for model, steps in ((a, h.base + h.a), (b, h.base + h.b)):
        for step in steps:
            before = snapshot(model)
            check_step(model, before, step, sm.apply_step(model, step, gen))
    # each class at least 5 times in at least one direction before the sync
    ab, ba = check_compare(a, b), check_compare(b, a)
    for k in range(1, 6):
        assert max(ab.counts[k], ba.counts[k]) >= 5, (k, ab.counts, ba.counts)
    digest = [a.keys()[p] for p in a.latest_of_all()]
    sent_ab, _ = check_ship(a, b, a.n)
    sent_ba, _ = check_ship(b, a, b.n)
    assert len(sent_ab) >= 5 and len(sent_ba) >= 5
    for x, y in ((a, b), (b, a)):
        c = check_compare(x, y)
        assert c.counts[4] == c.counts[0] and c.counts[1] == c.counts[2] == c.counts[3] == 0, c.counts
    ra, rb = check_reads(a, h.probes), check_reads(b, h.probes)
    assert [None if i is None else a.records[i][2] for i in ra] == [None if i is None else b.records[i][2] for i in rb]
    assert sum(i is None for i in ra) >= 20  # A's deletes reached B, and B's later forks won where they are later
    for x, y in ((a, b), (b, a)):  # a second sync ships nothing
        keys = list(x.keys()), list(y.keys())
        assert check_ship(x, y, 64)[0] == [] and (list(x.keys()), list(y.keys())) == keys
    # B ships once more against the digest of A taken before the sync: duplicates, which compaction frees
    keys_a = list(a.keys())
    again, _ = check_ship(b, a, 256, digest)
    assert len(again) == len(sent_ba) and a.valid == len(keys_a) + len(again)
    assert [None if i is None else a.records[i][2] for i in check_reads(a, h.probes)] == \
        [None if i is None else b.records[i][2] for i in rb]
    assert len(a.compact()) == len(again) and a.keys() == keys_a
