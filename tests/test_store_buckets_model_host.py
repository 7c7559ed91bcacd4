"""The many-collection store model (tests/store_buckets_model.py) against the
project's other host statement, honu_amd/keys.py, over the narrow and the wide
history, and the histories' coverage conditions. No GPU.

What tests/test_store_model_host.py is for the one-bucket model. After every
step the model's arena, offsets, counts and orders are recomputed with
keys.route, merge_buckets, delete, compact and reclaim over the state before
it, and every bucket's reads with keys.seek, scan, filter and fetch; a sync is
keys.compare, scan and fetch per bucket, then a route and a merge on the peer.
The coverage conditions are asserted here on the model: they hold before any
GPU run.
"""
import pytest

import store_buckets_model as bm
import store_model as sm
from honu_amd import keys as hkeys
from honu_amd.metadata import SEEK_NONE
from honu_amd.workload import gen_host_batch
from test_store_model_host import check_compare, check_reads

T = sm.TILE  # the GPU test asserts that the library's tiles are this
S = 160      # and that "merge_buckets_stage" is this


def gen(seed, n):
    return gen_host_batch(seed, "small", 0, n)


@pytest.fixture(scope="module")
def marshal(oracle_lib):
    return oracle_lib.marshal_batch


def views(model):
    """Per bucket (rows' keys, valid count, order in the store's numbering), from the arena's plain values."""
    a = model.arena()
    keys = [a["col"][29 * p:29 * p + 29] for p in range(a["off"][-1])]
    return [(keys[a["off"][c]:a["off"][c + 1]], a["count"][c], a["order"][a["off"][c]:a["off"][c + 1]])
            for c in range(model.k)]


def check_put(model, before, base, batch, first):
    """A put by keys.route and keys.merge_buckets over the views before it. base: the records each bucket held."""
    k, m = model.k, len(batch.keys)
    seq = sorted(range(m), key=lambda i: (batch.statuses[i] != 0, batch.keys[i] if batch.statuses[i] == 0 else b"", i))
    r = hkeys.route(batch.cids, model.table, batch.statuses, seq, batch.keys)
    segs = [r.keys[r.offsets[c]:r.offsets[c + 1]] for c in range(k)]
    merged = hkeys.merge_buckets([v[0] for v in before], segs, [v[1] for v in before])
    after = views(model)
    arrivals = [0] * k
    for c in range(k):
        keys, count, order = after[c]
        assert count == len(keys) == len(merged[c])                      # tight
        assert keys == [row.key for row in merged[c]]
        assert order == [before[c][2][row.index] if row.side == 0 else base[c] + row.index for row in merged[c]]
    # the route's rows name the records the model numbered: local + base is the store's index
    cls = model.classes(batch.cids, batch.statuses)
    for g, (c, _, i, _) in enumerate(r.rows):
        assert cls[i] == c
        if c < k:
            j = sum(1 for x in cls[:i] if x == c)                        # record i is the bucket's j-th arrival
            assert model.dev[c][first[c] + j] == base[c] + r.local[g]
            arrivals[c] += 1
    assert [model.buckets[c].n - first[c] for c in range(k)] == arrivals
    return r


def check_step(model, step, result, before, base):
    kind, c = step["kind"], step.get("bucket")
    after = views(model)
    if kind == "put":
        _, batch, _, first = result
        check_put(model, before, base, batch, first)
        return
    keys0, count0, order0 = before[c]
    keys1, count1, order1 = after[c]
    assert [after[j] for j in range(model.k) if j != c] == [before[j] for j in range(model.k) if j != c]
    if kind in ("drop", "compact"):
        kept, removed = (hkeys.delete(keys0[:count0], [bytes(p[:17]) for p in step["prefixes"]]) if kind == "drop"
                         else hkeys.compact(keys0[:count0]))
        assert keys1 == kept + removed + keys0[count0:] and count1 == len(kept)
        assert sorted(order1) == sorted(order0) and len(result) == len(removed)
        assert [model.buckets[c].records[i][0] for i in result] == removed
    elif kind == "reclaim":
        nrec = len(result["freed"]) + len(result["source"])
        old_dev = step["_dev_before"]
        values = [None] * nrec
        for i, d in enumerate(old_dev):
            values[d] = step["_records_before"][i][2]
        order_out, remap, source, values_out, *_ = hkeys.reclaim(order0, count0, values)
        assert keys1 == keys0 and count1 == count0 == len(source)
        assert order1 == order_out and model.records_on_device(c) == values_out
        assert all(x == SEEK_NONE for x in order1[count1:])


def drive(hist, steps, model, marshal, cover=None):
    for step in steps:
        before = views(model)
        base = [len(d) for d in model.dev]
        if step["kind"] == "reclaim":
            step = dict(step, _dev_before=list(model.dev[step["bucket"]]),
                        _records_before=list(model.buckets[step["bucket"]].records))
        result = bm.apply_step(model, step, gen, marshal, hist.ids)
        check_step(model, step, result, before, base)
        if cover is not None:
            cover.after(model, step, result)
        yield step, result, before


def test_narrow_history_on_the_model(marshal):
    hist = bm.Narrow(T)
    model, cover = bm.BucketsModel(marshal, hist.table), bm.NarrowCoverage(hist)
    for step, _, _ in drive(hist, hist.steps, model, marshal, cover):
        for c in range(hist.K):
            check_reads(model.buckets[c], hist.probes[c])
    cover.check(model)
    # honu_key_next's rules over the hot bucket stand on the per-bucket model as they are
    req, status = hist.next_requests
    for op in (sm.CREATE, sm.UPDATE, sm.MERGE, sm.DELETE):
        hot = bm.clone(model).buckets[hist.HOT]
        col0, keys0 = list(hot.column()), list(hot.keys())
        got = hot.write(op, req, status, sm.PID, sm.REGION, sm.NOW, gen(740 + op, len(req)))
        want = hkeys.next(keys0, [bytes(r) for r in req], op, sm.PID, live=lambda p: not hot.records[col0[p]][1],
                          skip=[s != 0 for s in status])
        assert [int(f) for f in got.rows["flags"]] == [g.flags for g in want]
        assert [bytes(k) for k in got.keys] == [g.key for g in want]

    # the replica: (a) and (b), a step of its own, then the first store ships to it and it ships back
    peer = bm.BucketsModel(marshal, hist.table)
    for _ in drive(hist, hist.base + hist.own, peer, marshal):
        pass
    for n, (x, y) in enumerate(((model, peer), (peer, model))):
        before, base = views(y), [len(d) for d in y.dev]
        for c in range(hist.K):
            check_compare(x.buckets[c], y.buckets[c])
        ships, batch, (_, first) = x.ship(y)
        for c, s in enumerate(ships):
            keys = x.buckets[c].keys()
            assert s.visits == hkeys.scan(keys, [(r[0], r[1]) for r in s.compared.rows])
            assert [x.buckets[c].records[i][2] for i in s.idx] == \
                hkeys.fetch([r[2] for r in x.buckets[c].records], s.visits, x.buckets[c].column())
        check_put(y, before, base, batch, first)
        if n == 0:
            bm.check_replica_coverage(ships, batch)
    for c in range(hist.K):  # both agree, bucket by bucket, on every object's latest version
        a, b = model.buckets[c], peer.buckets[c]
        assert [a.keys()[p] for p in a.latest_of_all()] == [b.keys()[p] for p in b.latest_of_all()]
        ia, ib = check_reads(a, hist.probes[c]), check_reads(b, hist.probes[c])
        assert [None if i is None else a.records[i][2] for i in ia] == [None if i is None else b.records[i][2] for i in ib]
        cmp = check_compare(a, b)
        assert cmp.counts[4] == cmp.counts[0]


def test_wide_history_on_the_model(marshal):
    hist = bm.Wide(T, S)
    model = bm.BucketsModel(marshal, hist.table)
    for step, result, before in drive(hist, hist.steps, model, marshal):
        if step["kind"] == "put":
            off = model.arena()["off"]
            assert all(len(t) > S for t in bm.tiles_touch(off, T)), step["name"]
            for c in hist.sample:
                check_reads(model.buckets[c], hist.probes[c])
    _, batch, cls, _ = result
    counts = [cls.count(c) for c in range(hist.k)]
    before_off = [0]
    for v in before:
        before_off.append(before_off[-1] + len(v[0]))
    bm.check_wide_coverage(hist, before_off, model.arena()["off"], counts)
    a = model.arena()
    assert a["off"][-1] == 2 * T
    assert all(a["count"][c] == 0 for c in hist.never) and len(hist.never) == hist.k // 10
    # the buckets that were dropped and not reclaimed hold more records than rows: no d_info over their views
    loose = [c for c in hist.drops if c not in hist.reclaimed]
    assert all(model.buckets[c].n > model.rows(c) for c in loose)
    assert all(model.buckets[c].n == model.rows(c) for c in hist.sample)
