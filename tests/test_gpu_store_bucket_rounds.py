"""Rounds of routed writes, deletes over views, reclaims and a replica sync of a
store of many collections on the GPU, against the many-collection store model.

tests/store_buckets.py's BucketRounds keeps all buckets in one bucketed column
and every bucket's record state beside it; each mixed batch is written by sort
-> route -> fetch -> honu_key_merge_buckets with nothing read on the host
between the route and the merge. After every step the whole arena, the offsets
and the counts are compared with tests/store_buckets_model.py (which tests/
test_store_buckets_model_host.py has checked against honu_amd/keys.py on the
same histories), and every per-bucket call runs over a view (d_sorted + 29
off[c], d_order + off[c], d_count + c) with that bucket's d_info: the checks of
tests/test_gpu_store_rounds.py, unchanged, on a Store whose column is the view.
The driver follows the header's recipe for d_info over views: a delete over a
view is followed by a honu_key_reclaim of that bucket before the counted merge
that squeezes it. Everything is bit-exact.
"""
import types
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import store_buckets_model as bm  # noqa: E402
import store_model as sm  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import NEXT_DTYPE, SEEK_FOUND, SEEK_NONE  # noqa: E402
from store_buckets import BucketRounds  # noqa: E402
from test_gpu_store_rounds import (MAX_RECORDS, _param, check_compare, check_shipped, check_store, gen, h,  # noqa: E402
                                   hosts)


@pytest.fixture(scope="module")
def codecs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cs = [hobj.Codec(0, MAX_RECORDS), hobj.Codec(0, MAX_RECORDS)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def T(codecs):
    tiles = {_param(codecs[0], name) for name in (b"merge_tile", b"delete_tile", b"list_tile", b"filter_tile")}
    assert tiles == {sm.TILE}  # the T the coverage conditions were shown for on the CPU
    return tiles.pop()


@pytest.fixture(scope="module")
def S(codecs):
    return _param(codecs[0], b"merge_buckets_stage")


@pytest.fixture(scope="module")
def marshal(oracle_lib):
    return oracle_lib.marshal_batch


# --------------------------------------------------------------------------
# the references: every history on the model alone, computed once and shared
# --------------------------------------------------------------------------
Ref = namedtuple("Ref", "step result arena views next")  # what the store is to hold and answer after a step
View = namedtuple("View", "n exp records freed")         # one bucket, in the store's numbering


def snapshot(model, probes, buckets, freed=None):
    """The buckets' expectations as plain values; freed: (bucket, the records a delete freed, numbered before it)."""
    out = {}
    for c in buckets:
        n = model.buckets[c].n
        exp = model.on_device(c, model.expectations(c, probes[c])) if n else None
        out[c] = View(n, exp, model.records_on_device(c), freed[1] if freed and freed[0] == c else None)
    return out


def next_wants(model, c, hist):
    """StoreModel.write of each op on a copy of bucket c's model: the rows (parent_record in the store's
    numbering), keys and statuses honu_key_next is to write."""
    req, status = hist.next_requests
    dev, out = model.dev[c], []
    for op in range(4):
        want = bm.clone(model).buckets[c].write(op, req, status, sm.PID, sm.REGION, sm.NOW, gen(740 + op, len(req)))
        rows = want.rows.copy()
        stored = rows["parent_record"] != SEEK_NONE
        rows["parent_record"][stored] = [dev[i] for i in rows["parent_record"][stored]]
        assert (op == sm.CREATE or stored.sum() >= 5) and len(set(rows["flags"].tolist())) >= 3, op
        out.append((rows, want.keys, want.status))
    return out


def reference(model, hist, steps, marshal, buckets=(), cover=None, next_at=()):
    """The steps on the model: a Ref per step, with the views of the buckets (of `buckets`) the step wrote."""
    refs = []
    for step in steps:
        c = step.get("bucket")
        dev = list(model.dev[c]) if c is not None else None
        result = bm.apply_step(model, step, gen, marshal, hist.ids)
        if cover is not None:
            cover.after(model, step, result)
        freed = (c, [dev[i] for i in result]) if step["kind"] in ("drop", "compact") else None
        assert freed is None or freed[1]
        which = buckets if step["kind"] == "put" else [b for b in buckets if b == c]
        refs.append(Ref(step, result, model.arena(), snapshot(model, hist.probes, which, freed),
                        next_wants(model, hist.HOT, hist) if step["name"] in next_at else None))
    return refs


@pytest.fixture(scope="module")
def narrow(T, marshal):
    """The narrow history on the model: (history, a Ref per step, the model at its end)."""
    hist = bm.Narrow(T)
    model, cover = bm.BucketsModel(marshal, hist.table), bm.NarrowCoverage(hist)
    refs = reference(model, hist, hist.steps, marshal, range(hist.K), cover, next_at=("c4 compact", "e put"))
    cover.check(model)
    return hist, refs, model


@pytest.fixture(scope="module")
def replicas(narrow, marshal):
    """The replica history on the model: the second store's steps, then per direction what every bucket
    ships, the mixed batch, and the receiver after it; at the end both models."""
    hist, _, first = narrow
    ma, mb = bm.clone(first), bm.BucketsModel(marshal, hist.table)
    own = reference(mb, hist, hist.base + hist.own, marshal)
    syncs = []
    for n, (mx, my) in enumerate(((ma, mb), (mb, ma))):
        senders = [([mx.buckets[c].records[i][0] for i in _by_device(mx, c)], mx.records_on_device(c), list(mx.dev[c]))
                   for c in range(hist.K)]
        ships, batch, (cls, _) = mx.ship(my)
        if n == 0:
            bm.check_replica_coverage(ships, batch)
        syncs.append((senders, ships, batch, cls, my.arena(), snapshot(my, hist.probes, range(hist.K))))
    agree = [(len(ma.buckets[c].groups()), ma.buckets[c].compare(mb.buckets[c])) for c in range(hist.K)]
    return own, syncs, agree


def _by_device(model, c):
    """The model's record indices of bucket c, by the store's index."""
    out = [None] * len(model.dev[c])
    for i, d in enumerate(model.dev[c]):
        out[d] = i
    return out


@pytest.fixture(scope="module")
def wide(T, S, marshal):
    hist = bm.Wide(T, S)
    model = bm.BucketsModel(marshal, hist.table)
    refs, before = [], None
    for step in hist.steps:
        if step["name"] == "3 put":  # after the drops and the reclaims: count < rows in the dropped buckets
            emptied, never = hist.sample[2], hist.sample[3]
            assert model.buckets[emptied].n == 0 < model.rows(emptied) and model.rows(never) == 0
            refs[-1] = refs[-1]._replace(views=snapshot(model, hist.probes, hist.sample))
            before = model.arena()["off"]
        refs += reference(model, hist, [step], marshal, hist.sample)
        if step["kind"] == "put":
            assert all(len(t) > S for t in bm.tiles_touch(model.arena()["off"], T))
    bm.check_wide_coverage(hist, before, model.arena()["off"], [refs[-1].result[2].count(c) for c in range(hist.k)])
    return hist, refs


# --------------------------------------------------------------------------
# the store against the references
# --------------------------------------------------------------------------
def check_arena(store, a):
    """The whole bucketed column in one host comparison: offsets, counts, every row's bytes and record index,
    the rows behind a bucket's valid ones included."""
    off, count, col, order = hosts(store.off, store.count, store.col, store.order)
    total = a["off"][-1]
    assert off.view(np.int64).tolist() == a["off"] == store.host_off.tolist()
    assert count.view(np.int64).tolist() == a["count"]
    assert col[:29 * total].tobytes() == a["col"]
    assert order.view(np.uint32)[:total].tolist() == a["order"]


def check_view(store, c, want: View, d_probes):
    """Bucket c's view and record state: everything check_store compares for a store, and the record bytes
    under every record index. A bucket without records has no d_info to give: its view finds nothing."""
    v = store.views[c]
    assert v.n == want.n
    if want.n == 0:
        rows = h(store.c.seek_keys(v.col, v.valid, d_probes, 17, m=d_probes.numel() // 29)).view(np.uint32)
        assert (rows[:, 4] & SEEK_FOUND == 0).all() and (rows[:, :2] == 0).all() and int(v.valid.item()) == 0
        return
    exp = want.exp
    check_store(v, exp, d_probes, v.probes(exp["live_status"]), want.freed, some_hit=bool(exp["hits"]))
    rec_off, arena = hosts(v.rec_off, v.arena)
    rec_off = rec_off.view(np.int64)
    assert [arena[rec_off[r]:rec_off[r + 1]].tobytes() for r in range(v.n)] == want.records


def run_step(store, step, result):
    kind = step["kind"]
    if kind == "put":
        return store.put(result[0], spoil=step["spoil"], counted=step["counted"])
    if kind == "drop":
        return store.drop(step["bucket"], step["prefixes"])
    if kind == "compact":
        return store.drop(step["bucket"], None, 29, superseded=True)
    return store.reclaim(step["bucket"])


def check_put(routed, batch, cls, k):
    """What the chain itself returned: the decoded keys and statuses, and every class's size."""
    keys, status, fetched, count = hosts(routed.keys, routed.key_status, routed.fetch_status, routed.route.bucket_count)
    ok = np.array([s == sm.OK for s in batch.statuses])
    assert np.array_equal(status.view(np.int32) == 0, ok)
    assert keys.reshape(-1, 29)[ok].tobytes() == b"".join(key for key, good in zip(batch.keys, ok) if good)
    assert count.view(np.int64).tolist() == [cls.count(c) for c in range(k + 2)]
    assert (fetched.view(np.int32)[:int(routed.bucket_off[k])] == 0).all()


def check_next(store, c, wants, hist):
    """One honu_key_next of each op over bucket c's view, outputs only."""
    v = store.views[c]
    req, status = hist.next_requests
    m = len(req)
    d_req, d_skip = v._upload(req, np.asarray(status, np.int32))
    got = [store.c.next_versions(v.col, v.valid, d_req, op, sm.PID, sm.REGION, sm.NOW, order=v.order, info=v.info,
                                 req_status=d_skip, m=m) for op in range(4)]
    out = hosts(*[t for g in got for t in g])
    for op, (rows, keys, status) in enumerate(wants):
        g_rows, g_keys, g_status = out[3 * op:3 * op + 3]
        bad = np.flatnonzero(g_rows.view(NEXT_DTYPE) != rows)
        assert not len(bad), (op, bad[:4], g_rows.view(NEXT_DTYPE)[bad[:4]], rows[bad[:4]])
        assert g_keys.tobytes() == keys.tobytes() and np.array_equal(g_status.view(np.int32), status)


def play(store, refs, hist=None, d_probes=None, checked=lambda step: True):
    """The steps on the store. With d_probes every step that `checked` names is compared with its Ref: the
    arena, what a put returned, the views of the buckets the step wrote, honu_key_next over the hot view."""
    for ref in refs:
        got = run_step(store, ref.step, ref.result)
        if d_probes is None or not checked(ref.step):
            continue
        check_arena(store, ref.arena)
        if ref.step["kind"] == "put":
            check_put(got, ref.result[1], ref.result[2], store.k)
        for c, want in ref.views.items():
            check_view(store, c, want, d_probes[c])
        if ref.next is not None:  # at (c) count < rows, after (e) rows == records
            v = store.views[hist.HOT]
            assert (int(v.valid.item()) < v.n) == (ref.step["kind"] != "put")
            check_next(store, hist.HOT, ref.next, hist)


@pytest.mark.parametrize("part", ["put", "drop compact reclaim"])
def test_narrow_rounds_against_the_model(codecs, narrow, part):
    """The whole narrow history on the store, twice: once with every put checked, once with every delete
    over a view and every reclaim (two tests, so that neither is longer than the one-bucket rounds)."""
    hist, refs, _ = narrow
    store = BucketRounds(codecs[0], hist.table)
    play(store, refs, hist, [store.front.probes(p) for p in hist.probes], lambda step: step["kind"] in part)


def test_replicas_of_a_bucketed_store_converge(codecs, narrow, replicas):
    hist, refs, _ = narrow
    own, syncs, agree = replicas
    a, b = BucketRounds(codecs[0], hist.table), BucketRounds(codecs[1], hist.table)
    play(a, refs)
    play(b, own)
    dp = {id(s): [s.front.probes(p) for p in hist.probes] for s in (a, b)}
    check_arena(a, refs[-1].arena)
    check_arena(b, own[-1].arena)
    for (x, y), (senders, ships, batch, cls, arena, views) in zip(((a, b), (b, a)), syncs):
        gathered = x.gather(y)
        torch.cuda.synchronize()
        for c, (got, want) in enumerate(zip(gathered, ships)):
            keys, records, dev = senders[c]
            if got is None:
                assert want.idx == [] and not records
                continue
            check_compare(got.compared, want.compared)
            sender = types.SimpleNamespace(records=[(key, None, rec) for key, rec in zip(keys, records)])
            check_shipped(sender, got, want.visits, [dev[i] for i in want.idx])
        routed = x.ship(y, gathered)
        assert routed.m == len(batch.keys) >= 50
        check_put(routed, batch, cls, y.k)
        check_arena(y, arena)
        for c, want in views.items():
            check_view(y, c, want, dp[id(y)][c])
    # both stores agree, bucket by bucket, on every object's latest version and on what a Retrieve reads
    for c, (objects, compared) in enumerate(agree):
        va, vb = a.views[c], b.views[c]
        if objects == 0:
            assert va.n == vb.n == 0
            continue
        la, lb = va.latest_of_all(want_keys=True), vb.latest_of_all(want_keys=True)
        ra, rb = va.retrieve(dp[id(a)][c]), vb.retrieve(dp[id(b)][c])
        torch.cuda.synchronize()
        assert objects == int(la[1].item()) == int(lb[1].item())
        assert h(la[2])[:29 * objects].tobytes() == h(lb[2])[:29 * objects].tobytes()
        total = int(ra.val_total.item())
        assert total == int(rb.val_total.item()) and h(ra.values)[:total].tobytes() == h(rb.values)[:total].tobytes()
        assert h(ra.range_off).tolist() == h(rb.range_off).tolist()
        counts = check_compare(va.compare(vb.col, vb.valid), compared)
        assert counts["equal"] == counts["objects"]


def test_wide_rounds_against_the_model(codecs, S, wide):
    hist, refs = wide
    assert hist.k == 3 * S < _param(codecs[0], b"route_stage")
    store = BucketRounds(codecs[0], hist.table, keep=hist.sample)
    d_probes = {c: store.front.probes(p) for c, p in hist.probes.items()}
    # all k buckets in one host comparison, the reads with d_info on the six sampled ones: after each put,
    # and after the drops and reclaims (the last step before the counted put carries those views)
    play(store, refs, hist, d_probes, lambda step: step["kind"] == "put" or step is refs[-2].step)
    assert store.views[hist.sample[3]].n == 0


@pytest.fixture(scope="module")
def replay_reference(T, marshal):
    """(a), (b) and a drop from HOT with no reclaim (count < rows), then two batches of one size and another
    spread, each put on a copy: the steps, the batches, the arenas wanted."""
    hist = bm.Narrow(T)
    model = bm.BucketsModel(marshal, hist.table)
    refs = reference(model, hist, hist.steps[:3], marshal)
    again = hist.steps[1]["spec"]  # (b) once more: every key is stored already, and HOT comes last
    again = [r for r in again if r[0] != hist.HOT] + [r for r in again if r[0] == hist.HOT]
    m = len(again) - T // 2 + T // 10
    specs = [hist.steps[-2]["spec"][:m], again[:m]]
    assert len(specs[0]) == len(specs[1]) == m > T // 4
    batches, wants = [], []
    for j, spec in enumerate(specs):
        hb = bm.build_batch(gen, 760 + j, spec, hist.ids)
        want = bm.clone(model)
        want.put(bm.model_batch(marshal, hb))
        batches.append(hb)
        wants.append(want.arena())
    assert wants[0]["count"] != wants[1]["count"] and wants[0]["off"][1] - wants[1]["off"][1] > 100  # another spread
    return hist, refs, m, batches, wants


def test_captured_chain_replays_over_another_batch(codecs, replay_reference):
    """sort -> route -> counted honu_key_merge_buckets captured once on one stream, then replayed over a
    second batch of another spread, written on the device into the same arrays."""
    hist, refs, m, batches, wants = replay_reference
    codec, k = codecs[0], hist.K
    store = BucketRounds(codec, hist.table, keep=[])
    play(store, refs)
    check_arena(store, refs[-1].arena)
    front, inputs = store.front, []
    for hb in batches:
        b, _ = front._batch(hb)
        cap = front._room(hb)
        arena, _, out_off, _ = front._encode(b, cap)
        d = front._decode(arena, out_off, m, cap)
        keys, st = codec.keys(d)
        inputs.append((keys[:29 * m].clone(), st[:4 * m].clone(), d.meta[:352 * m].view(m, 352)[:, 112:128].contiguous()))
    keys, st, ids = (t.clone() for t in inputs[0])

    def chain():
        order, _, _ = codec.sort_keys(keys, st, n=m)
        r = codec.route_keys(ids, m, store.table, k, id_stride=16, status=st, seq=order, keys=keys)
        return codec.merge_bucket_keys(k, store.col, store.order, store.off, r.keys, r.local, r.bucket_off,
                                       count_a=store.count, nb=m, base=store.base)

    chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = chain()
    for j, want in enumerate(wants):
        for dst, src in zip((keys, st, ids), inputs[j]):
            dst.copy_(src)
        for t in (res.sorted, res.order, res.off, res.count):  # (a stale result must not pass; what the capture's
            t.view(torch.uint8).fill_(0xEE)                    # pool lays behind row T is not the call's to keep)
        g.replay()
        torch.cuda.synchronize()
        off, count, col, order = hosts(res.off, res.count, res.sorted, res.order)
        total = want["off"][-1]
        assert off.view(np.int64).tolist() == want["off"] and count.view(np.int64).tolist() == want["count"], j
        assert col[:29 * total].tobytes() == want["col"] and order.view(np.uint32)[:total].tolist() == want["order"], j
