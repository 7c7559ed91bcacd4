"""Rounds of writes, deletes and replica syncs on the GPU against the store model.

Every honu_key_* call is documented as "fit for" the next one. Here a store
that holds only device state (tests/store_gpu.py) takes batch after batch, each
call's output the next call's input as the header says it may be, and after
every batch its whole state and every read path are compared with a
dict-and-list model (tests/store_model.py), which tests/test_store_model_host.py
has checked against honu_amd/keys.py on the same histories. What no one-step
chain sees is covered by construction (the coverage conditions, asserted on the
model there and here): delete outputs as inputs, with removed rows byte-equal
to live keys; record indices across many batches (b_base, the concatenated
info); valid far below n; every user of the context's scan state back to back;
Puts of stored keys and their compaction; two replicas end to end.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import store_model as sm  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (CMP_COUNTS_DTYPE, INFO_DTYPE, LIST_ROW_HEAD, LIST_ROW_TOMBSTONE, META_DTYPE,  # noqa: E402
                               NEXT_ASSIGNED, NEXT_DTYPE, SEEK_NONE)
from honu_amd.workload import gen_host_batch  # noqa: E402
from store_gpu import Store  # noqa: E402

L = hobj._lib
OK = hobj.OK
MAX_RECORDS = 1 << 14


@functools.lru_cache(maxsize=None)
def gen(seed, n):
    """The generator's batch: the model and the store are handed the same one, and neither changes a write's."""
    return gen_host_batch(seed, "small", 0, n)


def _param(c, name):
    v = L.C.c_int64(0)
    L.check(c.lib.honu_ctx_get_param(c.ctx, name, L.C.byref(v)), name.decode())
    return int(v.value)


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
    """The rows one workgroup takes: the common value of the tiles that count column or list rows.
    "compare_tile" counts objects, not rows; the replica test checks that its objects span more than one."""
    tiles = {_param(codecs[0], name) for name in (b"merge_tile", b"delete_tile", b"list_tile", b"filter_tile")}
    assert len(tiles) == 1
    return tiles.pop()


@pytest.fixture(scope="module")
def marshal(oracle_lib):
    return oracle_lib.marshal_batch


def h(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.reshape(-1).view(dtype)


def hosts(*tensors):
    """The bytes of several device tensors in ONE copy to the host: they are gathered on the device first,
    since every copy to pageable memory is a wait of its own."""
    flat = [t.reshape(-1).view(torch.uint8) for t in tensors]
    at = np.concatenate([[0], np.cumsum([-(-f.numel() // 8) * 8 for f in flat])])
    buf = torch.empty(max(int(at[-1]), 8), dtype=torch.uint8, device=tensors[0].device)
    for f, o in zip(flat, at):
        buf[o:o + f.numel()].copy_(f)
    host = buf[:int(at[-1])].cpu().numpy()
    return [host[o:o + f.numel()] for f, o in zip(flat, at)]


def uvarint(rec, at):
    x = shift = 0
    while True:
        x |= (rec[at] & 0x7F) << shift
        if rec[at] < 0x80:
            return x
        at, shift = at + 1, shift + 7


# --------------------------------------------------------------------------
# the store against the model
# --------------------------------------------------------------------------
def check_batch(marshal, step, got, want):
    """What the batch itself returned: next's rows, keys and statuses, and the stamped and encoded records.
    (The batch has read its byte total by now, so the stream is idle. A delete returns nothing to read.)"""
    if step["kind"] == "write":
        rows, keys, key_status, enc, dst, dkeys, goff, garena = hosts(
            got.rows, got.keys, got.key_status, got.enc_status, got.decoded_status, got.decoded_keys, got.out_off, got.arena)
        rows = rows.view(NEXT_DTYPE)
        bad = np.flatnonzero(rows != want.rows)
        assert not len(bad), (step["name"], len(bad), bad[:4], rows[bad[:4]], want.rows[bad[:4]])
        assert keys.tobytes() == want.keys.tobytes()
        assert np.array_equal(key_status.view(np.int32), want.status)
        assigned = (want.rows["flags"] & NEXT_ASSIGNED) != 0
        assert (enc.view(np.int32)[assigned] == OK).all() and (dst.view(np.int32)[assigned] == OK).all()
        # next -> encode -> decode -> keys gives the keys next assigned
        assert np.array_equal(dkeys.reshape(-1, 29)[assigned], want.keys[assigned])
        arena, off = want.arena, want.off
    else:
        hb, keys, _ = want
        arena, off, _ = marshal(hb)
        enc, key_status, gkeys, goff, garena = hosts(got.enc_status, got.key_status, got.keys, got.out_off, got.arena)
        assert (enc.view(np.int32) == OK).all() and (key_status.view(np.int32) == OK).all()
        assert gkeys.tobytes() == b"".join(keys)
    goff = goff.view(np.int64)
    assert np.array_equal(goff, off.astype(np.int64))
    assert garena[:int(goff[-1])].tobytes() == arena.tobytes()  # every record, the ASSIGNED rows stamped


def check_store(store, exp, d_probes, d_status, freed=None, some_hit=True):
    """The store's whole state and every read path against the model's expectations (store_model.
    expectations), after one synchronisation. some_hit: the probes are to find some objects and miss some
    (a caller whose store may hold no live object says False). d_probes and d_status (the keys' statuses with every
    non-live record not OK) were uploaded before the step was issued, so that nothing here waits: after a
    delete the context's scan state goes on to the sort, the lists, the filters and the fetch with no
    synchronisation between. One key_objects and one seek serve every read."""
    c = store.c
    n, valid, col = exp["n"], exp["valid"], exp["col"]
    m = d_probes.numel() // 29
    assert store.n == n
    # issue everything, then read once
    s_order, s_sorted, s_valid = c.sort_keys(store.keys, d_status, n=n, want_sorted=True)
    objects = store.objects()
    seeks = store.seek(d_probes)
    R = store.retrieve(d_probes, seeks)
    VD = store.versions(d_probes, True, seeks, objects)
    VT = store.versions(d_probes, False, seeks)
    l_rows, l_total, _ = store.latest_of_all(objects=objects)
    removed = store.removed if freed is not None else store.valid
    (g_valid, g_col, g_order, s_valid, s_order, s_sorted, g_removed, obj_off, latest, k, r_rows, r_off, r_total, r_keys,
     val_off, val_total, r_status, meta2, info2, vd_rows, vd_total, vd_all, vt_rows, vt_total, vt_all, l_rows,
     l_total) = hosts(store.valid, store.col, store.order, s_valid, s_order, s_sorted, removed, *objects, R.rows,
                   R.range_off, R.total, R.keys, R.val_off, R.val_total, R.status, R.decoded.meta[:352 * m],
                   R.decoded.info[:32 * m], VD.rows, VD.total, VD.unfiltered_total, VT.rows, VT.total,
                   VT.unfiltered_total, l_rows, l_total)
    one = lambda a: int(a.view(np.int64)[0])  # noqa: E731

    # valid, the column's prefix bit for bit, the whole order, the tail's bytes where they are specified
    assert one(g_valid) == valid
    g_col, g_order = g_col.reshape(n, 29), g_order.view(np.uint32)
    assert g_col[:valid].tobytes() == exp["keys"]
    assert g_order[:valid].tolist() == col
    assert g_order.tolist() == exp["order"]
    assert g_col[valid:][exp["tail_known"]].tobytes() == exp["tail_bytes"]
    # the same prefix from a from-scratch sort of the concatenated keys, every non-live record not OK
    assert one(s_valid) == valid
    assert s_order.view(np.uint32)[:valid].tolist() == col and s_sorted[:29 * valid].tobytes() == exp["keys"]
    # a delete's removed rows name exactly the freed records
    if freed is not None:
        assert one(g_removed) == len(freed)
        assert g_order[valid:valid + len(freed)].tolist() == freed
    # the objects
    k = one(k)
    assert k == len(exp["obj_latest"]) and obj_off.view(np.int64)[:k + 1].tolist() == exp["obj_off"]
    assert latest.view(np.uint32)[:k].tolist() == exp["obj_latest"]

    # Retrieve of every object ever named, and of absent ones
    hits, recs = exp["hits"], exp["hit_records"]
    t = one(r_total)
    rows = r_rows.view(np.uint32).reshape(-1, 4)[:t]
    assert t == len(hits) and (0 < t < m or not some_hit)
    assert rows[:, :3].tolist() == hits
    assert (rows[:, 3] == LIST_ROW_HEAD).all()
    found = np.array([i is not None for i in exp["retrieve"]])
    assert np.array_equal(np.diff(r_off.view(np.int64)), found.astype(np.int64))  # empty for deleted, dropped, absent
    assert r_keys[:29 * t].tobytes() == b"".join(exp["hit_keys"])
    val_off = val_off.view(np.int64)
    assert val_off[:t + 1].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in recs])]).tolist()
    assert (val_off[t:] == val_off[t]).all() and one(val_total) == val_off[t]
    assert (r_status.view(np.int32)[:t] == OK).all()
    assert h(R.values[:int(val_off[t])]).tobytes() == b"".join(recs)  # the model's latest records, byte for byte
    meta2, info2 = meta2.view(META_DTYPE), info2.view(INFO_DTYPE)
    assert (info2["meta_status"][:t] == OK).all() and (info2["tombstone"][:t] == 0).all()
    assert meta2["object_id"][:t].tobytes() == b"".join(k[1:17] for k in exp["hit_keys"])
    assert meta2["vid"][:t].tolist() == [int.from_bytes(k[17:25], "big") for k in exp["hit_keys"]]
    assert meta2["pid"][:t].tolist() == [int.from_bytes(k[25:29], "big") for k in exp["hit_keys"]]
    assert info2["data_len"][:t].tolist() == [uvarint(r, 1) for r in recs]

    # Versions, most recent first: a deleted object's all gone, or the tombstone rows alone
    for j, (rv, tv, all_rows) in enumerate(((vd_rows, vd_total, vd_all), (vt_rows, vt_total, vt_all))):
        wantv = exp["versions"][j]
        rv = rv.view(np.uint32).reshape(-1, 4)[:one(tv)]
        assert one(tv) == len(wantv) and one(all_rows) == valid
        assert rv[:, :2].tolist() == wantv
        assert rv[:, 2].tolist() == exp["version_records"][j]
    # one row per object, at its latest version
    rl = l_rows.view(np.uint32).reshape(-1, 4)[:one(l_total)]
    assert one(l_total) == len(exp["tops"]) and (rl[:, 0] == 0).all() and rl[:, 1].tolist() == exp["tops"]
    assert rl[:, 2].tolist() == exp["top_records"]
    assert ((rl[:, 3] & LIST_ROW_TOMBSTONE) != 0).tolist() == exp["top_tombstones"]
    return g_col, valid


@pytest.fixture(scope="module")
def rounds_reference(marshal):
    """The first history on the model alone, computed once: what each step returns and what the store holds
    and answers after it. tests/test_store_model_host.py checks the same run against honu_amd/keys.py."""
    return sm.run_rounds(sm.TILE, marshal, gen)


def test_rounds_against_the_model(codecs, T, marshal, rounds_reference):
    assert T == sm.TILE  # the T the coverage conditions were shown for on the CPU
    rounds, steps, cover, model = rounds_reference
    store = Store(codecs[0])
    d_probes = store.probes(rounds.probes)
    kept_bytes = None
    for step, want, exp in steps:
        name, kind = step["name"], step["kind"]
        d_status = store.probes(exp["live_status"])  # before the step is issued: nothing waits after it
        freed = None
        if kind == "write":
            req, status = step["requests"]
            got = store.write(step["op"], req, status, sm.PID, sm.REGION, sm.NOW + step["seed"], gen(step["seed"], len(req)))
            check_batch(marshal, step, got, want)
        elif kind == "put_stored":
            got = store.put_raw(want[0])
            check_batch(marshal, step, got, want)
        elif kind == "drop":
            store.drop(step["prefixes"])
            freed = want
        else:
            store.compact()
            freed = want
        g_col, valid = check_store(store, exp, d_probes, d_status, freed)
        idx = exp["retrieve"]
        latest_bytes = [None if i is None else model.records[i][2] for i in idx]
        if name >= "3":
            assert exp["versions"][0] != exp["versions"][1]  # the two filters differ once there are tombstones
        if kind == "put_stored":  # the later arrival's bytes win: check_store compared them with the fetched arena
            tops = {model.records[i][0]: i for i in idx if i is not None}
            hit = [k for k in want[1] if k in tops]
            assert len(hit) >= 10 and all(tops[k] >= want[2] for k in hit)
            kept_bytes = latest_bytes
        if kind == "compact":
            assert len(freed) >= 50 and latest_bytes == kept_bytes
        # the coverage conditions that can be read off the device state
        if name == "2 update":
            assert valid > T
        if name >= "5":
            assert valid < T and store.n >= 2 * T + 1
        if name == "6b update":
            have = {r.tobytes() for r in g_col[:valid]}
            assert sum(r.tobytes() in have for r in g_col[valid:]) >= 10
    cover.check(model)


def check_model(store, model, probes, d_probes, freed=None, d_status=None):
    """check_store against the model as it stands."""
    exp = sm.expectations(model, probes)
    check_store(store, exp, d_probes, store.probes(exp["live_status"]) if d_status is None else d_status, freed)
    return exp["retrieve"]


# --------------------------------------------------------------------------
# two replicas
# --------------------------------------------------------------------------
def check_compare(got, want):
    k = int(got.objects.item())
    assert k == len(want.rows)
    rows = h(got.rows, np.uint32).reshape(-1, 5)
    assert [(int(r[0]), int(r[1]), int(r[4])) for r in rows[:k]] == [(r[0], r[1], r[2]) for r in want.rows]
    assert (rows[k:] == 0).all()
    assert h(got.peer, np.uint32)[:k].tolist() == [SEEK_NONE if r[3] is None else r[3] for r in want.rows]
    assert h(got.counts, np.uint64).tolist() == want.counts
    return h(got.counts, CMP_COUNTS_DTYPE)[0]


def check_shipped(sender, got, visits, idx):
    """The shipped rows and bytes: the model's [pos, end) gather."""
    t = int(got.total.item())
    rows = h(got.rows, np.uint32).reshape(-1, 4)[:t]
    assert t == len(visits) and [(int(q), int(p)) for q, p in rows[:, :2]] == visits and rows[:, 2].tolist() == idx
    recs = [sender.records[i][2] for i in idx]
    val_off = h(got.val_off)
    assert int(got.val_total.item()) == val_off[t] == sum(len(r) for r in recs) and (val_off[t:] == val_off[t]).all()
    assert h(got.values)[:int(val_off[t])].tobytes() == b"".join(recs)
    assert h(got.keys)[:29 * t].tobytes() == b"".join(sender.records[i][0] for i in idx)
    assert (h(got.status)[:t] == OK).all()
    return t


def test_two_replicas_converge(codecs, marshal):
    hist = sm.Replicas()
    assert len(hist.objs) > _param(codecs[0], b"compare_tile")  # the objects of a column span two workgroups
    ma, mb = sm.StoreModel(marshal), sm.StoreModel(marshal)
    a, b = Store(codecs[0]), Store(codecs[1])
    for model, store, steps in ((ma, a, hist.base + hist.a), (mb, b, hist.base + hist.b)):
        for step in steps:
            want = sm.apply_step(model, step, gen)
            req, status = step["requests"]
            got = store.write(step["op"], req, status, step["pid"], sm.REGION, sm.NOW + step["seed"],
                              gen(step["seed"], len(req)))
            check_batch(marshal, step, got, want)
    dp = {id(a): a.probes(hist.probes), id(b): b.probes(hist.probes)}  # the probes, on the device once
    check_model(a, ma, hist.probes, dp[id(a)])
    check_model(b, mb, hist.probes, dp[id(b)])

    # before the sync: each direction's rows, peer rows and counts
    cab = check_compare(a.compare(b.col, b.valid), ma.compare(mb))
    cba = check_compare(b.compare(a.col, a.valid), mb.compare(ma))
    for name in ("only_mine", "later", "earlier", "equal", "forks"):
        assert max(cab[name], cba[name]) >= 5, (name, cab, cba)
    _, _, digest_keys = a.latest_of_all(want_keys=True)  # one key per object of A, before the sync
    digest_model = [ma.keys()[p] for p in ma.latest_of_all()]
    digest = (digest_keys[:29 * len(digest_model)].clone(), torch.tensor([len(digest_model)], dtype=torch.int64,
                                                                         device=a.c.torch_device))
    assert h(digest[0]).tobytes() == b"".join(digest_model)

    # A ships to B, then B to A
    sent = []
    for x, mx, y, my in ((a, ma, b, mb), (b, mb, a, ma)):
        cap = x.n
        want_cmp = mx.compare(my)
        visits, idx = mx.ship(my, cap)
        got = x.ship_to(y)
        torch.cuda.synchronize()
        check_compare(got.compared, want_cmp)
        sent.append(check_shipped(mx, got, visits, idx))
        status = h(y.key_status)[got.first:got.first + cap]
        assert (status[:sent[-1]] == OK).all() and (status[sent[-1]:] != OK).all()  # the empty records past the total
        check_model(y, my, hist.probes, dp[id(y)])  # and they are no rows: valid and the whole order are the model's
    assert min(sent) >= 5

    # after the sync every object is equal in both directions, and reads are the same bytes on both
    for x, mx, y, my in ((a, ma, b, mb), (b, mb, a, ma)):
        c = check_compare(x.compare(y.col, y.valid), mx.compare(my))
        assert c["equal"] == c["objects"] and c["only_mine"] == c["later"] == c["earlier"] == 0
    ia = check_model(a, ma, hist.probes, dp[id(a)])
    ib = check_model(b, mb, hist.probes, dp[id(b)])
    winners = [None if i is None else ma.records[i][2] for i in ia]
    assert winners == [None if i is None else mb.records[i][2] for i in ib]
    ra, rb = a.retrieve(dp[id(a)]), b.retrieve(dp[id(b)])
    torch.cuda.synchronize()
    ta = int(ra.val_total.item())
    assert ta == int(rb.val_total.item()) and h(ra.values)[:ta].tobytes() == h(rb.values)[:ta].tobytes()
    assert h(ra.range_off).tolist() == h(rb.range_off).tolist()

    # a second sync ships nothing and leaves each [0, valid) as it was
    for x, mx, y, my in ((a, ma, b, mb), (b, mb, a, ma)):
        before = h(y.col)[:29 * my.valid].tobytes(), h(y.order)[:my.valid].tolist(), my.valid
        visits, idx = mx.ship(my, 64)
        got = x.ship_to(y, cap=64)
        torch.cuda.synchronize()
        assert visits == [] and int(got.total.item()) == 0 and int(got.val_total.item()) == 0
        assert (h(y.col)[:29 * my.valid].tobytes(), h(y.order)[:my.valid].tolist(), int(y.valid.item())) == before
        check_model(y, my, hist.probes, dp[id(y)])

    # B ships once more, against the digest of A taken before the sync: A merges duplicates, its reads do
    # not change, and compaction frees exactly the rows that were shipped again
    keys_before = h(a.col)[:29 * ma.valid].tobytes()
    valid_before = ma.valid
    want_cmp = mb.compare(ma, digest_model)
    visits, idx = mb.ship(ma, 256, digest_model)
    got = b.ship_to(a, cap=256, digest=digest)
    torch.cuda.synchronize()
    check_compare(got.compared, want_cmp)
    again = check_shipped(mb, got, visits, idx)
    assert again == sent[1] and int(a.valid.item()) == valid_before + again
    ia2 = check_model(a, ma, hist.probes, dp[id(a)])
    assert [None if i is None else ma.records[i][2] for i in ia2] == winners
    freed = ma.compact()
    d_status = a.probes(sm.expectations(ma, hist.probes)["live_status"])  # before the delete: nothing waits after it
    a.compact()
    check_model(a, ma, hist.probes, dp[id(a)], freed, d_status)
    assert len(freed) == again and h(a.col)[:29 * ma.valid].tobytes() == keys_before
