"""honu_sort_keys and honu_key_objects on the GPU against numpy.

Expected order: np.lexsort over the 29 key bytes of the valid rows (stable),
then the invalid indices ascending; the sorted column is keys[order]; the
objects are the cut points of adjacent 17-byte prefixes. Independently of the
key bytes, d_latest is checked against the per-object maximum of
(VID, PID, index) taken from integer columns, which pins byte order to
lamport.Compare order (lamport/scalar.go:50-78) by a second route.

Every output and the workspace is a guarded view (tests/guards.py) under both
fills; the key column is passed at byte phases 0, 1 and 3.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import HAS_VERSION  # noqa: E402
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE, ERR_PANIC = -1, -2, 8
BIG = 1 << 17  # max_records of the shared context


# --------------------------------------------------------------------------
# expected values (numpy)
# --------------------------------------------------------------------------
def expected_order(k, st):
    ok = np.flatnonzero(st == 0)
    bad = np.flatnonzero(st != 0)
    rows = k[ok]
    srt = np.lexsort(rows.T[::-1]) if len(ok) else np.zeros(0, np.int64)  # stable; column 0 the primary key
    return np.concatenate([ok[srt], bad]).astype(np.uint32), len(ok)


def expected_objects(k, order, valid):
    if valid == 0:
        return np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    pre = k[order[:valid], :17]
    head = np.concatenate([[True], (pre[1:] != pre[:-1]).any(axis=1)])
    off = np.concatenate([np.flatnonzero(head), [valid]]).astype(np.uint64)
    latest = order[off[1:].astype(np.int64) - 1]
    return off, latest


def latest_by_columns(oid_label, vid, pid, st):
    """label -> the index with the largest (VID, PID, index) among the
    object's valid rows. No key byte is involved."""
    best = {}
    for i in np.flatnonzero(st == 0):
        t = (int(vid[i]), int(pid[i]), int(i))
        lab = oid_label[i]
        if lab not in best or t > best[lab][0]:
            best[lab] = (t, int(i))
    return {lab: v[1] for lab, v in best.items()}


def keys_from_columns(oid, vid, pid):
    """0x01 | oid | BE64(VID) | BE32(PID) (keys.go:42-51)."""
    n = len(vid)
    k = np.zeros((n, 29), np.uint8)
    k[:, 0] = 1
    k[:, 1:17] = oid
    k[:, 17:25] = vid.astype(">u8").view(np.uint8).reshape(n, 8)
    k[:, 25:29] = pid.astype(">u4").view(np.uint8).reshape(n, 4)
    return k


# --------------------------------------------------------------------------
# contexts: max_records == n for the small sizes (the count table of one tile
# has 256 rows, more than the scan state of such a context covers)
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codecs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(n):
        cap = max(n, 1) if n <= 257 else BIG
        if cap not in made:
            made[cap] = hobj.Codec(0, cap)
        return made[cap]

    yield get
    for c in made.values():
        c.close()


def sort_tile(codec):
    v = L.C.c_int64(0)
    L.check(codec.lib.honu_ctx_get_param(codec.ctx, b"sort_tile", L.C.byref(v)), "sort_tile")
    return int(v.value)


@pytest.fixture(scope="module")
def T(codecs):
    return sort_tile(codecs(BIG))


# --------------------------------------------------------------------------
# one guarded run of sort + objects
# --------------------------------------------------------------------------
class Run:
    pass


def guarded_run(codec, k, st, phase, fill, with_status=True, want_sorted=True, want_latest=True):
    n = len(k)
    dev = codec.torch_device
    g = lambda nbytes, ph=0: guards.guarded(nbytes, phase=ph, fill=fill, device=dev)  # noqa: E731
    r = Run()
    r.n = n
    r.keys = g(29 * n, phase)
    if n:
        r.keys.copy_(torch.from_numpy(np.ascontiguousarray(k).reshape(-1)).to(dev))
    r.status = hobj._dev_bytes(st.astype(np.int32), dev) if with_status else None
    r.work_bytes = int(codec.lib.honu_sort_keys_workspace(n))
    r.work = g(r.work_bytes)
    r.order, r.sorted, r.valid = g(4 * n), (g(29 * n, 1) if want_sorted else None), g(8)
    r.obj_off, r.latest, r.objects = g(8 * (n + 1)), (g(4 * n) if want_latest else None), g(8)
    return r


def call_sort(codec, r, work_bytes=None, n=None, order="own"):
    return codec.lib.honu_sort_keys(
        codec.ctx, guards.address(r.keys), L.ptr(r.status), r.n if n is None else n,
        guards.address(r.order) if order == "own" else 0, guards.address(r.sorted), guards.address(r.valid),
        guards.address(r.work), r.work_bytes if work_bytes is None else work_bytes, codec.stream)


def call_objects(codec, r, work_bytes=None, n=None):
    return codec.lib.honu_key_objects(
        codec.ctx, guards.address(r.keys), guards.address(r.order), guards.address(r.valid),
        r.n if n is None else n, guards.address(r.obj_off), guards.address(r.latest), guards.address(r.objects),
        guards.address(r.work), r.work_bytes if work_bytes is None else work_bytes, codec.stream)


def view(t, dtype):
    return guards.block_of(t).bytes().view(dtype)


def check_run(r, k, st, columns=None):
    """Outputs equal to numpy's, nothing written outside what the calls own."""
    n = r.n
    order, valid = expected_order(k, st)
    got_valid = int(view(r.valid, np.uint64)[0])
    assert got_valid == valid
    got_order = view(r.order, np.uint32)
    assert np.array_equal(np.sort(got_order), np.arange(n, dtype=np.uint32))  # a permutation
    bad = np.flatnonzero(got_order != order)
    assert not len(bad), (len(bad), bad[:5], got_order[bad[:5]], order[bad[:5]])
    if r.sorted is not None:
        assert np.array_equal(view(r.sorted, np.uint8).reshape(n, 29), k[order])
    assert np.array_equal(view(r.keys, np.uint8).reshape(n, 29), k)  # the input is only read
    off, latest = expected_objects(k, order, valid)
    objects = len(off) - 1
    assert int(view(r.objects, np.uint64)[0]) == objects
    assert np.array_equal(view(r.obj_off, np.uint64)[:objects + 1], off)
    if r.latest is not None:
        got_latest = view(r.latest, np.uint32)[:objects]
        assert np.array_equal(got_latest, latest)
        if columns is not None:  # the second route: no key byte compared
            label, vid, pid = columns
            want = latest_by_columns(label, vid, pid, st)
            assert len(want) == objects
            assert {label[i]: int(i) for i in got_latest} == want
    guards.assert_untouched(r.order, [(0, 4 * n)])
    if r.sorted is not None:
        guards.assert_untouched(r.sorted, [(0, 29 * n)])
    guards.assert_untouched(r.valid, [(0, 8)])
    guards.assert_untouched(r.keys, [(0, 29 * n)])  # (its bytes: compared above)
    guards.assert_untouched(r.obj_off, [(0, 8 * (objects + 1))])
    if r.latest is not None:
        guards.assert_untouched(r.latest, [(0, 4 * objects)])
    guards.assert_untouched(r.objects, [(0, 8)])
    guards.assert_untouched(r.work, [(0, r.work_bytes)])


def sort_and_check(codec, k, st, phase, columns=None, **kw):
    def body(fill):
        r = guarded_run(codec, k, st, phase, fill, **kw)
        L.check(call_sort(codec, r), "honu_sort_keys")
        L.check(call_objects(codec, r), "honu_key_objects")  # same stream, d_valid stays on the device
        torch.cuda.synchronize()
        check_run(r, k, st, columns)

    guards.twice(body)


# --------------------------------------------------------------------------
# key sets
# --------------------------------------------------------------------------
def set_random(n, rng):
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def set_equal(n, rng):
    return np.tile(rng.integers(0, 256, (1, 29), dtype=np.uint8), (n, 1))


def set_one_byte(byte):
    def make(n, rng):
        k = set_equal(n, rng)
        k[:, byte] = rng.integers(0, 256, n, dtype=np.uint8)
        return k
    return make


def set_sorted(n, rng):
    k = set_random(n, rng)
    return k[np.lexsort(k.T[::-1])]


def set_reversed(n, rng):
    return set_sorted(n, rng)[::-1].copy()


def columns_versions(n, rng):
    """40 objects x many versions: VID a small value shifted by 0-59 bits, PID
    0..3; heavy duplicates, every digit position of the version in use, and
    object IDs that differ in every byte."""
    oids = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    which = rng.integers(0, 40, n)
    vid = rng.integers(1, 16, n).astype(np.uint64) << rng.integers(0, 60, n).astype(np.uint64)
    pid = rng.integers(0, 4, n).astype(np.uint32)
    return oids[which], which, vid, pid


def set_two_values(n, rng):
    lo, hi = rng.integers(0, 128, 29, dtype=np.uint8), rng.integers(128, 256, 29, dtype=np.uint8)
    return np.where(rng.integers(0, 2, (n, 29)).astype(bool), hi, lo).astype(np.uint8)


PLAIN_SETS = {
    "random": set_random, "equal": set_equal, "byte28": set_one_byte(28), "byte0": set_one_byte(0),
    "byte17": set_one_byte(17), "sorted": set_sorted, "reversed": set_reversed, "two_values": set_two_values,
}
EDGES = ("T-1", "T", "T+1", "2T+1", "3T+17")


def edge_size(T, name):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "3T+17": 3 * T + 17}[name]


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 3])
@pytest.mark.parametrize("size", [0, 1, 2, 63, 64, 65, 255, 256, 257, "T-1", "T", "T+1", "2T+1", "3T+17", 100003])
def test_sizes_random_keys(codecs, T, size, phase):
    """Random 29-byte keys, as randKey() (keys_test.go:283-287): byte 0 too."""
    n = edge_size(T, size) if isinstance(size, str) else size
    rng = np.random.default_rng(1000 + n)
    sort_and_check(codecs(n), set_random(n, rng), np.zeros(n, np.int32), phase)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("name", list(PLAIN_SETS))
def test_key_sets(codecs, T, name, edge):
    n = edge_size(T, edge)
    rng = np.random.default_rng(sum(map(ord, name)) + n)
    k = PLAIN_SETS[name](n, rng)
    phase = (1, 3, 0)[list(PLAIN_SETS).index(name) % 3]
    sort_and_check(codecs(n), k, np.zeros(n, np.int32), phase)
    if name == "equal":  # the order is the identity (checked against numpy's above: the same)
        assert np.array_equal(expected_order(k, np.zeros(n, np.int32))[0], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("invalid", [False, True], ids=["versions", "versions_quarter_invalid"])
def test_object_versions(codecs, T, edge, invalid):
    """Sets (e) and (g): objects with many versions; in (g) every fourth
    status is not OK, the first and the last key among them."""
    n = edge_size(T, edge)
    rng = np.random.default_rng(77 + n)
    oid, which, vid, pid = columns_versions(n, rng)
    k = keys_from_columns(oid, vid, pid)
    st = np.zeros(n, np.int32)
    if invalid:
        st[::4] = ERR_PANIC
        st[n - 1] = 2
        k[st != 0] = rng.integers(0, 256, (int((st != 0).sum()), 29), dtype=np.uint8)  # whatever bytes
    sort_and_check(codecs(n), k, st, 3 if invalid else 1, columns=(which, vid, pid))


def test_optional_outputs_and_null_status(codecs, T):
    """d_sorted, d_latest and d_key_status are optional."""
    n = T + 1
    rng = np.random.default_rng(9)
    oid, which, vid, pid = columns_versions(n, rng)
    k = keys_from_columns(oid, vid, pid)
    sort_and_check(codecs(n), k, np.zeros(n, np.int32), 1, with_status=False, want_sorted=False,
                   want_latest=False)


def test_all_invalid(codecs):
    n = 300
    k = set_random(n, np.random.default_rng(3))
    sort_and_check(codecs(n), k, np.full(n, ERR_PANIC, np.int32), 1)


def test_refusals_store_nothing(codecs, T):
    n = T + 1
    codec = codecs(n)
    k = set_random(n, np.random.default_rng(4))
    st = np.zeros(n, np.int32)

    def body(fill):
        r = guarded_run(codec, k, st, 1, fill)
        assert call_sort(codec, r, work_bytes=r.work_bytes - 1) == E_ARG
        assert call_objects(codec, r, work_bytes=r.work_bytes - 1) == E_ARG
        assert call_sort(codec, r, n=BIG + 1) == E_WORKSPACE
        assert call_objects(codec, r, n=BIG + 1) == E_WORKSPACE
        assert call_sort(codec, r, order=None) == E_ARG
        torch.cuda.synchronize()
        for t in (r.order, r.sorted, r.valid, r.obj_off, r.latest, r.objects, r.work):
            guards.assert_untouched(t, [])

    guards.twice(body)


def test_codec_methods(codecs):
    """Codec.sort_keys / Codec.key_objects size their own workspace."""
    n = 1000
    codec = codecs(n)
    rng = np.random.default_rng(21)
    oid, which, vid, pid = columns_versions(n, rng)
    k = keys_from_columns(oid, vid, pid)
    st = np.zeros(n, np.int32)
    st[[0, 500, n - 1]] = ERR_PANIC
    dk, dst = hobj._dev_bytes(k, codec.torch_device), hobj._dev_bytes(st, codec.torch_device)
    order, srt, valid = codec.sort_keys(dk, dst, n=n, want_sorted=True)
    obj_off, latest, objects = codec.key_objects(dk, order, valid)
    torch.cuda.synchronize()
    eorder, evalid = expected_order(k, st)
    eoff, elatest = expected_objects(k, eorder, evalid)
    assert int(valid.item()) == evalid and int(objects.item()) == len(elatest)
    assert np.array_equal(order.cpu().numpy().view(np.uint32), eorder)
    assert np.array_equal(srt[:29 * n].cpu().numpy().reshape(n, 29), k[eorder])
    assert np.array_equal(obj_off.cpu().numpy().view(np.uint64)[:len(eoff)], eoff)
    assert np.array_equal(latest.cpu().numpy().view(np.uint32)[:len(elatest)], elatest)
    assert codec.sort_keys(dk, n=n)[1] is None  # no status: every key takes part; no sorted column


def test_pipeline_and_graph_replay():
    """marshal -> honu_decode_batch -> honu_decode_keys -> sort -> objects on a
    mixed batch of 300 records over 37 objects, a few without a Version (key
    status HONU_ERR_PANIC); then the same sequence captured into a graph and
    replayed after zeroing the outputs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 300
    rng = np.random.default_rng(11)
    hb = gen_host_batch(41, "mixed", 0, n)
    oids = rng.integers(0, 256, (37, 16), dtype=np.uint8)
    which = np.concatenate([np.arange(37), rng.integers(0, 37, n - 37)])
    rng.shuffle(which)
    hb.meta["object_id"] = oids[which]
    nover = np.array([0, 5, 123, 299])
    hb.meta["present"][nover] &= ~np.uint32(HAS_VERSION)
    st = np.zeros(n, np.int32)
    st[nover] = ERR_PANIC
    c = hobj.Codec(0, n)
    try:
        db = hobj.DeviceBatch.from_host(hb, c.torch_device)
        enc = c.marshal(db)
        total = int(enc.out_off.view(torch.int64)[n].item())
        out_off, status, out = c._empty(8 * (n + 1)), c._empty(4 * n), c._empty(total)
        meta, info, totals = c._empty(352 * n), c._empty(32 * n), c._empty(32)
        acl, reg = c._empty(20 * total), c._empty(4 * total)
        keys, kst = c._empty(29 * n), c._empty(4 * n)
        order, srt, valid = c._empty(4 * n), c._empty(29 * n), c._empty(8)
        obj_off, latest, objects = c._empty(8 * (n + 1)), c._empty(4 * n), c._empty(8)
        work, wb = c.sort_workspace(n)
        outs = (out, meta, info, keys, kst, order, srt, valid, obj_off, latest, objects)

        def seq():
            c.marshal_into(db, out, total, out_off, status)
            L.check(c.lib.honu_decode_batch(c.ctx, L.ptr(out), L.ptr(out_off), n, L.ptr(meta), L.ptr(info),
                                            L.ptr(acl), total, L.ptr(reg), total, 0, 0, L.ptr(totals),
                                            c.stream), "decode")
            L.check(c.lib.honu_decode_keys(c.ctx, L.ptr(meta), L.ptr(info), n, L.ptr(keys), L.ptr(kst),
                                           c.stream), "keys")
            L.check(c.lib.honu_sort_keys(c.ctx, L.ptr(keys), L.ptr(kst), n, L.ptr(order), L.ptr(srt),
                                         L.ptr(valid), L.ptr(work), wb, c.stream), "sort")
            L.check(c.lib.honu_key_objects(c.ctx, L.ptr(keys), L.ptr(order), L.ptr(valid), n, L.ptr(obj_off),
                                           L.ptr(latest), L.ptr(objects), L.ptr(work), wb, c.stream), "objects")

        def results():
            torch.cuda.synchronize()
            nobj = int(hobj._to_host(objects, 8, np.uint64)[0])
            return (hobj._to_host(keys, 29 * n, np.uint8).reshape(n, 29).copy(),
                    hobj._to_host(kst, 4 * n, np.int32).copy(), hobj._to_host(order, 4 * n, np.uint32).copy(),
                    hobj._to_host(srt, 29 * n, np.uint8).reshape(n, 29).copy(),
                    int(hobj._to_host(valid, 8, np.uint64)[0]), nobj,
                    hobj._to_host(obj_off, 8 * (nobj + 1), np.uint64).copy(),
                    hobj._to_host(latest, 4 * nobj, np.uint32).copy())

        for t in outs:
            t.zero_()
        seq()
        k, gst, gorder, gsrt, gvalid, gobjects, goff, glatest = eager = results()
        assert np.array_equal(gst, st)
        want_keys = keys_from_columns(oids[which], hb.meta["vid"], hb.meta["pid"])
        want_keys[nover] = 0  # honu_decode_keys zeroes the key of a record it refuses
        assert np.array_equal(k, want_keys)
        eorder, evalid = expected_order(k, st)
        assert gvalid == evalid == n - len(nover)
        assert np.array_equal(gorder, eorder) and np.array_equal(gsrt, k[eorder])
        eoff, elatest = expected_objects(k, eorder, evalid)
        assert gobjects == len(eoff) - 1 == 37
        assert np.array_equal(goff, eoff) and np.array_equal(glatest, elatest)
        want = latest_by_columns(which, hb.meta["vid"], hb.meta["pid"], st)
        assert {int(which[i]): int(i) for i in glatest} == want

        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            seq()
        for t in outs:
            t.zero_()
        g.replay()
        for a, b in zip(eager, results()):
            assert np.array_equal(a, b)
    finally:
        c.close()
