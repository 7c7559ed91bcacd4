"""honu_key_seek on the GPU against keys.seek on the host.

Expected pos / end come from honu_amd.keys.seek over the valid rows as a list
of bytes (bisect in Python's bytes order, which is bytes.Compare); expected
first / latest / LIVE bits from numpy columns. Every shape runs under
"seek_variant" 1 (direct), 2 (fenced) and 0 (auto), each under both fills of a
guarded output (tests/guards.py) whose write set is exactly the m result rows.
The sorted column and the probe column are passed at byte phases 0, 1 and 3.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (HAS_VERSION, INFO_DTYPE, SEEK_END, SEEK_EXACT, SEEK_FIRST_LIVE,  # noqa: E402
                               SEEK_FOUND, SEEK_LATEST_LIVE, SEEK_NONE, SEEK_SKIPPED)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE, ERR_PANIC = -1, -2, 8
VARIANTS = (1, 2, 0)
PHASES = ((0, 0), (1, 3), (3, 1))  # (sorted column, probe column)
PROBE_LENS = (0, 1, 15, 16, 17, 28, 29)
PROBE_COUNTS = (0, 1, 63, 64, 65, 257, 5000)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 1024)
    yield c
    c.close()


def get_param(codec, name):
    v = L.C.c_int64(0)
    L.check(codec.lib.honu_ctx_get_param(codec.ctx, name.encode(), L.C.byref(v)), name)
    return int(v.value)


def set_variant(codec, variant):
    L.check(codec.lib.honu_ctx_set_param(codec.ctx, b"seek_variant", variant), "seek_variant")
    assert get_param(codec, "seek_variant") == variant


@pytest.fixture(scope="module")
def F(codec):
    return get_param(codec, "seek_fence")


# --------------------------------------------------------------------------
# expected rows
# --------------------------------------------------------------------------
def expected_rows(S, valid, P, plen, st=None, order=None, tomb=None):
    """The honu_seek rows as uint32 (m, 5). S: the whole column (n, 29), its
    rows [0, valid) sorted; tomb: the records' tombstone column."""
    srt = [bytes(r) for r in S[:valid]]
    out = np.zeros((len(P), 5), np.uint32)
    for q in range(len(P)):
        if st is not None and st[q] != 0:
            out[q] = (0, 0, SEEK_NONE, SEEK_NONE, SEEK_SKIPPED)
            continue
        pos, end = hkeys.seek(srt, bytes(P[q, :plen]))
        flags, first, latest = (SEEK_END if pos == valid else 0), SEEK_NONE, SEEK_NONE
        if pos < end:
            flags |= SEEK_FOUND | (SEEK_EXACT if plen == 29 else 0)
            if order is not None:
                first, latest = int(order[pos]), int(order[end - 1])
                if tomb is not None:
                    flags |= 0 if tomb[first] else SEEK_FIRST_LIVE
                    flags |= 0 if tomb[latest] else SEEK_LATEST_LIVE
        out[q] = (pos, end, first, latest, flags)
    return out


# --------------------------------------------------------------------------
# one guarded call
# --------------------------------------------------------------------------
def put(codec, a, phase, fill):
    """The bytes of `a` in a guarded block at a byte phase (an input)."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = guards.guarded(a.nbytes, phase=phase, fill=fill, device=codec.torch_device)
    if a.nbytes:
        t.copy_(torch.from_numpy(a.copy()).to(codec.torch_device))
    return t


def info_rows(tomb):
    info = np.zeros(len(tomb), INFO_DTYPE)
    info["tombstone"] = tomb
    return info


def seek_call(codec, S, valid, P, plen, fill, st=None, order=None, tomb=None, phases=(0, 0)):
    """One honu_key_seek into a guarded output; returns the output view."""
    n, m = len(S), len(P)
    d_s, d_p = put(codec, S, phases[0], fill), put(codec, P, phases[1], fill)
    d_valid = put(codec, np.array([valid], np.uint64), 0, fill)
    d_st = None if st is None else put(codec, st.astype(np.int32), 0, fill)
    d_order = None if order is None else put(codec, order.astype(np.uint32), 0, fill)
    d_info = None if tomb is None else put(codec, info_rows(tomb), 0, fill)
    out = guards.guarded(20 * m, fill=fill, device=codec.torch_device)
    L.check(codec.lib.honu_key_seek(codec.ctx, guards.address(d_s), guards.address(d_valid), n, guards.address(d_p),
                                    guards.address(d_st), plen, m, guards.address(d_order), guards.address(d_info),
                                    guards.address(out), codec.stream), "honu_key_seek")
    torch.cuda.synchronize()
    for t, a in ((d_s, S), (d_p, P)):  # the inputs are only read
        assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(a).tobytes()
    return out


def seek_and_check(codec, S, valid, P, plen, st=None, order=None, tomb=None, phases=(0, 0), variants=VARIANTS):
    m = len(P)
    eff = min(valid, len(S))
    want = expected_rows(S, eff, P, plen, st, order, tomb)
    for variant in variants:
        set_variant(codec, variant)

        def body(fill):
            out = seek_call(codec, S, valid, P, plen, fill, st, order, tomb, phases)
            got = guards.block_of(out).bytes().view(np.uint32).reshape(m, 5)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (variant, plen, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])
            guards.assert_untouched(out, [(0, 20 * m)])

        guards.twice(body)
    set_variant(codec, 0)
    return want


# --------------------------------------------------------------------------
# key sets (rows in sorted order) and probes
# --------------------------------------------------------------------------
def sort_rows(k):
    return k[np.lexsort(k.T[::-1])] if len(k) else k


def set_random(n, rng):
    return sort_rows(rng.integers(0, 256, (n, 29), dtype=np.uint8))


def set_equal(n, rng):
    return np.tile(rng.integers(0, 256, (1, 29), dtype=np.uint8), (n, 1))


def set_one_byte(byte):
    """Keys that differ only in byte `byte`, which takes values on both sides of 0x7f/0x80."""
    def make(n, rng):
        k = set_equal(n, rng)
        k[:, byte] = rng.choice(np.array([0, 1, 0x7E, 0x7F, 0x80, 0x81, 0xFE, 0xFF], np.uint8), n)
        return sort_rows(k)
    return make


def keys_from_columns(oid, vid, pid):
    """0x01 | oid | BE64(VID) | BE32(PID) (keys.go:42-51)."""
    n = len(vid)
    k = np.zeros((n, 29), np.uint8)
    k[:, 0] = 1
    k[:, 1:17] = oid
    k[:, 17:25] = vid.astype(">u8").view(np.uint8).reshape(n, 8)
    k[:, 25:29] = pid.astype(">u4").view(np.uint8).reshape(n, 4)
    return k


def set_versions(n, rng):
    """40 objects x many versions, heavy duplicates; some ids end in 0xff."""
    oids = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    oids[::5, 15] = 0xFF
    oids[7, 14:] = 0xFF
    which = rng.integers(0, 40, n)
    vid = rng.integers(1, 16, n).astype(np.uint64) << rng.integers(0, 60, n).astype(np.uint64)
    return sort_rows(keys_from_columns(oids[which], vid, rng.integers(0, 4, n).astype(np.uint32)))


def set_two_values(n, rng):
    """Every byte one of two values that straddle 0x7f/0x80: a signed compare gets these wrong."""
    lo, hi = rng.integers(0x70, 0x80, 29, dtype=np.uint8), rng.integers(0x80, 0x90, 29, dtype=np.uint8)
    return sort_rows(np.where(rng.integers(0, 2, (n, 29)).astype(bool), hi, lo).astype(np.uint8))


def probes_of(S, plen, rng, m=None):
    """Every stored key, each with its last significant byte +1 and -1, all
    0x00 and all 0xff; the bytes past plen are noise the call must not read
    into the comparison. m: that many of them (the two constant rows first)."""
    rows = [np.zeros((1, 29), np.uint8), np.full((1, 29), 0xFF, np.uint8)]
    if len(S):
        rows.append(S.copy())
        if plen:
            for d in (1, 255):
                k = S.copy()
                k[:, plen - 1] += np.uint8(d)
                rows.append(k)
    P = np.concatenate(rows)
    if m is not None:
        take = np.arange(m) % len(P) if m <= 2 or len(P) <= 2 else np.concatenate(
            [[0, 1], 2 + rng.integers(0, len(P) - 2, m - 2)])
        P = P[take]
    P = P.copy()
    P[:, plen:] = rng.integers(0, 256, (len(P), 29 - plen), dtype=np.uint8)
    return P


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, "F-1", "F", "F+1", "2F+1", 100003)


def size_of(F, s):
    return {"F-1": F - 1, "F": F, "F+1": F + 1, "2F+1": 2 * F + 1}[s] if isinstance(s, str) else s


@pytest.mark.parametrize("size", SIZES)
def test_sizes(codec, F, size):
    """Random keys; n crossed sparsely with m, probe_len and the byte phases."""
    n = size_of(F, size)
    i = SIZES.index(size)
    rng = np.random.default_rng(3000 + n)
    S = set_random(n, rng)
    for j in range(3):
        m, plen = PROBE_COUNTS[(i + 3 * j) % 7], PROBE_LENS[(2 * i + 5 * j + 6) % 7]
        seek_and_check(codec, S, n, probes_of(S, plen, rng, m), plen, phases=PHASES[(i + j) % 3])


def test_many_probes(codec, F):
    """More probes than auto's threshold, over more rows than the fence holds."""
    rng = np.random.default_rng(31)
    S = set_random(100003, rng)
    seek_and_check(codec, S, len(S), probes_of(S, 29, rng, 20000), 29, phases=(1, 1))
    seek_and_check(codec, S, len(S), probes_of(S, 2, rng, 20000), 2, phases=(3, 0))


PLAIN_SETS = {"random": set_random, "equal": set_equal, "versions": set_versions, "two_values": set_two_values}


@pytest.mark.parametrize("name", list(PLAIN_SETS))
def test_key_sets(codec, F, name):
    """Every stored key, its neighbours and the two constant probes, at every probe length."""
    n = 2 * F + 1
    rng = np.random.default_rng(sum(map(ord, name)))
    S = PLAIN_SETS[name](n, rng)
    for i, plen in enumerate(PROBE_LENS):
        want = seek_and_check(codec, S, n, probes_of(S, plen, rng), plen, phases=PHASES[i % 3])
        stored = want[2:2 + n]
        assert (stored[:, 4] & SEEK_FOUND).all() and (stored[:, 0] < stored[:, 1]).all()
    if name == "versions":  # ids that end in 0xff keep their range (keys.go:88-91 wraps there)
        ff = S[S[:, 16] == 0xFF]
        assert len(ff)
        want = seek_and_check(codec, S, n, ff, 17)
        assert (want[:, 1] > want[:, 0]).all()


@pytest.mark.parametrize("byte", range(29))
def test_one_byte_sets(codec, F, byte):
    """Keys that differ only in byte j: every word boundary of the big-endian
    compare and the overlap of the two loads at byte 13."""
    n = 2 * F + 1
    rng = np.random.default_rng(500 + byte)
    S = set_one_byte(byte)(n, rng)
    for plen in sorted({byte, byte + 1, 29}):
        P = probes_of(S[::7], plen, rng)
        seek_and_check(codec, S, n, P, plen, phases=PHASES[byte % 3])


@pytest.mark.parametrize("size", [65, "2F+1"])
def test_invalid_rows_are_never_returned(codec, F, size):
    """A quarter of the rows are past valid and hold copies of the probes."""
    n = size_of(F, size)
    valid = n - n // 4
    rng = np.random.default_rng(40 + n)
    S = set_versions(n, rng)
    for plen in (17, 29):
        P = probes_of(S[:valid], plen, rng)
        S2 = S.copy()
        S2[valid:] = P[rng.integers(0, len(P), n - valid)]
        want = seek_and_check(codec, S2, valid, P, plen, phases=(1, 3))
        assert (want[:, :2] <= valid).all()
    # none valid: END for every probe, whatever the rows hold; and a count above n means n
    P = probes_of(S, 29, rng, 300)
    want = seek_and_check(codec, S, 0, P, 29)
    assert (want == np.array([0, 0, SEEK_NONE, SEEK_NONE, SEEK_END], np.uint32)).all()
    seek_and_check(codec, S, n + 5, P, 29)


def versions_table(rng, objects=30, versions=5):
    """objects x versions records in random record order, (VID, PID) distinct
    within an object: (keys by record, object label, rank of the version
    within its object, 0 the lowest)."""
    oids = rng.integers(0, 256, (objects, 16), dtype=np.uint8)
    label = np.repeat(np.arange(objects), versions)
    rank = np.tile(np.arange(versions), objects)
    vid = (rank // 2 + 1).astype(np.uint64) << np.uint64(24)
    pid = (rank % 2 + 1).astype(np.uint32)
    perm = rng.permutation(len(label))
    label, rank, vid, pid = label[perm], rank[perm], vid[perm], pid[perm]
    return keys_from_columns(oids[label], vid, pid), label, rank


def test_optional_inputs(codec):
    """d_probe_status, d_order and d_info, each absent and present; tombstones
    on the lowest version only, the latest only and both."""
    rng = np.random.default_rng(8)
    objects, versions = 30, 5
    K, label, rank = versions_table(rng, objects, versions)
    n = len(K)
    order = np.lexsort(K.T[::-1]).astype(np.uint32)
    S = K[order]
    tomb = np.zeros(n, np.uint8)
    tomb[(label % 4 == 1) & (rank == 0)] = 1                           # lowest only
    tomb[(label % 4 == 2) & (rank == versions - 1)] = 1                # latest only
    tomb[(label % 4 == 3) & ((rank == 0) | (rank == versions - 1))] = 1  # both
    P = K.copy()
    st = np.zeros(n, np.int32)
    st[[0, 77, n - 1]] = (ERR_PANIC, 2, ERR_PANIC)
    seek_and_check(codec, S, n, P, 17)
    seek_and_check(codec, S, n, P, 17, st=st)
    seek_and_check(codec, S, n, P, 17, st=st, order=order)
    want = seek_and_check(codec, S, n, P, 17, st=st, order=order, tomb=tomb)
    # the same from the columns, no key byte involved
    rec_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(label, rank))}
    for q in np.flatnonzero(st == 0):
        lo, hi = rec_of[(int(label[q]), 0)], rec_of[(int(label[q]), versions - 1)]
        live = (0 if tomb[lo] else SEEK_FIRST_LIVE) | (0 if tomb[hi] else SEEK_LATEST_LIVE)
        assert tuple(want[q, 2:]) == (lo, hi, SEEK_FOUND | live), q
        assert want[q, 1] - want[q, 0] == versions
    live = want[st == 0][:, 4] & (SEEK_FIRST_LIVE | SEEK_LATEST_LIVE)
    assert {0, SEEK_FIRST_LIVE, SEEK_LATEST_LIVE, SEEK_FIRST_LIVE | SEEK_LATEST_LIVE} == set(live.tolist())
    # probe_len 29: one version each, so first == latest == the record itself
    want = seek_and_check(codec, S, n, P, 29, order=order, tomb=tomb)
    assert np.array_equal(want[:, 2], np.arange(n)) and np.array_equal(want[:, 3], np.arange(n))
    assert ((want[:, 4] & SEEK_EXACT) != 0).all()


def test_order_index_out_of_range_reads_the_last_info_row(codec):
    rng = np.random.default_rng(12)
    S = set_random(4, rng)
    order = np.array([0, 1, 2, 77], np.uint32)
    for last in (0, 1):
        tomb = np.array([0, 0, 0, last], np.uint8)
        for variant in VARIANTS:
            set_variant(codec, variant)
            out = seek_call(codec, S, 4, S, 29, 0x00, order=order, tomb=tomb)
            got = guards.block_of(out).bytes().view(np.uint32).reshape(4, 5)
            live = 0 if last else SEEK_FIRST_LIVE | SEEK_LATEST_LIVE
            assert tuple(got[3]) == (3, 4, 77, 77, SEEK_FOUND | SEEK_EXACT | live)
            assert tuple(got[1]) == (1, 2, 1, 1, SEEK_FOUND | SEEK_EXACT | SEEK_FIRST_LIVE | SEEK_LATEST_LIVE)
    set_variant(codec, 0)


def test_refusals_store_nothing(codec):
    rng = np.random.default_rng(4)
    n, m = 300, 70
    S = set_random(n, rng)
    P = probes_of(S, 29, rng, m)

    def body(fill):
        dev = codec.torch_device
        d_s, d_p = put(codec, S, 1, fill), put(codec, P, 3, fill)
        d_valid = put(codec, np.array([n, n], np.uint64), 0, fill)
        d_st = put(codec, np.zeros(m + 1, np.int32), 0, fill)
        d_order = put(codec, np.arange(n + 1, dtype=np.uint32), 0, fill)
        d_info = put(codec, info_rows(np.zeros(n + 1, np.uint8)), 0, fill)
        out = guards.guarded(20 * m + 4, fill=fill, device=dev)
        A = guards.address
        base = dict(ctx=codec.ctx, s=A(d_s), valid=A(d_valid), n=n, p=A(d_p), st=A(d_st), plen=29, m=m,
                    order=A(d_order), info=A(d_info), out=A(out))

        def call(**kw):
            a = dict(base, **kw)
            return codec.lib.honu_key_seek(a["ctx"], a["s"], a["valid"], a["n"], a["p"], a["st"], a["plen"],
                                           a["m"], a["order"], a["info"], a["out"], codec.stream)

        assert call(n=1 << 32) == E_WORKSPACE
        assert call(m=1 << 32) == E_WORKSPACE
        for kw in (dict(ctx=None), dict(valid=0), dict(out=0), dict(s=0), dict(p=0), dict(plen=30),
                   dict(order=0), dict(out=A(out) + 2), dict(order=A(d_order) + 2), dict(st=A(d_st) + 2),
                   dict(valid=A(d_valid) + 4), dict(info=A(d_info) + 4)):
            assert call(**kw) == E_ARG, kw
        assert call(m=0) == 0  # nothing launched or stored
        assert call(m=0, p=0, out=0) == 0
        torch.cuda.synchronize()
        guards.assert_untouched(out, [])
        assert call() == 0  # and the arguments were good
        torch.cuda.synchronize()
        guards.assert_untouched(out, [(0, 20 * m)])

    guards.twice(body)


def test_codec_seek_keys(codec):
    """Codec.seek_keys equals the raw call."""
    rng = np.random.default_rng(21)
    K, label, rank = versions_table(rng, 50, 4)
    n = len(K)
    st = np.zeros(n, np.int32)
    st[[3, n - 1]] = ERR_PANIC
    tomb = (rng.integers(0, 3, n) == 0).astype(np.uint8)
    dev = codec.torch_device
    dk, dst, dinfo = hobj._dev_bytes(K, dev), hobj._dev_bytes(st, dev), hobj._dev_bytes(info_rows(tomb), dev)
    order, srt, valid = codec.sort_keys(dk, dst, n=n, want_sorted=True)
    torch.cuda.synchronize()
    h_order = order.cpu().numpy().view(np.uint32)
    h_valid = int(valid.item())
    S = srt[:29 * n].cpu().numpy().reshape(n, 29)
    assert h_valid == n - 2
    for plen in (17, 29):
        rows = codec.seek_keys(srt[:29 * n], valid, dk[:29 * n], plen, probe_status=dst, order=order, info=dinfo)
        assert rows.shape == (n, 5) and rows.dtype == torch.int32
        got = rows.cpu().numpy().view(np.uint32)
        want = seek_and_check(codec, S, h_valid, K, plen, st=st, order=h_order, tomb=tomb)
        assert np.array_equal(got, want)
    bare = codec.seek_keys(srt[:29 * n], valid, dk[:29 * n])  # probe_len 29, nothing optional
    want = expected_rows(S, h_valid, K, 29)
    assert np.array_equal(bare.cpu().numpy().view(np.uint32), want)
    assert codec.seek_keys(srt[:29 * n], valid, dk[:29 * n], m=0).shape == (0, 5)


def test_pipeline_and_graph_replay():
    """marshal -> honu_decode_batch -> honu_decode_keys -> honu_sort_keys ->
    honu_key_objects -> honu_key_seek on 300 mixed records over 37 objects, a
    few without a Version, with the batch's own key column and key status as
    probes; then the sequence captured into a graph and replayed."""
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
        seek29, seek17 = c._empty(20 * n), c._empty(20 * n)
        work, wb = c.sort_workspace(n)
        outs = (out, meta, info, keys, kst, order, srt, valid, obj_off, latest, objects, seek29, seek17)

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
            for plen, rows in ((29, seek29), (17, seek17)):
                L.check(c.lib.honu_key_seek(c.ctx, L.ptr(srt), L.ptr(valid), n, L.ptr(keys), L.ptr(kst), plen, n,
                                            L.ptr(order), L.ptr(info), L.ptr(rows), c.stream), "seek")

        def results():
            torch.cuda.synchronize()
            nobj = int(hobj._to_host(objects, 8, np.uint64)[0])
            return (hobj._to_host(order, 4 * n, np.uint32).copy(), int(hobj._to_host(valid, 8, np.uint64)[0]),
                    hobj._to_host(obj_off, 8 * (nobj + 1), np.uint64).copy(),
                    hobj._to_host(latest, 4 * nobj, np.uint32).copy(),
                    hobj._to_host(info, 32 * n, INFO_DTYPE).copy(),
                    hobj._to_host(seek29, 20 * n, np.uint32).reshape(n, 5).copy(),
                    hobj._to_host(seek17, 20 * n, np.uint32).reshape(n, 5).copy())

        for variant in VARIANTS:
            L.check(c.lib.honu_ctx_set_param(c.ctx, b"seek_variant", variant), "seek_variant")
            for t in outs:
                t.zero_()
            seq()
            gorder, gvalid, goff, glatest, ginfo, r29, r17 = eager = results()
            assert gvalid == n - len(nover) and len(glatest) == 37
            tomb = ginfo["tombstone"]
            for i in range(n):
                if i in nover:
                    for r in (r29, r17):
                        assert tuple(r[i]) == (0, 0, SEEK_NONE, SEEK_NONE, SEEK_SKIPPED)
                    continue
                pos, end, first, last, flags = (int(x) for x in r29[i])
                assert flags & (SEEK_FOUND | SEEK_EXACT | SEEK_END | SEEK_SKIPPED) == SEEK_FOUND | SEEK_EXACT
                assert i in gorder[pos:end] and first == gorder[pos] and last == gorder[end - 1]
                pos, end, first, last, flags = (int(x) for x in r17[i])
                assert flags & (SEEK_FOUND | SEEK_EXACT | SEEK_END | SEEK_SKIPPED) == SEEK_FOUND
                j = int(np.searchsorted(goff, pos))
                assert goff[j] == pos and goff[j + 1] == end  # the object's range: end - pos its version count
                assert last == glatest[j] and first == gorder[pos]
                assert bool(flags & SEEK_FIRST_LIVE) == (not tomb[first])
                assert bool(flags & SEEK_LATEST_LIVE) == (not tomb[last])

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
