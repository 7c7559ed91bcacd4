"""The read feed (honu_feed_*) and the write feed (honu_put_feed_*) through the
C ABI on the GPU: the multi-threaded host fills (batches from
kParallelCopyMin bytes on), honu_feed_reserve, the two-slot protocol, exact
capacities, the write feed's budget and output bound, put_plan's refusals,
slot reuse and destroy with a batch in flight. Everything is bit-exact
against the oracle; tests/test_feed_host.py runs the same host code under the
sanitizers and checks PARALLEL_COPY_MIN against the header."""
import ctypes as C

import numpy as np
import pytest

from corpora import random_metas
from fixtures import extreme_metas
from honu_amd import _lib
from honu_amd.metadata import (ACL_INPLACE, ACL_SIZED, HAS_ENCRYPTION, HAS_META, HAS_PUBLISHER,
                               HAS_SCHEMA, AccessControl, Compression, Encryption, HostBatch,
                               Metadata, Publisher, Scalar, SchemaVersion, Version, normalize,
                               pack_batch, unpack_row)
from honu_amd.workload import gen_host_batch

pytestmark = pytest.mark.gpu

# honu::kParallelCopyMin (csrc/host_copy.h): from this many bytes on a batch's
# host copies run on several threads. tests/test_feed_host.py compares it
# with the header's value.
PARALLEL_COPY_MIN = 8 << 20
E_ARG, E_CAPACITY, E_INPUT = -1, 9, 10


@pytest.fixture(autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def _with_payloads(hb, lens, seed):
    """The batch's rows with payloads of the given lengths (random bytes)."""
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    pay = np.random.default_rng(seed).integers(0, 256, int(off[-1]) + 1, dtype=np.uint8)
    return HostBatch(hb.meta[: len(lens)], hb.var, hb.acl, hb.regions, pay, off)


def _objects(oracle_lib, n, seed, lens=None):
    """n valid records (oracle-marshalled generator rows), as bytes."""
    hb = gen_host_batch(seed, "small", 0, n)
    if lens is not None:
        hb = _with_payloads(hb, lens, seed)
    rec, off, st = oracle_lib.marshal_batch(hb)
    assert (st == 0).all()
    return [rec[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]


def _csr(objs, lead=0):
    """(arena, off) of the records, the first starting at byte `lead`."""
    off = np.zeros(len(objs) + 1, np.uint64)
    off[1:] = np.cumsum([len(o) for o in objs])
    off += np.uint64(lead)
    return np.frombuffer(b"\xA7" * lead + b"".join(objs) + b"\0", np.uint8), off


def _raw(v):
    return None if v is None else np.ascontiguousarray(v).view(np.uint8).tobytes()


def _snapshot(res):
    """Every view of a result, as bytes (results are views of pinned memory)."""
    return {k: (_raw(v) if isinstance(v, np.ndarray) else v) for k, v in vars(res).items()}


def _check_read(oracle_lib, res, objs, headers=False):
    """A read-feed result against the records it was given and the oracle's decode."""
    n = len(objs)
    arena, off = _csr(objs)
    assert np.array_equal(res.rec_off, off)
    assert res.records.tobytes() == b"".join(objs)
    assert len(res.info) == n
    if n == 0:
        assert res.acl_needed == 0 and res.regions_needed == 0
        return
    meta, info, acl, reg, _, tot = oracle_lib.decode_batch(arena[:-1], off)
    if headers:
        for f in ("data_off", "data_len", "data_status", "storage_version", "tombstone"):
            assert np.array_equal(res.info[f], info[f]), f
        assert (res.info["meta_status"] == 11).all() and res.meta is None
        return
    assert res.info.tobytes() == info.tobytes()
    assert res.meta.tobytes() == meta.tobytes()
    assert res.acl.tobytes() == acl.tobytes() and res.regions.tobytes() == reg.tobytes()
    assert res.acl_needed == int(tot[0]) and res.regions_needed == int(tot[1])
    for i in range(n):
        st, key = oracle_lib.key(meta[i], int(info[i]["meta_status"]))
        assert int(res.key_status[i]) == st and res.keys[i].tobytes() == key, i


def _check_put(oracle_lib, res, hb):
    """A write-feed result against the oracle's Marshal of the same rows."""
    oout, ooff, ost = oracle_lib.marshal_batch(hb)
    assert np.array_equal(res.status, ost)
    assert np.array_equal(res.rec_off, ooff)
    assert res.records.tobytes() == oout.tobytes()  # every record, to its last byte


def _need(hb, i):
    """honu_codec.h, honu_put_feed_create: the bytes a row's spans reference +
    its payload + 20 per ACL entry + 4 per region (absent sub-structs: nothing)."""
    r = hb.meta[i]
    p = int(r["present"])
    dl = int(hb.payload_off[i + 1]) - int(hb.payload_off[i])
    if not p & HAS_META:
        return dl
    live = ["mime"] + (["schema_name"] if p & HAS_SCHEMA else []) + \
        (["ip_address", "user_agent"] if p & HAS_PUBLISHER else []) + \
        (["public_key_id", "encryption_key", "hmac_secret", "signature"] if p & HAS_ENCRYPTION else [])
    return sum(int(r[f]["len"]) for f in live) + dl + 20 * int(r["acl_count"]) + 4 * int(r["regions_count"])


def _put_append_raw(feed, hb, i=0, data=None, row=None, **over):
    """honu_put_feed_append of row i of hb with any argument replaced."""
    if data is None:
        data = hb.payload[int(hb.payload_off[i]):int(hb.payload_off[i + 1])].tobytes()
    row = np.ascontiguousarray(hb.meta[i:i + 1] if row is None else row)
    a = dict(var=hb.var.ctypes.data, var_len=len(hb.var),
             acl=hb.acl.ctypes.data if len(hb.acl) else None, acl_len=len(hb.acl),
             reg=hb.regions.ctypes.data if len(hb.regions) else None, reg_len=len(hb.regions))
    a.update(over)
    return feed.lib.honu_put_feed_append(feed.feed, row.ctypes.data, a["var"], a["var_len"], a["acl"],
                                         a["acl_len"], a["reg"], a["reg_len"], data or None, len(data))


def _put_append_batch_raw(feed, hb, payload="own", payload_off=None):
    got = C.c_uint64(77)
    off = hb.payload_off if payload_off is None else payload_off
    st = feed.lib.honu_put_feed_append_batch(
        feed.feed, hb.meta.ctypes.data, len(hb), hb.var.ctypes.data, len(hb.var),
        hb.acl.ctypes.data if len(hb.acl) else None, len(hb.acl),
        hb.regions.ctypes.data if len(hb.regions) else None, len(hb.regions),
        hb.payload.ctypes.data if payload == "own" else payload, off.ctypes.data, C.byref(got))
    return st, got.value


def _sub(hb, a, b):
    """Rows [a, b) of a host batch (the tables stay whole)."""
    return HostBatch(hb.meta[a:b], hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off[a:b + 1])


def _full_meta(rng, nacl=5, nreg=4):
    return Metadata(
        ObjectID=rng.bytes(16), CollectionID=rng.bytes(16),
        Version=Version(Scalar(7, 9), 11, Scalar(1, 2), False, 12345),
        Schema=SchemaVersion("schema", 1, 2, 3), MIME="text/plain", Owner=rng.bytes(16),
        Group=rng.bytes(16), Permissions=0x5A,
        ACL=[AccessControl(rng.bytes(16), j) if j != 2 else None for j in range(nacl)] or None,
        WriteRegions=[100 + j for j in range(nreg)] or None,
        Publisher=Publisher(rng.bytes(16), rng.bytes(16), rng.bytes(16), "agent"),
        Encryption=Encryption("key-id", rng.bytes(32), rng.bytes(32), rng.bytes(64), 1, 2, 4),
        Compression=Compression(1, 6), Flags=3, Created=1, Modified=2)


@pytest.fixture(scope="module")
def random_rows():
    """2000 random_metas rows (spans, ACL lists with nil entries, regions), packed once."""
    metas, datas = random_metas(2000, 71)
    return pack_batch(metas, datas)


# --------------------------------------------------------------------------
# read feed
# --------------------------------------------------------------------------
def test_read_threaded_page(oracle_lib):
    """One append_batch whose run is above kParallelCopyMin (host_copy's byte
    ranges over several threads), from record 7 of its arena (off[0] != 0)."""
    from honu_amd.feed import RecordFeed
    n = 1500
    lens = np.random.default_rng(3).integers(0, 16385, n)
    objs = _objects(oracle_lib, n, 61, lens)
    arena, off = _csr(objs)
    first = 7
    assert int(off[-1] - off[first]) >= PARALLEL_COPY_MIN and off[first] != 0
    feed = RecordFeed(0, batch_records=2048, batch_bytes=16 << 20)
    assert feed.append_batch(arena, off, first) == (0, n - first)
    assert feed.pending == n - first
    _check_read(oracle_lib, feed.wait(feed.submit()), objs[first:])
    # the same page behind two records already in the slot (the copy lands past them)
    assert feed.append(objs[5]) == 0 and feed.append(objs[6]) == 0
    assert feed.append_batch(arena, off, first) == (0, n - first) and feed.pending == n - 5
    _check_read(oracle_lib, feed.wait(feed.submit()), objs[5:])
    feed.close()


def test_read_runs_around_the_thread_threshold(oracle_lib):
    """Runs of exactly kParallelCopyMin - 1, kParallelCopyMin and
    kParallelCopyMin + 1 bytes (the last fills the batch exactly), reached with
    one filler record of random bytes between valid ones."""
    from honu_amd.feed import RecordFeed
    small = _objects(oracle_lib, 40, 62)
    rng = np.random.default_rng(4)
    feed = RecordFeed(0, batch_records=64, batch_bytes=PARALLEL_COPY_MIN + 1)
    for size in (PARALLEL_COPY_MIN - 1, PARALLEL_COPY_MIN, PARALLEL_COPY_MIN + 1):
        filler = bytearray(rng.integers(0, 256, size - sum(map(len, small)), dtype=np.uint8).tobytes())
        filler[0] = 1  # the storage version: the parse goes on into the random bytes
        objs = small[:20] + [bytes(filler)] + small[20:]
        arena, off = _csr(objs, lead=5)
        assert int(off[-1] - off[0]) == size
        assert feed.append_batch(arena, off) == (0, 41)
        res = feed.wait(feed.submit())
        _check_read(oracle_lib, res, objs)
        assert res.info["meta_status"][20] != 0 and (np.delete(res.info["meta_status"], 20) == 0).all()
    feed.close()


def _fits(lens, cap_n, cap_bytes, n0=0, b0=0):
    """The header's rule for append_batch: records go in until the first that
    does not fit (the batch holds cap_n records and cap_bytes bytes)."""
    k, b = 0, b0
    for ln in lens:
        if n0 + k == cap_n or ln > cap_bytes - b:
            break
        k, b = k + 1, b + ln
    return k


def test_read_exact_fits():
    from honu_amd.feed import RecordFeed
    feed = RecordFeed(0, batch_records=8, batch_bytes=4096)
    assert feed.append(b"\x01" * 4000) == 0 and feed.append(b"\x02" * 96) == 0  # exactly batch_bytes
    assert feed.append(b"") == 0 and feed.pending == 3  # a zero-length record still goes in
    assert feed.append(b"x") == E_CAPACITY and feed.pending == 3
    assert feed.reserve(1) is None and feed.reserve(0) is not None and feed.pending == 4
    res = feed.wait(feed.submit())
    assert res.records.tobytes() == b"\x01" * 4000 + b"\x02" * 96
    assert list(res.rec_off) == [0, 4000, 4096, 4096, 4096]
    # the batch_records-th record goes in, the next does not, even when empty
    for i in range(8):
        assert feed.append(b"r") == 0
    assert feed.append(b"") == E_CAPACITY and feed.reserve(0) is None and feed.pending == 8
    assert list(feed.wait(feed.submit()).rec_off) == list(range(9))
    # append_batch that stops on records, and one that stops on bytes
    for lens, n0 in (([10] * 12, 0), ([10] * 12, 3), ([1000, 0, 2000, 1096, 0, 1, 5], 0),
                     ([4096, 0, 0, 1], 0), ([4097, 1], 0), ([0] * 9, 0), ([100, 3997], 2)):
        for _ in range(n0):
            assert feed.append(b"") == 0
        objs = [bytes([65 + i]) * ln for i, ln in enumerate(lens)]
        arena, off = _csr(objs, lead=3)
        k = _fits(lens, 8, 4096, n0)
        assert feed.append_batch(arena, off) == (0 if k == len(lens) else E_CAPACITY, k), lens
        assert feed.pending == n0 + k
        res = feed.wait(feed.submit())
        assert res.records.tobytes() == b"".join(objs[:k])
        assert list(res.rec_off) == [0] * n0 + list(np.cumsum([0] + lens[:k]))
    # offsets that decrease: refused, nothing appended
    assert feed.append(b"kept") == 0
    arena, off = _csr([b"aa", b"bbb", b"c"])
    off[2] = 1
    got = C.c_uint64(5)
    st = feed.lib.honu_feed_append_batch(feed.feed, arena.ctypes.data, off.ctypes.data, 3, C.byref(got))
    assert (st, got.value, feed.pending) == (E_ARG, 0, 1)
    assert feed.wait(feed.submit()).records.tobytes() == b"kept"
    feed.close()


def test_read_reserve(oracle_lib):
    """Records written through reserved pointers, interleaved with append,
    give the batch appends alone give; the refusals of honu_feed_reserve."""
    from honu_amd.feed import RecordFeed
    objs = _objects(oracle_lib, 60, 63) + [b"", b"\x01"]
    cap = 1 << 19
    a, b = RecordFeed(0, 64, cap), RecordFeed(0, 64, cap)
    for i, o in enumerate(objs):
        assert a.append(o) == 0
        if i % 3 == 1:
            assert b.append(o) == 0
        else:
            v = b.reserve(len(o))
            assert v is not None and len(v) == len(o)
            v[:] = np.frombuffer(o, np.uint8)
        assert b.pending == i + 1
    ra, rb = a.wait(a.submit()), b.wait(b.submit())
    _check_read(oracle_lib, rb, objs)
    assert _snapshot(ra) == _snapshot(rb)
    # capacity, at both limits
    assert b.reserve(cap + 1) is None and b.pending == 0
    assert b.reserve(cap) is not None and b.reserve(1) is None and b.pending == 1
    b.submit()
    for _ in range(64):
        assert b.reserve(0) is not None
    assert b.reserve(0) is None and b.pending == 64
    b.submit()
    # both slots in flight, and a NULL feed
    err = _lib.I32(0)
    assert not b.lib.honu_feed_reserve(b.feed, 1, C.byref(err)) and err.value == E_ARG
    err = _lib.I32(0)
    assert not b.lib.honu_feed_reserve(None, 1, C.byref(err)) and err.value == E_ARG
    assert not b.lib.honu_feed_reserve(None, 1, None)
    a.close()
    b.close()


class _ReadSide:
    """The read feed behind the calls the protocol tests make."""

    def __init__(self, oracle_lib, headers):
        from honu_amd import feed as F
        self.oracle, self.headers, self.F = oracle_lib, headers, F
        self.items = _objects(oracle_lib, 12, 64) + [b"\x01\x00", b""]
        self.feed = F.RecordFeed(0, 8, 1 << 16, headers_only=headers)
        self.lib, self.h = self.feed.lib, self.feed.feed

    def pending(self):
        return self.feed.pending

    def add(self, i):
        return self.lib.honu_feed_append(self.h, self.items[i], len(self.items[i]))

    def add_batch(self, idx):
        arena, off = _csr([self.items[i] for i in idx])
        got = C.c_uint64(77)
        st = self.lib.honu_feed_append_batch(self.h, arena.ctypes.data, off.ctypes.data, len(idx), C.byref(got))
        return st, got.value

    def others(self):  # the remaining calls that fill a slot
        err = _lib.I32(0)
        p = self.lib.honu_feed_reserve(self.h, 1, C.byref(err))
        return [err.value if not p else 0]

    def submit(self):
        t = C.c_uint64(0)
        return self.lib.honu_feed_submit(self.h, C.byref(t)), t.value

    def wait(self, t):
        r = self.F._Result()
        return self.lib.honu_feed_wait(self.h, t, C.byref(r)), bytes(r)

    def result(self, t):
        return self.feed.wait(t)

    def check(self, res, idx):
        _check_read(self.oracle, res, [self.items[i] for i in idx], self.headers)


class _PutSide:
    """The write feed behind the same calls."""

    def __init__(self, oracle_lib):
        from honu_amd import feed as F
        self.oracle, self.F = oracle_lib, F
        metas, datas = random_metas(13, 65)
        self.hb = pack_batch(metas + [None], datas + [b"nil"])
        self.feed = F.PutFeed(0, 8, 1 << 16)
        self.lib, self.h = self.feed.lib, self.feed.feed

    def pending(self):
        return self.feed.pending

    def add(self, i):
        return _put_append_raw(self.feed, self.hb, i)

    def _pick(self, idx):
        lens = [int(self.hb.payload_off[i + 1] - self.hb.payload_off[i]) for i in idx]
        off = np.zeros(len(idx) + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        pay = b"".join(self.hb.payload[int(self.hb.payload_off[i]):int(self.hb.payload_off[i + 1])].tobytes()
                       for i in idx)
        return HostBatch(np.ascontiguousarray(self.hb.meta[list(idx)]), self.hb.var, self.hb.acl,
                         self.hb.regions, np.frombuffer(pay + b"\0", np.uint8), off)

    def add_batch(self, idx):
        return _put_append_batch_raw(self.feed, self._pick(idx))

    def others(self):
        return []

    def submit(self):
        t = C.c_uint64(0)
        return self.lib.honu_put_feed_submit(self.h, C.byref(t)), t.value

    def wait(self, t):
        r = self.F._PutResult()
        return self.lib.honu_put_feed_wait(self.h, t, C.byref(r)), bytes(r)

    def result(self, t):
        return self.feed.wait(t)

    def check(self, res, idx):
        _check_put(self.oracle, res, self._pick(idx))
        if 13 in idx:
            assert res.objects()[list(idx).index(13)] == 8  # Marshal(nil, data): HONU_ERR_PANIC


def _side(kind, oracle_lib):
    return _PutSide(oracle_lib) if kind == "put" else _ReadSide(oracle_lib, kind == "headers")


@pytest.mark.parametrize("kind", ["full", "headers", "put"])
def test_protocol(oracle_lib, kind):
    """Tickets, wait on unknown / stale / repeated tickets, every filling call
    against two slots in flight, pending at every step, an empty submit."""
    s = _side(kind, oracle_lib)
    assert s.pending() == 0
    assert s.wait(0)[0] == E_ARG and s.wait(1)[0] == E_ARG  # nothing was issued yet
    assert [s.add(i) for i in (0, 1, 2)] == [0, 0, 0] and s.pending() == 3
    assert s.submit() == (0, 1) and s.pending() == 0  # tickets count from 1
    assert s.add_batch([3, 4]) == (0, 2) and s.pending() == 2
    assert s.wait(2)[0] == E_ARG  # not issued yet
    assert s.submit() == (0, 2) and s.pending() == 0
    # both slots in flight: every call that fills or submits is refused
    assert s.submit()[0] == E_ARG and s.add(5) == E_ARG and s.add_batch([5, 6]) == (E_ARG, 0)
    assert all(e == E_ARG for e in s.others()) and s.pending() == 0
    assert s.wait(3)[0] == E_ARG  # the refused submit issued no ticket
    st, a1 = s.wait(1)
    assert st == 0
    ra = s.result(1)
    s.check(ra, [0, 1, 2])  # the refused calls changed nothing
    snap = _snapshot(ra)
    assert s.wait(1) == (0, a1) and _snapshot(s.result(1)) == snap  # a second wait: the same views
    st, b1 = s.wait(2)
    s.check(s.result(2), [3, 4])
    assert st == 0 and s.wait(2) == (0, b1) and _snapshot(ra) == snap and s.pending() == 0
    # the next append refills slot 0: ticket 1 is gone, ticket 2 is not
    assert s.add(5) == 0 and s.pending() == 1
    assert s.wait(1)[0] == E_ARG and s.wait(2) == (0, b1)
    assert s.submit() == (0, 3) and s.pending() == 0
    # an empty submit (slot 1, which held a batch)
    assert s.submit() == (0, 4) and s.wait(2)[0] == E_ARG
    re = s.result(4)
    assert len(re.rec_off) == 1 and re.rec_off[0] == 0 and len(re.records) == 0
    s.check(re, [])
    s.check(s.result(3), [5])
    # a batch through each slot after all that
    assert s.add_batch([13, 6, 7]) == (0, 3) and s.submit() == (0, 5)
    assert s.add(12) == 0 and s.submit() == (0, 6)
    s.check(s.result(6), [12])
    s.check(s.result(5), [13, 6, 7])
    assert s.wait(7)[0] == E_ARG and s.wait(4)[0] == E_ARG and s.wait(3)[0] == E_ARG
    s.feed.close()


@pytest.mark.parametrize("kind", ["full", "headers", "put"])
def test_lifetime(oracle_lib, kind):
    """A result's views stay valid until the next append into its slot: they
    are unchanged while the other slot's batch is in flight and after it was
    waited for."""
    s = _side(kind, oracle_lib)
    assert s.add_batch([0, 1, 2, 3]) == (0, 4) and s.submit() == (0, 1)
    ra = s.result(1)
    s.check(ra, [0, 1, 2, 3])
    snap, addr = _snapshot(ra), s.wait(1)
    assert s.add_batch([4, 5, 6, 7, 8, 9, 10, 11]) == (0, 8) and s.submit() == (0, 2)
    assert _snapshot(ra) == snap and s.wait(1) == addr  # B in flight
    s.check(s.result(2), [4, 5, 6, 7, 8, 9, 10, 11])
    assert _snapshot(ra) == snap and s.wait(1) == addr  # B waited for
    s.check(ra, [0, 1, 2, 3])
    assert s.pending() == 0 and s.wait(1) == addr  # pending() does not release the slot
    assert s.add(12) == 0 and s.wait(1)[0] == E_ARG  # the documented invalidation point
    s.feed.close()


@pytest.mark.parametrize("headers", [False, True], ids=["full", "headers"])
def test_read_slot_reuse(oracle_lib, headers):
    """Both slots hold a full batch; then three short records run through one
    and a batch of only zero-length records (no H2D copy of records) through
    the other. Nothing of the earlier batches shows through."""
    from honu_amd.feed import RecordFeed
    objs = _objects(oracle_lib, 60, 66)
    feed = RecordFeed(0, batch_records=256, batch_bytes=1 << 16, headers_only=headers)
    arena, off = _csr(objs)
    first = 0
    for _ in range(2):
        st, got = feed.append_batch(arena, off, first)
        assert st == E_CAPACITY and got > 8  # full by bytes
        _check_read(oracle_lib, feed.wait(feed.submit()), objs[first:first + got], headers)
        first += got
    short = [objs[50], b"\x01\x00", objs[51][:9]]
    for batch in (short, [b""] * 5, [b""], short[::-1]):
        for o in batch:
            assert feed.append(o) == 0
        _check_read(oracle_lib, feed.wait(feed.submit()), batch, headers)
    feed.close()


@pytest.mark.parametrize("kind", ["full", "headers", "put"])
def test_destroy_with_a_batch_in_flight(oracle_lib, kind):
    """destroy synchronises: submit, never wait, close; a feed made afterwards works."""
    s = _side(kind, oracle_lib)
    assert s.add_batch(list(range(8))) == (0, 8) and s.submit() == (0, 1)
    assert s.add_batch([8, 9]) == (0, 2) and s.submit() == (0, 2)
    s.feed.close()
    s = _side(kind, oracle_lib)
    assert s.add_batch([3, 1, 2]) == (0, 3) and s.submit() == (0, 1)
    s.check(s.result(1), [3, 1, 2])
    s.feed.close()


# --------------------------------------------------------------------------
# write feed
# --------------------------------------------------------------------------
def _threaded_shape(rows, shape):
    """The rows and payload lengths of one append_batch of >= kParallelCopyMin input bytes."""
    if shape == "even":
        return rows, [4500] * 2000
    if shape == "big_first":
        return _sub(rows, 0, 501), [9 << 20] + [100] * 500
    if shape == "big_last":
        return _sub(rows, 0, 501), [100] * 500 + [9 << 20]
    if shape == "two":
        return _sub(rows, 0, 2), [5 << 20, 4 << 20]
    # a batch of exactly `shape` input bytes: the last payload makes up the rest
    part = _sub(rows, 0, 50)
    rest = sum(_need(_with_payloads(part, [0] * 50, 1), i) for i in range(50))
    return part, [0] * 49 + [shape - rest]


@pytest.mark.parametrize("shape", ["even", "big_first", "big_last", "two", PARALLEL_COPY_MIN - 1,
                                   PARALLEL_COPY_MIN])
def test_put_threaded_fill(oracle_lib, random_rows, shape):
    """One append_batch above kParallelCopyMin: put_fill runs on several
    threads over equal-byte record ranges (one giant record first or last, two
    records, even records), and batches just below and exactly at the threshold."""
    from honu_amd.feed import PutFeed
    part, lens = _threaded_shape(random_rows, shape)
    hb = _with_payloads(part, lens, 7)
    total = sum(_need(hb, i) for i in range(len(hb)))
    if isinstance(shape, int):
        assert total == shape
    else:
        assert total >= PARALLEL_COPY_MIN
    feed = PutFeed(0, batch_records=2048, batch_bytes=12 << 20)
    assert feed.append_batch(hb) == (0, len(hb)) and feed.pending == len(hb)
    res = feed.wait(feed.submit())
    assert (res.status == 0).all()
    _check_put(oracle_lib, res, hb)
    if shape == "even":  # the threaded fill behind records already in the slot (first > 0)
        for i in range(3):
            assert _put_append_raw(feed, hb, i) == 0
        assert feed.append_batch(hb, 3) == (0, len(hb) - 3) and feed.pending == len(hb)
        _check_put(oracle_lib, feed.wait(feed.submit()), hb)
    feed.close()


def test_put_budget(oracle_lib, random_rows):
    """batch_bytes counts span bytes + payload + 20 per ACL entry + 4 per
    region: a batch filled to exactly that, one more byte refused; absent
    sub-structs' spans cost nothing and are not validated."""
    from honu_amd.feed import PutFeed
    cap = 1 << 17
    feed = PutFeed(0, batch_records=64, batch_bytes=cap)
    hb = _sub(random_rows, 100, 120)
    used = sum(_need(hb, i) for i in range(20))
    assert used < cap - 1000
    assert feed.append_batch(hb) == (0, 20)
    # rows whose absent sub-structs carry spans outside the arena
    metas = [Metadata(MIME="a/b", ObjectID=bytes(range(16))), None,
             Metadata(MIME="c", Schema=SchemaVersion("only", 1, 2, 3), ACL=[None, None])]
    odd = pack_batch(metas, [b"12345", b"nil", None])
    for f in ("schema_name", "ip_address", "user_agent", "public_key_id", "encryption_key",
              "hmac_secret", "signature"):
        for i in (0, 1, 2):
            if not (f == "schema_name" and i == 2):
                odd.meta[i][f] = (2**64 - 1 - i, 2**63 + 5)
    odd.meta[1]["mime"] = (2**40, 2**41)  # no HONU_HAS_META: not even MIME counts
    odd.meta[1]["acl_count"], odd.meta[1]["regions_count"] = 2**50, 2**51
    needs = [3 + 5, 3, 1 + 4 + 40]
    assert [_need(odd, i) for i in range(3)] == needs
    assert _put_append_batch_raw(feed, odd) == (0, 3)
    used += sum(needs)
    # exactly the rest, then one byte more
    one = pack_batch([Metadata(MIME="x" * 100, WriteRegions=[1, 2, 3])], [None])
    rest = cap - used - 112
    assert _put_append_raw(feed, one, data=b"z" * (rest + 1)) == E_CAPACITY and feed.pending == 23
    assert _put_append_raw(feed, one, data=b"z" * rest) == 0 and feed.pending == 24
    nothing = pack_batch([Metadata()], [None])
    assert _put_append_raw(feed, nothing) == 0  # a record that needs no byte still goes in
    assert _put_append_raw(feed, nothing, data=b"1") == E_CAPACITY and feed.pending == 25
    assert _need(random_rows, 0) > 0
    assert _put_append_batch_raw(feed, _sub(random_rows, 0, 1)) == (E_CAPACITY, 0)
    res = feed.wait(feed.submit())
    objs = res.objects()
    assert len(objs) == 25
    _check_put(oracle_lib, HostBatchView(res, 0, 20), hb)
    _check_put(oracle_lib, HostBatchView(res, 20, 23), odd)
    assert objs[21] == 8
    _check_put(oracle_lib, HostBatchView(res, 23, 24), _with_fixed_payload(one, b"z" * rest))
    _check_put(oracle_lib, HostBatchView(res, 24, 25), nothing)
    feed.close()


def test_put_record_limit(oracle_lib):
    """The batch_records-th record goes in, the next does not, even when it
    needs no byte; append_batch stops there."""
    from honu_amd.feed import PutFeed
    feed = PutFeed(0, batch_records=4, batch_bytes=1 << 16)
    nothing = pack_batch([Metadata()], [None])
    metas, datas = random_metas(6, 12)
    six = pack_batch(metas, datas)
    for _ in range(4):
        assert _put_append_raw(feed, nothing) == 0
    assert _put_append_raw(feed, nothing) == E_CAPACITY and feed.pending == 4
    assert _put_append_batch_raw(feed, six) == (E_CAPACITY, 0) and feed.pending == 4
    res = feed.wait(feed.submit())
    assert len(res.status) == 4
    for i in range(4):
        _check_put(oracle_lib, HostBatchView(res, i, i + 1), nothing)
    assert _put_append_raw(feed, nothing) == 0
    assert _put_append_batch_raw(feed, six) == (E_CAPACITY, 3) and feed.pending == 4
    res = feed.wait(feed.submit())
    _check_put(oracle_lib, HostBatchView(res, 1, 4), _sub(six, 0, 3))
    assert feed.append_batch(six, 3) == (0, 3)  # the rest fits the next batch
    _check_put(oracle_lib, feed.wait(feed.submit()), _sub_payload(six, 3, 6))
    feed.close()


class HostBatchView:
    """Records [a, b) of a write-feed result, offsets from 0, as a result."""

    def __init__(self, res, a, b):
        base = int(res.rec_off[a])
        self.status = res.status[a:b]
        self.rec_off = res.rec_off[a:b + 1] - np.uint64(base)
        self.records = res.records[base:int(res.rec_off[b])]


def _with_fixed_payload(hb, data):
    return HostBatch(hb.meta, hb.var, hb.acl, hb.regions, np.frombuffer(data + b"\0", np.uint8),
                     np.array([0, len(data)], np.uint64))


def test_put_refusals(oracle_lib):
    """One representative of each class of put_plan's refusals through the
    ABI: nothing is appended, and the batch marshals as if the call had not
    been made."""
    from honu_amd.feed import PutFeed
    rng = np.random.default_rng(8)
    cap = 1 << 16
    feed = PutFeed(0, batch_records=32, batch_bytes=cap)
    good = pack_batch([_full_meta(rng), _full_meta(rng, 0, 0), _full_meta(rng, 9, 1)], [b"abc", None, b"de"])
    bad = pack_batch([_full_meta(rng)], [b"xyz"])

    def row(**fields):
        r = bad.meta.copy()
        for k, v in fields.items():
            r[0][k] = v
        return r

    huge = 1 << 40
    refusals = [
        (E_INPUT, dict(row=row(mime=(len(bad.var) + 1, 1)))),            # off > var_len
        (E_INPUT, dict(row=row(user_agent=(len(bad.var) - 2, 3)))),      # off + len > var_len
        (E_INPUT, dict(row=row(signature=(2**64 - 1, 2)))),              # a sum that wraps
        (E_INPUT, dict(var=None)),                                       # no arena
        (E_INPUT, dict(row=row(acl_off=len(bad.acl)))),                  # a list outside its array
        (E_INPUT, dict(row=row(regions_off=2**64 - 1))),
        (E_INPUT, dict(reg=None)),                                       # a NULL array
        (E_INPUT, dict(row=row(present=int(bad.meta[0]["present"]) | ACL_INPLACE))),
        (E_INPUT, dict(row=row(present=int(bad.meta[0]["present"]) | (1 << 9)))),
        (E_CAPACITY, dict(row=row(acl_count=cap // 20 + 1), acl_len=huge)),   # more than a batch holds
        (E_CAPACITY, dict(row=row(regions_count=cap // 4 + 1), reg_len=huge)),
    ]
    for i in range(3):
        for st, kw in refusals[i::3]:
            assert _put_append_raw(feed, bad, **kw) == st, kw
            assert feed.pending == i
        assert _put_append_raw(feed, good, i) == 0
    assert feed.lib.honu_put_feed_append(feed.feed, good.meta.ctypes.data, None, 0, None, 0, None, 0, None, 5) == E_ARG
    assert feed.pending == 3
    _check_put(oracle_lib, feed.wait(feed.submit()), good)
    # append_batch refused at row j: the rows before it are in
    metas, datas = random_metas(10, 9)
    hb = pack_batch(metas, datas)
    j = 6
    hb.meta[j]["mime"] = (len(hb.var) - 1, 2)
    assert _put_append_batch_raw(feed, hb) == (E_INPUT, j) and feed.pending == j
    _check_put(oracle_lib, feed.wait(feed.submit()), _sub(hb, 0, j))
    # payload offsets that decrease
    hb = pack_batch(metas, [b"0123456789"] * 10)
    off = hb.payload_off.copy()
    off[4] = off[3] - 1
    assert _put_append_batch_raw(feed, hb, payload_off=off) == (E_INPUT, 3) and feed.pending == 3
    _check_put(oracle_lib, feed.wait(feed.submit()), _sub(hb, 0, 3))
    # a NULL payload arena with a non-empty range
    hb = pack_batch(metas, [None, None, b"x"] + [None] * 7)
    assert _put_append_batch_raw(feed, hb, payload=None) == (E_ARG, 2) and feed.pending == 2
    _check_put(oracle_lib, feed.wait(feed.submit()), _sub(hb, 0, 2))
    feed.close()


def _widest():
    """Every field at its widest at once: 5- and 10-byte varints, every
    sub-struct, ACL entries, regions of 5 bytes."""
    u32, u64, i64 = 2**32 - 1, 2**64 - 1, -2**63
    b = lambda c: bytes([c]) * 16384  # noqa: E731
    return Metadata(
        ObjectID=b"\xff" * 16, CollectionID=b"\xfe" * 16,
        Version=Version(Scalar(u32, u64), u32, Scalar(u32, u64), True, i64),
        Schema=SchemaVersion("s" * 16384, u32, u32, u32), MIME="m" * 16384, Owner=b"\xfd" * 16,
        Group=b"\xfc" * 16, Permissions=255, ACL=[AccessControl(b"\xfb" * 16, 255)] * 7,
        WriteRegions=[u32] * 9, Publisher=Publisher(b"\xfa" * 16, b"\xf9" * 16, b(1), "u" * 16384),
        Encryption=Encryption("k" * 16384, b(2), b(3), b(4), 255, 255, 255),
        Compression=Compression(255, i64), Flags=255, Created=i64, Modified=i64), b(5)


def test_put_output_bound(oracle_lib):
    """submit() copies back an upper bound of the batch's encoded bytes
    (kFixedBound + span bytes + payload + 18 per ACL entry + 5 per region per
    record), never the exact total: rows with every varint at its widest come
    back complete, the widest one last in its batch and alone in a batch; and
    a record of batch_bytes / 4 five-byte regions (output 5/4 of the input)
    fits the output arena."""
    from honu_amd.feed import PutFeed
    metas, datas = extreme_metas()
    wm, wd = _widest()
    hb = pack_batch(metas + [wm], datas + [wd])
    feed = PutFeed(0, batch_records=128, batch_bytes=1 << 20)
    first, nb = 0, 0
    while first < len(hb):
        st, got = feed.append_batch(hb, first)
        assert got > 0 and (st == 0) == (first + got == len(hb))
        _check_put(oracle_lib, feed.wait(feed.submit()), _sub_payload(hb, first, first + got))
        first, nb = first + got, nb + 1
    assert nb >= 2
    alone = pack_batch([wm], [wd])
    for _ in range(2):  # both slots (each held longer batches)
        assert feed.append_batch(alone) == (0, 1)
        res = feed.wait(feed.submit())
        _check_put(oracle_lib, res, alone)
        assert res.status[0] == 0
    feed.close()
    cap = 1 << 16
    regions = pack_batch([Metadata(WriteRegions=[2**32 - 1] * (cap // 4))], [None])
    assert _need(regions, 0) == cap
    feed = PutFeed(0, batch_records=1, batch_bytes=cap)
    for _ in range(2):
        assert feed.append_batch(regions) == (0, 1)
        res = feed.wait(feed.submit())
        assert res.status[0] == 0 and int(res.rec_off[1]) > 5 * (cap // 4)
        _check_put(oracle_lib, res, regions)
    feed.close()


def _sub_payload(hb, a, b):
    """Rows [a, b) with the payload offsets rebased to their own arena."""
    base = int(hb.payload_off[a])
    return HostBatch(hb.meta[a:b], hb.var, hb.acl, hb.regions, hb.payload[base:],
                     hb.payload_off[a:b + 1] - np.uint64(base))


def test_put_acl_sized(oracle_lib):
    """Rows without HONU_ACL_SIZED (append computes the list's length, nil
    entries 1 byte each) and rows that carry it encode alike."""
    from honu_amd.feed import PutFeed
    rng = np.random.default_rng(10)
    metas = [_full_meta(rng, k, k % 3) for k in (0, 1, 3, 4, 40)] + \
        [Metadata(ACL=[None] * 6), Metadata(ACL=[None, AccessControl(bytes(16), 1)], MIME="q")]
    hb = pack_batch(metas, [b"p%d" % i for i in range(len(metas))])
    assert all(int(r["present"]) & ACL_SIZED for r in hb.meta if r["acl_count"])
    bare = HostBatch(hb.meta.copy(), hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off)
    bare.meta["present"] &= ~np.uint32(ACL_SIZED)
    bare.meta["acl_bytes"] = 0
    oout, ooff, ost = oracle_lib.marshal_batch(hb)
    assert (ost == 0).all()
    feed = PutFeed(0, batch_records=16, batch_bytes=1 << 16)
    for rows in (bare, hb):
        assert _put_append_batch_raw(feed, rows) == (0, len(metas))
        _check_put(oracle_lib, feed.wait(feed.submit()), hb)
        for i in range(len(metas)):
            assert _put_append_raw(feed, rows, i) == 0
        _check_put(oracle_lib, feed.wait(feed.submit()), hb)
    feed.close()


def test_put_slot_reuse(oracle_lib, random_rows):
    """A smaller batch through a slot that held a larger one (the device
    arenas and the pinned output keep the earlier bytes)."""
    from honu_amd.feed import PutFeed
    feed = PutFeed(0, batch_records=256, batch_bytes=1 << 18)
    first = 200
    for _ in range(2):
        st, got = feed.append_batch(random_rows, first)
        assert st == E_CAPACITY and got > 50
        _check_put(oracle_lib, feed.wait(feed.submit()), _sub_payload(random_rows, first, first + got))
        first += got
    small = pack_batch([Metadata(MIME="s"), None, Metadata()], [b"1", None, None])
    for hb in (small, pack_batch([Metadata()], [None]), _sub_payload(random_rows, 3, 5)):
        assert feed.append_batch(hb) == (0, len(hb))
        _check_put(oracle_lib, feed.wait(feed.submit()), hb)
    feed.close()


def test_round_trip(oracle_lib):
    """The write feed's records through the read feed: the oracle's decode,
    and the Metadata that went in."""
    from honu_amd.feed import PutFeed, RecordFeed
    metas, datas = random_metas(300, 11)
    hb = pack_batch(metas, datas)
    put = PutFeed(0, batch_records=512, batch_bytes=1 << 20)
    assert put.append_batch(hb) == (0, 300)
    enc = put.wait(put.submit())
    _check_put(oracle_lib, enc, hb)
    arena, off = enc.records.copy(), enc.rec_off.copy()
    put.close()
    feed = RecordFeed(0, batch_records=512, batch_bytes=1 << 20)
    assert feed.append_batch(np.append(arena, np.uint8(0)), off) == (0, 300)
    res = feed.wait(feed.submit())
    objs = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(300)]
    _check_read(oracle_lib, res, objs)
    assert (res.info["meta_status"] == 0).all() and (res.info["data_status"] == 0).all()
    for i in range(300):
        assert unpack_row(res.meta[i], res.records, res.acl, res.regions) == normalize(metas[i]), i
        o, ln = int(res.info[i]["data_off"]), int(res.info[i]["data_len"])
        assert res.records[o:o + ln].tobytes() == (datas[i] or b""), i
    feed.close()
