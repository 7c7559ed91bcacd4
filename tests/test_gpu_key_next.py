"""honu_key_next on the GPU against numpy and keys.next.

The expectation is the host's alone: keys.next (honu_amd/keys.py, itself
checked against a sequential simulation in tests/test_key_next_host.py) over
the first min(valid, n) rows of the column, its rows laid out with numpy as
honu_next rows, keys, key statuses and stamped honu_meta rows. It never calls
the library. Every input and output is a guarded view (tests/guards.py) under
both fills, d_sorted, d_requests and d_keys_out at byte phases 0, 1 and 3; the
write set is exactly d_out[0, m), d_keys_out[0, 29 m), d_key_status[0, m), the
named fields of the ASSIGNED rows of d_meta and the workspace, and the inputs
are unchanged. Sizes are in units of S, the param "sort_tile": the requests are
sorted, so S is where the call's one multi-workgroup step changes shape.

The context covers 4096 records. m = 2 S + 77 is more than that with S = 2048,
and the call refuses m above max_records, so that one size runs on a context
of its own that covers exactly 2 S + 77 records.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (HAS_META, HAS_PARENT, HAS_VERSION, INFO_DTYPE, META_DTYPE, NEXT_ASSIGNED,  # noqa: E402
                               NEXT_BAD_KEY, NEXT_CREATE, NEXT_DELETE, NEXT_DTYPE, NEXT_EXISTS, NEXT_FOUND,
                               NEXT_HAS_PARENT, NEXT_LIVE, NEXT_MERGE, NEXT_NOT_FOUND, NEXT_SKIPPED, NEXT_TOMBSTONE,
                               NEXT_UPDATE, NEXT_WRAPPED, SEEK_DTYPE, SEEK_NONE, Scalar)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
OK, INPUT = hobj.OK, hobj.INPUT
OPS = (NEXT_CREATE, NEXT_UPDATE, NEXT_MERGE, NEXT_DELETE)
PHASES = ((0, 0, 0), (1, 3, 0), (3, 1, 1), (0, 1, 3))  # (d_sorted, d_requests, d_keys_out)
MAX_RECORDS = 4096
PID, REGION, NOW = 0x01020304, 0xA1B2C3D4, 0x1122334455667788
M64 = (1 << 64) - 1


def _param(c, name):
    v = L.C.c_int64(0)
    L.check(c.lib.honu_ctx_get_param(c.ctx, name, L.C.byref(v)), name.decode())
    return int(v.value)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, MAX_RECORDS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def S(codec):
    s = _param(codec, b"sort_tile")
    assert s >= 256 and s % 64 == 0 and s + 1 <= MAX_RECORDS
    return s


# --------------------------------------------------------------------------
# columns and requests
# --------------------------------------------------------------------------
class Column:
    """A resident column of n rows: sorted keys, the order (a record index per
    position) and the records' tombstone bytes. Object IDs start with a byte in
    [0x10, 0xef], so an ID of zeros lies before the first key and one of 0xff
    after the last."""

    def __init__(self, n, objects, seed):
        rng = np.random.default_rng(seed)
        self.n = n
        objects = max(1, min(objects, n)) if n else 0
        self.oids = rng.integers(0, 256, (objects, 16), dtype=np.uint8)
        if objects:
            self.oids[:, 0] = rng.integers(0x10, 0xF0, objects)
            self.oids[0, 15] = 0xFF  # no ObjectLimit wrap
        which = np.concatenate([np.arange(objects), rng.integers(0, max(objects, 1), n - objects)]) if n else \
            np.zeros(0, np.int64)
        keys = np.zeros((n, 29), np.uint8)
        keys[:, 0] = 1
        if n:
            keys[:, 1:17] = self.oids[which]
            vid = rng.permutation(n).astype(np.uint64) * np.uint64(0x0000010000000101) + np.uint64(1)  # every byte in use
            keys[:, 17:25] = vid.astype(">u8").view(np.uint8).reshape(n, 8)
            keys[:, 25:29] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
        self.keys = keys[np.lexsort(keys.T[::-1])] if n else keys
        self.order = rng.permutation(n).astype(np.uint32)
        self.tomb = (rng.integers(0, 3, n) == 0).astype(np.uint8)

    def rows(self, valid, seed=5):
        """The column as the call is given it: the rows at and past min(valid, n) hold noise."""
        v = min(valid, self.n)
        rows = self.keys.copy()
        rows[v:] = np.random.default_rng(seed).integers(0, 256, (self.n - v, 29), dtype=np.uint8)
        return rows


def request_rows(oids, tail_seed=1):
    """29-byte request rows of the object IDs: keyVersion, the ID, then 12 bytes of noise that no call reads."""
    oids = np.asarray(oids, np.uint8).reshape(-1, 16)
    req = np.random.default_rng(tail_seed).integers(0, 256, (len(oids), 29), dtype=np.uint8)
    req[:, 0] = 1
    req[:, 1:17] = oids
    return req


def mixed_requests(col, m, seed, spoil=True):
    """(requests, statuses): stored and absent objects, an ID of zeros and one
    of 0xff among them, drawn with repeats from a pool of about m / 3 so that
    runs form and interleave; with `spoil` every seventh row is skipped
    (status not OK) and every eleventh has a bad first byte."""
    rng = np.random.default_rng(seed)
    k = max(2, m // 3)
    stored = col.oids[rng.integers(0, len(col.oids), k)] if len(col.oids) else np.zeros((0, 16), np.uint8)
    absent = rng.integers(0, 256, (max(2, k // 3), 16), dtype=np.uint8)
    absent[0], absent[1] = 0x00, 0xFF
    pool = np.concatenate([stored, absent])
    req = request_rows(pool[rng.integers(0, len(pool), m)], seed)
    status = np.zeros(m, np.int32)
    if spoil:
        status[3::7] = rng.choice([3, 10, -1, 1 << 30], len(status[3::7]))
        req[5::11, 0] = rng.choice([0, 2, 0x81, 0xFF], len(req[5::11]))
    return req, status


# --------------------------------------------------------------------------
# expectations
# --------------------------------------------------------------------------
def expected(rows, valid, reqs, status, op, pid=PID, order=None, tomb=None):
    """(honu_next rows, keys uint8[m, 29], key statuses) of keys.next over the column's first min(valid, n) rows."""
    n, m = len(rows), len(reqs)
    sorted_keys = [bytes(r) for r in rows[:min(valid, n)]]
    live = None
    if order is not None and tomb is not None:
        live = lambda p: not tomb[min(int(order[p]), n - 1)]  # noqa: E731
    res = hkeys.next(sorted_keys, [bytes(r) for r in reqs], op, pid, live=live,
                     skip=None if status is None else [s != OK for s in status])
    out = np.zeros(m, NEXT_DTYPE)
    out["parent_record"] = SEEK_NONE
    for i, g in enumerate(res):
        out["flags"][i] = g.flags
        if g.scalar is not None:
            out["vid"][i], out["pid"][i] = g.scalar.VID, g.scalar.PID
        if g.parent is not None:
            out["parent_vid"][i], out["parent_pid"][i] = g.parent.VID, g.parent.PID
        if g.parent_pos is not None and order is not None:
            out["parent_record"][i] = order[g.parent_pos]
    keys = np.frombuffer(b"".join(g.key for g in res), np.uint8).reshape(m, 29)
    assigned = (out["flags"] & NEXT_ASSIGNED) != 0
    return out, keys, np.where(assigned, OK, INPUT).astype(np.int32)


def stamped(meta, out, reqs, op, region=REGION, now=NOW):
    """The caller's rows after the call: the named fields of the ASSIGNED rows, and nothing else."""
    meta = meta.view(np.uint8).copy().view(META_DTYPE)  # (a copy of the bytes: the struct's padding too)
    a = (out["flags"] & NEXT_ASSIGNED) != 0
    par = a & ((out["flags"] & NEXT_HAS_PARENT) != 0)
    for f in ("vid", "pid", "parent_vid", "parent_pid"):
        meta[f][a] = out[f][a]
    meta["tombstone"][a] = op == NEXT_DELETE
    meta["region"][a] = region
    meta["version_created"][a] = now
    meta["modified"][a] = now
    meta["created"][a & ~par] = now
    meta["object_id"][a] = reqs[a, 1:17]
    meta["present"][a] = (meta["present"][a] | np.uint32(HAS_META | HAS_VERSION)) & ~np.uint32(HAS_PARENT)
    meta["present"][par] |= np.uint32(HAS_PARENT)
    return meta


def noise_meta(m, seed=9):
    if m == 0:
        return np.zeros(0, META_DTYPE)
    return np.random.default_rng(seed).integers(0, 256, 352 * m, dtype=np.uint8).view(META_DTYPE)


# --------------------------------------------------------------------------
# one guarded call
# --------------------------------------------------------------------------
def put(codec, a, phase, fill):
    """The bytes of `a` in a guarded block at a byte phase."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = guards.guarded(a.nbytes, phase=phase, fill=fill, device=codec.torch_device)
    if a.nbytes:
        t.copy_(torch.from_numpy(a.copy()).to(codec.torch_device))
    return t


def u64(x):
    return np.array([x], np.uint64)


class Call:
    """The guarded device arguments of one call. order / tomb / status / meta None: the pointer is NULL."""

    def __init__(self, codec, rows, valid, reqs, status, fill, phases=(0, 0, 0), order=None, tomb=None, meta=None):
        self.codec, self.n, self.m = codec, len(rows), len(reqs)
        self.host = {"sorted": rows, "valid": u64(valid), "requests": reqs}
        if order is not None:
            self.host["order"] = np.asarray(order, np.uint32)
        if tomb is not None:
            info = np.zeros(self.n, INFO_DTYPE)
            info["tombstone"], info["data_len"] = tomb, 0x1112131415161718
            self.host["info"] = info
        if status is not None:
            self.host["req_status"] = np.asarray(status, np.int32)
        phase = {"sorted": phases[0], "requests": phases[1]}
        self.dev = {k: put(codec, a, phase.get(k, 0), fill) for k, a in self.host.items()}
        dev = codec.torch_device
        self.work_bytes = int(codec.lib.honu_key_next_workspace(self.m))
        self.out = guards.guarded(32 * self.m, fill=fill, device=dev)
        self.keys_out = guards.guarded(29 * self.m, phase=phases[2], fill=fill, device=dev)
        self.key_status = guards.guarded(4 * self.m, fill=fill, device=dev)
        self.work = guards.guarded(self.work_bytes, fill=fill, device=dev)
        self.meta0 = meta
        self.meta = put(codec, meta, 0, fill) if meta is not None else None
        self.outs = (self.out, self.keys_out, self.key_status, self.work)

    def args(self, op, **kw):
        A = guards.address
        d = self.dev
        x = dict(ctx=self.codec.ctx, sorted=A(d["sorted"]), valid=A(d["valid"]), n=self.n, order=A(d.get("order")),
                 info=A(d.get("info")), requests=A(d["requests"]), req_status=A(d.get("req_status")), m=self.m, op=op,
                 pid=PID, region=REGION, now=NOW, out=A(self.out), keys_out=A(self.keys_out),
                 key_status=A(self.key_status), meta=A(self.meta), work=A(self.work), work_bytes=self.work_bytes)
        x.update(kw)
        return x

    def run(self, op, **kw):
        x = self.args(op, **kw)
        return self.codec.lib.honu_key_next(
            x["ctx"], x["sorted"], x["valid"], x["n"], x["order"], x["info"], x["requests"], x["req_status"], x["m"],
            x["op"], x["pid"], x["region"], x["now"], x["out"], x["keys_out"], x["key_status"], x["meta"], x["work"],
            x["work_bytes"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs:
            guards.assert_untouched(t, [])
        if self.meta is not None:
            assert guards.block_of(self.meta).bytes().tobytes() == self.meta0.view(np.uint8).tobytes()
            guards.assert_untouched(self.meta, [(0, 352 * self.m)])
        self.inputs_unchanged()

    def check(self, want, meta_want=None):
        """The outputs against (rows, keys, key statuses), the stamped rows and the write set."""
        torch.cuda.synchronize()
        out, keys, status = want
        m = self.m
        got = guards.block_of(self.out).bytes().view(NEXT_DTYPE)
        bad = np.flatnonzero(got != out)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], out[bad[:4]])
        got = guards.block_of(self.keys_out).bytes().reshape(m, 29)
        bad = np.flatnonzero((got != keys).any(axis=1))
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], keys[bad[:4]])
        got = guards.block_of(self.key_status).bytes().view(np.int32)
        bad = np.flatnonzero(got != status)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], status[bad[:4]])
        guards.assert_untouched(self.out, [(0, 32 * m)])
        guards.assert_untouched(self.keys_out, [(0, 29 * m)])
        guards.assert_untouched(self.key_status, [(0, 4 * m)])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        if self.meta is not None:
            got = guards.block_of(self.meta).bytes()
            diff = np.flatnonzero(got != meta_want.view(np.uint8))
            assert not len(diff), (len(diff), [(int(b) // 352, int(b) % 352) for b in diff[:6]])
            guards.assert_untouched(self.meta, [(0, 352 * m)])
        self.inputs_unchanged()


def next_and_check(codec, rows, valid, reqs, status, op, phases=(0, 0, 0), order=None, tomb=None, with_meta=True):
    """One call under both fills against the host's answer, which it returns."""
    want = expected(rows, valid, reqs, status, op, order=order, tomb=tomb)
    meta = noise_meta(len(reqs)) if with_meta else None
    meta_want = stamped(meta, want[0], reqs, op) if with_meta else None

    def body(fill):
        c = Call(codec, rows, valid, reqs, status, fill, phases, order, tomb, meta)
        assert c.run(op) == 0
        c.check(want, meta_want)

    guards.twice(body)
    return want


def flags_of(want):
    return want[0]["flags"]


# --------------------------------------------------------------------------
# 1. sizes of the batch
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def col1025():
    return Column(1025, 300, 20)


@pytest.mark.parametrize("size", ("1", "63", "64", "65", "S-1", "S", "S+1"))
def test_request_counts(codec, S, col1025, size):
    m = eval(size, {"S": S})
    col = col1025
    reqs, status = mixed_requests(col, m, 30 + m % 17)
    for j, op in enumerate(OPS):
        want = next_and_check(codec, col.rows(col.n), col.n, reqs, status, op, PHASES[j], col.order, col.tomb)
        if m >= 63:
            f = flags_of(want)
            assert (f & NEXT_ASSIGNED).any() and (f == NEXT_SKIPPED).any() and (f == NEXT_BAD_KEY).any()
            assert (f & (NEXT_EXISTS if op == NEXT_CREATE else NEXT_HAS_PARENT)).any()


def test_two_tiles_and_77_requests(S):
    """m = 2 S + 77 on a context that covers exactly that many records, and one more is refused."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m = 2 * S + 77
    big = hobj.Codec(0, m)
    try:
        col = Column(1025, 300, 21)
        reqs, status = mixed_requests(col, m + 1, 33)
        for j, op in enumerate((NEXT_UPDATE, NEXT_MERGE)):
            want = next_and_check(big, col.rows(col.n), col.n, reqs[:m], status[:m], op, PHASES[j + 1], col.order, col.tomb)
            assert (want[0]["vid"][(flags_of(want) & NEXT_ASSIGNED) != 0] > 0).all()

        def body(fill):
            c = Call(big, col.rows(col.n), col.n, reqs, status, fill, meta=noise_meta(m + 1))
            assert c.run(NEXT_MERGE) == E_WORKSPACE
            c.nothing_stored()

        guards.twice(body)
    finally:
        big.close()


def test_no_requests_nothing_stored(codec, col1025):
    col = col1025
    reqs, status = mixed_requests(col, 0, 1)

    def body(fill):
        c = Call(codec, col.rows(col.n), col.n, reqs, status, fill, order=col.order, tomb=col.tomb, meta=noise_meta(0))
        assert c.work_bytes == 0
        assert c.run(NEXT_UPDATE) == 0 and c.run(NEXT_UPDATE, work=0, requests=0, out=0, keys_out=0, key_status=0) == 0
        c.nothing_stored()

    guards.twice(body)


# --------------------------------------------------------------------------
# 2. sizes of the column and its valid count
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 1023, 1024, 1025, 4096))
def test_column_rows_and_valid_counts(codec, n):
    col = Column(n, max(1, n // 4), 40 + n)
    reqs, status = mixed_requests(col, 150, 41 + n)
    valids = sorted({v for v in (0, 1, n - 5, n, n + 5, 1 << 40) if v >= 0})
    for j, valid in enumerate(valids):
        op = OPS[(j + n) % 4]
        want = next_and_check(codec, col.rows(valid), valid, reqs, status, op, PHASES[j % 4], col.order, col.tomb)
        if min(valid, n) == 0:
            assert not (flags_of(want) & NEXT_FOUND).any()


# --------------------------------------------------------------------------
# 3. ops with and without the order and the info
# --------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_ops_with_and_without_order_and_info(codec, col1025, op):
    col = col1025
    reqs, status = mixed_requests(col, 333, 50)
    rows = col.rows(col.n - 5)
    plain = next_and_check(codec, rows, col.n - 5, reqs, status, op, PHASES[1])
    no_status = next_and_check(codec, rows, col.n - 5, reqs, None, op, PHASES[2], with_meta=False)
    ordered = next_and_check(codec, rows, col.n - 5, reqs, status, op, PHASES[2], col.order)
    informed = next_and_check(codec, rows, col.n - 5, reqs, status, op, PHASES[3], col.order, col.tomb)
    assert not (flags_of(no_status) & NEXT_SKIPPED).any()
    assert (plain[0]["parent_record"] == SEEK_NONE).all()
    assert np.array_equal(flags_of(plain), flags_of(ordered))  # without the info a stored object is live
    if op != NEXT_CREATE:
        assert (ordered[0]["parent_record"] != SEEK_NONE).any()
    found = (flags_of(informed) & NEXT_FOUND) != 0
    dead = found & ((flags_of(informed) & NEXT_LIVE) == 0)
    assert dead.any() and (found & ~dead).any()
    if op in (NEXT_UPDATE, NEXT_DELETE):  # a deleted object is not found; Merge writes to it all the same
        assert ((flags_of(informed)[dead] & NEXT_NOT_FOUND) != 0).all()
    if op == NEXT_MERGE:
        assert ((flags_of(informed) & NEXT_ASSIGNED) != 0)[(flags_of(informed) & (NEXT_SKIPPED | NEXT_BAD_KEY)) == 0].all()


def test_order_values_at_or_above_n(codec, col1025):
    """An order that is no order: values at and above n read info row n - 1, and nothing faults."""
    col = col1025
    rng = np.random.default_rng(60)
    order = rng.integers(0, 1 << 32, col.n, dtype=np.uint64).astype(np.uint32)
    order[::3] = col.n + np.arange(len(order[::3]))
    order[1::9] = 0xFFFFFFFF
    assert (order >= col.n).all()
    reqs, status = mixed_requests(col, 400, 61)
    for last, op in ((0, NEXT_UPDATE), (0, NEXT_DELETE), (1, NEXT_UPDATE)):
        tomb = col.tomb.copy()
        tomb[-1] = last  # the row every such index reads
        want = next_and_check(codec, col.rows(col.n), col.n, reqs, status, op, PHASES[1], order, tomb)
        f = flags_of(want)
        found = (f & NEXT_FOUND) != 0
        assert found.any() and (((f & NEXT_LIVE) != 0) == (found & (last == 0))).all()
        if last == 0:
            assert (want[0]["parent_record"][(f & NEXT_ASSIGNED) != 0] >= col.n).all()


# --------------------------------------------------------------------------
# 4. runs: the ranks
# --------------------------------------------------------------------------
def run_requests(col, runs, seed, interleave):
    """Requests in which object j of `runs` (an object ID, a run length) is
    asked for that many times, the runs one after the other or, with
    `interleave`, shuffled among each other and among single requests."""
    rng = np.random.default_rng(seed)
    oids = [np.tile(np.asarray(o, np.uint8), (k, 1)) for o, k in runs]
    singles = col.oids[rng.integers(0, len(col.oids), 50)]
    oids = np.concatenate(oids + [singles])
    if interleave:
        oids = oids[rng.permutation(len(oids))]
    return request_rows(oids, seed)


@pytest.mark.parametrize("interleave", (False, True))
def test_runs_cross_a_wave_a_workgroup_and_a_sort_tile(codec, S, col1025, interleave):
    col = col1025
    absent = np.full(16, 0x55, np.uint8)
    absent[0] = 0x05
    runs = [(col.oids[3], 2), (col.oids[7], 64), (absent, 65), (col.oids[0], S + 1), (np.zeros(16), 3),
            (np.full(16, 0xFF), 3)]
    reqs = run_requests(col, runs, 70, interleave)
    status = np.zeros(len(reqs), np.int32)
    status[10::13] = 7  # skipped rows inside the runs: they shift no rank
    reqs[11::17, 0] = 9
    assert len(reqs) <= MAX_RECORDS
    for j, op in enumerate(OPS):
        want = next_and_check(codec, col.rows(col.n), col.n, reqs, status, op, PHASES[j], col.order)
        out, f = want[0], flags_of(want)
        counted = (f & (NEXT_SKIPPED | NEXT_BAD_KEY)) == 0
        long_run = counted & (reqs[:, 1:17] == col.oids[0]).all(axis=1)
        assert long_run.sum() > S - 400
        if op in (NEXT_UPDATE, NEXT_MERGE):  # the run's VIDs count up by one from the stored latest, in request order
            vids = out["vid"][long_run]
            assert (np.diff(vids.astype(np.int64)) == 1).all()
            assert (out["parent_vid"][long_run][1:] == vids[:-1]).all() and (out["parent_pid"][long_run][1:] == PID).all()
        else:  # one Create / Delete per object at the most
            assert (f[long_run] & NEXT_ASSIGNED != 0).sum() == (op == NEXT_DELETE)


def test_every_request_the_same_object(codec, S, col1025):
    col = col1025
    m = S + 65
    for oid, op in ((col.oids[5], NEXT_UPDATE), (np.full(16, 0xFF), NEXT_MERGE), (np.zeros(16), NEXT_CREATE),
                    (col.oids[5], NEXT_DELETE)):
        reqs = request_rows(np.tile(np.asarray(oid, np.uint8), (m, 1)), 80)
        want = next_and_check(codec, col.rows(col.n), col.n, reqs, None, op, PHASES[3], col.order)
        n_assigned = int(((flags_of(want) & NEXT_ASSIGNED) != 0).sum())
        assert n_assigned == (m if op in (NEXT_UPDATE, NEXT_MERGE) else 1)


def test_skipped_and_bad_rows_shift_no_rank(codec, col1025):
    """The same counted requests with and without spoiled rows between them get the same versions."""
    col = col1025
    clean = run_requests(col, [(col.oids[2], 40), (col.oids[9], 70)], 90, True)
    m = len(clean)
    reqs = np.repeat(clean, 2, axis=0)  # every request, then a spoiled copy of it
    status = np.zeros(2 * m, np.int32)
    status[1::4] = 4
    reqs[3::4, 0] = 0
    a = next_and_check(codec, col.rows(col.n), col.n, clean, np.zeros(m, np.int32), NEXT_UPDATE, PHASES[1], col.order)
    b = next_and_check(codec, col.rows(col.n), col.n, reqs, status, NEXT_UPDATE, PHASES[2], col.order)
    assert np.array_equal(b[0][0::2], a[0]) and np.array_equal(b[1][0::2], a[1])
    assert (b[0]["flags"][1::4] == NEXT_SKIPPED).all() and (b[0]["flags"][3::4] == NEXT_BAD_KEY).all()


# --------------------------------------------------------------------------
# 5. the VID wraps
# --------------------------------------------------------------------------
@pytest.mark.parametrize("stored", (M64, M64 - 1))
def test_vid_wraps(codec, stored):
    oid = np.full(16, 0xEE, np.uint8)
    keys = sorted([hkeys.new(bytes(oid), Scalar(2, 5)), hkeys.new(bytes(oid), Scalar(2, stored)),
                   hkeys.new(bytes(16), Scalar(1, 1))])
    rows = np.frombuffer(b"".join(keys), np.uint8).reshape(3, 29)
    reqs = request_rows(np.tile(oid, (3, 1)), 95)
    for op in (NEXT_UPDATE, NEXT_MERGE):
        want = next_and_check(codec, rows, 3, reqs, None, op, PHASES[1], np.array([7, 8, 9], np.uint32))
        vids = [(stored + 1 + r) & M64 for r in range(3)]
        assert want[0]["vid"].tolist() == vids
        assert want[0]["parent_vid"].tolist() == [stored] + vids[:2] and want[0]["parent_pid"].tolist() == [2, PID, PID]
        assert want[0]["parent_record"].tolist() == [9, SEEK_NONE, SEEK_NONE]
        assert ((flags_of(want) & NEXT_WRAPPED) != 0).tolist() == [stored + 1 + r > M64 for r in range(3)]


# --------------------------------------------------------------------------
# 6. refusals
# --------------------------------------------------------------------------
def test_refusals_store_nothing(codec, col1025):
    col = col1025
    reqs, status = mixed_requests(col, 200, 100)
    rows = col.rows(col.n)
    want = expected(rows, col.n, reqs, status, NEXT_MERGE, order=col.order, tomb=col.tomb)
    meta = noise_meta(len(reqs))

    def body(fill):
        c = Call(codec, rows, col.n, reqs, status, fill, (1, 3, 3), col.order, col.tomb, meta)
        a = c.args(NEXT_MERGE)
        for kw in (dict(m=MAX_RECORDS + 1), dict(m=1 << 32), dict(n=1 << 32), dict(m=(1 << 64) - 1),
                   dict(n=(1 << 64) - 1)):
            assert c.run(NEXT_MERGE, **kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(sorted=0), dict(valid=0), dict(requests=0), dict(out=0), dict(keys_out=0),
                   dict(key_status=0), dict(op=4), dict(op=1 << 31), dict(order=0),
                   dict(work_bytes=c.work_bytes - 1), dict(work_bytes=0), dict(work=0), dict(work=a["work"] + 128),
                   dict(keys_out=a["requests"]),
                   dict(order=a["order"] + 2), dict(req_status=a["req_status"] + 2),
                   dict(key_status=a["key_status"] + 2), dict(out=a["out"] + 4), dict(valid=a["valid"] + 4),
                   dict(info=a["info"] + 4), dict(meta=a["meta"] + 4)):
            kw.setdefault("op", NEXT_MERGE)
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run(NEXT_MERGE) == 0  # and the arguments were good
        c.check(want, stamped(meta, want[0], reqs, NEXT_MERGE))

    guards.twice(body)


# --------------------------------------------------------------------------
# 7. graph
# --------------------------------------------------------------------------
def test_graph_replays_after_the_inputs_changed(codec, S, col1025):
    """Replays after d_valid and the requests were changed on the device."""
    col = col1025
    m = S + 130
    reqs, status = mixed_requests(col, m, 110)
    reqs2, _ = mixed_requests(col, m, 111)
    rows = col.rows(col.n)
    dev = codec.torch_device
    rounds = [(reqs, col.n), (reqs2, col.n // 2)]

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        meta = noise_meta(m)
        c = Call(codec, rows, col.n, reqs, status, fill, (3, 1, 1), col.order, col.tomb, meta)
        assert c.run(NEXT_UPDATE) == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run(NEXT_UPDATE) == 0
        found = []
        for r, valid in rounds:
            for t in c.outs:
                refill(t, fill)
            c.meta.copy_(torch.from_numpy(meta.view(np.uint8).copy()).to(dev))
            c.dev["requests"].copy_(torch.from_numpy(r.reshape(-1).copy()).to(dev))
            c.dev["valid"].copy_(torch.from_numpy(u64(valid).view(np.uint8)).to(dev))
            c.host["requests"], c.host["valid"] = r, u64(valid)
            g.replay()
            # (the rows past the new valid count are still the column's: no call may read them as rows)
            want = expected(rows, valid, r, status, NEXT_UPDATE, order=col.order, tomb=col.tomb)
            c.check(want, stamped(meta, want[0], r, NEXT_UPDATE))
            found.append(int(((flags_of(want) & NEXT_FOUND) != 0).sum()))
        assert 0 < found[1] < found[0]

    guards.twice(body)


# --------------------------------------------------------------------------
# 8. the chain: next -> encode -> decode -> keys; next -> sort -> merge -> seek, nothing read on the host
# --------------------------------------------------------------------------
def chain_column(n, objects=23):
    """Generator Small records of `objects` objects, every fifth a tombstone
    with no data, which is what Object.Tombstone() asks (object.go:103-112)."""
    rng = np.random.default_rng(120)
    oids = rng.integers(0, 256, (objects, 16), dtype=np.uint8)
    hb = gen_host_batch(121, "small", 0, n)
    which = rng.integers(0, objects - 3, n)  # the last three objects are not stored
    hb.meta["object_id"] = oids[which]
    hb.meta["vid"] = rng.permutation(n) + 1
    hb.meta["pid"] = rng.integers(1, 4, n)
    dead = np.arange(n) % 5 == 3
    hb.meta["tombstone"] = dead & ((hb.meta["present"] & HAS_VERSION) != 0)
    lens = np.diff(hb.payload_off.astype(np.int64))
    payload = hb.payload[:int(hb.payload_off[n])][np.repeat(~dead, lens)]
    lens[dead] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return type(hb)(hb.meta, hb.var, hb.acl, hb.regions, payload, off), oids


@pytest.mark.parametrize("op", (NEXT_UPDATE, NEXT_DELETE))
def test_next_encode_decode_sort_merge_seek_chain(codec, op):
    n, m = 200, 60
    hb, oids = chain_column(n)
    dev = codec.torch_device
    enc = codec.marshal(hobj.DeviceBatch.from_host(hb, dev))
    rec_bytes = int(enc.out_off.view(torch.int64)[n].item())
    d1 = codec.decode(enc.out, enc.out_off, n, rec_bytes=rec_bytes)
    dk, dst = codec.keys(d1)
    order, col, valid = codec.sort_keys(dk[:29 * n], dst[:4 * n], n=n, want_sorted=True)
    # the batch of writes: rows of another seed, a Delete's without payload; requests with repeats and absent objects
    rng = np.random.default_rng(122)
    reqs = request_rows(oids[rng.integers(0, len(oids), m)], 123)
    hb2 = gen_host_batch(124, "small", 0, m)
    if op == NEXT_DELETE:
        hb2 = type(hb2)(hb2.meta, hb2.var, hb2.acl, hb2.regions, np.zeros(1, np.uint8), np.zeros(m + 1, np.uint64))
    b2 = hobj.DeviceBatch.from_host(hb2, dev)
    d_reqs = hobj._dev_bytes(reqs, dev)
    cap = 1 << 20  # of the new records' arena: known without asking the device
    out_off, status, arena = codec._empty(8 * (m + 1)), codec._empty(4 * m), codec._empty(cap)
    # nothing is read on the host from here ...
    rows, keys_out, key_status = codec.next_versions(col[:29 * n], valid, d_reqs[:29 * m], op, PID, REGION, NOW,
                                                     order=order, info=d1.info, meta=b2.meta)
    codec.encode_sizes(b2, out_off, status)
    codec.scan(out_off, m, out_off)
    codec.marshal_into(b2, arena, cap, out_off, status)
    d2 = codec.decode(arena, out_off, m, rec_bytes=cap)
    k2, st2 = codec.keys(d2)
    order_b, sorted_b, valid_b = codec.sort_keys(keys_out, key_status.view(torch.uint8), n=m, want_sorted=True)
    merged, morder, mvalid = codec.merge_keys(col[:29 * n], order, valid, sorted_b[:29 * m], order_b, valid_b)
    seeks = codec.seek_keys(merged, mvalid, d_reqs[:29 * m], 17, order=morder)
    # ... to here
    torch.cuda.synchronize()
    sorted_keys = [bytes(r) for r in col[:29 * n].cpu().numpy().reshape(n, 29)]
    host_order = order.cpu().numpy().view(np.uint32)
    meta1, info1, _, _, _, _ = d1.host()
    assert int(valid.item()) == n
    want, want_keys, want_status = expected(np.frombuffer(b"".join(sorted_keys), np.uint8).reshape(n, 29), n, reqs,
                                            None, op, order=host_order, tomb=info1["tombstone"])
    got = rows.cpu().numpy().reshape(-1).view(NEXT_DTYPE)
    assert np.array_equal(got, want)
    assigned = (want["flags"] & NEXT_ASSIGNED) != 0
    refused = (want["flags"] & NEXT_NOT_FOUND) != 0
    assert assigned.sum() > 10 and (refused & ((want["flags"] & NEXT_FOUND) != 0)).any()  # deleted objects
    assert (refused & ((want["flags"] & NEXT_FOUND) == 0)).any()  # absent ones
    assert keys_out.cpu().numpy().tobytes() == want_keys.tobytes()
    assert (((want["flags"][assigned] & NEXT_TOMBSTONE) != 0) == (op == NEXT_DELETE)).all()
    assert np.array_equal(key_status.cpu().numpy(), want_status)
    # the encoded and decoded records carry the assigned version, and their keys are the call's
    meta2, info2, _, _, _, _ = d2.host()
    assert (info2["meta_status"][assigned] == OK).all() and (hobj._to_host(status, 4 * m, np.int32)[assigned] == OK).all()
    for f in ("vid", "pid", "parent_vid", "parent_pid"):
        assert np.array_equal(meta2[f][assigned], want[f][assigned]), f
    assert (meta2["region"][assigned] == REGION).all() and (meta2["version_created"][assigned] == NOW).all()
    assert np.array_equal(info2["tombstone"][assigned] != 0, np.full(assigned.sum(), op == NEXT_DELETE))
    got_k2 = k2.cpu().numpy()[:29 * m].reshape(m, 29)
    assert (hobj._to_host(st2, 4 * m, np.int32)[assigned] == OK).all()
    assert np.array_equal(got_k2[assigned], want_keys[assigned])
    # the parents: the scalar that was latest before, in the column for a rank 0, the request before for the others
    for i in np.flatnonzero(assigned):
        stored = (want["flags"][i] & NEXT_HAS_PARENT) and want["parent_record"][i] != SEEK_NONE
        if stored:
            r = int(want["parent_record"][i])
            mine = [j for j in range(n) if bytes(meta1["object_id"][j]) == bytes(reqs[i, 1:17])]
            top = max(mine, key=lambda j: (int(meta1["vid"][j]), int(meta1["pid"][j])))
            assert r == top and meta2["parent_vid"][i] == meta1["vid"][r] and meta2["parent_pid"][i] == meta1["pid"][r]
    # after the merge, Seek of every request's object ends on the object's newest record
    sk = seeks.cpu().numpy().reshape(-1).view(SEEK_DTYPE)
    assert int(mvalid.item()) == n + int(assigned.sum())
    last = {}
    for i in np.flatnonzero(assigned):
        last[bytes(reqs[i, :17])] = n + int(i)
    for i in np.flatnonzero(assigned):
        assert sk["latest"][i] == last[bytes(reqs[i, :17])], i
    if op == NEXT_UPDATE:
        assert len(last) < assigned.sum()  # some object was written more than once
