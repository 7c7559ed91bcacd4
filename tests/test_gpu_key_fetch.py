"""honu_key_fetch on the GPU against numpy.

The expectation is numpy's alone: per row the length from rec_off (0 for a
row past min(total, cap), a tombstone under HONU_FETCH_LIVE, an index not
below nrec or offsets out of order or out of the arena), their cumsum, and the
concatenation of the records' bytes. It never calls the library. Every input
and output is a guarded view (tests/guards.py) under both fills, d_rec and
d_values at byte phases 0, 1 and 3; the write set is exactly
d_val_off[0, cap + 1), d_val_total[0], d_status[0, w) and the bytes of the
rows with d_val_off[g + 1] <= val_cap in d_values, and the inputs are
unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (ACL_INPLACE, FETCH_LIVE, HAS_VERSION, LIST_ROW_DTYPE, LIST_ROW_HEAD,  # noqa: E402
                               LIST_ROW_TOMBSTONE, SEEK_NONE)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
OK, INPUT = hobj.OK, hobj.INPUT
REGIONS_INPLACE = 1 << 9
PHASES = ((0, 0), (1, 3), (3, 1))  # (d_rec, d_values)
MAX_RECORDS = 4096


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, MAX_RECORDS)
    yield c
    c.close()


# --------------------------------------------------------------------------
# expectations
# --------------------------------------------------------------------------
def arena(lengths, seed):
    """(bytes, offsets uint64[n + 1]): records of the given lengths, arbitrary bytes, packed tight."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint64)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


def list_rows(records, flags=None):
    """honu_list_row rows naming the given records; range and pos hold values no test expects read."""
    rows = np.zeros(len(records), LIST_ROW_DTYPE)
    rows["range"], rows["pos"] = 0xDEADBEEF, 0xFEEDF00D
    rows["record"] = np.asarray(records, np.uint64).astype(np.uint32)
    rows["flags"] = LIST_ROW_HEAD if flags is None else flags
    return rows


def expected_fetch(rows, total, cap, rec, rec_off, nrec, rec_bytes, flags=0):
    """(values of every row concatenated, val_off uint64[cap + 1], status int32[w])."""
    w = min(int(total), cap)
    r = rows["record"][:w].astype(np.int64)
    left_out = (rows["flags"][:w] & LIST_ROW_TOMBSTONE) != 0 if flags & FETCH_LIVE else np.zeros(w, bool)
    inside = r < nrec
    rc = np.where(inside, r, 0)
    a, b = rec_off[rc], rec_off[rc + 1]
    good = inside & (a <= b) & (b <= np.uint64(rec_bytes)) & ~left_out
    lens = np.zeros(cap, np.int64)
    lens[:w] = np.where(good, b.astype(np.int64) - a.astype(np.int64), 0)
    val_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    status = np.where(good | left_out, OK, INPUT).astype(np.int32)
    parts = [rec[int(x):int(y)] for x, y, g in zip(a, b, good) if g]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), val_off, status


def copied_bytes(val_off, val_cap):
    """The prefix of the values that fits: the greatest offset at or below val_cap."""
    return int(val_off[val_off <= np.uint64(val_cap)].max())


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


def u64(x):
    return np.array([x], np.uint64)


class Call:
    """The guarded device arguments of one fetch."""

    def __init__(self, codec, rows, total, cap, rec, rec_off, val_cap, fill, phases=(0, 0), rec_bytes=None):
        self.codec, self.cap, self.val_cap = codec, int(cap), int(val_cap)
        self.nrec = len(rec_off) - 1
        self.rec_bytes = len(rec) if rec_bytes is None else rec_bytes
        assert len(rows) == self.cap
        self.host = {"rows": rows, "total": u64(total), "rec": rec, "rec_off": rec_off}
        self.dev = {k: put(codec, a, phases[0] if k == "rec" else 0, fill) for k, a in self.host.items()}
        dev = codec.torch_device
        self.val_off = guards.guarded(8 * (self.cap + 1), fill=fill, device=dev)
        self.status = guards.guarded(4 * self.cap, fill=fill, device=dev)
        self.values = guards.guarded(self.val_cap, phase=phases[1], fill=fill, device=dev)
        self.val_total = guards.guarded(8, fill=fill, device=dev)
        self.outs = (self.val_off, self.status, self.values, self.val_total)

    def args(self, flags=0, **kw):
        A = guards.address
        d = self.dev
        x = dict(ctx=self.codec.ctx, rows=A(d["rows"]), total=A(d["total"]), cap=self.cap, rec=A(d["rec"]),
                 rec_off=A(d["rec_off"]), nrec=self.nrec, rec_bytes=self.rec_bytes, flags=flags,
                 val_off=A(self.val_off), status=A(self.status), values=A(self.values), val_cap=self.val_cap,
                 val_total=A(self.val_total))
        x.update(kw)
        return x

    def run(self, flags=0, **kw):
        x = self.args(flags, **kw)
        return self.codec.lib.honu_key_fetch(
            x["ctx"], x["rows"], x["total"], x["cap"], x["rec"], x["rec_off"], x["nrec"], x["rec_bytes"], x["flags"],
            x["val_off"], x["status"], x["values"], x["val_cap"], x["val_total"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs:
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def check(self, want, with_status=True, with_values=True):
        """The outputs against (values, val_off, status) and the write set."""
        torch.cuda.synchronize()
        values, val_off, status = want
        w = len(status)
        got_total = int(guards.block_of(self.val_total).bytes().view(np.uint64)[0])
        assert got_total == int(val_off[-1]) == len(values), (got_total, int(val_off[-1]), len(values))
        got = guards.block_of(self.val_off).bytes().view(np.uint64)
        bad = np.flatnonzero(got != val_off)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], val_off[bad[:4]])
        if with_status:
            got = guards.block_of(self.status).bytes()[:4 * w].view(np.int32)
            bad = np.flatnonzero(got != status)
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], status[bad[:4]])
        fit = copied_bytes(val_off, self.val_cap) if with_values else 0
        if with_values:
            got = guards.block_of(self.values).bytes()[:fit]
            bad = np.flatnonzero(got != values[:fit])
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], values[bad[:4]])
        guards.assert_untouched(self.val_off, [(0, 8 * (self.cap + 1))])
        guards.assert_untouched(self.val_total, [(0, 8)])
        guards.assert_untouched(self.status, [(0, 4 * w)] if with_status else [])
        guards.assert_untouched(self.values, [(0, fit)])
        self.inputs_unchanged()
        return fit


def fetch_and_check(codec, rows, total, rec, rec_off, cap=None, val_cap=None, flags=0, phases=(0, 0), rec_bytes=None,
                    repeat=1, **how):
    """One call (or `repeat` calls) under both fills against numpy; cap None:
    the rows given; val_cap None: the need + 5."""
    cap = len(rows) if cap is None else cap
    rows = rows[:cap] if len(rows) >= cap else np.concatenate([rows, np.zeros(cap - len(rows), LIST_ROW_DTYPE)])
    want = expected_fetch(rows, total, cap, rec, rec_off, len(rec_off) - 1,
                          len(rec) if rec_bytes is None else rec_bytes, flags)
    room = len(want[0]) + 5 if val_cap is None else val_cap

    def body(fill):
        for _ in range(repeat):
            c = Call(codec, rows, total, cap, rec, rec_off, room, fill, phases, rec_bytes)
            assert c.run(flags, **how) == 0
            c.check(want, with_status=how.get("status", 1) != 0, with_values=how.get("values", 1) != 0)

    guards.twice(body)
    return want


# --------------------------------------------------------------------------
# 1. lengths and phases
# --------------------------------------------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 31, 63, 64, 65, 255, 4097)


@pytest.fixture(scope="module")
def records():
    """40 records of arbitrary bytes with lengths from LENGTHS, packed tight:
    sixteen lengths of 1 mod 16 first, so the records start at every phase."""
    up = [x for x in LENGTHS if x % 16 == 1]
    rest = [x for x in LENGTHS if x % 16 != 1]
    lengths = [up[i % len(up)] for i in range(16)] + [rest[i % len(rest)] for i in range(24)]
    rec, off = arena(lengths, 2)
    assert set(lengths) == set(LENGTHS) and len({int(o) % 16 for o in off[:-1]}) == 16
    return rec, off


def mixed_rows(nrec, seed):
    """A permutation of the records, some repeated, one named three times,
    and indices that name no record."""
    rng = np.random.default_rng(seed)
    r = rng.permutation(nrec).tolist()
    thrice = r[5]
    r += r[3:9] + [thrice, thrice]
    for at, bad in ((4, nrec), (17, nrec + 5), (30, SEEK_NONE)):
        r.insert(at, bad)
    assert r.count(thrice) >= 3
    return list_rows(r)


@pytest.mark.parametrize("phases", PHASES)
def test_lengths_and_phases(codec, records, phases):
    rec, off = records
    rows = mixed_rows(40, 3)
    values, val_off, status = fetch_and_check(codec, rows, len(rows), rec, off, phases=phases)
    assert (status != OK).sum() == 3 and status[4] == status[17] == status[30] == INPUT
    assert len(values) > int(off[-1])  # the repeats: more bytes than the arena holds
    # without d_status the same bytes
    fetch_and_check(codec, rows, len(rows), rec, off, phases=phases, status=0)


# --------------------------------------------------------------------------
# 2. row count
# --------------------------------------------------------------------------
@pytest.mark.parametrize("total", ("below", "cap", "above", "zero"))
def test_row_count(codec, records, total):
    rec, off = records
    rows = mixed_rows(40, 4)  # rows past w would fetch if read: they name good records
    cap = len(rows)
    t = {"below": cap - 7, "cap": cap, "above": cap + 1000, "zero": 0}[total]
    for ph in PHASES:
        values, val_off, status = fetch_and_check(codec, rows, t, rec, off, phases=ph)
        w = min(t, cap)
        assert len(status) == w and (val_off[w:] == val_off[-1]).all() and len(val_off) == cap + 1
    if total == "above":
        fetch_and_check(codec, rows, (1 << 64) - 1, rec, off)


def test_cap_zero_writes_two_zeros(codec, records):
    rec, off = records

    def body(fill):
        for kw in ({}, dict(rows=0), dict(rows=0, status=0, values=0)):
            c = Call(codec, list_rows([]), 5, 0, rec, off, 64 if kw.get("values", 1) else 0, fill, (1, 3))
            assert c.run(**kw) == 0
            torch.cuda.synchronize()
            assert guards.block_of(c.val_off).bytes().view(np.uint64).tolist() == [0]
            assert guards.block_of(c.val_total).bytes().view(np.uint64).tolist() == [0]
            guards.assert_untouched(c.val_off, [(0, 8)])
            guards.assert_untouched(c.val_total, [(0, 8)])
            guards.assert_untouched(c.status, [])
            guards.assert_untouched(c.values, [])
            c.inputs_unchanged()

    guards.twice(body)


# --------------------------------------------------------------------------
# 3. tombstones
# --------------------------------------------------------------------------
def test_tombstones(codec, records):
    rec, off = records
    rows = mixed_rows(40, 5)
    flagged = np.zeros(len(rows), bool)
    flagged[1::3] = True
    flagged[[4, 17]] = True  # two of the rows whose record is out of range; row 30 stays unflagged
    rows["flags"] = np.where(flagged, LIST_ROW_TOMBSTONE | LIST_ROW_HEAD, LIST_ROW_HEAD)
    rows["flags"][1::5] |= np.uint32(0xFFFFFF00)  # no other bit matters
    assert not flagged[30]
    for j, ph in enumerate(PHASES):
        plain = fetch_and_check(codec, rows, len(rows), rec, off, flags=0, phases=ph)
        live = fetch_and_check(codec, rows, len(rows), rec, off, flags=FETCH_LIVE, phases=PHASES[(j + 1) % 3])
        # without the flag a tombstone row fetches like any other
        assert (plain[2][[4, 17, 30]] == INPUT).all() and (np.diff(plain[1].astype(np.int64))[flagged] > 0).any()
        # with it: length 0 and OK, also where the record is out of range
        assert (np.diff(live[1].astype(np.int64))[flagged] == 0).all() and (live[2][flagged] == OK).all()
        assert live[2][30] == INPUT and len(live[0]) < len(plain[0])


# --------------------------------------------------------------------------
# 4. byte capacity
# --------------------------------------------------------------------------
@pytest.mark.parametrize("room", ("total", "interior", "interior-1", "zero"))
def test_byte_capacity(codec, records, room):
    rec, off = records
    rows = mixed_rows(40, 6)
    _, val_off, _ = expected_fetch(rows, len(rows), len(rows), rec, off, 40, len(rec))
    k = next(g for g in range(15, len(rows)) if val_off[g] > val_off[g - 1])  # row k - 1 has bytes
    assert 0 < val_off[k] < val_off[-1]
    val_cap = {"total": int(val_off[-1]), "interior": int(val_off[k]), "interior-1": int(val_off[k]) - 1,
               "zero": 0}[room]
    fit = {"total": int(val_off[-1]), "interior": int(val_off[k]), "interior-1": int(val_off[k - 1]), "zero": 0}[room]
    assert copied_bytes(val_off, val_cap) == fit
    for ph in PHASES:
        how = dict(values=0) if room == "zero" else {}  # d_values NULL: a sizing call
        want = fetch_and_check(codec, rows, len(rows), rec, off, val_cap=val_cap, phases=ph, **how)
        assert int(want[1][-1]) == int(val_off[-1])  # the full need every time


# --------------------------------------------------------------------------
# 5. untrusted offsets
# --------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ("descending", "above", "last_above"))
def test_untrusted_offsets(codec, records, damage):
    rec, off = records
    bad = off.copy()
    n = 40
    if damage == "descending":
        assert bad[10] > 0
        bad[11] = bad[10] - np.uint64(1)  # record 10 descends (record 11 then starts a byte early, in order)
        hit = {10}
    elif damage == "above":
        bad[20] = np.uint64(len(rec) + 1)  # record 19 ends past the arena, record 20 starts there
        hit = {19, 20}
    else:
        bad[n] = np.uint64(len(rec) + 7)
        hit = {n - 1}
    rows = list_rows(list(range(n)) + [10, 19, 20, n - 1, 3])
    for ph in PHASES:
        values, val_off, status = fetch_and_check(codec, rows, len(rows), rec, bad, phases=ph)
        lens = np.diff(val_off.astype(np.int64))
        for g, r in enumerate(rows["record"].astype(np.int64)):
            if int(r) in hit:
                assert status[g] == INPUT and lens[g] == 0, (g, r)
            elif bad[r] == off[r] and bad[r + 1] == off[r + 1]:  # every record the damage does not touch
                assert status[g] == OK and lens[g] == int(off[r + 1]) - int(off[r]), (g, r)
    # offsets up to the very top of 64 bits, and a rec_bytes below the arena's size
    wild = off.copy()
    wild[5], wild[6] = np.uint64((1 << 64) - 1), np.uint64(1 << 63)
    fetch_and_check(codec, rows, len(rows), rec, wild, phases=PHASES[1])
    fetch_and_check(codec, rows, len(rows), rec, off, phases=PHASES[2], rec_bytes=int(off[25]))


# --------------------------------------------------------------------------
# 6. the copy's classes
# --------------------------------------------------------------------------
def test_long_rows_with_a_short_one(codec):
    """(a) mean >= 64 KB: the few-waves form, the 5-byte row its short class."""
    rec, off = arena([5, 70000, 3, 200000], 60)
    for ph in PHASES:
        values, val_off, _ = fetch_and_check(codec, list_rows([1, 3, 0]), 3, rec, off, phases=ph)
        assert int(val_off[-1]) // 3 >= 64 << 10


def test_rows_of_20000_bytes_twice(codec):
    """(b) mean in [16 KB, 64 KB): the range tails from the ticket line; (c)
    twice on the same context: the line came back to zero."""
    rec, off = arena([20000] * 3, 61)
    for ph in PHASES:
        values, val_off, _ = fetch_and_check(codec, list_rows([2, 0, 1, 0]), 4, rec, off, phases=ph, repeat=2)
        assert 16 << 10 <= int(val_off[-1]) // 4 < 64 << 10


def test_3000_short_rows(codec):
    """(d) 3000 rows of 1 to 40 bytes, the short form."""
    rng = np.random.default_rng(62)
    rec, off = arena(rng.integers(1, 41, 700), 63)
    rows = list_rows(rng.integers(0, 700, 3000))
    for ph in PHASES:
        fetch_and_check(codec, rows, 3000, rec, off, phases=ph)


# --------------------------------------------------------------------------
# 7. scan bound, 8. refusals
# --------------------------------------------------------------------------
def test_cap_beyond_the_contexts_scan_is_refused(records):
    """The cap + 1 lengths go through the context's scan, whose state covers
    max_records rows: a context of R records takes cap = R - 1 and refuses R."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    R = 8
    small = hobj.Codec(0, R)
    try:
        rec, off = records
        rows = mixed_rows(40, 7)
        assert int(small.lib.honu_ctx_max_records(small.ctx)) == R
        fetch_and_check(small, rows[:R - 1], R - 1, rec, off, phases=PHASES[1])

        def body(fill):
            c = Call(small, rows[:R], R, R, rec, off, 1 << 16, fill)
            assert c.run() == E_WORKSPACE
            c.nothing_stored()

        guards.twice(body)
    finally:
        small.close()


def test_refusals_store_nothing(codec, records):
    rec, off = records
    rows = mixed_rows(40, 8)
    want = expected_fetch(rows, len(rows), len(rows), rec, off, 40, len(rec), FETCH_LIVE)

    def body(fill):
        c = Call(codec, rows, len(rows), len(rows), rec, off, len(want[0]) + 9, fill, (1, 3))
        a = c.args()
        for kw in (dict(cap=1 << 32), dict(nrec=1 << 32), dict(cap=(1 << 64) - 1), dict(nrec=(1 << 64) - 1),
                   dict(cap=MAX_RECORDS), dict(cap=MAX_RECORDS, val_cap=0, values=0)):
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(total=0), dict(val_off=0), dict(val_total=0), dict(rows=0), dict(rec_off=0),
                   dict(rec=0), dict(values=0), dict(flags=2), dict(flags=3), dict(flags=1 << 31),
                   dict(status=a["status"] + 2), dict(total=a["total"] + 4), dict(rec_off=a["rec_off"] + 4),
                   dict(val_off=a["val_off"] + 4), dict(val_total=a["val_total"] + 4), dict(rows=a["rows"] + 8),
                   dict(rows=a["rows"] + 4)):
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run(FETCH_LIVE) == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)


# --------------------------------------------------------------------------
# 9. graph
# --------------------------------------------------------------------------
def test_graph_replays_after_the_rows_changed(codec, records):
    rec, off = records
    rows = mixed_rows(40, 9)
    cap = len(rows)
    rows2 = rows.copy()
    rows2["record"][2], rows2["record"][11] = rows["record"][20], 40  # another record, and one out of range
    rounds = [(rows, cap), (rows2, cap - 9)]
    dev = codec.torch_device

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        c = Call(codec, rows, cap, cap, rec, off, 2 * len(rec), fill, (3, 1))
        assert c.run() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run() == 0
        needs = []
        for r, total in rounds:
            for t in c.outs:
                refill(t, fill)
            c.dev["rows"].copy_(torch.from_numpy(r.view(np.uint8).copy()).to(dev))
            c.dev["total"].copy_(torch.from_numpy(u64(total).view(np.uint8)).to(dev))
            c.host["rows"], c.host["total"] = r, u64(total)
            g.replay()
            want = expected_fetch(r, total, cap, rec, off, 40, len(rec))
            c.check(want)
            needs.append(len(want[0]))
        assert len(set(needs)) == 2 and min(needs) > 0

    guards.twice(body)


# --------------------------------------------------------------------------
# 10. the chain: seek -> list -> fetch -> decode with nothing read on the host
# --------------------------------------------------------------------------
SPANS = ("schema_name", "mime", "ip_address", "user_agent", "public_key_id", "encryption_key", "hmac_secret",
         "signature")


def uvarints(buf, at, count):
    """The bytes of `count` uvarints from buf[at]."""
    end = at
    for _ in range(count):
        while buf[end] & 0x80:
            end += 1
        end += 1
    return buf[at:end].tobytes()


def resolved(meta, info, arena_bytes, acl, reg):
    """A decoded row (meta and info as arrays of one) with everything it
    points at looked up: comparable between arenas."""
    m = meta.copy()
    out = []
    for s in SPANS:
        o, ln = int(m[s]["off"][0]), int(m[s]["len"][0])
        out.append(arena_bytes[o:o + ln].tobytes())
        m[s]["off"] = 0
    ao, ac, ro, rc = (int(m[f][0]) for f in ("acl_off", "acl_count", "regions_off", "regions_count"))
    present = int(m["present"][0])
    out.append(arena_bytes[ao:ao + 18 * ac].tobytes() if present & ACL_INPLACE else acl[ao:ao + ac].tobytes())
    out.append(uvarints(arena_bytes, ro, rc) if present & REGIONS_INPLACE else reg[ro:ro + rc].tobytes())
    m["acl_off"] = 0
    m["regions_off"] = 0
    i = info.copy()
    if int(i["data_status"][0]) == OK:
        o, ln = int(i["data_off"][0]), int(i["data_len"][0])
        out.append(arena_bytes[o:o + ln].tobytes())
    i["data_off"] = 0
    return m.tobytes(), i.tobytes(), out


def chain_batch(n):
    """(host batch, tombstones, one record index per object): generator
    records of 19 objects; every seventh record has no data, which is what
    Object.Tombstone() asks (object.go:103-112)."""
    rng = np.random.default_rng(100)
    oids = rng.integers(0, 256, (19, 16), dtype=np.uint8)
    hb = gen_host_batch(101, "small", 0, n)
    which = rng.integers(0, 19, n)
    hb.meta["object_id"] = oids[which]
    hb.meta["vid"] = rng.integers(1, 40, n)
    hb.meta["pid"] = rng.integers(1, 4, n)
    dead = np.arange(n) % 7 == 3
    hb.meta["tombstone"] = dead & ((hb.meta["present"] & HAS_VERSION) != 0)
    lens = np.diff(hb.payload_off.astype(np.int64))
    payload = hb.payload[:int(hb.payload_off[n])][np.repeat(~dead, lens)]
    lens[dead] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    hb = type(hb)(hb.meta, hb.var, hb.acl, hb.regions, payload, off)
    first = [int(np.flatnonzero(which == j)[0]) for j in range(19) if (which == j).any()]
    return hb, dead, first


def test_seek_list_fetch_decode_chain(codec):
    n = 200
    hb, dead, first = chain_batch(n)  # first: one probe per object
    enc = codec.marshal(hobj.DeviceBatch.from_host(hb, codec.torch_device))
    rec_bytes = int(enc.out_off.view(torch.int64)[n].item())
    d1 = codec.decode(enc.out, enc.out_off, n, rec_bytes=rec_bytes)
    dk, dst = codec.keys(d1)
    order, col, valid = codec.sort_keys(dk[:29 * n], dst[:4 * n], n=n, want_sorted=True)
    ipick = torch.tensor(first, device=codec.torch_device)
    probes = dk[:29 * n].view(n, 29)[ipick].reshape(-1).contiguous()
    pstatus = dst[:4 * n].view(torch.int32)[ipick].contiguous().view(torch.uint8)
    cap = n  # distinct objects: no row twice
    # nothing is read on the host from here ...
    seeks = codec.seek_keys(col[:29 * n], valid, probes, 17, probe_status=pstatus, order=order, info=d1.info)
    rows, _, total, _ = codec.list_keys(col[:29 * n], order, valid, seeks, cap, reverse=True, info=d1.info)
    values, val_off, val_total, status = codec.fetch_objects(rows, total, cap, enc.out, enc.out_off, n, rec_bytes,
                                                             rec_bytes)
    d2 = codec.decode(values, val_off, cap, rec_bytes=rec_bytes)
    # ... to here
    torch.cuda.synchronize()
    t = int(total.item())
    assert 150 < t <= cap and int(val_total.item()) <= rec_bytes
    got = rows.cpu().numpy().view(np.uint32)[:t]
    r = got[:, 2].astype(np.int64)
    assert (status.cpu().numpy()[:t] == OK).all() and len(set(r.tolist())) == t
    tomb = (got[:, 3] & LIST_ROW_TOMBSTONE) != 0
    assert (tomb == dead[r]).all() and 5 < tomb.sum() < t
    off1 = hobj._to_host(enc.out_off, 8 * (n + 1), np.uint64).astype(np.int64)
    off2 = val_off.cpu().numpy()
    assert np.array_equal(np.diff(off2)[:t], off1[r + 1] - off1[r]) and (off2[t:] == off2[t]).all()
    arena1 = hobj._to_host(enc.out, rec_bytes, np.uint8)
    arena2 = hobj._to_host(values, int(off2[t]), np.uint8)
    assert arena2.tobytes() == b"".join(arena1[off1[i]:off1[i + 1]].tobytes() for i in r)
    meta1, info1, acl1, reg1, _, _ = d1.host()
    meta2, info2, acl2, reg2, _, _ = d2.host()
    assert (info1["meta_status"] == OK).all()
    for g in range(t):
        a = resolved(meta1[r[g]:r[g] + 1], info1[r[g]:r[g] + 1], arena1, acl1, reg1)
        b = resolved(meta2[g:g + 1], info2[g:g + 1], arena2, acl2, reg2)
        assert a == b, g
    # and with live: the tombstones' values are empty, the rows in place
    _, live_off, _, live_status = codec.fetch_objects(rows, total, cap, enc.out, enc.out_off, n, rec_bytes, rec_bytes,
                                                      live=True)
    torch.cuda.synchronize()
    lens = np.diff(live_off.cpu().numpy())[:t]
    assert (lens[tomb] == 0).all() and np.array_equal(lens[~tomb], np.diff(off2)[:t][~tomb])
    assert (live_status.cpu().numpy()[:t] == OK).all()
