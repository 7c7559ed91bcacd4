"""honu_key_reclaim on the GPU against numpy.

The expectation is numpy's alone: the records that order[0, v) names, v =
min(valid, n), in ascending index; the remap and the renumbered order; per
kept record the length from rec_off (0 and INPUT for offsets out of order or
out of the arena), their cumsum, and the concatenation of the records' bytes.
It never calls the library. Every input and output is a guarded view
(tests/guards.py) under both fills, d_rec and d_values at byte phases (0, 0),
(1, 3) and (3, 1), d_keys and d_keys_out at phases 0 and 1; the write set is
exactly d_kept[0], d_val_total[0], d_order_out[0, n), d_remap[0, nrec),
d_source[0, kept), rows [0, kept) of the gathered arrays, d_status[0, kept),
d_rec_off_out[0, nrec + 1) and the bytes of the records with
d_rec_off_out[j + 1] <= val_cap, and the inputs are unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import INFO_DTYPE, LIST_ROW_TOMBSTONE, SEEK_NONE  # noqa: E402
from test_gpu_key_fetch import chain_batch, resolved  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
OK, INPUT = hobj.OK, hobj.INPUT
PHASES = ((0, 0), (1, 3), (3, 1))  # (d_rec, d_values)
KEY_PHASES = (0, 1)
MAX_RECORDS = 4096
TILE = 1024
NONE = np.uint32(SEEK_NONE)
LENGTHS = (0, 1, 15, 16, 17, 300)


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


def per_record(nrec, seed):
    """(keys uint8[nrec, 29], key_status int32[nrec], info INFO_DTYPE[nrec]) of arbitrary bytes."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (nrec, 29), dtype=np.uint8)
    kst = rng.integers(-3, 11, nrec).astype(np.int32)
    info = rng.integers(0, 256, 32 * nrec, dtype=np.uint8).view(INFO_DTYPE)
    return keys, kst, info


class Want:
    """numpy's reclaim."""

    def __init__(self, order, valid, rec, rec_off, rec_bytes=None):
        n, nrec = len(order), len(rec_off) - 1
        rec_bytes = len(rec) if rec_bytes is None else rec_bytes
        v = min(int(valid), n)
        o = np.asarray(order, np.uint32)[:v].astype(np.int64)
        inside = o < nrec
        mark = np.zeros(nrec, bool)
        mark[o[inside]] = True
        self.source = np.flatnonzero(mark).astype(np.uint32)
        self.kept = kept = len(self.source)
        self.remap = np.full(nrec, NONE, np.uint32)
        self.remap[self.source] = np.arange(kept, dtype=np.uint32)
        self.order = np.full(n, NONE, np.uint32)
        self.order[:v][inside] = self.remap[o[inside]]
        s = self.source.astype(np.int64)
        a, b = rec_off[s], rec_off[s + 1]
        good = (a <= b) & (b <= np.uint64(rec_bytes))
        lens = np.where(good, b.astype(np.int64) - a.astype(np.int64), 0)
        self.status = np.where(good, OK, INPUT).astype(np.int32)
        self.rec_off = np.zeros(nrec + 1, np.uint64)
        self.rec_off[1:kept + 1] = np.cumsum(lens)
        self.rec_off[kept + 1:] = self.rec_off[kept]
        self.total = int(self.rec_off[kept])
        parts = [rec[int(x):int(y)] for x, y, g in zip(a, b, good) if g]
        self.values = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        assert len(self.values) == self.total

    def fit(self, val_cap):
        """The prefix of the values that fits: the greatest offset at or below val_cap."""
        return int(self.rec_off[self.rec_off <= np.uint64(val_cap)].max())


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


def now(t, dtype=np.uint8):
    return guards.block_of(t).bytes().view(dtype)


class Call:
    """The guarded device arguments of one reclaim. arrays: which of keys, key_status, info are given."""

    def __init__(self, codec, order, valid, rec, rec_off, val_cap, fill, phases=(0, 0), key_phase=0, rec_bytes=None,
                 arrays=("keys", "key_status", "info"), seed=1):
        self.codec, self.n, self.nrec, self.val_cap = codec, len(order), len(rec_off) - 1, int(val_cap)
        self.rec_bytes = len(rec) if rec_bytes is None else rec_bytes
        n, nrec, dev = self.n, self.nrec, codec.torch_device
        keys, kst, info = per_record(nrec, seed)
        self.host = {"order": np.asarray(order, np.uint32), "valid": u64(valid), "rec": rec, "rec_off": rec_off}
        for name, a in (("keys", keys), ("key_status", kst), ("info", info)):
            if name in arrays:
                self.host[name] = a
        ph = {"rec": phases[0], "keys": key_phase}
        self.dev = {k: put(codec, a, ph.get(k, 0), fill) for k, a in self.host.items()}
        g = lambda nbytes, phase=0: guards.guarded(nbytes, phase=phase, fill=fill, device=dev)  # noqa: E731
        self.order_out, self.remap, self.source = g(4 * n), g(4 * nrec), g(4 * nrec)
        self.keys_out, self.kst_out, self.info_out = g(29 * nrec, key_phase), g(4 * nrec), g(32 * nrec)
        self.off_out, self.status = g(8 * (nrec + 1)), g(4 * nrec)
        self.values = g(self.val_cap, phases[1])
        self.kept, self.val_total = g(8), g(8)
        self.work_bytes = int(codec.lib.honu_key_reclaim_workspace(nrec))
        self.work = g(self.work_bytes)
        self.outs = (self.order_out, self.remap, self.source, self.keys_out, self.kst_out, self.info_out,
                     self.off_out, self.status, self.values, self.kept, self.val_total)

    def args(self, **kw):
        A = guards.address
        d = self.dev
        has = lambda k, t: A(t) if k in d else 0  # noqa: E731
        x = dict(ctx=self.codec.ctx, order=A(d["order"]), valid=A(d["valid"]), n=self.n, keys=A(d.get("keys")),
                 key_status=A(d.get("key_status")), info=A(d.get("info")), rec=A(d["rec"]), rec_off=A(d["rec_off"]),
                 nrec=self.nrec, rec_bytes=self.rec_bytes, flags=0, order_out=A(self.order_out),
                 remap=A(self.remap), source=A(self.source), keys_out=has("keys", self.keys_out),
                 key_status_out=has("key_status", self.kst_out), info_out=has("info", self.info_out),
                 rec_off_out=A(self.off_out), status=A(self.status), values=A(self.values), val_cap=self.val_cap,
                 kept=A(self.kept), val_total=A(self.val_total), work=A(self.work), work_bytes=self.work_bytes)
        x.update(kw)
        return x

    def run(self, **kw):
        x = self.args(**kw)
        return self.codec.lib.honu_key_reclaim(
            x["ctx"], x["order"], x["valid"], x["n"], x["keys"], x["key_status"], x["info"], x["rec"], x["rec_off"],
            x["nrec"], x["rec_bytes"], x["flags"], x["order_out"], x["remap"], x["source"], x["keys_out"],
            x["key_status_out"], x["info_out"], x["rec_off_out"], x["status"], x["values"], x["val_cap"], x["kept"],
            x["val_total"], x["work"], x["work_bytes"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs + (self.work,):
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def check(self, w, with_remap=True, with_status=True, with_values=True):
        """The outputs against numpy's reclaim `w` and the write set."""
        torch.cuda.synchronize()
        n, nrec, k = self.n, self.nrec, w.kept

        def same(name, got, want):
            bad = np.flatnonzero(got != want)
            assert not len(bad), (name, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])

        assert int(now(self.kept, np.uint64)[0]) == k
        assert int(now(self.val_total, np.uint64)[0]) == w.total
        same("order_out", now(self.order_out, np.uint32), w.order)
        same("source", now(self.source, np.uint32)[:k], w.source)
        same("rec_off_out", now(self.off_out, np.uint64), w.rec_off)
        if with_remap:
            same("remap", now(self.remap, np.uint32), w.remap)
        if with_status:
            same("status", now(self.status, np.int32)[:k], w.status)
        s = w.source.astype(np.int64)
        if "keys" in self.dev:
            same("keys_out", now(self.keys_out)[:29 * k], self.host["keys"][s].reshape(-1))
        if "key_status" in self.dev:
            same("key_status_out", now(self.kst_out, np.int32)[:k], self.host["key_status"][s])
        if "info" in self.dev:
            rows = self.host["info"].view(np.uint8).reshape(-1, 32)  # as bytes: the row's padding moves too
            same("info_out", now(self.info_out)[:32 * k], rows[s].reshape(-1))
        fit = w.fit(self.val_cap) if with_values else 0
        if with_values:
            same("values", now(self.values)[:fit], w.values[:fit])
        guards.assert_untouched(self.kept, [(0, 8)])
        guards.assert_untouched(self.val_total, [(0, 8)])
        guards.assert_untouched(self.order_out, [(0, 4 * n)])
        guards.assert_untouched(self.remap, [(0, 4 * nrec)] if with_remap else [])
        guards.assert_untouched(self.source, [(0, 4 * k)])
        guards.assert_untouched(self.keys_out, [(0, 29 * k)] if "keys" in self.dev else [])
        guards.assert_untouched(self.kst_out, [(0, 4 * k)] if "key_status" in self.dev else [])
        guards.assert_untouched(self.info_out, [(0, 32 * k)] if "info" in self.dev else [])
        guards.assert_untouched(self.off_out, [(0, 8 * (nrec + 1))])
        guards.assert_untouched(self.status, [(0, 4 * k)] if with_status else [])
        guards.assert_untouched(self.values, [(0, fit)])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        self.inputs_unchanged()
        return fit


def reclaim_and_check(codec, h_order, valid, h_rec, h_off, val_cap=None, phases=(0, 0), key_phase=0, rec_bytes=None,
                      arrays=("keys", "key_status", "info"), repeat=1, **how):
    """One call (or `repeat` calls) under both fills against numpy; val_cap None: the need + 5.
    `how`: arguments of the call to replace, 0 for a NULL pointer."""
    w = Want(h_order, valid, h_rec, h_off, rec_bytes)
    room = w.total + 5 if val_cap is None else val_cap

    def body(fill):
        for _ in range(repeat):
            c = Call(codec, h_order, valid, h_rec, h_off, room, fill, phases, key_phase, rec_bytes, arrays)
            assert c.run(**how) == 0
            c.check(w, with_remap=how.get("remap", 1) != 0, with_status=how.get("status", 1) != 0,
                    with_values=how.get("values", 1) != 0)

    guards.twice(body)
    return w


# --------------------------------------------------------------------------
# 1. sizes and kept patterns
# --------------------------------------------------------------------------
PATTERNS = ("all", "none", "every_other", "tile_freed", "first", "last", "sixteenth", "fifteen_sixteenths")


def keep_mask(nrec, pattern, rng):
    keep = np.zeros(nrec, bool)
    if pattern in ("all", "none"):  # none: every record named, by rows at or past a valid count of 0
        keep[:] = True
    elif pattern == "every_other":
        keep[::2] = True
    elif pattern == "tile_freed":  # a whole tile between two kept ones; below three tiles the middle third
        keep[:] = True
        lo, hi = (TILE, 2 * TILE) if nrec > 2 * TILE else (nrec // 3, nrec - nrec // 3)
        keep[lo:hi] = False
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "sixteenth":
        keep = rng.random(nrec) < 1 / 16
    else:
        keep = rng.random(nrec) < 15 / 16
    return keep


def column_order(keep, rng, valid=None):
    """(order, valid): a random permutation of the kept records, then one of the freed records."""
    k, f = np.flatnonzero(keep), np.flatnonzero(~keep)
    order = np.concatenate([rng.permutation(k), rng.permutation(f)]).astype(np.uint32)
    return order, len(k) if valid is None else valid


@pytest.mark.parametrize("nrec", (1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 77, 4095))
def test_sizes_and_kept_patterns(codec, nrec):
    rng = np.random.default_rng(nrec)
    rec, off = arena(rng.choice(LENGTHS, nrec), nrec + 1)
    for i, pattern in enumerate(PATTERNS):
        keep = keep_mask(nrec, pattern, rng)
        order, valid = column_order(keep, rng, 0 if pattern == "none" else None)
        w = reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[i % 3], key_phase=KEY_PHASES[i % 2])
        assert w.kept == (0 if pattern == "none" else int(keep.sum()))
        assert (w.order[:valid] != NONE).all() and (w.order[valid:] == NONE).all()
        if pattern == "tile_freed" and nrec > 2 * TILE:
            assert (w.remap[TILE:2 * TILE] == NONE).all() and w.remap[2 * TILE] == TILE


def test_scan_bound_is_refused(codec):
    """The nrec + 1 lengths go through the context's scan, whose state covers
    max_records rows: a context of 4096 takes nrec 4095 and refuses 4096."""
    rng = np.random.default_rng(5)
    rec, off = arena(rng.choice(LENGTHS, MAX_RECORDS), 6)
    order = rng.permutation(MAX_RECORDS).astype(np.uint32)

    def body(fill):
        c = Call(codec, order, MAX_RECORDS, rec, off, len(rec), fill)
        assert c.run() == E_WORKSPACE
        assert c.run(val_cap=0, values=0) == E_WORKSPACE
        c.nothing_stored()

    guards.twice(body)


@pytest.mark.parametrize("phases", PHASES)
@pytest.mark.parametrize("key_phase", KEY_PHASES)
def test_phases(codec, phases, key_phase):
    nrec = 300
    rng = np.random.default_rng(7)
    rec, off = arena(rng.choice(LENGTHS + (4097,), nrec), 8)
    order, valid = column_order(rng.random(nrec) < 0.6, rng)
    reclaim_and_check(codec, order, valid, rec, off, phases=phases, key_phase=key_phase)


# --------------------------------------------------------------------------
# 2. the column's length against the records'
# --------------------------------------------------------------------------
def test_fewer_rows_than_records(codec):
    nrec, n = 1500, 700
    rng = np.random.default_rng(11)
    rec, off = arena(rng.choice(LENGTHS, nrec), 12)
    named = rng.permutation(nrec)[:n].astype(np.uint32)
    named[600:] = (nrec, nrec + 5, SEEK_NONE, nrec + 1000) * 25  # a tail that names no record
    for ph, valid in zip(PHASES, (500, 600, 0)):
        w = reclaim_and_check(codec, named, valid, rec, off, phases=ph)
        assert w.kept == valid < nrec


def test_more_rows_than_records(codec):
    nrec, n = 700, 1500
    rng = np.random.default_rng(13)
    rec, off = arena(rng.choice(LENGTHS, nrec), 14)
    order = np.concatenate([rng.permutation(nrec)[:400], rng.integers(nrec, 1 << 32, n - 400)]).astype(np.uint32)
    order[-1] = SEEK_NONE
    for ph, valid in zip(PHASES, (400, 333, 1)):
        w = reclaim_and_check(codec, order, valid, rec, off, phases=ph, key_phase=1)
        assert w.kept == valid


def test_no_records(codec):
    """nrec == 0: the two counts, d_rec_off_out[0] and an order of NONE."""
    rec, off = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    order = np.array([0, 5, SEEK_NONE, 1], np.uint32)
    for valid in (0, 4):
        reclaim_and_check(codec, order, valid, rec, off, val_cap=0, values=0, rec=0)
        reclaim_and_check(codec, order, valid, rec, off, val_cap=16, arrays=())
    reclaim_and_check(codec, order[:0], 3, rec, off, val_cap=0, values=0, rec=0, order=0, order_out=0)


def test_no_rows(codec):
    """n == 0 with records: every record is freed."""
    rec, off = arena([5, 0, 300], 15)
    w = reclaim_and_check(codec, np.zeros(0, np.uint32), 9, rec, off, order=0, order_out=0)
    assert w.kept == 0 and (w.remap == NONE).all()


# --------------------------------------------------------------------------
# 3. the copy's three launch forms at their smallest
# --------------------------------------------------------------------------
def test_twelve_records_of_20_kb(codec):
    """Mean >= 16 KB: range tails from the ticket line; twice on one context: the line came back to zero."""
    rec, off = arena([20000] * 12, 20)
    rng = np.random.default_rng(21)
    for ph in PHASES:
        w = reclaim_and_check(codec, rng.permutation(12).astype(np.uint32), 12, rec, off, phases=ph, repeat=2)
        assert 16 << 10 <= w.total // 12 < 64 << 10
    keep = np.ones(12, bool)
    keep[4] = False
    order, valid = column_order(keep, rng)
    w = reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[1])
    assert w.kept == 11 and w.total // 12 >= 16 << 10


def test_six_records_of_96_kb_and_three_short_ones(codec):
    """Mean >= 64 KB: the few-waves form, the 100-byte records its short class."""
    big, small = 96 << 10, 100
    rec, off = arena([big, big, small, big, small, big, big, small, big], 22)
    rng = np.random.default_rng(23)
    for ph in PHASES:
        w = reclaim_and_check(codec, rng.permutation(9).astype(np.uint32), 9, rec, off, phases=ph)
        assert w.total // 9 >= 64 << 10


# --------------------------------------------------------------------------
# 4. optional arrays
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """1300 records, two tiles, 60 % named."""
    nrec = 1300
    rng = np.random.default_rng(30)
    rec, off = arena(rng.choice(LENGTHS, nrec), 31)
    order, valid = column_order(rng.random(nrec) < 0.6, rng)
    return order, valid, rec, off


@pytest.mark.parametrize("arrays", (("keys", "key_status", "info"), (), ("info",)))
def test_optional_arrays(codec, pool, arrays):
    order, valid, rec, off = pool
    reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[1], key_phase=1, arrays=arrays)


def test_without_remap_and_without_status(codec, pool):
    order, valid, rec, off = pool
    reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[2], remap=0)
    reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[1], status=0)
    reclaim_and_check(codec, order, valid, rec, off, remap=0, status=0, arrays=())


# --------------------------------------------------------------------------
# 5. garbage in
# --------------------------------------------------------------------------
def test_repeated_and_wild_indices_among_the_valid_rows(codec, pool):
    order, valid, rec, off = pool
    nrec = len(off) - 1
    bad = order.copy()
    bad[10], bad[11], bad[500] = bad[3], bad[3], bad[3]      # one record named four times
    bad[20], bad[21], bad[22] = nrec, nrec + 5, SEEK_NONE
    assert valid > 500
    for ph in PHASES:
        w = reclaim_and_check(codec, bad, valid, rec, off, phases=ph)
        assert w.order[10] == w.order[11] == w.order[500] == w.order[3] != NONE
        assert (w.order[20:23] == NONE).all() and w.kept == valid - 6


@pytest.mark.parametrize("valid", ("n+5", "2^40", "2^63"))
def test_valid_counts_above_n_are_clamped(codec, pool, valid):
    order, _, rec, off = pool
    v = {"n+5": len(order) + 5, "2^40": 1 << 40, "2^63": 1 << 63}[valid]
    w = reclaim_and_check(codec, order, v, rec, off, phases=PHASES[1])
    assert w.kept == len(order) == len(off) - 1


def test_untrusted_offsets(codec, pool):
    order, valid, rec, off = pool
    nrec = len(off) - 1
    kept = np.sort(order[:valid].astype(np.int64))
    r = int(next(x for x in kept[10:] if off[x] > 0 and x + 1 < nrec))
    down = off.copy()
    down[r + 1] = down[r] - np.uint64(1)  # record r descends
    w = reclaim_and_check(codec, order, valid, rec, down, phases=PHASES[1])
    j = int(w.remap[r])
    assert w.status[j] == INPUT and w.rec_off[j] == w.rec_off[j + 1] and (w.status != OK).sum() <= 2
    q = int(kept[-3])
    above = off.copy()
    above[q + 1:] = np.uint64(len(rec) + 7)  # record q ends past the arena; the ones after it are empty there
    w = reclaim_and_check(codec, order, valid, rec, above, phases=PHASES[2])
    bad = np.flatnonzero(w.status != OK)
    assert w.status[int(w.remap[q])] == INPUT and len(bad) >= 1 and (w.source[bad] >= q).all()
    assert (w.status[:int(w.remap[q])] == OK).all()
    # one pair past rec_bytes: that row alone
    past = off.copy()
    past[nrec] += np.uint64(7)
    w = reclaim_and_check(codec, order, len(order), rec, past, phases=PHASES[1])
    assert np.flatnonzero(w.status != OK).tolist() == [nrec - 1] and w.kept == nrec
    # a rec_bytes below the arena's size: the records that end past it
    w = reclaim_and_check(codec, order, valid, rec, off, phases=PHASES[1], rec_bytes=int(off[nrec]) - 1)
    last = np.flatnonzero(off[1:] == off[nrec])  # the records that end at the arena's end
    assert set(w.source[w.status != OK].tolist()) == set(last.tolist()) & set(kept.tolist())
    # offsets up to the very top of 64 bits
    wild = off.copy()
    wild[5], wild[6] = np.uint64((1 << 64) - 1), np.uint64(1 << 63)
    reclaim_and_check(codec, order, len(order), rec, wild)


# --------------------------------------------------------------------------
# 6. byte capacity
# --------------------------------------------------------------------------
@pytest.mark.parametrize("room", ("total", "total-1", "interior", "zero"))
def test_byte_capacity(codec, pool, room):
    order, valid, rec, off = pool
    w0 = Want(order, valid, rec, off)
    k = next(j for j in range(w0.kept // 2, w0.kept) if w0.rec_off[j] > w0.rec_off[j - 1])  # record k - 1 has bytes
    last = int(w0.rec_off[w0.rec_off < np.uint64(w0.total)].max())  # where the last record with bytes starts
    val_cap = {"total": w0.total, "total-1": w0.total - 1, "interior": int(w0.rec_off[k]), "zero": 0}[room]
    fit = {"total": w0.total, "total-1": last, "interior": int(w0.rec_off[k]), "zero": 0}[room]
    assert w0.fit(val_cap) == fit and 0 < int(w0.rec_off[k]) < last < w0.total
    for ph in PHASES:
        how = dict(values=0) if room == "zero" else {}  # d_values NULL: a sizing call
        w = reclaim_and_check(codec, order, valid, rec, off, val_cap=val_cap, phases=ph, **how)
        assert w.total == w0.total  # the full need every time


# --------------------------------------------------------------------------
# 7. refusals
# --------------------------------------------------------------------------
def test_refusals_store_nothing(codec, pool):
    order, valid, rec, off = pool
    w = Want(order, valid, rec, off)

    def body(fill):
        c = Call(codec, order, valid, rec, off, w.total + 9, fill, (1, 3), 1)
        a = c.args()
        for kw in (dict(n=1 << 32), dict(nrec=1 << 32), dict(n=(1 << 64) - 1), dict(nrec=(1 << 64) - 1),
                   dict(nrec=MAX_RECORDS), dict(nrec=MAX_RECORDS, val_cap=0, values=0)):
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(valid=0), dict(kept=0), dict(val_total=0), dict(rec_off=0),
                   dict(rec_off_out=0), dict(source=0), dict(order=0), dict(order_out=0), dict(rec=0),
                   dict(values=0), dict(keys=0), dict(keys_out=0), dict(key_status=0), dict(key_status_out=0),
                   dict(info=0), dict(info_out=0), dict(flags=1), dict(flags=2), dict(flags=1 << 31),
                   dict(work_bytes=c.work_bytes - 1), dict(work_bytes=0), dict(work=0), dict(work=a["work"] + 128),
                   dict(order=a["order"] + 2), dict(order_out=a["order_out"] + 2), dict(remap=a["remap"] + 2),
                   dict(source=a["source"] + 2), dict(key_status=a["key_status"] + 2),
                   dict(key_status_out=a["key_status_out"] + 2), dict(status=a["status"] + 2),
                   dict(valid=a["valid"] + 4), dict(kept=a["kept"] + 4), dict(val_total=a["val_total"] + 4),
                   dict(rec_off=a["rec_off"] + 4), dict(rec_off_out=a["rec_off_out"] + 4),
                   dict(info=a["info"] + 4), dict(info_out=a["info_out"] + 4)):
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run() == 0  # and the arguments were good
        c.check(w)

    guards.twice(body)


def test_reclaim_tile_param(codec):
    v = L.C.c_int64(0)
    assert codec.lib.honu_ctx_get_param(codec.ctx, b"reclaim_tile", L.C.addressof(v)) == 0 and v.value == TILE
    assert codec.lib.honu_ctx_set_param(codec.ctx, b"reclaim_tile", 512) == E_ARG


# --------------------------------------------------------------------------
# 8. graph
# --------------------------------------------------------------------------
def test_graph_replays_after_valid_and_order_changed(codec, pool):
    order, valid, rec, off = pool
    rng = np.random.default_rng(40)
    rounds = [(order, valid), (order, valid // 2), (rng.permutation(order), valid // 2)]
    dev = codec.torch_device

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        c = Call(codec, order, valid, rec, off, len(rec), fill, (3, 1), 1)
        assert c.run() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run() == 0
        kept = []
        for o, v in rounds:
            for t in c.outs:
                refill(t, fill)
            c.dev["order"].copy_(torch.from_numpy(o.view(np.uint8).copy()).to(dev))
            c.dev["valid"].copy_(torch.from_numpy(u64(v).view(np.uint8)).to(dev))
            c.host["order"], c.host["valid"] = o, u64(v)
            g.replay()
            w = Want(o, v, rec, off)
            c.check(w)
            kept.append((w.kept, w.total))
        assert kept[0][0] == valid and kept[1][0] == kept[2][0] == valid // 2 and kept[1] != kept[2]

    guards.twice(body)


# --------------------------------------------------------------------------
# 9. the chain: sort -> delete -> reclaim -> objects / seek / list / fetch / decode
# --------------------------------------------------------------------------
def host(t, dtype, count):
    return t.cpu().numpy().view(np.uint8).reshape(-1)[:count * np.dtype(dtype).itemsize].view(dtype)


def read_chain(codec, col, keys, order, valid, n, arena_, arena_off, nrec, rec_bytes, info, probes, pstatus):
    """objects, then seek -> list -> fetch -> decode of every probe's object, newest version first."""
    obj_off, latest, objects = codec.key_objects(keys, order, valid)  # the unsorted keys, by record
    seeks = codec.seek_keys(col[:29 * n], valid, probes, 17, probe_status=pstatus, order=order, info=info)
    rows, range_off, total, _ = codec.list_keys(col[:29 * n], order, valid, seeks, n, reverse=True, info=info)
    values, val_off, val_total, status = codec.fetch_objects(rows, total, n, arena_, arena_off, nrec, rec_bytes,
                                                             rec_bytes)
    dec = codec.decode(values, val_off, n, rec_bytes=rec_bytes)
    torch.cuda.synchronize()
    t = int(total.item())
    k = int(objects.item())
    return dict(objects=k, obj_off=obj_off.cpu().numpy()[:k + 1], latest=host(latest, np.uint32, k), t=t,
                seeks=host(seeks, np.uint32, 5 * len(pstatus) // 4).reshape(-1, 5),
                rows=host(rows, np.uint32, 4 * t).reshape(-1, 4), range_off=range_off.cpu().numpy(),
                status=status.cpu().numpy()[:t], val_off=val_off.cpu().numpy()[:t + 1],
                values=hobj._to_host(values, int(val_total.item()), np.uint8), dec=dec.host())


def test_sort_delete_reclaim_read_chain(codec):
    n = 1500
    dev = codec.torch_device
    hb, dead, first = chain_batch(n)  # 19 objects; first: one record index per object
    enc = codec.marshal(hobj.DeviceBatch.from_host(hb, dev))
    rec_bytes = int(enc.out_off.view(torch.int64)[n].item())
    d1 = codec.decode(enc.out, enc.out_off, n, rec_bytes=rec_bytes)
    dk, dst = codec.keys(d1)
    dk, dst = dk[:29 * n], dst[:4 * n]
    order, col, valid = codec.sort_keys(dk, dst, n=n, want_sorted=True)

    def rows_of(idx):
        pick = torch.tensor(idx, device=dev)
        return (dk.view(n, 29)[pick].reshape(-1).contiguous(),
                dst.view(torch.int32)[pick].contiguous().view(torch.uint8))

    gone = first[::3]  # a third of the objects
    od, sd, vd = codec.sort_keys(*rows_of(gone), n=len(gone), want_sorted=True)
    s3, o3, v3, r3 = codec.delete_keys(col[:29 * n], order, valid, sd[:29 * len(gone)], vd, probe_len=17)
    R = codec.reclaim_records(o3, v3, n, enc.out, enc.out_off, n, rec_bytes, rec_bytes, keys=dk, key_status=dst,
                              info=d1.info[:32 * n], want_remap=True)
    torch.cuda.synchronize()
    kept = int(R.kept.item())  # the one host read that follows a reclaim
    assert kept == int(v3.item()) and 0 < int(r3.item()) < n and 0 < kept < n
    total_bytes = int(R.val_total.item())
    assert 0 < total_bytes < rec_bytes
    probes, pstatus = rows_of(first)  # every object, the dropped ones included

    a = read_chain(codec, s3, dk, o3, v3, n, enc.out, enc.out_off, n, rec_bytes, d1.info, probes, pstatus)
    b = read_chain(codec, s3[:29 * kept], R.keys, R.order[:kept], v3, kept, R.values, R.rec_off, kept, total_bytes, R.info,
                   probes, pstatus)
    remap = R.remap.cpu().numpy().view(np.uint32)
    # the column did not move: the same objects, ranges and rows, the record indices through the remap
    assert a["objects"] == b["objects"] and np.array_equal(a["obj_off"], b["obj_off"])
    assert np.array_equal(remap[a["latest"]], b["latest"])
    t = a["t"]
    assert kept // 2 < t == b["t"] <= kept and np.array_equal(a["range_off"], b["range_off"])
    assert np.array_equal(a["seeks"][:, [0, 1, 4]], b["seeks"][:, [0, 1, 4]])
    found = a["seeks"][:, 2] != SEEK_NONE
    assert 0 < found.sum() < len(first)
    assert np.array_equal(remap[a["seeks"][found][:, 2]], b["seeks"][found][:, 2])
    assert np.array_equal(remap[a["seeks"][found][:, 3]], b["seeks"][found][:, 3])
    assert np.array_equal(a["rows"][:, [0, 1, 3]], b["rows"][:, [0, 1, 3]])
    assert np.array_equal(remap[a["rows"][:, 2]], b["rows"][:, 2])
    tomb = (a["rows"][:, 3] & LIST_ROW_TOMBSTONE) != 0
    assert np.array_equal(tomb, dead[a["rows"][:, 2]]) and 0 < tomb.sum() < t
    assert (a["status"] == OK).all() and (b["status"] == OK).all()
    # the same payloads and the same decoded rows, record for record
    assert np.array_equal(a["val_off"], b["val_off"]) and a["values"].tobytes() == b["values"].tobytes()
    meta1, info1, acl1, reg1, _, _ = a["dec"]
    meta2, info2, acl2, reg2, _, _ = b["dec"]
    assert (info1["meta_status"][:t] == OK).all()
    for g in range(0, t, 7):
        x = resolved(meta1[g:g + 1], info1[g:g + 1], a["values"], acl1, reg1)
        y = resolved(meta2[g:g + 1], info2[g:g + 1], b["values"], acl2, reg2)
        assert x == y, g
    assert info1[:t].tobytes() == info2[:t].tobytes()
    # the reclaimed arena is the kept records in arrival order, and decodes to the gathered keys
    src = host(R.source, np.uint32, kept).astype(np.int64)
    assert (np.diff(src) > 0).all() and np.array_equal(remap[src], np.arange(kept))
    off1 = hobj._to_host(enc.out_off, 8 * (n + 1), np.uint64).astype(np.int64)
    arena1 = hobj._to_host(enc.out, rec_bytes, np.uint8)
    arena2 = hobj._to_host(R.values, total_bytes, np.uint8)
    assert arena2.tobytes() == b"".join(arena1[off1[r]:off1[r + 1]].tobytes() for r in src)
    d2 = codec.decode(R.values, R.rec_off, kept, rec_bytes=total_bytes)
    k2, st2 = codec.keys(d2)
    torch.cuda.synchronize()
    assert k2[:29 * kept].cpu().numpy().tobytes() == R.keys[:29 * kept].cpu().numpy().tobytes()
    assert st2[:4 * kept].cpu().numpy().tobytes() == R.key_status[:kept].cpu().numpy().tobytes()
    keys1 = dk.cpu().numpy().reshape(n, 29)
    assert R.keys[:29 * kept].cpu().numpy().tobytes() == keys1[src].tobytes()
    assert R.info[:32 * kept].cpu().numpy().tobytes() == d1.info[:32 * n].cpu().numpy().reshape(n, 32)[src].tobytes()
