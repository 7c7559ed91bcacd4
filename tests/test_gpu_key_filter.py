"""honu_key_filter on the GPU against numpy.

The expectation is numpy's alone: a keep mask over the rows below w =
min(total, cap) (the row's TOMBSTONE flag; with HONU_FILTER_DELETED the
tombstone byte of the info row that d_latest names for the object found by
searchsorted over the clamped d_obj_off), the kept rows in order, a cumsum of
the mask looked up at the clamped range offsets, and HEAD where a kept row
lands on its range's new offset. It never calls the library. Every input and
output is a guarded view (tests/guards.py) under both fills, d_keys and
d_keys_out at byte phases 0, 1 and 3; the write set is exactly
d_rows_out[0, kept), d_keys_out[0, 29 kept), d_range_off_out[0, m + 1),
d_total_out[0] and the workspace, and the inputs are unchanged. Sizes are in
units of the tile T, the param "filter_tile".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (FILTER_DELETED, FILTER_TOMBSTONE, HAS_VERSION, INFO_DTYPE, LIST_ROW_DTYPE,  # noqa: E402
                               LIST_ROW_HEAD, LIST_ROW_TOMBSTONE)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
OK = hobj.OK
PHASES = ((0, 0), (1, 3), (3, 1))  # (d_keys, d_keys_out)
MAX_RECORDS = 4096
BOTH = FILTER_TOMBSTONE | FILTER_DELETED
HEAD, TOMB = np.uint32(LIST_ROW_HEAD), np.uint32(LIST_ROW_TOMBSTONE)


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
def T(codec):
    t = _param(codec, b"filter_tile")
    assert t >= 128 and t % 64 == 0
    return t


# --------------------------------------------------------------------------
# expectations
# --------------------------------------------------------------------------
class Column:
    """What HONU_FILTER_DELETED reads: the column's valid count and rows n,
    honu_key_objects' outputs and the records' tombstone bytes."""

    def __init__(self, valid, n, obj_off, latest, objects, tomb, order=None):
        self.valid, self.n, self.objects = int(valid), int(n), int(objects)
        self.order = order  # the column's d_order, for the tests that make its lists: the call does not read it
        self.obj_off = np.asarray(obj_off, np.uint64)
        self.latest = np.asarray(latest, np.uint32)
        self.tomb = np.asarray(tomb, np.uint8)
        assert len(self.obj_off) == n + 1 and len(self.latest) == n and len(self.tomb) == n

    def info(self):
        info = np.zeros(self.n, INFO_DTYPE)
        info["tombstone"] = self.tomb
        info["data_off"], info["data_len"] = 0x0102030405060708, 0x1112131415161718
        return info

    def deleted(self, pos):
        """Which of the positions lie in an object whose latest record is a tombstone."""
        pos = np.asarray(pos, np.int64)
        v, objs = min(self.valid, self.n), min(self.objects, self.n)
        if self.n == 0 or objs == 0:
            return np.zeros(len(pos), bool)
        ends = np.minimum(self.obj_off[1:objs + 1], np.uint64(v)).astype(np.int64)
        j = np.minimum(np.searchsorted(ends, pos, side="right"), objs - 1)
        r = np.minimum(self.latest[j].astype(np.int64), self.n - 1)
        return (pos < v) & (self.tomb[r] != 0)


def keep_mask(rows, w, flags, col=None):
    keep = np.ones(w, bool)
    if flags & FILTER_TOMBSTONE:
        keep &= (rows["flags"][:w] & TOMB) == 0
    if flags & FILTER_DELETED:
        keep &= ~col.deleted(rows["pos"][:w])
    return keep


def from_keep(rows, keys, range_off, w, keep):
    """(rows_out, range_off_out uint64[m + 1], keys_out) of a keep mask over the first w rows."""
    m = len(range_off) - 1
    kept = int(keep.sum())
    rank = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    off = np.empty(m + 1, np.uint64)
    off[:m] = rank[np.minimum(range_off[:m], np.uint64(w)).astype(np.int64)]
    off[m] = kept
    out = rows[:w][keep].copy()
    head = np.zeros(kept, bool)
    if m:
        q = np.minimum(out["range"].astype(np.int64), m - 1)
        head = off[q] == np.arange(kept, dtype=np.uint64)
    out["flags"] = (out["flags"] & ~HEAD) | np.where(head, HEAD, np.uint32(0))
    return out, off, keys[:w][keep]


def expected_filter(rows, keys, range_off, total, cap, flags, col=None):
    w = min(int(total), cap)
    return from_keep(rows, keys, range_off, w, keep_mask(rows, w, flags, col))


def heads_are_first_of_their_range(out):
    """Over a list: HEAD on exactly the first kept row of each range."""
    first = np.ones(len(out), bool)
    first[1:] = out["range"][1:] != out["range"][:-1]
    assert np.array_equal((out["flags"] & HEAD) != 0, first)


# --------------------------------------------------------------------------
# lists
# --------------------------------------------------------------------------
def make_list(counts, seed, extra=0, pos_below=1 << 20):
    """(rows, keys, range_off) of a list whose range q has counts[q] rows,
    then `extra` rows behind the total that no call may read as rows: random
    positions and keys, the record a number of its own per row, HEAD where the
    list sets it and a high flag bit on some rows."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    rows = np.zeros(total + extra, LIST_ROW_DTYPE)
    rows["range"][:total] = np.repeat(np.arange(len(counts)), counts)
    rows["range"][total:] = 0
    rows["pos"] = rng.integers(0, pos_below, total + extra)
    rows["record"] = np.arange(total + extra) + 1000
    range_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    rows["flags"][range_off[:-1][counts > 0].astype(np.int64)] = HEAD
    rows["flags"][::5] |= np.uint32(1 << 30)
    keys = rng.integers(0, 256, (total + extra, 29), dtype=np.uint8)
    return rows, keys, range_off


def split(total, pieces, seed, empties=0):
    """`pieces` counts that sum to `total`, with `empties` zeros among them."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, total + 1, pieces - 1)) if pieces > 1 else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [total]])).tolist()
    for _ in range(empties):
        counts.insert(int(rng.integers(0, len(counts) + 1)), 0)
    return counts


PATTERNS = ("all", "none", "half", "one_per_tile", "hole", "straddle")


def removed(pattern, n, T, seed=0):
    """The rows of [0, n) a pattern removes."""
    gone = np.zeros(n, bool)
    if pattern == "none":
        gone[:] = True
    elif pattern == "half":
        gone = np.random.default_rng(seed).integers(0, 2, n).astype(bool)
    elif pattern == "one_per_tile":  # the tile's row 70, or its last where it is shorter
        gone[:] = True
        for t0 in range(0, n, T):
            gone[min(t0 + 70, n - 1)] = False
    elif pattern == "hole":  # a wholly removed tile (the second) between kept ones; a short list loses its middle
        a, b = (T, min(2 * T, n)) if n > T else (n // 3, n - n // 3)
        gone[a:b] = True
    elif pattern == "straddle":  # a removed run over the first tile boundary; a short list loses its end
        a, b = (T - 37, min(T + 29, n)) if n > T - 37 else (n // 2, n)
        gone[a:b] = True
    return gone


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
    """The guarded device arguments of one filter."""

    def __init__(self, codec, rows, keys, range_off, total, cap, fill, phases=(0, 0), col=None):
        self.codec, self.cap, self.m = codec, int(cap), len(range_off) - 1
        assert len(rows) == self.cap and (keys is None or len(keys) == self.cap)
        self.host = {"rows": rows, "range_off": range_off, "total": u64(total)}
        if keys is not None:
            self.host["keys"] = keys
        self.n = 0
        if col is not None:
            self.n = col.n
            self.host.update(valid=u64(col.valid), obj_off=col.obj_off, latest=col.latest, objects=u64(col.objects),
                             info=col.info())
        self.dev = {k: put(codec, a, phases[0] if k == "keys" else 0, fill) for k, a in self.host.items()}
        dev = codec.torch_device
        self.work_bytes = int(codec.lib.honu_key_filter_workspace(self.cap))
        self.rows_out = guards.guarded(16 * self.cap, fill=fill, device=dev)
        self.keys_out = guards.guarded(29 * self.cap, phase=phases[1], fill=fill, device=dev)
        self.range_off_out = guards.guarded(8 * (self.m + 1), fill=fill, device=dev)
        self.total_out = guards.guarded(8, fill=fill, device=dev)
        self.work = guards.guarded(self.work_bytes, fill=fill, device=dev)
        self.outs = (self.rows_out, self.keys_out, self.range_off_out, self.total_out, self.work)

    def args(self, flags=0, **kw):
        A = guards.address
        d = self.dev
        with_keys = "keys" in d
        x = dict(ctx=self.codec.ctx, rows=A(d["rows"]), keys=A(d.get("keys")), range_off=A(d["range_off"]), m=self.m,
                 total=A(d["total"]), cap=self.cap, flags=flags, valid=A(d.get("valid")), n=self.n,
                 obj_off=A(d.get("obj_off")), latest=A(d.get("latest")), objects=A(d.get("objects")),
                 info=A(d.get("info")), rows_out=A(self.rows_out), keys_out=A(self.keys_out) if with_keys else 0,
                 range_off_out=A(self.range_off_out), total_out=A(self.total_out), work=A(self.work),
                 work_bytes=self.work_bytes)
        x.update(kw)
        return x

    def run(self, flags=0, **kw):
        x = self.args(flags, **kw)
        return self.codec.lib.honu_key_filter(
            x["ctx"], x["rows"], x["keys"], x["range_off"], x["m"], x["total"], x["cap"], x["flags"], x["valid"],
            x["n"], x["obj_off"], x["latest"], x["objects"], x["info"], x["rows_out"], x["keys_out"],
            x["range_off_out"], x["total_out"], x["work"], x["work_bytes"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs:
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def kept_records(self):
        """The record fields of the rows the call kept."""
        torch.cuda.synchronize()
        kept = int(guards.block_of(self.total_out).bytes().view(np.uint64)[0])
        assert kept <= self.cap
        return guards.block_of(self.rows_out).bytes()[:16 * kept].view(LIST_ROW_DTYPE)["record"]

    def check(self, want, with_keys=True):
        """The outputs against (rows_out, range_off_out, keys_out) and the write set."""
        torch.cuda.synchronize()
        rows, range_off, keys = want
        kept = len(rows)
        got_total = int(guards.block_of(self.total_out).bytes().view(np.uint64)[0])
        assert got_total == kept == int(range_off[-1]), (got_total, kept, int(range_off[-1]))
        got = guards.block_of(self.range_off_out).bytes().view(np.uint64)
        bad = np.flatnonzero(got != range_off)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], range_off[bad[:4]])
        got = guards.block_of(self.rows_out).bytes()[:16 * kept].view(np.uint32).reshape(kept, 4)
        exp = np.ascontiguousarray(rows).view(np.uint32).reshape(kept, 4)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], exp[bad[:4]])
        if with_keys:
            got = guards.block_of(self.keys_out).bytes()[:29 * kept].reshape(kept, 29)
            bad = np.flatnonzero((got != keys).any(axis=1))
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], keys[bad[:4]])
        guards.assert_untouched(self.rows_out, [(0, 16 * kept)])
        guards.assert_untouched(self.keys_out, [(0, 29 * kept)] if with_keys else [])
        guards.assert_untouched(self.range_off_out, [(0, 8 * (self.m + 1))])
        guards.assert_untouched(self.total_out, [(0, 8)])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        self.inputs_unchanged()


def filter_and_check(codec, rows, keys, range_off, total, flags, cap=None, phases=(0, 0), col=None, with_keys=True,
                     wellformed=True):
    """One call under both fills against numpy; cap None: the rows given."""
    cap = len(rows) if cap is None else cap
    assert len(rows) >= cap
    rows, keys = rows[:cap], keys[:cap]
    want = expected_filter(rows, keys, range_off, total, cap, flags, col)
    if wellformed:
        heads_are_first_of_their_range(want[0])

    def body(fill):
        c = Call(codec, rows, keys if with_keys else None, range_off, total, cap, fill, phases, col)
        assert c.run(flags) == 0
        c.check(want, with_keys)

    guards.twice(body)
    return want


def flag_rows(rows, gone):
    """The rows with TOMBSTONE on those of `gone` (a mask over the rows' first len(gone))."""
    rows = rows.copy()
    rows["flags"][:len(gone)] |= np.where(gone, TOMB, np.uint32(0))
    return rows


# --------------------------------------------------------------------------
# 1. empty and small lists
# --------------------------------------------------------------------------
def test_cap_zero_writes_the_offsets_and_the_total(codec):
    rows, keys, _ = make_list([], 1)
    for m in (0, 3):
        off = np.full(m + 1, 7, np.uint64)  # a counting list call's offsets: not read as rows
        for flags in (0, FILTER_TOMBSTONE):
            want = filter_and_check(codec, rows, keys, off, 7, flags, cap=0, phases=PHASES[1])
            assert len(want[0]) == 0 and not want[1].any()


def test_total_zero(codec, T):
    rows, keys, _ = make_list([], 2, extra=T + 5)  # rows behind the total: none is one
    off = np.zeros(4, np.uint64)
    want = filter_and_check(codec, rows, keys, off, 0, FILTER_TOMBSTONE, phases=PHASES[2])
    assert len(want[0]) == 0 and not want[1].any()


def test_no_ranges(codec):
    """m == 0: a list has no rows then. With rows all the same (total is not
    the list's): they are filtered, none is a HEAD, and the one offset is the
    kept count."""
    rows, keys, _ = make_list([], 3, extra=70)
    rows = flag_rows(rows, removed("half", 70, 64, 3))
    rows["flags"][:9] |= HEAD
    for total in (0, 70):
        want = filter_and_check(codec, rows, keys, np.zeros(1, np.uint64), total, FILTER_TOMBSTONE, phases=PHASES[1],
                                wellformed=False)
        assert len(want[1]) == 1 and not (want[0]["flags"] & HEAD).any() and (total == 0) == (len(want[0]) == 0)


def test_no_flags_copies_the_list(codec, T):
    counts = split(T + 9, 7, 4, empties=3)
    rows, keys, off = make_list(counts, 4, extra=3)
    rows = flag_rows(rows, removed("half", T + 9, T, 4))  # flagged rows stay: nothing asks
    for ph in PHASES:
        out, off_out, keys_out = filter_and_check(codec, rows, keys, off, T + 9, 0, phases=ph)
        assert out.tobytes() == rows[:T + 9].tobytes() and np.array_equal(off_out, off)
        assert keys_out.tobytes() == keys[:T + 9].tobytes()


# --------------------------------------------------------------------------
# 2. lengths and patterns
# --------------------------------------------------------------------------
LENGTHS = ("1", "63", "64", "65", "T-1", "T", "T+1", "2T+77")


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_and_patterns(codec, T, length):
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+77": 2 * T + 77}.get(length) or int(length)
    counts = split(n, min(n, 9), n, empties=4)
    rows, keys, off = make_list(counts, n, extra=2)  # two rows of room behind the total
    for j, pattern in enumerate(PATTERNS):
        gone = removed(pattern, n, T, seed=j)
        out, off_out, _ = filter_and_check(codec, flag_rows(rows, gone), keys, off, n, FILTER_TOMBSTONE,
                                           phases=PHASES[j % 3])
        assert len(out) == n - int(gone.sum())
        assert np.array_equal(out["record"], rows["record"][:n][~gone])
        per_range = np.add.reduceat(np.concatenate([~gone, [False]]).astype(np.int64), off[:-1].astype(np.int64))
        per_range[np.diff(off.astype(np.int64)) == 0] = 0  # (reduceat gives an empty slice its next element)
        assert np.array_equal(np.diff(off_out.astype(np.int64)), per_range)
    # and without keys
    filter_and_check(codec, flag_rows(rows, removed("half", n, T, 9)), keys, off, n, FILTER_TOMBSTONE, with_keys=False)


# --------------------------------------------------------------------------
# 3. truncated lists
# --------------------------------------------------------------------------
@pytest.mark.parametrize("total", ("above", "far"))
def test_truncated_list(codec, T, total):
    """d_total above cap: the cap rows that were written are filtered, and the
    offsets past them all come out as the kept count."""
    full = 3 * T
    counts = split(full, 11, 30, empties=2)
    rows, keys, off = make_list(counts, 30)
    cap = T + 90
    t = full if total == "above" else (1 << 64) - 1
    gone = removed("half", cap, T, 31)
    for ph in PHASES[:2]:
        out, off_out, _ = filter_and_check(codec, flag_rows(rows, gone), keys, off, t, FILTER_TOMBSTONE, cap=cap,
                                           phases=ph)
        assert len(out) == cap - int(gone.sum()) and (off > cap).sum() > 2
        assert (off_out[off >= cap] == len(out)).all()


# --------------------------------------------------------------------------
# 4. ranges and HEAD
# --------------------------------------------------------------------------
def test_ranges_and_heads(codec, T):
    """4 T + 77 rows: empty ranges between full ones, a range wholly removed,
    a range that starts on a tile boundary, one longer than two tiles, a range
    whose first rows go, trailing empty ranges."""
    counts = [T, 0, 0, 5, 2 * T + 50, 0, 9, T + 13, 0, 0]
    n = sum(counts)
    assert n == 4 * T + 77
    rows, keys, off = make_list(counts, 40)
    o = off.astype(np.int64)
    gone = removed("half", n, T, 41)
    gone[o[3]:o[4]] = True            # the 5-row range vanishes
    gone[o[4]:o[4] + 70] = True       # the long range loses its first 70 rows: HEAD moves on
    gone[o[4] + 70] = False
    gone[o[0]] = False                # a range keeps its first row: HEAD stays
    gone[o[6]:o[7]] = False
    gone[o[7]] = True                 # one first row gone ...
    gone[o[7] + 1] = False            # ... HEAD on the next
    assert o[1] % T == 0 and o[3] % T == 0
    for ph in PHASES:
        out, off_out, _ = filter_and_check(codec, flag_rows(rows, gone), keys, off, n, FILTER_TOMBSTONE, phases=ph)
        oo = off_out.astype(np.int64)
        assert oo[3] == oo[4] and not (out["range"] == 3).any()  # the vanished range: empty, no HEAD of its own
        assert out["record"][oo[4]] == rows["record"][o[4] + 70] and out["flags"][oo[4]] & HEAD
        assert not rows["flags"][o[4] + 70] & HEAD
        assert out["record"][oo[7]] == rows["record"][o[7] + 1]
        assert (oo[8:] == len(out)).all() and (out["flags"] & HEAD != 0).sum() == 4  # five ranges had rows


def test_more_single_row_ranges_than_a_tile(codec, T):
    m = T + 9
    rows, keys, off = make_list([1] * m, 42)
    gone = removed("half", m, T, 43)
    out, off_out, _ = filter_and_check(codec, flag_rows(rows, gone), keys, off, m, FILTER_TOMBSTONE, phases=PHASES[1])
    assert (out["flags"] & HEAD).all() and np.array_equal(np.diff(off_out.astype(np.int64)), (~gone).astype(np.int64))


# --------------------------------------------------------------------------
# 5. HONU_FILTER_DELETED
# --------------------------------------------------------------------------
def object_column(versions, seed, dead_latest=(), dead_old=(), tail=0):
    """A column of len(versions) objects, object j with versions[j] rows, and
    `tail` invalid rows behind them: (Column, first row of each object). The
    order is a random permutation; the latest record of the objects in
    dead_latest and one older record of those in dead_old are tombstones."""
    rng = np.random.default_rng(seed)
    versions = np.asarray(versions, np.int64)
    v = int(versions.sum())
    n = v + tail
    starts = np.concatenate([[0], np.cumsum(versions)])
    order = rng.permutation(n).astype(np.uint32)
    obj_off = np.full(n + 1, 0x7777777777777777, np.uint64)
    obj_off[:len(starts)] = starts
    latest = np.full(n, 0xDEADBEEF, np.uint32)
    latest[:len(versions)] = order[starts[1:] - 1]
    tomb = np.zeros(n, np.uint8)
    for j in dead_latest:
        tomb[order[starts[j + 1] - 1]] = 1
    for j in dead_old:
        assert versions[j] > 1
        tomb[order[starts[j] + (versions[j] - 1) // 2]] = 1
    return Column(v, n, obj_off, latest, len(versions), tomb, order), starts


def list_of(col, ranges, seed, reverse=False):
    """The list honu_key_list writes for (pos, end) ranges over the column, with info."""
    counts = [max(e - p, 0) for p, e in ranges]
    rows, keys, off = make_list(counts, seed)
    pos = np.concatenate([np.arange(p, e)[::-1] if reverse else np.arange(p, e) for p, e in ranges] or
                         [np.zeros(0, np.int64)]).astype(np.int64)
    rows["pos"] = pos
    rows["record"] = col.order[pos]
    rows["flags"] |= np.where(col.tomb[col.order[pos]] != 0, TOMB, np.uint32(0))
    return rows, keys, off


VERSIONS = [1, 2, 16, 16, 1, 2, 16, 3, 1, 16, 2, 5] * 6  # 72 objects, 486 rows


def deleted_column(tail=0):
    dead_latest = [1, 2, 4, 13, 14, 30, 71]   # objects of 2, 16, 1, 2, 16, 16 and 5 versions
    dead_old = [3, 5, 14, 18, 23]             # 16, 2, 16 (its latest too), 16, 5 versions
    return object_column(VERSIONS, 50, dead_latest, dead_old, tail) + (dead_latest, dead_old)


def test_deleted_objects_go_whole(codec):
    col, starts, dead_latest, dead_old = deleted_column()
    v = col.valid
    s = starts
    ranges = [(0, v),                               # List() over the whole column
              (s[2], s[3]), (s[3], s[4]),           # Versions of a deleted and of a live object with an old tombstone
              (s[2], s[2] + 8),                     # only the older half of a deleted object
              (s[1], s[2]), (s[4], s[5]), (s[0], s[1]),
              (s[14], s[15])]                       # latest and an old version both tombstones
    for reverse, ph in ((False, PHASES[0]), (True, PHASES[1])):
        rows, keys, off = list_of(col, ranges, 51, reverse)
        out, off_out, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, phases=ph, col=col)
        n_out = np.diff(off_out.astype(np.int64))
        gone_rows = sum(VERSIONS[j] for j in dead_latest)
        assert n_out[0] == v - gone_rows
        assert n_out[1] == 0 and n_out[3] == 0 and n_out[4] == 0 and n_out[5] == 0 and n_out[7] == 0
        assert n_out[2] == 16 and (out["flags"][off_out[2]:off_out[3]] & TOMB != 0).sum() == 1  # the old tombstone stays
        assert n_out[6] == 1
        # both flags: the old tombstones of live objects go too
        both, both_off, _ = filter_and_check(codec, rows, keys, off, len(rows), BOTH, phases=ph, col=col)
        assert not (both["flags"] & TOMB).any() and np.diff(both_off.astype(np.int64))[2] == 15
        assert len(both) < len(out)
        # the row's own flag alone: the deleted objects' live history stays
        own, _, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_TOMBSTONE, phases=ph, col=col)
        assert len(own) > len(out)


def test_rows_past_the_valid_count_stay(codec):
    """d_valid below n, rows whose pos is at or past it, and a d_objects above n."""
    col, starts, dead_latest, _ = deleted_column(tail=40)
    assert col.valid + 40 == col.n
    rows, keys, off = list_of(col, [(0, col.valid), (starts[2], starts[3])], 52)
    extra, ekeys, _ = make_list([30], 53)
    extra["range"], extra["flags"] = 1, 0
    extra["pos"] = np.arange(col.valid, col.valid + 30)  # invalid rows of the column: they name no object
    rows, keys = np.concatenate([rows, extra]), np.concatenate([keys, ekeys])
    off = off.copy()
    off[2] += 30
    out, off_out, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, phases=PHASES[2], col=col)
    assert np.diff(off_out.astype(np.int64)).tolist() == [col.valid - sum(VERSIONS[j] for j in dead_latest), 30]
    # valid lowered on the device's side: the rows at or past it stay, whatever their object
    low = Column(starts[2] + 3, col.n, col.obj_off, col.latest, col.objects, col.tomb)
    out2, _, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, phases=PHASES[1], col=low)
    assert len(out2) > len(out)
    # objects above n: clamped to n, the offsets past the objects clamped to valid
    many = Column(col.valid, col.n, col.obj_off, col.latest, col.n + 1000, col.tomb)
    out3, _, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, col=many)
    assert out3.tobytes() == out.tobytes()
    # no object at all, and a column of no rows: every row stays
    none = Column(col.valid, col.n, col.obj_off, col.latest, 0, col.tomb)
    out4, _, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, col=none)
    assert len(out4) == len(rows)
    empty = Column(0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0, np.zeros(0, np.uint8))
    out5, _, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, col=empty)
    assert len(out5) == len(rows)


def test_deleted_over_more_than_one_tile(codec, T):
    """A column of 2 T + 100 rows, 16 versions an object, a third deleted: the whole column listed."""
    objs = (2 * T + 100) // 16 + 1
    versions = [16] * objs
    dead = list(range(0, objs, 3))
    col, starts = object_column(versions, 54, dead, [1, 5])
    rows, keys, off = list_of(col, [(0, col.valid), (5, 5), (starts[3], starts[5])], 55)
    assert 2 * T < len(rows) <= 4 * T + 77
    out, off_out, _ = filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, phases=PHASES[1], col=col)
    assert np.diff(off_out.astype(np.int64)).tolist() == [16 * (objs - len(dead)), 0, 16]


# --------------------------------------------------------------------------
# 6. garbage in device data: wrong rows at most, every index clamped
# --------------------------------------------------------------------------
def garbage_list(col, starts):
    return list_of(col, [(0, col.valid), (starts[2], starts[3]), (starts[5], starts[9])], 60)


def test_pos_at_or_above_n(codec):
    col, starts, _, _ = deleted_column()
    rows, keys, off = garbage_list(col, starts)
    rows["pos"][3::7] = col.n
    rows["pos"][5::11] = 0xFFFFFFFF
    rows["pos"][6::13] = col.n + 12345
    before = expected_filter(rows, keys, off, len(rows), len(rows), BOTH, col)[0]
    out, _, _ = filter_and_check(codec, rows, keys, off, len(rows), BOTH, phases=PHASES[1], col=col)
    assert (out["pos"] >= col.n).sum() == (rows["pos"][(rows["flags"] & TOMB) == 0] >= col.n).sum() > 20
    assert out.tobytes() == before.tobytes()


def test_range_at_or_above_m(codec):
    col, starts, _, _ = deleted_column()
    rows, keys, off = garbage_list(col, starts)
    rows["range"][2::5] = 3
    rows["range"][4::9] = 0xFFFFFFFF
    out, _, _ = filter_and_check(codec, rows, keys, off, len(rows), BOTH, phases=PHASES[2], col=col, wellformed=False)
    assert (out["range"] >= 3).sum() > 20  # the field comes out as it went in


def test_non_monotone_range_off(codec, T):
    n = 2 * T + 77
    rows, keys, off = make_list(split(n, 40, 61), 61)
    rng = np.random.default_rng(62)
    bad = off.copy()
    bad[1:-1] = rng.permutation(bad[1:-1])
    bad[5], bad[9], bad[-1] = (1 << 64) - 1, n + 1, 3  # past the rows; entry m is the kept count whatever it holds
    gone = removed("half", n, T, 63)
    out, off_out, _ = filter_and_check(codec, flag_rows(rows, gone), keys, bad, n, FILTER_TOMBSTONE, phases=PHASES[1],
                                       wellformed=False)
    assert off_out[5] == off_out[9] == off_out[-1] == len(out) and (np.diff(off_out.astype(np.int64)) < 0).any()


def test_latest_at_or_above_n(codec):
    """A d_latest value that is not below n reads info row n - 1."""
    col, starts, _, _ = deleted_column()
    rows, keys, off = garbage_list(col, starts)
    outs = []
    for last in (0, 1):
        lat = col.latest.copy()
        lat[0::3] = col.n
        lat[1::3] = 0xFFFFFFFF
        tomb = col.tomb.copy()
        tomb[col.n - 1] = last
        c = Column(col.valid, col.n, col.obj_off, lat, col.objects, tomb)
        outs.append(filter_and_check(codec, rows, keys, off, len(rows), FILTER_DELETED, phases=PHASES[last], col=c)[0])
    assert len(outs[1]) < len(outs[0])  # two thirds of the objects are judged by the last info row


def test_non_monotone_obj_off(codec):
    """Offsets in no order, some past the rows: which object a row is judged by
    is then whatever the search ends on, so the kept rows are read back from
    the call and everything else must follow from them; a row at or past
    valid stays, and so does every row when no record is a tombstone."""
    col, starts, _, _ = deleted_column(tail=9)
    rows, keys, off = garbage_list(col, starts)
    rows["pos"][7::17] = col.valid + 2
    rows["record"] = np.arange(len(rows)) + 5000  # a number of its own per row (the ranges overlap): which rows were kept
    rng = np.random.default_rng(64)
    bad = col.obj_off.copy()
    bad[1:col.objects] = rng.permutation(bad[1:col.objects])
    bad[4], bad[11], bad[20] = (1 << 64) - 1, col.n + 7, 0
    tomb = col.tomb.copy()
    tomb[::2] = 1
    w = len(rows)
    for t in (tomb, np.zeros(col.n, np.uint8)):
        c = Column(col.valid, col.n, bad, col.latest, col.objects, t)

        def body(fill):
            call = Call(codec, rows, keys, off, w, w, fill, PHASES[1], c)
            assert call.run(FILTER_DELETED) == 0
            keep = np.isin(rows["record"], call.kept_records())
            assert keep[rows["pos"] >= c.valid].all()
            if not t.any():
                assert keep.all()
            call.check(from_keep(rows, keys, off, w, keep))

        guards.twice(body)


# --------------------------------------------------------------------------
# 7. scan bound, 8. refusals
# --------------------------------------------------------------------------
def test_cap_beyond_the_contexts_scan_is_refused(T):
    """The tiles' counts go through the context's scan, whose state covers
    max_records rows: a context of R records takes cap = R T and refuses R T + 1."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    R = 2
    small = hobj.Codec(0, R)
    try:
        assert int(small.lib.honu_ctx_max_records(small.ctx)) == R
        rows, keys, off = make_list(split(R * T, 5, 70), 70, extra=1)
        rows = flag_rows(rows, removed("half", R * T, T, 71))
        filter_and_check(small, rows, keys, off, R * T, FILTER_TOMBSTONE, cap=R * T, phases=PHASES[1])

        def body(fill):
            c = Call(small, rows, keys, off, R * T, R * T + 1, fill)
            assert c.run(FILTER_TOMBSTONE) == E_WORKSPACE
            c.nothing_stored()

        guards.twice(body)
    finally:
        small.close()


def test_refusals_store_nothing(codec):
    col, starts, _, _ = deleted_column()
    rows, keys, off = garbage_list(col, starts)
    w = len(rows)
    want = expected_filter(rows, keys, off, w, w, BOTH, col)

    def body(fill):
        c = Call(codec, rows, keys, off, w, w, fill, (1, 3), col)
        a = c.args()
        for kw in (dict(cap=1 << 32), dict(m=1 << 32), dict(n=1 << 32), dict(cap=(1 << 64) - 1), dict(m=(1 << 64) - 1),
                   dict(n=(1 << 64) - 1), dict(cap=MAX_RECORDS * 1024 + 1)):
            assert c.run(BOTH, **kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(rows=0), dict(rows_out=0), dict(range_off=0), dict(total=0),
                   dict(range_off_out=0), dict(total_out=0),
                   dict(valid=0), dict(obj_off=0), dict(latest=0), dict(objects=0), dict(info=0),
                   dict(keys=0), dict(keys_out=0),
                   dict(flags=4), dict(flags=BOTH | 4), dict(flags=1 << 31),
                   dict(work_bytes=c.work_bytes - 1), dict(work_bytes=0), dict(work=0), dict(work=a["work"] + 128),
                   dict(rows_out=a["rows"]), dict(range_off_out=a["range_off"]), dict(total_out=a["total"]),
                   dict(keys_out=a["keys"]),
                   dict(rows=a["rows"] + 8), dict(rows=a["rows"] + 4), dict(rows_out=a["rows_out"] + 8),
                   dict(range_off=a["range_off"] + 4), dict(total=a["total"] + 4), dict(valid=a["valid"] + 4),
                   dict(obj_off=a["obj_off"] + 4), dict(objects=a["objects"] + 4), dict(info=a["info"] + 4),
                   dict(latest=a["latest"] + 2), dict(range_off_out=a["range_off_out"] + 4),
                   dict(total_out=a["total_out"] + 4)):
            kw.setdefault("flags", BOTH)
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run(BOTH) == 0  # and the arguments were good
        c.check(want)
        # what HONU_FILTER_TOMBSTONE alone does not need may be NULL (it keeps the rows BOTH kept, and more)
        assert c.run(FILTER_TOMBSTONE, valid=0, obj_off=0, latest=0, objects=0, info=0, n=0) == 0
        c.check(expected_filter(rows, keys, off, w, w, FILTER_TOMBSTONE))

    guards.twice(body)


# --------------------------------------------------------------------------
# 9. graph
# --------------------------------------------------------------------------
def test_graph_replays_after_the_inputs_changed(codec, T):
    """Replays after d_total, a row's flags and an info tombstone byte were changed on the device."""
    objs = (T + 200) // 16
    versions = [16] * objs
    col, starts = object_column(versions, 80, [2, 7], [4])
    rows, keys, off = list_of(col, [(0, col.valid), (starts[2], starts[3]), (starts[6], starts[9])], 81)
    cap = len(rows)
    assert cap > T
    dev = codec.torch_device
    # round 2: fewer rows, a live row flagged, and another object's latest record a tombstone
    rows2, tomb2 = rows.copy(), col.tomb.copy()
    rows2["flags"][starts[5] + 3] |= TOMB
    tomb2[col.latest[9]] = 1
    col2 = Column(col.valid, col.n, col.obj_off, col.latest, col.objects, tomb2)
    rounds = [(rows, cap, col), (rows2, cap - 40, col2)]

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        c = Call(codec, rows, keys, off, cap, cap, fill, (3, 1), col)
        assert c.run(BOTH) == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run(BOTH) == 0
        kept = []
        for r, total, cl in rounds:
            for t in c.outs:
                refill(t, fill)
            c.dev["rows"].copy_(torch.from_numpy(r.view(np.uint8).copy()).to(dev))
            c.dev["total"].copy_(torch.from_numpy(u64(total).view(np.uint8)).to(dev))
            c.dev["info"].copy_(torch.from_numpy(cl.info().view(np.uint8).copy()).to(dev))
            c.host["rows"], c.host["total"], c.host["info"] = r, u64(total), cl.info()
            g.replay()
            want = expected_filter(r, keys, off, total, cap, BOTH, cl)
            c.check(want)
            kept.append(len(want[0]))
        assert 0 < kept[1] < kept[0] - 17  # an object's 16 rows, the flagged row and kept rows past the total went

    guards.twice(body)


# --------------------------------------------------------------------------
# 10. the chain: seek -> list -> filter -> fetch -> decode with nothing read on the host
# --------------------------------------------------------------------------
def chain_batch(n, objects=23):
    """(host batch, tombstones, one record index per object): generator Small
    records of `objects` objects; every fifth record has no data, which is
    what Object.Tombstone() asks (object.go:103-112)."""
    rng = np.random.default_rng(100)
    oids = rng.integers(0, 256, (objects, 16), dtype=np.uint8)
    hb = gen_host_batch(101, "small", 0, n)
    which = rng.integers(0, objects, n)
    hb.meta["object_id"] = oids[which]
    hb.meta["vid"] = rng.permutation(n) + 1  # no two versions alike: every key once
    hb.meta["pid"] = rng.integers(1, 4, n)
    dead = np.arange(n) % 5 == 3
    hb.meta["tombstone"] = dead & ((hb.meta["present"] & HAS_VERSION) != 0)
    lens = np.diff(hb.payload_off.astype(np.int64))
    payload = hb.payload[:int(hb.payload_off[n])][np.repeat(~dead, lens)]
    lens[dead] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    hb = type(hb)(hb.meta, hb.var, hb.acl, hb.regions, payload, off)
    first = [int(np.flatnonzero(which == j)[0]) for j in range(objects) if (which == j).any()]
    return hb, dead, first


def test_seek_list_filter_fetch_decode_chain(codec):
    n = 200
    hb, dead, first = chain_batch(n)
    enc = codec.marshal(hobj.DeviceBatch.from_host(hb, codec.torch_device))
    rec_bytes = int(enc.out_off.view(torch.int64)[n].item())
    d1 = codec.decode(enc.out, enc.out_off, n, rec_bytes=rec_bytes)
    dk, dst = codec.keys(d1)
    order, col, valid = codec.sort_keys(dk[:29 * n], dst[:4 * n], n=n, want_sorted=True)
    obj_off, latest, objects = codec.key_objects(dk[:29 * n], order, valid)
    ipick = torch.tensor(first, device=codec.torch_device)
    probes = dk[:29 * n].view(n, 29)[ipick].reshape(-1).contiguous()
    pstatus = dst[:4 * n].view(torch.int32)[ipick].contiguous().view(torch.uint8)
    m, cap = len(first), n
    # nothing is read on the host from here ...
    seeks = codec.seek_keys(col[:29 * n], valid, probes, 17, probe_status=pstatus, order=order, info=d1.info)
    # Retrieve of every object: its latest version, "not found" when that is a tombstone
    rows, range_off, total, lkeys = codec.list_keys(col[:29 * n], order, valid, seeks, cap, limit=1, reverse=True,
                                                    info=d1.info, want_keys=True)
    frows, foff, ftotal, fkeys = codec.filter_rows(rows, range_off, total, cap, tombstones=True, keys=lkeys)
    values, val_off, val_total, status = codec.fetch_objects(frows, ftotal, cap, enc.out, enc.out_off, n, rec_bytes,
                                                             rec_bytes)
    d2 = codec.decode(values, val_off, cap, rec_bytes=rec_bytes)
    # Versions of every object, most recent first: a deleted object has none
    vrows, voff, vtotal, _ = codec.list_keys(col[:29 * n], order, valid, seeks, cap, reverse=True, info=d1.info)
    drows, doff, dtotal, _ = codec.filter_rows(vrows, voff, vtotal, cap,
                                               deleted=(valid, n, obj_off, latest, objects, d1.info))
    # ... to here
    torch.cuda.synchronize()
    # the composition on the host
    sorted_keys = [bytes(r) for r in col[:29 * n].cpu().numpy().reshape(n, 29)]
    host_order = order.cpu().numpy().view(np.uint32).tolist()
    assert int(valid.item()) == n and len(set(sorted_keys)) == n
    host_probes = probes.cpu().numpy().reshape(m, 29)
    ranges = [hkeys.seek(sorted_keys, bytes(p[:17])) for p in host_probes]
    tomb = lambda r: bool(dead[r])  # noqa: E731
    retrieve = hkeys.filter(sorted_keys, hkeys.scan(sorted_keys, ranges, reverse=True, limit=1), tomb, host_order)
    versions = hkeys.filter(sorted_keys, hkeys.scan(sorted_keys, ranges, reverse=True), tomb, host_order, deleted=True)
    off1 = hobj._to_host(enc.out_off, 8 * (n + 1), np.uint64).astype(np.int64)
    arena1 = hobj._to_host(enc.out, rec_bytes, np.uint8)
    records = [arena1[off1[i]:off1[i + 1]].tobytes() for i in range(n)]
    fetched = hkeys.fetch(records, retrieve, host_order)

    t = int(ftotal.item())
    got = frows.cpu().numpy().view(np.uint32)[:t]
    assert [(int(q), int(p)) for q, p in got[:, :2]] == retrieve and 5 < t < m
    assert (got[:, 3] == LIST_ROW_HEAD).all()  # each the first of its range, none a tombstone
    assert fkeys.cpu().numpy()[:29 * t].tobytes() == b"".join(sorted_keys[p] for _, p in retrieve)
    fo = foff.cpu().numpy()
    found = {q for q, _ in retrieve}
    gone = [q for q in range(m) if q not in found]
    assert len(gone) >= 2 and all(fo[q + 1] == fo[q] for q in gone) and all(fo[q + 1] == fo[q] + 1 for q in found)
    assert fo[m] == t
    # no empty record reaches the decoder, and the arena is the host's fetch
    off2 = val_off.cpu().numpy()
    assert (np.diff(off2)[:t] > 0).all() and (off2[t:] == off2[t]).all() and int(val_total.item()) == off2[t]
    assert (status.cpu().numpy()[:t] == OK).all()
    assert hobj._to_host(values, int(off2[t]), np.uint8).tobytes() == b"".join(fetched)
    meta1, info1, _, _, _, _ = d1.host()
    meta2, info2, _, _, _, _ = d2.host()
    r = got[:, 2].astype(np.int64)
    assert (info2["tombstone"][:t] == 0).all() and (info2["meta_status"][:t] == OK).all()
    assert np.array_equal(meta2["object_id"][:t], meta1["object_id"][r])
    assert np.array_equal(meta2["vid"][:t], meta1["vid"][r]) and np.array_equal(info2["data_len"][:t],
                                                                               info1["data_len"][r])
    # Versions: the deleted objects' ranges are empty, the others whole, their old tombstones included
    td = int(dtotal.item())
    gotd = drows.cpu().numpy().view(np.uint32)[:td]
    assert [(int(q), int(p)) for q, p in gotd[:, :2]] == versions and td < int(vtotal.item())
    do = doff.cpu().numpy()
    assert all(do[q + 1] == do[q] for q in gone) and do[m] == td
    assert all(do[q + 1] - do[q] == ranges[q][1] - ranges[q][0] for q in found)
    assert (gotd[:, 3] & LIST_ROW_TOMBSTONE).any()
