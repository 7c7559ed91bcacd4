"""honu_key_list on the GPU against numpy.

The expectation is numpy's alone: per range the positions arange(pos', end')
(or, with HONU_LIST_LATEST, the last rows of the objects that lie in the
range), reversed and cut at `limit` as asked, concatenated in range order. It
never calls the library. Every input and output is a guarded view
(tests/guards.py) under both fills, the column and d_keys_out at byte phases
0, 1 and 3; the write set is exactly d_range_off[0, m + 1), d_total[0],
d_rows[0, w) and d_keys_out[0, 29 w), w = min(total, cap), and the inputs are
unchanged. Sizes are in units of the tile T and the stage S, the params
"list_tile" and "list_stage".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (HAS_VERSION, INFO_DTYPE, LIST_LATEST, LIST_REVERSE, LIST_ROW_DTYPE,  # noqa: E402
                               LIST_ROW_HEAD, LIST_ROW_TOMBSTONE, SEEK_DTYPE, SEEK_FOUND, SEEK_NONE, SEEK_SKIPPED)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
PHASES = ((0, 0), (1, 3), (3, 1), (0, 3))  # (the column, d_keys_out)


def _param(c, name):
    v = L.C.c_int64(0)
    L.check(c.lib.honu_ctx_get_param(c.ctx, name, L.C.byref(v)), name.decode())
    return int(v.value)


@pytest.fixture(scope="module")
def sizes():
    """(T, S): read from a context of one record."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 1)
    try:
        T, S = _param(c, b"list_tile"), _param(c, b"list_stage")
    finally:
        c.close()
    assert T >= 128 and S >= 64
    return T, S


@pytest.fixture(scope="module")
def codec(sizes):
    T, S = sizes
    c = hobj.Codec(0, 2 * S + 4 * T)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(sizes):
    return sizes[0]


@pytest.fixture(scope="module")
def S(sizes):
    return sizes[1]


# --------------------------------------------------------------------------
# expectations
# --------------------------------------------------------------------------
def seek_rows(pairs, flags=SEEK_FOUND):
    """honu_seek rows with the given (pos, end); first and latest hold a value no test expects back."""
    r = np.zeros(len(pairs), SEEK_DTYPE)
    if len(pairs):
        p = np.asarray(pairs, np.int64).reshape(-1, 2)
        r["pos"], r["end"] = p[:, 0], p[:, 1]
    r["first"], r["latest"], r["flags"] = 0xDEADBEEF, 0xFEEDF00D, flags
    return r


def expected_list(S, valid, ranges, limit=0, flags=0, order=None, tomb=None, latest=None):
    """(rows as LIST_ROW_DTYPE, range_off uint64[m + 1], keys (total, 29))."""
    n = len(S)
    v = min(int(valid), n)
    last = None
    if flags & LIST_LATEST:
        off, objects = latest
        objects = min(int(objects), n)
        last = np.minimum(off[1:objects + 1], np.uint64(v)).astype(np.int64) - 1
    parts, counts = [], []
    for r in ranges:
        end = min(int(r["end"]), v)
        pos = min(int(r["pos"]), end)
        if int(r["flags"]) & SEEK_SKIPPED:
            pos = end = 0
        p = np.arange(pos, end, dtype=np.int64) if last is None else last[(last >= pos) & (last < end)]
        if flags & LIST_REVERSE:
            p = p[::-1]
        if limit:
            p = p[:limit]
        parts.append(p)
        counts.append(len(p))
    range_off = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.uint64)
    total = int(range_off[-1])
    pos = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    rows = np.zeros(total, LIST_ROW_DTYPE)
    rows["range"] = np.repeat(np.arange(len(ranges)), counts) if total else 0
    rows["pos"] = pos
    rows["record"] = SEEK_NONE if order is None else order[pos]
    head = np.zeros(total, bool)
    head[range_off[:-1][np.asarray(counts, np.int64) > 0].astype(np.int64)] = True
    rows["flags"] = np.where(head, LIST_ROW_HEAD, 0)
    if tomb is not None:
        rec = np.minimum(order[pos].astype(np.int64), n - 1)
        rows["flags"] |= np.where(tomb[rec] != 0, LIST_ROW_TOMBSTONE, 0).astype(np.uint32)
    return rows, range_off, S[pos]


def objects_of(S, valid):
    """What honu_key_objects writes for a sorted column: (offsets uint64[n + 1]
    of which objects + 1 are set, the rest a value no test expects read, objects)."""
    n, v = len(S), min(int(valid), len(S))
    cut = np.flatnonzero((S[1:v, :17] != S[:v - 1, :17]).any(axis=1)) + 1 if v > 1 else np.zeros(0, np.int64)
    starts = np.concatenate([[0], cut]) if v else np.zeros(0, np.int64)
    off = np.full(n + 1, 0x7777777777777777, np.uint64)
    off[:len(starts)] = starts
    off[len(starts)] = v
    return off, len(starts)


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
    """The guarded device arguments of one list."""

    def __init__(self, codec, S, valid, ranges, cap, fill, phases=(0, 0), order=None, tomb=None, latest=None):
        self.codec, self.n, self.m, self.cap = codec, len(S), len(ranges), int(cap)
        self.host = {"s": S, "v": u64(valid), "r": ranges}
        if order is not None:
            self.host["o"] = order
        if tomb is not None:
            info = np.zeros(self.n, INFO_DTYPE)
            info["tombstone"] = tomb
            info["data_off"], info["data_len"] = 0x0102030405060708, 0x1112131415161718
            self.host["i"] = info
        if latest is not None:
            self.host["f"], self.host["j"] = latest[0], u64(latest[1])
        self.dev = {k: put(codec, a, phases[0] if k == "s" else 0, fill) for k, a in self.host.items()}
        dev = codec.torch_device
        self.range_off = guards.guarded(8 * (self.m + 1), fill=fill, device=dev)
        self.rows = guards.guarded(16 * self.cap, fill=fill, device=dev)
        self.keys = guards.guarded(29 * self.cap, phase=phases[1], fill=fill, device=dev)
        self.total = guards.guarded(8, fill=fill, device=dev)
        self.outs = (self.range_off, self.rows, self.keys, self.total)

    def args(self, limit=0, flags=0, with_rows=True, with_keys=True, **kw):
        A = guards.address
        d = self.dev
        x = dict(ctx=self.codec.ctx, s=A(d["s"]), o=A(d.get("o")), v=A(d["v"]), n=self.n, r=A(d["r"]), m=self.m,
                 limit=limit, flags=flags, f=A(d.get("f")), j=A(d.get("j")), i=A(d.get("i")),
                 range_off=A(self.range_off), rows=A(self.rows) if with_rows else 0,
                 keys=A(self.keys) if with_keys else 0, cap=self.cap, total=A(self.total))
        x.update(kw)
        return x

    def run(self, limit=0, flags=0, **kw):
        x = self.args(limit, flags, **kw)
        return self.codec.lib.honu_key_list(
            x["ctx"], x["s"], x["o"], x["v"], x["n"], x["r"], x["m"], x["limit"], x["flags"], x["f"], x["j"], x["i"],
            x["range_off"], x["rows"], x["keys"], x["cap"], x["total"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs:
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def check(self, want, with_rows=True, with_keys=True):
        """The outputs against (rows, range_off, keys) and the write set."""
        torch.cuda.synchronize()
        rows, range_off, keys = want
        total = len(rows)
        w = min(total, self.cap)
        got_total = int(guards.block_of(self.total).bytes().view(np.uint64)[0])
        assert got_total == total, (got_total, total)
        got = guards.block_of(self.range_off).bytes().view(np.uint64)
        bad = np.flatnonzero(got != range_off)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], range_off[bad[:4]])
        if with_rows:
            got = guards.block_of(self.rows).bytes()[:16 * w].view(np.uint32).reshape(w, 4)
            exp = rows[:w].view(np.uint32).reshape(w, 4)
            bad = np.flatnonzero((got != exp).any(axis=1))
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], exp[bad[:4]])
        if with_keys and with_rows:
            got = guards.block_of(self.keys).bytes()[:29 * w].reshape(w, 29)
            bad = np.flatnonzero((got != keys[:w]).any(axis=1))
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], keys[bad[:4]])
        guards.assert_untouched(self.range_off, [(0, 8 * (self.m + 1))])
        guards.assert_untouched(self.total, [(0, 8)])
        guards.assert_untouched(self.rows, [(0, 16 * w)] if with_rows else [])
        guards.assert_untouched(self.keys, [(0, 29 * w)] if with_keys and with_rows else [])
        self.inputs_unchanged()


def list_and_check(codec, S, valid, ranges, cap=None, limit=0, flags=0, phases=(0, 0), order=None, tomb=None,
                   latest=None, **how):
    """One call under both fills against numpy; cap None: total + 3."""
    want = expected_list(S, valid, ranges, limit, flags, order, tomb, latest)
    cap = len(want[0]) + 3 if cap is None else cap

    def body(fill):
        c = Call(codec, S, valid, ranges, cap, fill, phases, order, tomb, latest)
        assert c.run(limit, flags, **how) == 0
        c.check(want, how.get("with_rows", True), how.get("with_keys", True))

    guards.twice(body)
    return want


# --------------------------------------------------------------------------
# columns
# --------------------------------------------------------------------------
def random_keys(n, rng):
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def column(n, seed):
    """(rows, order, tombstones): the list reads the column's bytes and the
    order's values as they are, so any will do: random rows, a random
    permutation, about a third of the records tombstones."""
    rng = np.random.default_rng(seed)
    return random_keys(n, rng), rng.permutation(n).astype(np.uint32), (rng.integers(0, 3, n) == 0).astype(np.uint8)


def object_column(versions, seed):
    """A sorted column of len(versions) objects, object j with versions[j] versions."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 256, (len(versions), 16), dtype=np.uint8)
    rows = []
    for oid, c in zip(ids, versions):
        for v in range(c):
            rows.append(b"\x01" + oid.tobytes() + int(v + 1).to_bytes(8, "big") + int(1 + v % 3).to_bytes(4, "big"))
    rows.sort()
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 29).copy()


def numpy_seek(S, valid, probes, probe_len):
    """(pos, end) of each probe's first probe_len bytes over rows [0, valid), by the host statement keys.seek."""
    rows = [r.tobytes() for r in S[:valid]]
    return [hkeys.seek(rows, p[:probe_len].tobytes()) for p in probes]


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", (False, True))
def test_one_range_cut_by_tiles(codec, T, reverse):
    """One range over a column of 3 T + 5 rows: the tiles are cut inside it."""
    n = 3 * T + 5
    S_, order, tomb = column(n, 1)
    for j, ph in enumerate(PHASES[:3]):
        rows, off, _ = list_and_check(codec, S_, n, seek_rows([(0, n)]), flags=LIST_REVERSE if reverse else 0,
                                      phases=ph, order=order, tomb=tomb)
        assert len(rows) == n and rows["pos"][0] == (n - 1 if reverse else 0)
        assert (rows["flags"] & LIST_ROW_HEAD).sum() == 1


def test_many_ranges_in_one_tile(codec, T):
    """2 T + 3 ranges of one row each: a tile's slice is T + 1 ranges, staged."""
    n = 3 * T
    S_, order, tomb = column(n, 2)
    rng = np.random.default_rng(20)
    pos = rng.integers(0, n, 2 * T + 3)
    rows, off, _ = list_and_check(codec, S_, n, seek_rows(np.stack([pos, pos + 1], 1)), phases=PHASES[1], order=order,
                                  tomb=tomb)
    assert len(rows) == 2 * T + 3 and (rows["flags"] & LIST_ROW_HEAD).all()


@pytest.mark.parametrize("reverse", (False, True))
def test_range_ends_beside_wave_and_tile_boundaries(codec, T, reverse):
    n = 2 * T + 9
    S_, order, tomb = column(n, 3)
    lengths = [0, 1, 63, 64, 65, T - 1, T, T + 1]
    for j, shift in enumerate((0, 1)):  # the same lengths one output row later
        pairs = [(0, shift)] + [(7 * i, 7 * i + c) for i, c in enumerate(lengths)]
        rows, off, _ = list_and_check(codec, S_, n, seek_rows(pairs), flags=LIST_REVERSE if reverse else 0,
                                      phases=PHASES[2 + j], order=order, tomb=tomb)
        assert len(rows) == sum(lengths) + shift


@pytest.mark.parametrize("empties", ("S-2", "S-1", "S+7"))
def test_run_of_empty_ranges(codec, T, S, empties):
    """Two non-empty ranges in one output tile with a run of empty ranges
    between them: a slice of S entries is the longest that is staged, one of S
    + 1 and one of S + 9 are searched in global memory. Then the run at the
    very start and the very end of the list."""
    e = {"S-2": S - 2, "S-1": S - 1, "S+7": S + 7}[empties]
    n = 2 * T
    S_, order, tomb = column(n, 4)
    empty = [(5, 5), (9, 3), (n + 4, n + 9)]  # three ways to be empty
    run = [empty[i % 3] for i in range(e)]
    rows, off, _ = list_and_check(codec, S_, n, seek_rows([(3, 40)] + run + [(100, 170)]), phases=PHASES[1],
                                  order=order, tomb=tomb)
    assert len(rows) == 37 + 70 < T and off[1] == off[e + 1] == 37
    rows, off, _ = list_and_check(codec, S_, n, seek_rows(run + [(3, 40), (T, 2 * T + 9), (0, 2)] + run),
                                  flags=LIST_REVERSE, phases=PHASES[2], order=order, tomb=tomb)
    assert len(rows) == 37 + T + 2 and off[e] == 0 and off[-1] == off[e + 3]
    # and a run that spans a tile boundary of the output: T - 1 rows before it, T + 1 after
    list_and_check(codec, S_, n, seek_rows([(1, T)] + run + [(0, T + 1)]), order=order)


@pytest.mark.parametrize("m", [4097, 4225])
def test_tile_ends_searched_over_a_long_list(codec, T, m):
    """m ranges, all empty but every 64th (40 rows each): some 2600 output rows
    in three tiles, each tile's two wave searches over all m offsets, a bracket
    of more than 4096 (and, at 4225, above the 4160 from which the search
    takes a third step)."""
    n = 2 * T
    S_, order, tomb = column(n, 6)
    empty = [(5, 5), (9, 3), (n + 4, n + 9)]
    pairs = [(7 * i % (n - 40), 7 * i % (n - 40) + 40) if i % 64 == 1 else empty[i % 3] for i in range(m)]
    for flags, ph in ((0, PHASES[1]), (LIST_REVERSE, PHASES[2])):
        rows, off, _ = list_and_check(codec, S_, n, seek_rows(pairs), flags=flags, phases=ph, order=order, tomb=tomb)
        assert len(rows) == 40 * len(range(1, m, 64)) > 2 * T and off[-1] == len(rows)
        assert (rows["flags"] & LIST_ROW_HEAD).sum() == len(range(1, m, 64))


def test_overlapping_repeated_out_of_order_and_clamped(codec, T):
    n = T + 77
    S_, order, tomb = column(n, 5)
    v = n - 20
    good = [(50, 90), (0, v), (50, 90), (10, 60), (v - 5, v), (0, v), (30, 31)]
    beyond = [(v - 3, v + 9), (v, n), (v + 2, n + 5), (n, n + 1), (0xFFFFFFF0, 0xFFFFFFFF), (10, 0xFFFFFFFF), (70, 12)]
    ranges = seek_rows(good + beyond + good[::-1])
    skipped = seek_rows([(0xFFFFFFFF, 0xFFFFFFFF), (3, 0xDEADBEEF), (0, v)], flags=SEEK_SKIPPED | SEEK_FOUND)
    ranges = np.concatenate([ranges[:5], skipped, ranges[5:]])
    ranges["flags"][::3] |= 0xFFFFFFC0 | SEEK_FOUND  # no other flag bit is trusted
    ranges["flags"][1::3] = 0
    skipped_at = [5, 6, 7]
    ranges["flags"][skipped_at] |= SEEK_SKIPPED
    for reverse in (0, LIST_REVERSE):
        rows, off, _ = list_and_check(codec, S_, v, ranges, flags=reverse, phases=PHASES[1], order=order, tomb=tomb)
        assert len(rows) > 4 * n // 2 and len(rows) > n  # more rows than the column has
        assert (off[np.array(skipped_at) + 1] == off[skipped_at]).all()
        assert rows["pos"].max() == v - 1
    # d_valid above n is n; d_valid 0 empties every range
    rows, _, _ = list_and_check(codec, S_, n + 1000, ranges, order=order, tomb=tomb)
    assert rows["pos"].max() == n - 1
    rows, _, _ = list_and_check(codec, S_, (1 << 64) - 1, ranges, flags=LIST_REVERSE, order=order)
    assert rows["pos"].max() == n - 1
    rows, off, _ = list_and_check(codec, S_, 0, ranges, order=order, tomb=tomb)
    assert len(rows) == 0 and not off.any()


@pytest.mark.parametrize("limit", (1, 2, "T", "above"))
def test_limit_and_head(codec, T, limit):
    n = 2 * T + 50
    S_, order, tomb = column(n, 6)
    pairs = [(0, n), (4, 4), (10, 11), (20, 22), (30, 33), (0, T), (7, T + 8), (1, T + 3), (n - 1, n), (n, n)]
    limit = {"T": T, "above": n + 1}.get(limit, limit)
    for reverse in (0, LIST_REVERSE):
        rows, off, _ = list_and_check(codec, S_, n, seek_rows(pairs), limit=limit, flags=reverse, phases=PHASES[3],
                                      order=order, tomb=tomb)
        counts = np.diff(off.astype(np.int64))
        assert counts.tolist() == [min(b - a, limit) for a, b in pairs]
        # HEAD exactly on each non-empty range's first emitted row
        head = np.flatnonzero(rows["flags"] & LIST_ROW_HEAD)
        assert head.tolist() == [int(o) for o, c in zip(off[:-1], counts) if c]
        firsts = [(b - 1 if reverse else a) for (a, b), c in zip(pairs, counts) if c]
        assert rows["pos"][head].tolist() == firsts
    if limit == 1:  # Retrieve: the row at end - 1
        assert rows["pos"].tolist() == [b - 1 for a, b in pairs if b > a]


def test_cap(codec, T):
    """Rows at or past min(total, cap) keep their poison; d_total is the full need every time."""
    n = T + 300
    S_, order, tomb = column(n, 7)
    ranges = seek_rows([(0, n), (5, 5), (100, 400), (0, 17)])
    total = n + 300 + 17
    for cap, how in ((0, dict(with_rows=False, with_keys=False)), (0, dict(with_rows=False)), (0, {}), (1, {}),
                     (total - 1, {}), (total, {}), (total + T, {}), (total - T - 1, dict(with_keys=False))):
        rows, off, _ = list_and_check(codec, S_, n, ranges, cap=cap, phases=PHASES[1], order=order, tomb=tomb, **how)
        assert len(rows) == total and off[-1] == total


VERSIONS = (1, 2, 16, "T+1", 2, 1, 16, 1)


@pytest.fixture(scope="module")
def objects(T):
    """(column, offsets, object count): objects of 1, 2, 16 and T + 1 versions."""
    S_ = object_column([T + 1 if c == "T+1" else c for c in VERSIONS], 8)
    off, count = objects_of(S_, len(S_))
    assert count == len(VERSIONS) and sorted(np.diff(off[:count + 1].astype(np.int64)).tolist()) == sorted(
        T + 1 if c == "T+1" else c for c in VERSIONS)
    return S_, off, count


def test_latest_whole_column_and_object_ranges(codec, T, objects):
    S_, off, count = objects
    n = len(S_)
    order = np.random.default_rng(80).permutation(n).astype(np.uint32)
    tomb = (np.arange(n) % 3 == 0).astype(np.uint8)  # record r a tombstone when r % 3 == 0
    last = off[1:count + 1].astype(np.int64) - 1
    for reverse in (0, LIST_REVERSE):
        rows, _, _ = list_and_check(codec, S_, n, seek_rows([(0, n)]), flags=LIST_LATEST | reverse, phases=PHASES[1],
                                    order=order, tomb=tomb, latest=(off, count))
        assert rows["pos"].tolist() == (last[::-1] if reverse else last).tolist()
    rows, _, _ = list_and_check(codec, S_, n, seek_rows([(0, n), (0, n)]), limit=1, flags=LIST_LATEST | LIST_REVERSE,
                                order=order, latest=(off, count))
    assert rows["pos"].tolist() == [n - 1, n - 1]
    # per-object ranges, as honu_key_seek gives them at probe_len 17 (checked against the host statement)
    dS, dv = put(codec, S_, 0, 0), put(codec, u64(n), 0, 0)
    probes = S_[off[:count].astype(np.int64)]
    got = codec.seek_keys(dS, dv, put(codec, probes, 0, 0), 17).cpu().numpy().view(np.uint32)
    pairs = numpy_seek(S_, n, probes, 17)
    assert got[:, :2].tolist() == [list(p) for p in pairs] == [[int(off[j]), int(off[j + 1])] for j in range(count)]
    ranges = np.zeros(count, SEEK_DTYPE)
    ranges.view(np.uint32).reshape(count, 5)[:] = got
    for limit, reverse in ((0, 0), (1, LIST_REVERSE), (1, 0)):
        rows, _, _ = list_and_check(codec, S_, n, ranges, limit=limit, flags=LIST_LATEST | reverse, phases=PHASES[2],
                                    order=order, tomb=tomb, latest=(off, count))
        assert rows["pos"].tolist() == last.tolist() and rows["range"].tolist() == list(range(count))
    # a range that ends inside an object omits that object; one that starts inside it keeps it
    big = int(np.argmax(np.diff(off[:count + 1].astype(np.int64))))
    cut = seek_rows([(0, int(off[big]) + 5), (int(off[big]) + 5, n), (int(off[big]) + 1, int(off[big + 1]) - 1),
                     (int(off[big + 1]) - 1, int(off[big + 1]))])
    for reverse in (0, LIST_REVERSE):
        rows, o, _ = list_and_check(codec, S_, n, cut, flags=LIST_LATEST | reverse, order=order, latest=(off, count))
        assert np.diff(o.astype(np.int64)).tolist() == [big, count - big, 0, 1]
    # a probe_len 29 range: empty on a row that is not its object's last, one row on one that is
    whole = np.stack([S_[int(off[big]) + 3], S_[int(off[big + 1]) - 1], S_[int(off[2 if big != 2 else 3])]])
    pairs = numpy_seek(S_, n, whole, 29)
    rows, o, _ = list_and_check(codec, S_, n, seek_rows(pairs), flags=LIST_LATEST, order=order, latest=(off, count))
    assert np.diff(o.astype(np.int64))[:2].tolist() == [0, 1] and rows["pos"][0] == int(off[big + 1]) - 1
    # a lower valid count cuts the last object short: its last valid row is its latest
    v = n - 3
    off_v, count_v = objects_of(S_, v)
    rows, _, _ = list_and_check(codec, S_, v, seek_rows([(0, n)]), flags=LIST_LATEST, order=order, latest=(off_v, count_v))
    assert rows["pos"][-1] == v - 1
    # the offsets of the whole column with the lower count: every offset is clamped to v
    list_and_check(codec, S_, v, seek_rows([(0, n), (v - 1, n)]), flags=LIST_LATEST | LIST_REVERSE, order=order,
                   latest=(off, count))


def test_latest_with_garbage_offsets_stays_in_bounds(codec, T, objects):
    """d_objects above the true count and d_obj_off poisoned past `objects`:
    the only requirement is that the call stays in bounds and ends."""
    S_, off, count = objects
    n = len(S_)
    rng = np.random.default_rng(81)
    bad = off.copy()
    bad[count + 1:] = rng.integers(0, 1 << 63, n - count, dtype=np.int64).astype(np.uint64)
    bad[count + 1::2] = rng.integers(0, 2 * n, len(bad[count + 1::2])).astype(np.uint64)
    ranges = seek_rows([(0, n), (5, 5), (3, n - 3), (0, n)])
    cap = 4 * n

    def body(fill):
        for objs in (n, (1 << 64) - 1, count + 7):
            for flags in (LIST_LATEST, LIST_LATEST | LIST_REVERSE):
                c = Call(codec, S_, n, ranges, cap, fill, PHASES[1], order=np.arange(n, dtype=np.uint32),
                         latest=(bad, objs))
                assert c.run(0, flags) == 0
                torch.cuda.synchronize()
                total = int(guards.block_of(c.total).bytes().view(np.uint64)[0])
                assert total <= 4 * n
                w = min(total, cap)
                rows = guards.block_of(c.rows).bytes()[:16 * w].view(LIST_ROW_DTYPE)
                assert (rows["pos"] < n).all() and (rows["range"] < len(ranges)).all()
                guards.assert_untouched(c.rows, [(0, 16 * w)])
                guards.assert_untouched(c.keys, [(0, 29 * w)])
                guards.assert_untouched(c.range_off, [(0, 8 * (len(ranges) + 1))])
                guards.assert_untouched(c.total, [(0, 8)])
                c.inputs_unchanged()

    guards.twice(body)


def test_optional_pointers(codec, T):
    n = T + 40
    S_, order, tomb = column(n, 9)
    assert 0.2 < tomb.mean() < 0.45
    ranges = seek_rows([(3, 90), (0, n), (17, 17), (n - 9, n)])
    for reverse in (0, LIST_REVERSE):
        rows, _, _ = list_and_check(codec, S_, n, ranges, flags=reverse, phases=PHASES[1])  # no order, no info
        assert (rows["record"] == SEEK_NONE).all() and not (rows["flags"] & LIST_ROW_TOMBSTONE).any()
        rows, _, _ = list_and_check(codec, S_, n, ranges, flags=reverse, phases=PHASES[2], order=order)
        assert (rows["record"] == order[rows["pos"]]).all() and not (rows["flags"] & LIST_ROW_TOMBSTONE).any()
        rows, _, _ = list_and_check(codec, S_, n, ranges, flags=reverse, phases=PHASES[3], order=order, tomb=tomb)
        assert (((rows["flags"] & LIST_ROW_TOMBSTONE) != 0) == (tomb[rows["record"]] != 0)).all()
        assert 0.2 < ((rows["flags"] & LIST_ROW_TOMBSTONE) != 0).mean() < 0.45
        list_and_check(codec, S_, n, ranges, flags=reverse, phases=PHASES[1], order=order, tomb=tomb, with_keys=False)
    # an index of the order that is not below n reads info row n - 1
    wild = order.copy()
    wild[::5] = np.array([n, n + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)[np.arange(len(wild[::5])) % 5]
    for last in (0, 1):
        t2 = tomb.copy()
        t2[n - 1] = last
        rows, _, _ = list_and_check(codec, S_, n, ranges, order=wild, tomb=t2)
        out = rows["record"] >= n
        assert out.any() and (((rows["flags"][out] & LIST_ROW_TOMBSTONE) != 0) == bool(last)).all()


def test_m_zero_and_n_zero(codec, T):
    S_, order, tomb = column(10, 10)
    none = seek_rows([])
    rows, off, _ = list_and_check(codec, S_, 10, none, cap=5, order=order)
    assert len(rows) == 0 and off.tolist() == [0]
    empty = np.zeros((0, 29), np.uint8)
    ranges = seek_rows([(0, 5), (0, 0), (3, 0xFFFFFFFF)])
    for flags in (0, LIST_REVERSE):
        rows, off, _ = list_and_check(codec, empty, 7, ranges, cap=5, flags=flags)
        assert len(rows) == 0 and off.tolist() == [0, 0, 0, 0]
    list_and_check(codec, empty, 0, ranges, cap=5, flags=LIST_LATEST, latest=(np.zeros(1, np.uint64), 0))

    def body(fill):  # NULL for everything a call of no rows may leave out
        c = Call(codec, empty, 0, none, 0, fill)
        assert c.run(s=0, r=0, with_rows=False, with_keys=False) == 0
        c.check(expected_list(empty, 0, none), with_rows=False)

    guards.twice(body)


def test_refusals_store_nothing(codec, T):
    n = 300
    S_, order, tomb = column(n, 11)
    ranges = seek_rows([(0, n), (10, 40)])
    off, count = objects_of(np.sort(S_, axis=0), n)
    want = expected_list(S_, n, ranges, order=order, tomb=tomb)
    max_records = int(codec.lib.honu_ctx_max_records(codec.ctx))

    def body(fill):
        c = Call(codec, S_, n, ranges, n + 50, fill, (1, 3), order, tomb, (off, count))
        a = c.args()
        for kw in (dict(n=1 << 32), dict(m=1 << 32), dict(cap=1 << 32), dict(n=(1 << 64) - 1), dict(m=(1 << 64) - 1),
                   dict(cap=(1 << 64) - 1), dict(m=max_records), dict(m=max_records, cap=0, rows=0)):
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(v=0), dict(range_off=0), dict(total=0), dict(r=0), dict(s=0), dict(rows=0),
                   dict(flags=4), dict(flags=7), dict(flags=1 << 31), dict(flags=LIST_LATEST, f=0),
                   dict(flags=LIST_LATEST, j=0), dict(flags=LIST_LATEST | LIST_REVERSE, f=0, j=0), dict(o=0),
                   dict(r=a["r"] + 2), dict(o=a["o"] + 2), dict(v=a["v"] + 4), dict(j=a["j"] + 4), dict(f=a["f"] + 4),
                   dict(range_off=a["range_off"] + 4), dict(total=a["total"] + 4), dict(i=a["i"] + 4),
                   dict(rows=a["rows"] + 8), dict(rows=a["rows"] + 4), dict(f=a["f"] + 4, flags=LIST_LATEST)):
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run() == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)
    assert max_records >= 3


def test_ranges_beyond_the_contexts_scan_are_refused(T):
    """The m + 1 counts go through the context's scan, whose state covers
    max_records rows: a context of 4 records takes 3 ranges and refuses 4."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    small = hobj.Codec(0, 4)
    try:
        S_, order, tomb = column(T + 9, 12)
        n = len(S_)
        pairs = [(0, n), (3, 3), (5, T), (1, 2)]
        list_and_check(small, S_, n, seek_rows(pairs[:3]), order=order, tomb=tomb)

        def body(fill):
            c = Call(small, S_, n, seek_rows(pairs), 3 * n, fill, order=order)
            assert c.run() == E_WORKSPACE
            c.nothing_stored()

        guards.twice(body)
    finally:
        small.close()


# --------------------------------------------------------------------------
# seek and list in one captured graph
# --------------------------------------------------------------------------
def test_graph_of_seek_and_list(codec, T, objects):
    """One captured graph holding seek and list on a single stream, replayed
    three times with the probes and d_valid rewritten on the device in between."""
    S_, off, count = objects
    n = len(S_)
    rng = np.random.default_rng(13)
    order = rng.permutation(n).astype(np.uint32)
    tomb = (rng.integers(0, 3, n) == 0).astype(np.uint8)
    m = 40
    firsts = S_[off[:count].astype(np.int64)]

    def probes_of(seed):
        r = np.random.default_rng(seed)
        p = firsts[r.integers(0, count, m)].copy()
        p[::7] = random_keys(len(p[::7]), r)  # misses
        return p

    rounds = [(probes_of(1), n), (probes_of(2), n - T), (probes_of(3), 30)]
    dev = codec.torch_device

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        info = np.zeros(n, INFO_DTYPE)
        info["tombstone"] = tomb
        dS, do, di = put(codec, S_, 1, fill), put(codec, order, 0, fill), put(codec, info, 0, fill)
        dv, dp = put(codec, u64(n), 0, fill), put(codec, rounds[0][0], 0, fill)
        seek_out = guards.guarded(20 * m, fill=fill, device=dev)
        cap = 2 * n
        range_off = guards.guarded(8 * (m + 1), fill=fill, device=dev)
        rows = guards.guarded(16 * cap, fill=fill, device=dev)
        keys = guards.guarded(29 * cap, phase=3, fill=fill, device=dev)
        total = guards.guarded(8, fill=fill, device=dev)
        A = guards.address

        def both():
            assert codec.lib.honu_key_seek(codec.ctx, A(dS), A(dv), n, A(dp), 0, 17, m, A(do), A(di), A(seek_out),
                                           codec.stream) == 0
            assert codec.lib.honu_key_list(codec.ctx, A(dS), A(do), A(dv), n, A(seek_out), m, 0, LIST_REVERSE, 0, 0,
                                           A(di), A(range_off), A(rows), A(keys), cap, A(total), codec.stream) == 0

        both()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            both()
        totals = []
        for probes, valid in rounds:
            for t in (seek_out, range_off, rows, keys, total):
                refill(t, fill)
            dp.copy_(torch.from_numpy(probes.reshape(-1).copy()).to(dev))
            dv.copy_(torch.from_numpy(u64(valid).view(np.uint8)).to(dev))
            g.replay()
            torch.cuda.synchronize()
            want_rows, want_off, want_keys = expected_list(S_, valid, seek_rows(numpy_seek(S_, valid, probes, 17)),
                                                           flags=LIST_REVERSE, order=order, tomb=tomb)
            w = min(len(want_rows), cap)  # (the first round's need is above cap: the graph holds that too)
            assert int(guards.block_of(total).bytes().view(np.uint64)[0]) == len(want_rows)
            assert np.array_equal(guards.block_of(range_off).bytes().view(np.uint64), want_off)
            assert np.array_equal(guards.block_of(rows).bytes()[:16 * w].view(LIST_ROW_DTYPE), want_rows[:w])
            assert np.array_equal(guards.block_of(keys).bytes()[:29 * w].reshape(w, 29), want_keys[:w])
            guards.assert_untouched(rows, [(0, 16 * w)])
            guards.assert_untouched(keys, [(0, 29 * w)])
            guards.assert_untouched(range_off, [(0, 8 * (m + 1))])
            guards.assert_untouched(total, [(0, 8)])
            guards.assert_untouched(seek_out, [(0, 20 * m)])
            totals.append(len(want_rows))
        assert len(set(totals)) == 3 and min(totals) > 0

    guards.twice(body)


# --------------------------------------------------------------------------
# end to end on generated records: keys, sort, seek, list; merge, delete, list
# --------------------------------------------------------------------------
def key_columns(c, sizes):
    """Generator records of the given batch sizes -> marshal -> decode -> keys:
    [(device key column, device key status, host keys, host status)]. The
    batches share 23 objects; a few records have no Version (their key status
    is not OK)."""
    rng = np.random.default_rng(19)
    oids = rng.integers(0, 256, (23, 16), dtype=np.uint8)
    out = []
    for j, n in enumerate(sizes):
        hb = gen_host_batch(70 + j, "mixed", 0, n)
        hb.meta["object_id"] = oids[rng.integers(0, 23, n)]
        hb.meta["vid"] = rng.integers(1, 40, n)
        hb.meta["pid"] = rng.integers(1, 4, n)
        hb.meta["present"][[1, n // 2, n - 1]] &= ~np.uint32(HAS_VERSION)
        db = hobj.DeviceBatch.from_host(hb, c.torch_device)
        enc = c.marshal(db)
        total = int(enc.out_off.view(torch.int64)[n].item())
        d = c.decode(enc.out, enc.out_off, n, rec_bytes=total)
        dk, dst = c.keys(d)
        torch.cuda.synchronize()
        out.append((dk[:29 * n], dst[:4 * n], hobj._to_host(dk, 29 * n, np.uint8).reshape(n, 29).copy(),
                    hobj._to_host(dst, 4 * n, np.int32).copy()))
    return out


def test_end_to_end_on_generated_records(codec):
    (dka, dsa, ka, sta), (dkb, dsb, kb, stb) = key_columns(codec, (300, 129))
    na, nb = len(ka), len(kb)
    k_all = np.concatenate([ka, kb])

    def host_rows(k, st):
        return [r.tobytes() for r, s in zip(k, st) if s == 0]

    def compare(listed, sorted_host, probes, pstatus, n_rows):
        rows, range_off, total, keys_out = listed
        torch.cuda.synchronize()
        ranges = [hkeys.seek(sorted_host, p[:17].tobytes()) if s == 0 else (0, 0) for p, s in zip(probes, pstatus)]
        want = hkeys.scan(sorted_host, ranges, reverse=True)
        t = int(total.item())
        assert t == len(want) and 0 < t <= n_rows
        got = rows.cpu().numpy().view(np.uint32)[:t]
        assert list(zip(got[:, 0].tolist(), got[:, 1].tolist())) == want
        assert int(range_off[-1].item()) == t
        kk = keys_out.cpu().numpy()[:29 * t].reshape(t, 29)
        assert [r.tobytes() for r in kk] == [sorted_host[p] for _, p in want]
        assert [k_all[r].tobytes() for r in got[:, 2]] == [sorted_host[p] for _, p in want]  # the records carry the keys
        # Versions: most recent first within every range
        for q in set(got[:, 0].tolist()):
            mine = [r.tobytes() for r in kk[got[:, 0] == q]]
            assert mine == sorted(mine, reverse=True)
        return t

    # keys -> sort -> seek at probe_len 17 -> list, reversed: no synchronisation in between
    oa, sa, va = codec.sort_keys(dka, dsa, n=na, want_sorted=True)
    seeks = codec.seek_keys(sa[:29 * na], va, dka, 17, probe_status=dsa, order=oa)
    cap = 64 * na
    listed = codec.list_keys(sa[:29 * na], oa, va, seeks, cap, reverse=True, want_keys=True)
    t1 = compare(listed, hkeys.sort(host_rows(ka, sta)), ka, sta, cap)
    # a second batch merged in and a few objects' versions deleted: the same call over the new column
    ob, sb, vb = codec.sort_keys(dkb, dsb, n=nb, want_sorted=True)
    s2, o2, v2 = codec.merge_keys(sa[:29 * na], oa, va, sb[:29 * nb], ob, vb)
    pick = np.flatnonzero((ka[:, 1] < 0x50) & (sta == 0))[:6]
    assert len(pick) == 6
    ipick = torch.from_numpy(pick).to(codec.torch_device)
    dkd = dka.view(na, 29)[ipick].reshape(-1).contiguous()
    dsd = dsa.view(torch.int32)[ipick].contiguous().view(torch.uint8)
    od, sd, vd = codec.sort_keys(dkd, dsd, n=len(pick), want_sorted=True)
    s3, o3, v3, _ = codec.delete_keys(s2, o2, v2, sd[:29 * len(pick)], vd, probe_len=17)
    seeks = codec.seek_keys(s3, v3, dka, 17, probe_status=dsa, order=o3)
    listed = codec.list_keys(s3, o3, v3, seeks, cap, reverse=True, want_keys=True)
    merged = hkeys.merge(hkeys.sort(host_rows(ka, sta)), hkeys.sort(host_rows(kb, stb)))
    kept, removed = hkeys.delete(merged, [ka[i, :17].tobytes() for i in pick])
    assert removed
    t2 = compare(listed, kept, ka, sta, cap)
    assert t2 != t1
