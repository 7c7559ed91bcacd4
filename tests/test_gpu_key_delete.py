"""honu_key_delete on the GPU against numpy.

The expectation is numpy's alone: a boolean `drop` over the valid rows (the
row's first probe_len bytes are those of a valid delete row, or, with
HONU_DELETE_SUPERSEDED, the next valid row has its 29 bytes), then
concatenate([rows[~drop], rows[drop], tail]) and likewise for the order. It
never calls the library. Every input, output and the workspace is a guarded
view (tests/guards.py) under both fills, the key columns at byte phases 0, 1
and 3; the workspace is exactly honu_key_delete_workspace(n) bytes; the write
set is exactly the 29 n bytes of the column, the 4 n of the order and the two
8-byte counts, and the inputs are unchanged. Sizes are in units of the tile T,
the param "delete_tile".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import DELETE_SUPERSEDED, HAS_VERSION, SEEK_FOUND, SEEK_SKIPPED  # noqa: E402
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
PHASES = ((0, 0, 0), (1, 3, 1), (3, 1, 3), (0, 1, 3))  # (the column, the delete list, the output column)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(codec):
    v = L.C.c_int64(0)
    L.check(codec.lib.honu_ctx_get_param(codec.ctx, b"delete_tile", L.C.byref(v)), "delete_tile")
    assert v.value >= 64
    return int(v.value)


# --------------------------------------------------------------------------
# expectations
# --------------------------------------------------------------------------
def expected_order(k, st):
    """What honu_sort_keys writes for a key column and its status column
    (tests/test_gpu_sort.py): (order, valid)."""
    ok = np.flatnonzero(st == 0)
    bad = np.flatnonzero(st != 0)
    rows = k[ok]
    srt = np.lexsort(rows.T[::-1]) if len(ok) else np.zeros(0, np.int64)  # stable; column 0 the primary key
    return np.concatenate([ok[srt], bad]).astype(np.uint32), len(ok)


class Side:
    """A sorted column (n, 29), its order, and the valid count the device is told."""

    def __init__(self, S, order, valid):
        self.S = np.ascontiguousarray(S, np.uint8).reshape(-1, 29)
        self.order = np.asarray(order, np.uint32)
        self.valid = int(valid)
        self.n = len(self.S)


def side_of(k, st=None):
    """The sort's output for a key column and a status column."""
    k = np.ascontiguousarray(k, np.uint8).reshape(-1, 29)
    st = np.zeros(len(k), np.int32) if st is None else st
    order, valid = expected_order(k, st)
    return Side(k[order], order, valid)


NO_LIST = Side(np.zeros((0, 29), np.uint8), np.zeros(0, np.uint32), 0)


def expected_delete(col, dl, probe_len, flags=0):
    """(column, order, kept, removed)."""
    v, vd = min(col.valid, col.n), min(dl.valid, dl.n)
    rows, idx = col.S[:v], col.order[:v]
    drop = np.zeros(v, bool)
    if vd:
        named = {r.tobytes() for r in dl.S[:vd, :probe_len]}
        drop = np.array([r.tobytes() in named for r in rows[:, :probe_len]], bool).reshape(v)
    if flags & DELETE_SUPERSEDED and v > 1:
        drop[:-1] |= (rows[:-1] == rows[1:]).all(axis=1)
    S = np.concatenate([rows[~drop], rows[drop], col.S[v:]])
    order = np.concatenate([idx[~drop], idx[drop], col.order[v:]])
    return S, order.astype(np.uint32), int((~drop).sum()), int(drop.sum())


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
    """The guarded device arguments of one delete."""

    def __init__(self, codec, col, dl, fill, phases=(0, 0, 0)):
        self.codec, self.col, self.dl, self.n = codec, col, dl, col.n
        self.s, self.d = put(codec, col.S, phases[0], fill), put(codec, dl.S, phases[1], fill)
        self.o = put(codec, col.order, 0, fill)
        self.v, self.vd = put(codec, u64(col.valid), 0, fill), put(codec, u64(dl.valid), 0, fill)
        dev = codec.torch_device
        self.out = guards.guarded(29 * self.n, phase=phases[2], fill=fill, device=dev)
        self.order = guards.guarded(4 * self.n, fill=fill, device=dev)
        self.valid = guards.guarded(8, fill=fill, device=dev)
        self.removed = guards.guarded(8, fill=fill, device=dev)
        self.work_bytes = int(codec.lib.honu_key_delete_workspace(self.n))
        assert self.work_bytes % 256 == 0
        self.work = guards.guarded(self.work_bytes, fill=fill, device=dev)

    def run(self, probe_len=29, flags=0, with_order=True, input_order=True, with_removed=True, with_list=True):
        A = guards.address
        return self.codec.lib.honu_key_delete(
            self.codec.ctx, A(self.s), A(self.o) if input_order else 0, A(self.v), self.n,
            A(self.d) if with_list else 0, A(self.vd) if with_list else 0, self.dl.n if with_list else 0, probe_len,
            flags, A(self.out), A(self.order) if with_order else 0, A(self.valid),
            A(self.removed) if with_removed else 0, A(self.work), self.work_bytes, self.codec.stream)

    def inputs_unchanged(self):
        for t, h in ((self.s, self.col.S), (self.d, self.dl.S), (self.o, self.col.order), (self.v, u64(self.col.valid)),
                     (self.vd, u64(self.dl.valid))):
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(h).tobytes()
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def check(self, want, with_order=True, with_removed=True):
        """The four outputs against (column, order, kept, removed) and the write set."""
        torch.cuda.synchronize()
        S, order, kept, removed = want
        n = self.n
        got_kept = int(guards.block_of(self.valid).bytes().view(np.uint64)[0])
        assert got_kept == kept, (got_kept, kept)
        if with_removed:
            got_removed = int(guards.block_of(self.removed).bytes().view(np.uint64)[0])
            assert got_removed == removed, (got_removed, removed)
        got = guards.block_of(self.out).bytes().reshape(n, 29)
        bad = np.flatnonzero((got != S).any(axis=1))
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], S[bad[:4]])
        guards.assert_untouched(self.out, [(0, 29 * n)])
        if with_order:
            got = guards.block_of(self.order).bytes().view(np.uint32)
            bad = np.flatnonzero(got != order)
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], order[bad[:4]])
        guards.assert_untouched(self.order, [(0, 4 * n)] if with_order else [])
        guards.assert_untouched(self.valid, [(0, 8)])
        guards.assert_untouched(self.removed, [(0, 8)] if with_removed else [])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        self.inputs_unchanged()


def delete_and_check(codec, col, dl, probe_len=29, flags=0, phases=(0, 0, 0), **how):
    want = expected_delete(col, dl if how.get("with_list", True) else NO_LIST, probe_len, flags)
    S, order, kept, removed = want
    v = min(col.valid, col.n)
    assert kept + removed == v and sorted(order.tolist()) == sorted(col.order.tolist())  # a permutation

    def body(fill):
        c = Call(codec, col, dl, fill, phases)
        assert c.run(probe_len, flags, **how) == 0
        c.check(want, how.get("with_order", True), how.get("with_removed", True))

    guards.twice(body)
    return want


# --------------------------------------------------------------------------
# key columns
# --------------------------------------------------------------------------
def random_keys(n, rng):
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def pool_keys(n, rng, pool):
    """n keys drawn from `pool` distinct ones: many ties."""
    return pool[rng.integers(0, len(pool), n)]


VALUES = np.array([0, 1, 0x7E, 0x7F, 0x80, 0x81, 0xFE, 0xFF], np.uint8)  # both sides of 0x7f/0x80


def one_byte_keys(n, rng, base, byte, values=VALUES):
    """Keys that differ only in byte `byte`."""
    k = np.tile(base, (n, 1))
    k[:, byte] = rng.choice(values, n)
    return k


def statuses(n, rng, which="fifth"):
    if which == "all":
        return np.full(n, 8, np.int32)
    st = np.zeros(n, np.int32)
    st[rng.integers(0, 5, n) == 0] = 8
    return st


def size_of(T, s):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[s] if isinstance(s, str) else s


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
NS = (0, 1, 2, "T-1", "T", "T+1", "3T+5")
MS = (0, 1, 63, "T+1")


@pytest.mark.parametrize("sn", NS)
def test_sizes(codec, T, sn):
    """Random 29-byte keys, every n against every m: half of the delete rows
    drawn from the column, half random."""
    n = size_of(T, sn)
    for j, sm in enumerate(MS):
        m = size_of(T, sm)
        rng = np.random.default_rng(9000 + 10 * n + j)
        k = random_keys(n, rng)
        drawn = k[rng.integers(0, n, (m + 1) // 2)] if n else np.zeros((0, 29), np.uint8)
        dk = np.concatenate([drawn, random_keys(m - len(drawn), rng)])
        S, order, kept, removed = delete_and_check(codec, side_of(k), side_of(dk),
                                                   phases=PHASES[(NS.index(sn) + j) % len(PHASES)])
        assert removed == len({r.tobytes() for r in drawn}) and kept == n - removed


@pytest.mark.parametrize("m", [4097, 4225])
def test_range_search_over_a_long_list(codec, T, m):
    """A delete list of m rows over a column of T + 1: each tile's two wave
    searches run over the whole list, a bracket of more than 4096 rows (and,
    at 4225, above the 4160 from which the search takes a third step). Half of
    the delete rows are drawn from the column, half random."""
    rng = np.random.default_rng(9100 + m)
    n = T + 1
    k = random_keys(n, rng)
    drawn = k[rng.integers(0, n, m // 2)]
    dk = np.concatenate([drawn, random_keys(m - len(drawn), rng)])
    S, order, kept, removed = delete_and_check(codec, side_of(k), side_of(dk), phases=PHASES[m % len(PHASES)])
    assert removed == len({r.tobytes() for r in drawn}) and kept == n - removed


def test_nothing_removed(codec, T):
    rng = np.random.default_rng(81)
    col = side_of(random_keys(2 * T + 3, rng))
    _, order, kept, removed = delete_and_check(codec, col, side_of(random_keys(200, rng)), phases=PHASES[1])
    assert removed == 0 and np.array_equal(order, col.order)


def test_everything_removed(codec, T):
    """By probe_len 0 with one valid delete row (DeleteBucket, store.go:402),
    and by a list that names every key."""
    rng = np.random.default_rng(82)
    k = random_keys(2 * T + 3, rng)
    col = side_of(k, statuses(len(k), rng))
    one = Side(random_keys(5, rng), np.arange(5), 1)
    _, order, kept, removed = delete_and_check(codec, col, one, probe_len=0, phases=PHASES[2])
    assert kept == 0 and removed == col.valid and np.array_equal(order, col.order)
    _, order, kept, removed = delete_and_check(codec, col, side_of(k[rng.permutation(len(k))]), phases=PHASES[3])
    assert kept == 0 and removed == col.valid and np.array_equal(order, col.order)


def test_removed_range_covers_whole_tiles(codec, T):
    """128 delete rows whose byte 0 is 0..127 at probe_len 1: about half of
    4T + 9 random keys, tiles entirely removed, entirely kept, and one split."""
    rng = np.random.default_rng(83)
    n = 4 * T + 9
    col = side_of(random_keys(n, rng))
    dk = random_keys(128, rng)
    dk[:, 0] = np.arange(128)
    _, _, kept, removed = delete_and_check(codec, col, side_of(dk), probe_len=1, phases=PHASES[1])
    drop = col.S[:, 0] < 128
    assert removed == int(drop.sum()) and kept == n - removed
    per_tile = [drop[t:t + T] for t in range(0, n, T)]
    assert any(t.all() for t in per_tile) and any(not t.any() for t in per_tile)
    assert any(t.any() and not t.all() for t in per_tile)


def test_no_valid_delete_row(codec, T):
    """vd == 0 with m > 0: nothing goes, whatever the rows hold."""
    rng = np.random.default_rng(84)
    k = random_keys(T + 9, rng)
    col = side_of(k)
    for flags, probe_len in ((0, 29), (0, 0), (DELETE_SUPERSEDED, 17)):
        _, _, kept, removed = delete_and_check(codec, col, Side(col.S[:70], np.arange(70), 0), probe_len=probe_len,
                                               flags=flags, phases=PHASES[2])
        assert (kept, removed) == (col.n, 0)


@pytest.mark.parametrize("probe_len", [0, 1, 16, 17, 28, 29])
def test_prefix_lengths(codec, T, probe_len):
    """64 objects with small versions; the list is 9 ObjectPrefix rows (the
    version bytes zero): 17 removes those objects' versions, 29 nothing."""
    rng = np.random.default_rng(1)
    n = 2 * T + 77
    oids = rng.integers(0, 256, (64, 16), dtype=np.uint8)
    k = np.zeros((n, 29), np.uint8)
    k[:, 0] = 1
    which = rng.integers(0, 64, n)
    k[:, 1:17] = oids[which]
    k[:, 24] = rng.integers(1, 6, n)  # VID
    k[:, 28] = rng.integers(1, 4, n)  # PID
    dk = np.zeros((9, 29), np.uint8)
    dk[:, 0] = 1
    dk[:, 1:17] = oids[:9]
    col = side_of(k)
    for flags in (0, DELETE_SUPERSEDED):
        _, _, kept, removed = delete_and_check(codec, col, side_of(dk), probe_len=probe_len, flags=flags,
                                               phases=PHASES[probe_len % len(PHASES)])
        runs = n - len({r.tobytes() for r in k})  # rows that a later equal row supersedes
        named = int((which < 9).sum())
        if probe_len <= 1:
            assert kept == 0
        elif probe_len in (16, 17):
            assert removed > 0 and removed >= named and (flags or removed == named)
        else:
            assert removed == (runs if flags else 0)
        assert runs > 0 and 0 < named < n


@pytest.mark.parametrize("byte", [28, 0, 16, 13, 14, 15, 12, 17])
def test_the_byte_where_the_prefix_ends(codec, T, byte):
    """Keys that differ only in one byte b: at probe_len b every row matches,
    at b + 1 only the rows with a delete row's value (the last byte, the first,
    the ObjectPrefix edge 16 / 17, the overlap of the two 16-byte loads 13-15)."""
    rng = np.random.default_rng(840 + byte)
    base = random_keys(1, rng)
    n = T + 37
    k = one_byte_keys(n, rng, base, byte)
    named = np.array([1, 0x7F, 0x80, 0xFE], np.uint8)
    dk = one_byte_keys(9, rng, base, byte, named)
    col = side_of(k)
    _, _, kept, removed = delete_and_check(codec, col, side_of(dk), probe_len=byte, phases=PHASES[byte % len(PHASES)])
    assert (kept, removed) == (0, n)
    _, _, kept, removed = delete_and_check(codec, col, side_of(dk), probe_len=byte + 1,
                                           phases=PHASES[(byte + 1) % len(PHASES)])
    assert removed == int(np.isin(k[:, byte], dk[:, byte]).sum()) and 0 < removed < n


def test_superseded_one_run(codec, T):
    """One run of 3T + 5 equal keys over four tiles: the last row stays, with the last index."""
    rng = np.random.default_rng(85)
    n = 3 * T + 5
    col = side_of(np.tile(random_keys(1, rng), (n, 1)))
    S, order, kept, removed = delete_and_check(codec, col, NO_LIST, flags=DELETE_SUPERSEDED, phases=PHASES[1])
    assert (kept, removed) == (1, n - 1) and order[0] == n - 1 and np.array_equal(order[1:], np.arange(n - 1))


def test_superseded_two_runs_straddle_tile_boundaries(codec, T):
    """Two distinct keys, runs [0, 1.5T - 4) and [1.5T - 4, 3T + 5): the first
    crosses position T, the second 2T and 3T."""
    rng = np.random.default_rng(86)
    k = random_keys(2, rng)
    k = k[np.lexsort(k.T[::-1])]
    n, n0 = 3 * T + 5, T + T // 2 - 4
    keys = np.concatenate([np.tile(k[0], (n0, 1)), np.tile(k[1], (n - n0, 1))])[rng.permutation(n)]
    col = side_of(keys)
    S, order, kept, removed = delete_and_check(codec, col, NO_LIST, flags=DELETE_SUPERSEDED, phases=PHASES[3])
    assert kept == 2 and np.array_equal(S[:2], k)
    assert order[0] == col.order[n0 - 1] and order[1] == col.order[n - 1]
    # and with the first of the two named by the list: one row stays
    _, order, kept, _ = delete_and_check(codec, col, side_of(k[:1]), flags=DELETE_SUPERSEDED, phases=PHASES[2])
    assert kept == 1 and order[0] == col.order[n - 1]


def test_superseded_pool(codec, T):
    """A pool of 200 keys drawn 3T + 5 times: the distinct keys drawn stay;
    alone, with a list, and with m == 0 and d_del == NULL."""
    rng = np.random.default_rng(87)
    pool = random_keys(200, rng)
    k = pool_keys(3 * T + 5, rng, pool)
    col = side_of(k)
    distinct = len({r.tobytes() for r in k})
    S, order, kept, _ = delete_and_check(codec, col, NO_LIST, flags=DELETE_SUPERSEDED, phases=PHASES[1])
    assert kept == distinct
    last = {r.tobytes(): i for i, r in enumerate(k)}  # the highest index that carries the key
    assert [last[r.tobytes()] for r in S[:kept]] == order[:kept].tolist()
    _, _, kept, _ = delete_and_check(codec, col, side_of(pool[:50]), flags=DELETE_SUPERSEDED, with_list=False,
                                     phases=PHASES[2])
    assert kept == distinct
    dl = side_of(np.concatenate([pool[:60], random_keys(40, rng)]))
    _, _, kept, _ = delete_and_check(codec, col, dl, flags=DELETE_SUPERSEDED, phases=PHASES[3])
    assert kept == distinct - len({r.tobytes() for r in k} & {r.tobytes() for r in pool[:60]}) > 0


def test_superseded_at_the_end_of_the_valid_rows(codec, T):
    """A run whose last row is row v - 1 keeps it; equal rows of the invalid
    tail behind it do not supersede it."""
    rng = np.random.default_rng(88)
    k = random_keys(T + 40, rng)
    k[:, 0] &= 0x7F
    top = random_keys(1, rng)
    top[:, 0] = 0xFF
    k[-70:] = top  # the run at the end of the sorted column: 70 rows
    col = side_of(k)
    for v in (col.n, col.n - 30, col.n - 69, col.n - 70):  # the run whole, cut by v, its first row only, none of it
        S, order, kept, removed = delete_and_check(codec, Side(col.S, col.order, v), NO_LIST, flags=DELETE_SUPERSEDED,
                                                   phases=PHASES[v % len(PHASES)])
        in_run = v - (col.n - 70)
        assert kept == col.n - 70 + (1 if in_run else 0) and removed == max(in_run - 1, 0)
        if in_run:
            assert order[kept - 1] == col.order[v - 1]
        assert np.array_equal(S[v:], col.S[v:]) and np.array_equal(order[v:], col.order[v:])


def test_rows_that_take_no_part(codec, T):
    """A small pool, so the rows in question do match: invalid-tail rows equal
    to a delete row stay where they are; delete rows at or past vd delete
    nothing."""
    rng = np.random.default_rng(89)
    pool = random_keys(40, rng)
    k = pool_keys(2 * T + 11, rng, pool)
    st = statuses(len(k), rng)
    col = side_of(k, st)
    dl = side_of(pool[:20])
    S, order, kept, removed = delete_and_check(codec, col, dl, phases=PHASES[1])
    tail = np.flatnonzero(st != 0)
    assert np.array_equal(order[col.valid:], tail.astype(np.uint32)) and np.array_equal(S[col.valid:], k[tail])
    named = {r.tobytes() for r in pool[:20]}
    assert sum(r.tobytes() in named for r in k[tail]) > 20 and 0 < removed < col.valid
    # the list cut at vd = 7: rows 7.. equal column keys and delete nothing
    cut = Side(dl.S, dl.order, 7)
    _, _, kept2, removed2 = delete_and_check(codec, col, cut, phases=PHASES[2])
    assert 0 < removed2 < removed
    # a delete list with invalid rows of its own behind the valid ones
    dst = np.zeros(40, np.int32)
    dst[::2] = 8
    _, _, _, removed3 = delete_and_check(codec, col, side_of(pool, dst), flags=DELETE_SUPERSEDED, phases=PHASES[3])
    assert 0 < removed3 < col.valid


def test_valid_counts_above_n_are_clamped(codec, T):
    rng = np.random.default_rng(90)
    pool = random_keys(300, rng)
    col, dl = side_of(pool_keys(T + 9, rng, pool)), side_of(pool[:70])
    want = delete_and_check(codec, col, dl, flags=DELETE_SUPERSEDED)
    for dv, dd in ((5, 0), (0, 1 << 40), (1 << 63, 3)):
        got = delete_and_check(codec, Side(col.S, col.order, col.n + dv), Side(dl.S, dl.order, dl.n + dd),
                               flags=DELETE_SUPERSEDED, phases=PHASES[2])
        assert got[2:] == want[2:] and all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2]))


def test_duplicated_delete_rows_and_a_list_beyond_the_stage(codec, T):
    """T + 1 delete rows drawn from 30 of the column's 50 keys, all of them
    inside tile 0's key range: more than the workgroup stages in LDS, so the
    search runs over global memory; then 63 of them, staged."""
    rng = np.random.default_rng(91)
    pool = random_keys(50, rng)
    pool = pool[np.lexsort(pool.T[::-1])]
    k = np.concatenate([pool, pool_keys(T - 50, rng, pool)])  # one tile that holds every pool key
    col = side_of(k)
    named = pool[10:40]
    for m in (T + 1, 63):
        dl = side_of(pool_keys(m, rng, named))
        for flags in (0, DELETE_SUPERSEDED):
            _, _, kept, removed = delete_and_check(codec, col, dl, flags=flags, phases=PHASES[(m + flags) % len(PHASES)])
            gone = {r.tobytes() for r in dl.S}
            assert removed >= sum(r.tobytes() in gone for r in k) > 0 and kept >= 50 - len(gone) > 0
    # and against a column of several tiles
    col = side_of(pool_keys(2 * T + 5, rng, pool))
    delete_and_check(codec, col, side_of(pool_keys(T + 1, rng, named)), phases=PHASES[1])


def test_optional_outputs(codec, T):
    """d_order_out = NULL, with and without d_order; d_removed = NULL."""
    rng = np.random.default_rng(92)
    pool = random_keys(100, rng)
    k = pool_keys(2 * T + 3, rng, pool)
    col, dl = side_of(k, statuses(len(k), rng)), side_of(pool[:30])
    for how in (dict(with_order=False, input_order=False), dict(with_order=False, input_order=True),
                dict(with_removed=False), dict(with_order=False, input_order=False, with_removed=False)):
        delete_and_check(codec, col, dl, flags=DELETE_SUPERSEDED, phases=PHASES[1], **how)


def test_graph_capture_and_new_counts(codec, T):
    """One delete captured and replayed; then both valid counts lowered on
    the device and the same graph replayed."""
    rng = np.random.default_rng(93)
    pool = random_keys(300, rng)
    col = side_of(pool_keys(2 * T + 40, rng, pool))
    dl = side_of(pool[:120])
    fewer_col, fewer_dl = Side(col.S, col.order, col.n - T - 13), Side(dl.S, dl.order, 50)

    def refill(t, fill):
        """The view back to its pattern, so that what it holds afterwards is the replay's."""
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(codec.torch_device))

    def body(fill):
        c = Call(codec, col, dl, fill, PHASES[2])
        assert c.run(29, DELETE_SUPERSEDED) == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run(29, DELETE_SUPERSEDED) == 0
        outs = (c.out, c.order, c.valid, c.removed, c.work)
        for t in outs:
            refill(t, fill)
        g.replay()
        c.check(expected_delete(col, dl, 29, DELETE_SUPERSEDED))
        for t in outs:
            refill(t, fill)
        c.v.copy_(torch.from_numpy(u64(fewer_col.valid).view(np.uint8)).to(codec.torch_device))
        c.vd.copy_(torch.from_numpy(u64(fewer_dl.valid).view(np.uint8)).to(codec.torch_device))
        g.replay()
        torch.cuda.synchronize()
        c.col, c.dl = fewer_col, fewer_dl  # (inputs_unchanged compares the same columns and the new counts)
        want = expected_delete(fewer_col, fewer_dl, 29, DELETE_SUPERSEDED)
        assert want[2:] != expected_delete(col, dl, 29, DELETE_SUPERSEDED)[2:]
        c.check(want)

    guards.twice(body)


def test_refusals_store_nothing(codec, T):
    rng = np.random.default_rng(94)
    col, dl = side_of(random_keys(300, rng)), side_of(random_keys(70, rng))
    dl.S[:35] = col.S[::8][:35]
    dl = side_of(dl.S)
    want = expected_delete(col, dl, 29)
    assert want[3] == 35

    def body(fill):
        c = Call(codec, col, dl, fill, (1, 3, 1))
        A = guards.address
        base = dict(ctx=codec.ctx, s=A(c.s), o=A(c.o), v=A(c.v), n=col.n, d=A(c.d), vd=A(c.vd), m=dl.n, probe_len=29,
                    flags=0, out=A(c.out), order=A(c.order), valid=A(c.valid), removed=A(c.removed), work=A(c.work),
                    work_bytes=c.work_bytes)

        def call(**kw):
            x = dict(base, **kw)
            return codec.lib.honu_key_delete(x["ctx"], x["s"], x["o"], x["v"], x["n"], x["d"], x["vd"], x["m"],
                                             x["probe_len"], x["flags"], x["out"], x["order"], x["valid"],
                                             x["removed"], x["work"], x["work_bytes"], codec.stream)

        big = 1 << 62  # a workspace size that passes the size check of any n
        # refused before any launch, whatever the fake counts would index
        for kw in (dict(n=1 << 32, work_bytes=big), dict(m=1 << 32), dict(n=(1 << 64) - 1, work_bytes=big),
                   dict(m=(1 << 64) - 1)):
            assert call(**kw) == E_WORKSPACE, kw
        assert c.work_bytes >= 256
        for kw in (dict(ctx=None), dict(v=0), dict(valid=0), dict(vd=0), dict(s=0), dict(out=0), dict(d=0),
                   dict(probe_len=30), dict(probe_len=(1 << 32) - 1), dict(flags=2), dict(flags=3),
                   dict(flags=1 << 31), dict(work_bytes=c.work_bytes - 1), dict(work_bytes=0), dict(work=0),
                   dict(work=A(c.work) + 128), dict(work=A(c.work) + 8), dict(o=0),
                   dict(o=A(c.o) + 2), dict(order=A(c.order) + 2), dict(v=A(c.v) + 4), dict(vd=A(c.vd) + 4),
                   dict(valid=A(c.valid) + 4), dict(removed=A(c.removed) + 4)):
            assert call(**kw) == E_ARG, kw
        torch.cuda.synchronize()
        for t in (c.out, c.order, c.valid, c.removed, c.work):
            guards.assert_untouched(t, [])
        # n == 0 writes only the counts, columns and workspace given or not
        assert call(n=0) == 0
        torch.cuda.synchronize()
        for t in (c.valid, c.removed):
            assert int(guards.block_of(t).bytes().view(np.uint64)[0]) == 0
            guards.assert_untouched(t, [(0, 8)])
        for t in (c.out, c.order, c.work):
            guards.assert_untouched(t, [])
        assert call(n=0, s=0, o=0, out=0, order=0, work=0, work_bytes=0, removed=0) == 0
        assert call(n=0, m=0, d=0, vd=0, s=0, o=0, out=0, order=0, work=0, work_bytes=0) == 0
        assert c.run() == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)


def test_column_beyond_the_contexts_scan_is_refused(T):
    """The tiles' kept counts go through the context's scan, whose state covers
    max_records rows: a context of 2 records takes a column of two tiles (the
    scan then adds tile 0's count to tile 1's rows) and refuses one of three
    with HONU_E_WORKSPACE, storing nothing."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    small = hobj.Codec(0, 2)
    try:
        rng = np.random.default_rng(95)
        pool = random_keys(300, rng)
        dl = side_of(pool[:100])
        fits, beyond = side_of(pool_keys(2 * T, rng, pool)), side_of(pool_keys(2 * T + 1, rng, pool))
        _, _, kept, removed = delete_and_check(small, fits, dl, flags=DELETE_SUPERSEDED, phases=PHASES[1])
        assert 0 < kept < 300 and removed > T

        def body(fill):
            c = Call(small, beyond, dl, fill, PHASES[2])
            assert c.run(29, DELETE_SUPERSEDED) == E_WORKSPACE
            assert c.run(0, 0, with_list=False) == E_WORKSPACE
            torch.cuda.synchronize()
            for t in (c.out, c.order, c.valid, c.removed, c.work):
                guards.assert_untouched(t, [])
            c.inputs_unchanged()

        guards.twice(body)
    finally:
        small.close()


# --------------------------------------------------------------------------
# the life cycle: sort(A), sort(B), merge, sort(D), delete, seek on one stream
# --------------------------------------------------------------------------
def key_columns(c, sizes):
    """Generator records of the given batch sizes -> marshal -> decode -> keys:
    [(device key column, device key status, host keys, host status)]. The
    batches share 23 objects; batch 1 repeats keys of batch 0; a few records
    have no Version (their key status is not OK)."""
    rng = np.random.default_rng(17)
    oids = rng.integers(0, 256, (23, 16), dtype=np.uint8)
    out, first = [], None
    for j, n in enumerate(sizes):
        hb = gen_host_batch(50 + j, "mixed", 0, n)
        hb.meta["object_id"] = oids[rng.integers(0, 23, n)]
        hb.meta["vid"] = rng.integers(1, 6, n)
        hb.meta["pid"] = rng.integers(1, 4, n)
        if j == 0:
            first = hb.meta.copy()
        if j == 1:  # records 0, 3, 6, ... carry the keys of batch 0's records 0, 5, 10, ...
            take = np.arange(0, n, 3)
            src = (np.arange(len(take)) * 5) % len(first)
            for f in ("object_id", "vid", "pid"):
                hb.meta[f][take] = first[f][src]
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


@pytest.fixture(scope="module")
def columns(codec):
    return key_columns(codec, (300, 129))


@pytest.mark.parametrize("probe_len,superseded", [(29, True), (17, False)])
def test_life_cycle_on_one_stream(codec, columns, probe_len, superseded):
    (dka, dsa, ka, sta), (dkb, dsb, kb, stb) = columns
    na, nb = len(ka), len(kb)
    n = na + nb
    k, st = np.concatenate([ka, kb]), np.concatenate([sta, stb])
    # D: half of the records of the objects whose id starts below 0x50
    pick = np.flatnonzero(k[:, 1] < 0x50)[::2]
    assert 8 <= len(pick) < n // 2 and (st[pick] == 0).sum() >= 8
    dev = codec.torch_device
    probes, pstatus = torch.cat([dka, dkb]), torch.cat([dsa, dsb])
    ipick = torch.from_numpy(pick).to(dev)
    dkd = probes.view(n, 29)[ipick].reshape(-1).contiguous()
    dsd = pstatus.view(torch.int32)[ipick].contiguous().view(torch.uint8)
    torch.cuda.synchronize()
    # sort(A), sort(B), merge, sort(D), delete, seek: no synchronisation in between
    oa, sa, va = codec.sort_keys(dka, dsa, n=na, want_sorted=True)
    ob, sb, vb = codec.sort_keys(dkb, dsb, n=nb, want_sorted=True)
    s2, o2, v2 = codec.merge_keys(sa[:29 * na], oa, va, sb[:29 * nb], ob, vb)
    od, sd, vd = codec.sort_keys(dkd, dsd, n=len(pick), want_sorted=True)
    s3, o3, v3, r3 = codec.delete_keys(s2, o2, v2, sd[:29 * len(pick)], vd, probe_len=probe_len,
                                       superseded=superseded)
    rows = codec.seek_keys(s3, v3, probes, 29, probe_status=pstatus, order=o3)
    torch.cuda.synchronize()
    # which records go, by numpy
    ok = st == 0
    named = {r.tobytes() for r in k[pick[ok[pick]], :probe_len]}
    gone = ok & np.array([r.tobytes() in named for r in k[:, :probe_len]])
    last = {}  # key -> the highest record index that carries it
    for i in np.flatnonzero(ok):
        last[k[i].tobytes()] = int(i)
    if superseded:
        gone |= ok & np.array([last.get(r.tobytes()) != i for i, r in enumerate(k)])
    kept, removed = int((ok & ~gone).sum()), int(gone.sum())
    assert int(v3.item()) == kept and int(r3.item()) == removed and 0 < kept and 0 < removed
    assert s3.numel() == 29 * n and o3.numel() == n
    # the seek: D's keys are gone, every other key is there
    got = rows.cpu().numpy().view(np.uint32)
    assert ((got[~ok, 4] & SEEK_SKIPPED) != 0).all()
    count = {}
    for i in np.flatnonzero(ok):
        count[k[i].tobytes()] = count.get(k[i].tobytes(), 0) + 1
    checked = 0
    for i in np.flatnonzero(ok):
        key = k[i].tobytes()
        if key[:probe_len] in named:
            assert not got[i, 4] & SEEK_FOUND
            continue
        assert got[i, 4] & SEEK_FOUND and got[i, 3] == last[key]
        assert got[i, 1] - got[i, 0] == (1 if superseded else count[key])
        checked += 1
    assert checked >= 100
    # rows [0, kept) equal, bit for bit, the sort with the removed records' statuses set on the host
    st2 = st.copy()
    st2[gone] = 8
    wo, ws, wv = codec.sort_keys(probes, torch.from_numpy(st2).to(dev).view(torch.uint8), n=n, want_sorted=True)
    torch.cuda.synchronize()
    assert int(wv.item()) == kept
    assert torch.equal(o3[:kept], wo[:kept]) and torch.equal(s3[:29 * kept], ws[:29 * kept])
    # and numpy's: the removed rows in column order behind them, then the invalid tail
    order, valid = expected_order(k, st)
    col = Side(k[order], order, valid)
    S, want_order, want_kept, want_removed = expected_delete(
        col, side_of(k[pick], st[pick]), probe_len, DELETE_SUPERSEDED if superseded else 0)
    assert (want_kept, want_removed) == (kept, removed)
    assert np.array_equal(o3.cpu().numpy().view(np.uint32), want_order)
    assert np.array_equal(s3.cpu().numpy().reshape(n, 29), S)
