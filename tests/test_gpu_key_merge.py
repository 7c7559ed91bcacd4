"""honu_key_merge on the GPU against numpy.

The expectation is numpy's alone: np.lexsort (stable) over the concatenation
of the two sides' valid rows, A's first, so equal keys keep A before B and
each side's order; the invalid rows behind. Where the sides come from key and
status columns the three outputs must also equal what the sort of the
concatenated columns gives (expected_order, as in tests/test_gpu_sort.py).
Every column and output is a guarded view (tests/guards.py) under both fills,
the key columns at byte phases 0, 1 and 3; the write set is exactly the
29 (na + nb) bytes of the column, the 4 (na + nb) of the order and the 8 of
the valid count. Sizes are in units of the tile T, the param "merge_tile".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import HAS_VERSION, SEEK_FOUND, SEEK_SKIPPED  # noqa: E402
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
PHASES = ((0, 0, 0), (1, 3, 1), (3, 1, 3), (0, 1, 3))  # (A's column, B's column, the output column)


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
    L.check(codec.lib.honu_ctx_get_param(codec.ctx, b"merge_tile", L.C.byref(v)), "merge_tile")
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
    """One input: the sorted column (n, 29), its order, and the valid count the device is told."""

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


def expected_merge(a, b, b_base):
    """(column, order, valid count) by np.lexsort over the concatenation of the valid rows."""
    va, vb = min(a.valid, a.n), min(b.valid, b.n)
    rows = np.concatenate([a.S[:va], b.S[:vb]])
    idx = np.concatenate([a.order[:va].astype(np.uint64), b.order[:vb].astype(np.uint64) + b_base])
    perm = np.lexsort(rows.T[::-1]) if len(rows) else np.zeros(0, np.int64)
    S = np.concatenate([rows[perm], a.S[va:], b.S[vb:]])
    order = np.concatenate([idx[perm], a.order[va:].astype(np.uint64), b.order[vb:].astype(np.uint64) + b_base])
    return S, order.astype(np.uint32), va + vb


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


class Call:
    """The guarded device arguments of one merge."""

    def __init__(self, codec, a, b, fill, phases=(0, 0, 0)):
        self.codec, self.a, self.b, self.n = codec, a, b, a.n + b.n
        self.sa, self.sb = put(codec, a.S, phases[0], fill), put(codec, b.S, phases[1], fill)
        self.oa, self.ob = put(codec, a.order, 0, fill), put(codec, b.order, 0, fill)
        self.va, self.vb = put(codec, np.array([a.valid], np.uint64), 0, fill), put(
            codec, np.array([b.valid], np.uint64), 0, fill)
        dev = codec.torch_device
        self.out = guards.guarded(29 * self.n, phase=phases[2], fill=fill, device=dev)
        self.order = guards.guarded(4 * self.n, fill=fill, device=dev)
        self.valid = guards.guarded(8, fill=fill, device=dev)

    def run(self, b_base, with_order=True, input_orders=True):
        A = guards.address
        return self.codec.lib.honu_key_merge(
            self.codec.ctx, A(self.sa), A(self.oa) if input_orders else 0, A(self.va), self.a.n, A(self.sb),
            A(self.ob) if input_orders else 0, A(self.vb), self.b.n, b_base, A(self.out),
            A(self.order) if with_order else 0, A(self.valid), self.codec.stream)

    def inputs_unchanged(self):
        for t, h in ((self.sa, self.a.S), (self.sb, self.b.S), (self.oa, self.a.order), (self.ob, self.b.order)):
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(h).tobytes()
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def check(self, want, with_order=True):
        """The three outputs against (column, order, valid) and the write set."""
        torch.cuda.synchronize()
        S, order, valid = want
        n = self.n
        got_valid = int(guards.block_of(self.valid).bytes().view(np.uint64)[0])
        assert got_valid == valid, (got_valid, valid)
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
        self.inputs_unchanged()


def merge_and_check(codec, a, b, b_base=None, phases=(0, 0, 0)):
    b_base = a.n if b_base is None else b_base
    want = expected_merge(a, b, b_base)

    def body(fill):
        c = Call(codec, a, b, fill, phases)
        assert c.run(b_base) == 0
        c.check(want)

    guards.twice(body)
    return want


def merge_of_columns(codec, ka, sta, kb, stb, phases=(0, 0, 0)):
    """Sides from key and status columns: the merge must equal the sort of the concatenation."""
    a, b = side_of(ka, sta), side_of(kb, stb)
    S, order, valid = merge_and_check(codec, a, b, phases=phases)
    k = np.concatenate([a_rows(ka), a_rows(kb)])
    st = np.concatenate([np.zeros(len(ka), np.int32) if sta is None else sta,
                         np.zeros(len(kb), np.int32) if stb is None else stb])
    sort_order, sort_valid = expected_order(k, st)
    assert valid == sort_valid and np.array_equal(order, sort_order) and np.array_equal(S, k[sort_order])
    return S, order, valid


def a_rows(k):
    return np.ascontiguousarray(k, np.uint8).reshape(-1, 29)


# --------------------------------------------------------------------------
# key columns
# --------------------------------------------------------------------------
def random_keys(n, rng):
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def pool_keys(n, rng, pool):
    """n keys drawn from `pool` distinct ones: many ties within and across the sides."""
    return pool[rng.integers(0, len(pool), n)]


def one_byte_keys(n, rng, base, byte):
    """Keys that differ only in byte `byte`, which takes values on both sides of 0x7f/0x80."""
    k = np.tile(base, (n, 1))
    k[:, byte] = rng.choice(np.array([0, 1, 0x7E, 0x7F, 0x80, 0x81, 0xFE, 0xFF], np.uint8), n)
    return k


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
NA = (0, 1, 2, "T-1", "T", "T+1")
NB = (0, 1, 63, "T", "3T+5")


def size_of(T, s):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[s] if isinstance(s, str) else s


@pytest.mark.parametrize("sa", NA)
def test_sizes(codec, T, sa):
    """Random 29-byte keys, every na against every nb."""
    na = size_of(T, sa)
    for j, sb in enumerate(NB):
        nb = size_of(T, sb)
        rng = np.random.default_rng(7000 + 10 * na + j)
        S, order, valid = merge_of_columns(codec, random_keys(na, rng), None, random_keys(nb, rng), None,
                                           phases=PHASES[(NA.index(sa) + j) % len(PHASES)])
        assert valid == na + nb and sorted(order.tolist()) == list(range(na + nb))


@pytest.mark.parametrize("na,nb", [(4097, 63), (6000, 6000)])
def test_split_over_a_long_bracket(codec, T, na, nb):
    """The tile's split is a wave search over the bracket [max(d - nb, 0),
    min(d, na)) of a diagonal d. 4097 rows against 63: a long column beside a
    short one, the bracket never above 63 rows. 6000 against 6000: the diagonal
    5 T = 5120 has the bracket [0, 5120), above the 4160 rows from which the
    search takes a third step (64 mids a step: a bracket of s > 64 rows leaves
    at most ceil(s / 64) - 1)."""
    rng = np.random.default_rng(7100 + na)
    S, order, valid = merge_of_columns(codec, random_keys(na, rng), None, random_keys(nb, rng), None, phases=PHASES[1])
    assert valid == na + nb and sorted(order.tolist()) == list(range(na + nb))


def test_diagonal_extremes(codec, T):
    """Every A key below every B key, then every B key below every A key."""
    rng = np.random.default_rng(61)
    na, nb = 2 * T + 3, T + 1
    lo, hi = random_keys(na, rng), random_keys(nb, rng)
    lo[:, 0] &= 0x7F
    hi[:, 0] |= 0x80
    S, order, _ = merge_of_columns(codec, lo, None, hi, None, phases=PHASES[1])
    assert (order[:na] < na).all() and (order[na:] >= na).all()
    lo, hi = random_keys(nb, rng), random_keys(na, rng)
    lo[:, 0] &= 0x7F
    hi[:, 0] |= 0x80
    S, order, _ = merge_of_columns(codec, hi, None, lo, None, phases=PHASES[2])  # A = hi (na rows), B = lo
    assert (order[:nb] >= na).all() and (order[nb:] < na).all()


def test_all_keys_equal(codec, T):
    """One run of 3T + 5 equal keys over four tiles: A's indices, then B's, each ascending."""
    rng = np.random.default_rng(62)
    key = random_keys(1, rng)
    for na in (T + T // 2, 1, 3 * T + 4, T):
        nb = 3 * T + 5 - na
        _, order, valid = merge_of_columns(codec, np.tile(key, (na, 1)), None, np.tile(key, (nb, 1)), None,
                                           phases=PHASES[na % len(PHASES)])
        assert valid == 3 * T + 5 and np.array_equal(order, np.arange(3 * T + 5, dtype=np.uint32))


def test_two_runs_straddle_tile_boundaries(codec, T):
    """Two distinct keys, both in both sides; the merged runs are [0, 1.5T - 4)
    and [1.5T - 4, 3T + 5): the first crosses position T inside its B part, the
    second 2T and 3T."""
    rng = np.random.default_rng(63)
    k = random_keys(2, rng)
    k = k[np.lexsort(k.T[::-1])]
    na = T + T // 2
    nb = 3 * T + 5 - na
    a1, b1 = T // 2 + 3, T - 7
    ka = np.concatenate([np.tile(k[0], (a1, 1)), np.tile(k[1], (na - a1, 1))])
    kb = np.concatenate([np.tile(k[0], (b1, 1)), np.tile(k[1], (nb - b1, 1))])
    for perm_seed in (None, 1):  # the sides' columns in sorted order, then shuffled (the sort's order is not the identity)
        if perm_seed is not None:
            ka, kb = ka[rng.permutation(na)], kb[rng.permutation(nb)]
        a, b = side_of(ka), side_of(kb)
        _, order, _ = merge_of_columns(codec, ka, None, kb, None, phases=PHASES[3])
        want = np.concatenate([a.order[:a1], b.order[:b1] + na, a.order[a1:], b.order[b1:] + na])
        assert np.array_equal(order, want)
        for lo, hi in ((0, a1), (a1, a1 + b1), (a1 + b1, na + b1), (na + b1, na + nb)):
            assert (np.diff(order[lo:hi].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("byte", [28, 0, 16, 13, 14, 15, 12, 17])
def test_discriminating_byte(codec, T, byte):
    """Keys that differ only in one byte: the last, the first, the ObjectPrefix
    edge (16 / 17) and the overlap of the two 16-byte loads (13-15)."""
    rng = np.random.default_rng(640 + byte)
    base = random_keys(1, rng)
    merge_of_columns(codec, one_byte_keys(T + 37, rng, base, byte), None, one_byte_keys(T // 2 + 5, rng, base, byte),
                     None, phases=PHASES[byte % len(PHASES)])


def statuses(n, rng, which):
    if which == "all":
        return np.full(n, 8, np.int32)
    st = np.zeros(n, np.int32)
    st[rng.integers(0, 5, n) == 0] = 8
    return st


@pytest.mark.parametrize("bad_a,bad_b", [("fifth", "fifth"), ("all", "fifth"), ("fifth", "all"), ("all", "all")])
def test_invalid_rows(codec, T, bad_a, bad_b):
    """About 1/5 of each side invalid, or all of it: the tail is A's invalid
    rows then B's, bytes as they stand, indices unchanged / + b_base. The keys
    come from a small pool, so invalid rows equal valid ones."""
    rng = np.random.default_rng(65 + len(bad_a) + 2 * len(bad_b))
    pool = random_keys(200, rng)
    na, nb = T + 300, 2 * T - 11
    ka, kb = pool_keys(na, rng, pool), pool_keys(nb, rng, pool)
    sta, stb = statuses(na, rng, bad_a), statuses(nb, rng, bad_b)
    S, order, valid = merge_of_columns(codec, ka, sta, kb, stb, phases=PHASES[1])
    ia, ib = np.flatnonzero(sta != 0), np.flatnonzero(stb != 0)
    assert valid == na + nb - len(ia) - len(ib)
    assert np.array_equal(order[valid:], np.concatenate([ia, ib + na]).astype(np.uint32))
    assert np.array_equal(S[valid:], np.concatenate([ka[ia], kb[ib]]))


def test_valid_count_above_n_is_clamped(codec, T):
    rng = np.random.default_rng(66)
    a, b = side_of(random_keys(T + 9, rng)), side_of(random_keys(70, rng))
    want = merge_and_check(codec, a, b)
    for da, db in ((5, 0), (0, 1 << 40), (1 << 63, 3)):
        a2, b2 = Side(a.S, a.order, a.n + da), Side(b.S, b.order, b.n + db)
        got = merge_and_check(codec, a2, b2, phases=PHASES[2])
        assert got[2] == a.n + b.n and all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2]))


def test_b_base(codec, T):
    """b_base is what B's indices get, whatever na is."""
    rng = np.random.default_rng(67)
    pool = random_keys(50, rng)
    ka, kb = pool_keys(T + 1, rng, pool), pool_keys(333, rng, pool)
    a, b = side_of(ka, statuses(len(ka), rng, "fifth")), side_of(kb, statuses(len(kb), rng, "fifth"))
    for b_base in (0, 5000, (1 << 32) - 1 - b.n):
        S, order, valid = merge_and_check(codec, a, b, b_base=b_base, phases=PHASES[3])
        both = np.concatenate([a.order.astype(np.uint64), b.order.astype(np.uint64) + b_base])
        assert np.array_equal(np.sort(order.astype(np.uint64)), np.sort(both))  # A's as they are, B's shifted


def test_no_order(codec, T):
    """d_order_out = NULL: the column and the count as before, the input orders ignored."""
    rng = np.random.default_rng(68)
    pool = random_keys(100, rng)
    a = side_of(pool_keys(2 * T + 3, rng, pool), statuses(2 * T + 3, rng, "fifth"))
    b = side_of(pool_keys(T - 1, rng, pool), statuses(T - 1, rng, "fifth"))
    want = expected_merge(a, b, a.n)

    def body(fill):
        for input_orders in (False, True):
            c = Call(codec, a, b, fill, PHASES[1])
            assert c.run(a.n, with_order=False, input_orders=input_orders) == 0
            c.check(want, with_order=False)

    guards.twice(body)


def test_graph_capture_and_a_new_valid_count(codec, T):
    """One merge captured and replayed; then A's valid count lowered on the
    device (its rows from there on are then A's tail, as they stand) and the
    same graph replayed."""
    rng = np.random.default_rng(69)
    pool = random_keys(300, rng)
    a = side_of(pool_keys(2 * T + 40, rng, pool))
    b = side_of(pool_keys(T + 7, rng, pool), statuses(T + 7, rng, "fifth"))
    fewer = Side(a.S, a.order, a.n - T - 13)

    def refill(t, fill):
        """The view back to its pattern, so that what it holds afterwards is the replay's."""
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(codec.torch_device))

    def body(fill):
        c = Call(codec, a, b, fill, PHASES[2])
        assert c.run(a.n) == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run(a.n) == 0
        for t in (c.out, c.order, c.valid):
            refill(t, fill)
        g.replay()
        c.check(expected_merge(a, b, a.n))
        for t in (c.out, c.order, c.valid):
            refill(t, fill)
        c.va.copy_(torch.from_numpy(np.array([fewer.valid], np.uint64).view(np.uint8)).to(codec.torch_device))
        g.replay()
        torch.cuda.synchronize()
        c.a = fewer  # (inputs_unchanged compares the same column and order)
        c.check(expected_merge(fewer, b, a.n))

    guards.twice(body)


def test_refusals_store_nothing(codec, T):
    rng = np.random.default_rng(70)
    a, b = side_of(random_keys(300, rng)), side_of(random_keys(70, rng))
    want = expected_merge(a, b, a.n)

    def body(fill):
        c = Call(codec, a, b, fill, (1, 3, 1))
        A = guards.address
        base = dict(ctx=codec.ctx, sa=A(c.sa), oa=A(c.oa), va=A(c.va), na=a.n, sb=A(c.sb), ob=A(c.ob), vb=A(c.vb),
                    nb=b.n, b_base=a.n, out=A(c.out), order=A(c.order), valid=A(c.valid))

        def call(**kw):
            x = dict(base, **kw)
            return codec.lib.honu_key_merge(x["ctx"], x["sa"], x["oa"], x["va"], x["na"], x["sb"], x["ob"], x["vb"],
                                            x["nb"], x["b_base"], x["out"], x["order"], x["valid"], codec.stream)

        # refused before any launch, whatever the fake counts would index
        for kw in (dict(na=(1 << 32) - b.n), dict(na=1 << 32), dict(nb=1 << 32, b_base=0), dict(na=(1 << 64) - 1),
                   dict(na=(1 << 32) - 1, nb=1, b_base=0)):
            assert call(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(va=0), dict(vb=0), dict(valid=0), dict(sa=0), dict(sb=0), dict(out=0),
                   dict(oa=0), dict(ob=0), dict(oa=0, ob=0), dict(b_base=(1 << 32) - b.n),
                   dict(oa=A(c.oa) + 2), dict(ob=A(c.ob) + 2), dict(order=A(c.order) + 2),
                   dict(va=A(c.va) + 4), dict(vb=A(c.vb) + 4), dict(valid=A(c.valid) + 4)):
            assert call(**kw) == E_ARG, kw
        torch.cuda.synchronize()
        for t in (c.out, c.order, c.valid):
            guards.assert_untouched(t, [])
        # n == 0 writes only the count, columns given or not
        assert call(na=0, nb=0, b_base=0) == 0
        torch.cuda.synchronize()
        assert int(guards.block_of(c.valid).bytes().view(np.uint64)[0]) == 0
        guards.assert_untouched(c.valid, [(0, 8)])
        for t in (c.out, c.order):
            guards.assert_untouched(t, [])
        assert call(na=0, nb=0, b_base=0, sa=0, sb=0, out=0, oa=0, ob=0, order=0) == 0
        assert c.run(a.n) == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)


# --------------------------------------------------------------------------
# equals the sort: sort(A), sort(B), merge, merge, seek on one stream
# --------------------------------------------------------------------------
def key_columns(c, sizes):
    """Generator records of the given batch sizes -> marshal -> decode -> keys:
    [(device key column, device key status, host keys, host status)]. The
    batches share 23 objects; batch 2 repeats keys of batch 0; a few records
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
        if j == 2:  # records 0, 3, 6, ... carry the keys of batch 0's records 0, 5, 10, ...
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


def test_equals_the_sort_and_chains(codec):
    sizes = (300, 77, 129)
    (dka, dsa, ka, sta), (dkb, dsb, kb, stb), (dkc, dsc, kc, stc) = key_columns(codec, sizes)
    na, nb, nc = sizes
    n2, n3 = na + nb, na + nb + nc
    # sort(A), sort(B), merge, merge with C, seek: no synchronisation in between
    oa, sa, va = codec.sort_keys(dka, dsa, n=na, want_sorted=True)
    ob, sb, vb = codec.sort_keys(dkb, dsb, n=nb, want_sorted=True)
    oc, sc, vc = codec.sort_keys(dkc, dsc, n=nc, want_sorted=True)
    s2, o2, v2 = codec.merge_keys(sa[:29 * na], oa, va, sb[:29 * nb], ob, vb)
    s3, o3, v3 = codec.merge_keys(s2, o2, v2, sc[:29 * nc], oc, vc)  # b_base defaults to na + nb
    probes, pstatus = torch.cat([dka, dkb, dkc]), torch.cat([dsa, dsb, dsc])
    rows = codec.seek_keys(s3, v3, probes, 29, probe_status=pstatus, order=o3)
    # the parent's only way to the same result
    w2 = codec.sort_keys(torch.cat([dka, dkb]), torch.cat([dsa, dsb]), n=n2, want_sorted=True)
    w3 = codec.sort_keys(probes, pstatus, n=n3, want_sorted=True)
    torch.cuda.synchronize()
    for (s, o, v), (wo, ws, wv), n, k, st in (
            ((s2, o2, v2), w2, n2, np.concatenate([ka, kb]), np.concatenate([sta, stb])),
            ((s3, o3, v3), w3, n3, np.concatenate([ka, kb, kc]), np.concatenate([sta, stb, stc]))):
        assert s.numel() == 29 * n and o.numel() == n
        assert torch.equal(v, wv) and torch.equal(o, wo) and torch.equal(s, ws[:29 * n])
        order, valid = expected_order(k, st)  # and numpy's
        assert int(v.item()) == valid == n - int((st != 0).sum())
        assert np.array_equal(o.cpu().numpy().view(np.uint32), order)
        assert np.array_equal(s.cpu().numpy().reshape(n, 29), k[order])
    got = rows.cpu().numpy().view(np.uint32)
    st = np.concatenate([sta, stb, stc])
    assert ((got[st != 0, 4] & SEEK_SKIPPED) != 0).all()
    assert ((got[st == 0, 4] & SEEK_FOUND) != 0).all() and 9 <= (st != 0).sum() < n3 // 4
    # a key of A that C puts again: the run's last row, `latest`, is C's record
    k = np.concatenate([ka, kb, kc])
    checked = 0
    for j in range(0, nc, 3):
        i = (j // 3 * 5) % na
        if stc[j] != 0 or sta[i] != 0:
            continue
        assert np.array_equal(ka[i], kc[j])
        same = np.flatnonzero((k == kc[j]).all(axis=1) & (st == 0))
        assert got[i, 3] == got[n2 + j, 3] == same.max() >= n2 and got[i, 2] == same.min() < na
        checked += 1
    assert checked >= 30
    # Codec.merge_keys without orders merges the column alone
    s, o, v = codec.merge_keys(sa[:29 * na], None, va, sb[:29 * nb], None, vb)
    assert o is None and torch.equal(s, s2) and torch.equal(v, v2)
