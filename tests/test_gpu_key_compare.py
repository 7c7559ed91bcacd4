"""honu_key_compare on the GPU against numpy and keys.compare.

The expectation is the host's alone: keys.compare (honu_amd/keys.py, itself
checked against an independent simulation in tests/test_key_compare_host.py)
over the first min(valid, n) rows of both columns, laid out with numpy as
honu_seek rows, peer rows and counts; the objects of A (d_obj_off_a,
d_objects_a) are cut with numpy where the first 17 bytes change. It never
calls the library. Every input and output is a guarded view (tests/guards.py)
under both fills, the two columns at byte phases 0, 1 and 3; the write set is
exactly d_out[0, objects), d_peer[0, objects), d_counts[0, 8) and the
workspace, whose size is exactly honu_key_compare_workspace(na), and the
inputs are unchanged. Sizes are in units of T and S, the params
"compare_tile" (objects per workgroup) and "compare_stage" (the rows of B a
workgroup stages in LDS; a longer bracket is searched in global memory).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import (CMP_ANCESTOR, CMP_EARLIER, CMP_EQUAL, CMP_LATER, CMP_PEER_HAS, SEEK_DTYPE,  # noqa: E402
                               SEEK_FOUND, SEEK_NONE, Scalar)
from honu_amd.workload import gen_host_batch  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
OK = hobj.OK
PHASES = ((0, 0), (1, 3), (3, 1), (0, 1))  # (d_sorted_a, d_sorted_b)
MAX_RECORDS = 4096
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


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
    t = _param(codec, b"compare_tile")
    assert 64 <= t <= 1024
    return t


@pytest.fixture(scope="module")
def S(codec, T):
    s = _param(codec, b"compare_stage")
    assert T <= s <= 4096
    return s


# --------------------------------------------------------------------------
# columns
# --------------------------------------------------------------------------
def oid(j: int) -> bytes:
    """Object IDs that ascend with j; every fifth ends in 0xff, every seventh in 0x00."""
    tail = bytes([0xFF]) if j % 5 == 0 else (bytes([0x00]) if j % 7 == 0 else bytes([(j * 37) & 0xFF]))
    return bytes([0x20]) + j.to_bytes(3, "big") + bytes([(j * 131 + k) & 0xFF for k in range(11)]) + tail


def scalars(rng, m):
    """m distinct scalars in lamport order, every byte of the 12 in use."""
    vids = sorted({int(v) for v in rng.integers(1, 1 << 63, 2 * m + 4, dtype=np.uint64)})[:m]
    vids[0] = vids[0] & 0xFF  # a small VID among them
    vids.sort()
    return [Scalar(PID=int(rng.integers(0, 1 << 32)), VID=v) for v in vids]


SCENARIOS = ("only mine", "equal", "later ancestor", "later fork", "earlier ancestor", "earlier fork",
             "equal runs", "later ancestor runs")


def object_pair(rng, scenario, m):
    """(my scalars, the peer's), each in order, of one object: m >= 3 distinct scalars V dealt out by the scenario."""
    V = scalars(rng, m)
    k = int(rng.integers(1, m))  # 1 <= k < m
    if scenario == "only mine":
        return V, []
    if scenario == "equal":
        return V, V
    if scenario == "later ancestor":
        return V, V[:k]
    if scenario == "later fork":  # the peer's latest, V[1], is no row of mine
        return V[:1] + V[2:], V[:2]
    if scenario == "earlier ancestor":
        return V[:k], V
    if scenario == "earlier fork":  # my latest, V[0], is no row of the peer's
        return V[:1], V[1:]
    if scenario == "equal runs":
        return V + [V[-1]] * 2, V + [V[-1]]
    if scenario == "later ancestor runs":  # runs of the decisive key on both sides
        return V[:k] + [V[k - 1]] + V[k:], V[:k] + [V[k - 1]] * 2
    raise ValueError(scenario)


def make_pair(objects, seed, peer_only=True):
    """(a, b): sorted lists of keys; `objects` objects in a, every scenario
    among them as soon as there are eight, about a fifth with one version; b
    also holds objects that a lacks, between a's."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for j in range(objects):
        i = oid(2 * j)
        if rng.random() < 0.2:
            v = scalars(rng, 1)
            mine, theirs = v, (v if j % 2 else [])
        else:
            mine, theirs = object_pair(rng, SCENARIOS[j % len(SCENARIOS)], int(rng.integers(3, 6)))
        a += [hkeys.new(i, s) for s in mine]
        b += [hkeys.new(i, s) for s in theirs]
        if peer_only and j % 3 == 0:
            b += [hkeys.new(oid(2 * j + 1), s) for s in scalars(rng, 2)]
    return sorted(a), sorted(b)


def rows_of(keys, tail=0):
    """(n, 29) bytes: the keys, then `tail` invalid rows whose bytes equal live keys (noise where there is none)."""
    v = len(keys)
    rows = np.frombuffer(b"".join(keys), np.uint8).reshape(v, 29).copy() if v else np.zeros((0, 29), np.uint8)
    if tail:
        extra = rows[np.arange(tail) * 7 % v] if v else np.random.default_rng(3).integers(0, 256, (tail, 29), dtype=np.uint8)
        rows = np.concatenate([rows, extra])
    return rows


def objects_of(rows, valid):
    """(d_obj_off_a: na + 1 values of which objects + 1 are set, the others noise; objects) as honu_key_objects cuts them."""
    na = len(rows)
    v = min(valid, na)
    cut = np.flatnonzero((rows[1:v, :17] != rows[:v - 1, :17]).any(axis=1)) + 1 if v > 1 else np.zeros(0, np.int64)
    starts = np.concatenate([[0], cut]) if v else np.zeros(0, np.int64)
    off = np.full(na + 1, 0xDEADBEEFDEADBEEF, np.uint64)
    off[:len(starts)] = starts
    off[len(starts)] = v
    return off, len(starts)


def expected(a_rows, va, b_rows, vb, order=None):
    """(honu_seek rows, peer rows, counts) of keys.compare over the valid rows."""
    a = [bytes(r) for r in a_rows[:min(va, len(a_rows))]]
    b = [bytes(r) for r in b_rows[:min(vb, len(b_rows))]]
    res = hkeys.compare(a, b)
    out = np.zeros(len(res), SEEK_DTYPE)
    out["first"] = out["latest"] = SEEK_NONE
    peer = np.full(len(res), SEEK_NONE, np.uint32)
    for j, g in enumerate(res):
        out["pos"][j], out["end"][j], out["flags"][j] = g.pos, g.end, g.flags
        if order is not None and g.pos < g.end:
            out["first"][j], out["latest"][j] = order[g.pos], order[g.end - 1]
        if g.peer is not None:
            peer[j] = g.peer
    f = out["flags"]
    has, anc = (f & CMP_PEER_HAS) != 0, (f & CMP_ANCESTOR) != 0
    counts = np.array([len(res), (~has).sum(), (has & ((f & CMP_LATER) != 0)).sum(), ((f & CMP_EARLIER) != 0).sum(),
                       ((f & CMP_EQUAL) != 0).sum(), (has & ~anc).sum(), 0, 0], np.uint64)
    return out, peer, counts


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
    """The guarded device arguments of one call. order None / peer False / counts False: the pointer is NULL."""

    def __init__(self, codec, a_rows, va, b_rows, vb, fill, phases=(0, 0), order=None, peer=True, counts=True,
                 obj=None):
        self.codec, self.na, self.nb = codec, len(a_rows), len(b_rows)
        off, objects = objects_of(a_rows, va) if obj is None else obj
        self.objects = min(int(objects), self.na)
        self.host = {"sorted_a": a_rows, "valid_a": u64(va), "obj_off": off, "objects": u64(objects),
                     "sorted_b": b_rows, "valid_b": u64(vb)}
        if order is not None:
            self.host["order"] = np.asarray(order, np.uint32)
        phase = {"sorted_a": phases[0], "sorted_b": phases[1]}
        self.dev = {k: put(codec, a, phase.get(k, 0), fill) for k, a in self.host.items()}
        dev = codec.torch_device
        self.work_bytes = int(codec.lib.honu_key_compare_workspace(self.na))
        self.out = guards.guarded(20 * self.na, fill=fill, device=dev)
        self.peer = guards.guarded(4 * self.na, fill=fill, device=dev) if peer else None
        self.counts = guards.guarded(64, fill=fill, device=dev) if counts else None
        self.work = guards.guarded(self.work_bytes, fill=fill, device=dev)
        self.outs = [t for t in (self.out, self.peer, self.counts, self.work) if t is not None]

    def args(self, **kw):
        A = guards.address
        d = self.dev
        x = dict(ctx=self.codec.ctx, sorted_a=A(d["sorted_a"]), order=A(d.get("order")), valid_a=A(d["valid_a"]),
                 na=self.na, obj_off=A(d["obj_off"]), objects=A(d["objects"]), sorted_b=A(d["sorted_b"]),
                 valid_b=A(d["valid_b"]), nb=self.nb, out=A(self.out), peer=A(self.peer), counts=A(self.counts),
                 work=A(self.work), work_bytes=self.work_bytes)
        x.update(kw)
        return x

    def run(self, **kw):
        x = self.args(**kw)
        return self.codec.lib.honu_key_compare(
            x["ctx"], x["sorted_a"], x["order"], x["valid_a"], x["na"], x["obj_off"], x["objects"], x["sorted_b"],
            x["valid_b"], x["nb"], x["out"], x["peer"], x["counts"], x["work"], x["work_bytes"], self.codec.stream)

    def inputs_unchanged(self):
        for k, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[k]).tobytes(), k
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs:
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def write_set(self, objects=None):
        k = self.objects if objects is None else objects
        guards.assert_untouched(self.out, [(0, 20 * k)])
        if self.peer is not None:
            guards.assert_untouched(self.peer, [(0, 4 * k)])
        if self.counts is not None:
            guards.assert_untouched(self.counts, [(0, 64)])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        self.inputs_unchanged()

    def results(self):
        """(rows, peer or None, counts or None) as the device holds them: the first `objects` rows."""
        k = self.objects
        out = guards.block_of(self.out).bytes()[:20 * k].view(SEEK_DTYPE)
        peer = guards.block_of(self.peer).bytes()[:4 * k].view(np.uint32) if self.peer is not None else None
        counts = guards.block_of(self.counts).bytes().view(np.uint64) if self.counts is not None else None
        return out, peer, counts

    def check(self, want):
        torch.cuda.synchronize()
        out, peer, counts = want
        assert self.objects == len(out)
        got, got_peer, got_counts = self.results()
        bad = np.flatnonzero(got != out)
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], out[bad[:4]])
        if got_peer is not None:
            bad = np.flatnonzero(got_peer != peer)
            assert not len(bad), (len(bad), bad[:4], got_peer[bad[:4]], peer[bad[:4]])
        if got_counts is not None:
            assert got_counts.tolist() == counts.tolist()
        self.write_set()


def compare_and_check(codec, a_rows, va, b_rows, vb, phases=(0, 0), order=None, peer=True, counts=True):
    """One call under both fills against the host's answer, which it returns."""
    want = expected(a_rows, va, b_rows, vb, order)

    def body(fill):
        c = Call(codec, a_rows, va, b_rows, vb, fill, phases, order, peer, counts)
        assert c.run() == 0
        c.check(want)

    guards.twice(body)
    return want


def an_order(n, seed=8):
    """Record indices for the positions: any 32-bit values, the call only passes them on."""
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def classes_of(want):
    return {int(f) & ~SEEK_FOUND for f in want[0]["flags"]}


EVERY_CLASS = {CMP_LATER, CMP_LATER | CMP_PEER_HAS, CMP_LATER | CMP_PEER_HAS | CMP_ANCESTOR, CMP_EARLIER | CMP_PEER_HAS,
               CMP_EARLIER | CMP_PEER_HAS | CMP_ANCESTOR, CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR}


# --------------------------------------------------------------------------
# 1. object counts, and a peer of no row and of one
# --------------------------------------------------------------------------
@pytest.mark.parametrize("size", ("1", "T-1", "T", "T+1", "2*T+3"))
def test_object_counts(codec, T, size):
    objects = eval(size, {"T": T})
    a, b = make_pair(objects, 10 + objects % 13)
    a_rows, b_rows = rows_of(a), rows_of(b)
    for j, vb in enumerate((len(b), 0, 1)):
        want = compare_and_check(codec, a_rows, len(a), b_rows, vb, PHASES[j], an_order(len(a)))
        assert len(want[0]) == objects and int(want[2][0]) == objects
        if vb == 0:
            assert classes_of(want) == {CMP_LATER} and (want[0]["pos"] < want[0]["end"]).all()
        elif objects >= 8 and vb == len(b):
            assert classes_of(want) == EVERY_CLASS
    # a peer's column of one row, and of none
    compare_and_check(codec, a_rows, len(a), b_rows[:1], 1, PHASES[1], an_order(len(a)))
    compare_and_check(codec, a_rows, len(a), b_rows[:0], 0, PHASES[2])


def test_no_objects(codec):
    """va == 0 over a column of rows: no row is written. na == 0: only the counts are, zeros."""
    a, b = make_pair(20, 11)
    want = compare_and_check(codec, rows_of([], tail=40), 0, rows_of(b), len(b), PHASES[1], an_order(40))
    assert len(want[0]) == 0 and want[2].tolist() == [0] * 8
    b_rows = rows_of(b)

    def body(fill):
        c = Call(codec, rows_of([]), 0, b_rows, len(b), fill, PHASES[2])
        assert c.work_bytes == 0
        assert c.run() == 0 and c.run(work=0, sorted_a=0, out=0, order=0) == 0
        torch.cuda.synchronize()
        assert guards.block_of(c.counts).bytes().view(np.uint64).tolist() == [0] * 8
        c.write_set(0)
        d = Call(codec, rows_of([]), 0, b_rows, len(b), fill, counts=False)
        assert d.run() == 0
        d.nothing_stored()

    guards.twice(body)


# --------------------------------------------------------------------------
# 2. the staging boundary
# --------------------------------------------------------------------------
def staged_pair(T, per_tile, heavy=False):
    """Objects in tiles of T; the peer holds per_tile[t] rows of tile t's
    objects and of no other, so that is the tile's bracket: dealt evenly, or
    with `heavy` all but one each to the tile's first object. Object j of a
    holds, by j % 4, the peer's latest version (equal), that and the next
    (later, ancestor), only the next (later, fork), or the peer's first
    (earlier, ancestor; equal where the peer has one)."""
    a, b = [], []
    for t, rows in enumerate(per_tile):
        for r in range(T):
            j = t * T + r
            if heavy:
                c = rows - (T - 1) if r == 0 else 1
            else:
                c = rows // T + (1 if r < rows % T else 0)
            i = oid(j)
            b += [hkeys.new(i, Scalar(PID=7, VID=v)) for v in range(1, c + 1)]
            mine = ([c], [c, c + 1], [c + 1], [1])[j % 4] if c else [1]
            a += [hkeys.new(i, Scalar(PID=7, VID=v)) for v in mine]
    a += [hkeys.new(oid(len(per_tile) * T + r), Scalar(1, 1)) for r in range(3)]  # a third tile of three objects
    return sorted(a), sorted(b)


@pytest.mark.parametrize("heavy", (False, True))
def test_bracket_of_S_and_of_S_plus_1_rows(codec, T, S, heavy):
    """A tile whose bracket in B has S rows is staged, one of S + 1 rows is searched in global memory; both
    orders, so each path runs beside the other in one launch."""
    for j, per_tile in enumerate(((S, S + 1), (S + 1, S))):
        a, b = staged_pair(T, per_tile, heavy)
        assert len(b) == 2 * S + 1
        want = compare_and_check(codec, rows_of(a), len(a), rows_of(b), len(b), PHASES[j + 1], an_order(len(a)))
        assert len(want[0]) == 2 * T + 3
        assert classes_of(want) >= {CMP_LATER, CMP_LATER | CMP_PEER_HAS, CMP_LATER | CMP_PEER_HAS | CMP_ANCESTOR,
                                    CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR}
        if not heavy:
            assert CMP_EARLIER | CMP_PEER_HAS | CMP_ANCESTOR in classes_of(want)


# --------------------------------------------------------------------------
# 3. invalid tails and valid counts
# --------------------------------------------------------------------------
def test_invalid_tails_equal_live_keys(codec, T):
    a, b = make_pair(T + 9, 30)
    a_rows, b_rows = rows_of(a, tail=33), rows_of(b, tail=17)
    whole = compare_and_check(codec, a_rows, len(a), b_rows, len(b), PHASES[1], an_order(len(a_rows)))
    assert np.array_equal(whole[0], expected(rows_of(a), len(a), rows_of(b), len(b), an_order(len(a_rows)))[0])
    # fewer valid rows than keys: the cut falls inside an object of either side
    for j, (va, vb) in enumerate(((len(a) - 5, len(b)), (len(a), len(b) - 7), (len(a) // 2, len(b) // 3))):
        compare_and_check(codec, a_rows, va, b_rows, vb, PHASES[j], an_order(len(a_rows)))


def test_valid_counts_above_n(codec):
    a, b = make_pair(40, 31)
    a_rows, b_rows = rows_of(a), rows_of(b)
    base = expected(a_rows, len(a), b_rows, len(b))
    for j, (va, vb) in enumerate(((len(a) + 5, len(b) + 5), (1 << 40, M64), (M64, 1 << 32))):
        # (d_objects_a above na is clamped as well)
        def body(fill):
            off, objects = objects_of(a_rows, len(a))
            c = Call(codec, a_rows, va, b_rows, vb, fill, PHASES[j], obj=(off, objects))
            assert c.run() == 0
            c.check(base)

        guards.twice(body)


# --------------------------------------------------------------------------
# 4. every flag combination, runs at the decisive positions
# --------------------------------------------------------------------------
def test_flag_combinations_by_hand(codec):
    def K(j, vid, pid=0):
        return hkeys.new(oid(j), Scalar(PID=pid, VID=vid))

    cases = [  # (mine, the peer's, pos - a0, flags without FOUND)
        ([K(0, 1)], [], 0, CMP_LATER),
        ([K(1, 1), K(1, 2), K(1, 2), K(1, 3), K(1, 3)], [K(1, 1), K(1, 2), K(1, 2), K(1, 2)], 3,
         CMP_LATER | CMP_PEER_HAS | CMP_ANCESTOR),
        ([K(2, 1), K(2, 3)], [K(2, 1), K(2, 2), K(2, 2)], 1, CMP_LATER | CMP_PEER_HAS),
        ([K(3, 10, 10)], [K(3, 10, 1)], 0, CMP_LATER | CMP_PEER_HAS),  # the PID breaks the tie
        ([K(4, 1), K(4, 2), K(4, 2)], [K(4, 1), K(4, 2), K(4, 3)], 3, CMP_EARLIER | CMP_PEER_HAS | CMP_ANCESTOR),
        ([K(5, 1), K(5, 2, 7)], [K(5, 1), K(5, 2, 9), K(5, 3, 9)], 2, CMP_EARLIER | CMP_PEER_HAS),
        ([K(6, 1), K(6, M64, M32), K(6, M64, M32)], [K(6, M64, M32)] * 3, 3, CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR),
        ([K(7, M64, M32)], [K(7, M64, M32 - 1)], 0, CMP_LATER | CMP_PEER_HAS),
        ([K(8, 0, 0)], [K(8, 0, 0)], 1, CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR),
    ]
    a = [k for mine, _, _, _ in cases for k in mine]
    b = [k for _, theirs, _, _ in cases for k in theirs]
    assert a == sorted(a) and b == sorted(b)
    want = compare_and_check(codec, rows_of(a, 4), len(a), rows_of(b, 4), len(b), PHASES[1], an_order(len(a) + 4))
    a0 = 0
    for (mine, theirs, rel, flags), row, peer in zip(cases, want[0], want[1]):
        end = a0 + len(mine)
        assert (row["pos"], row["end"]) == (a0 + rel, end)
        assert row["flags"] == flags | (SEEK_FOUND if a0 + rel < end else 0)
        assert peer == (b.index(theirs[-1]) + theirs.count(theirs[-1]) - 1 if theirs else SEEK_NONE)
        a0 = end
    assert classes_of(want) == EVERY_CLASS
    assert want[2].tolist() == [9, 1, 4, 2, 2, 4, 0, 0]


# --------------------------------------------------------------------------
# 5. the optional arrays
# --------------------------------------------------------------------------
def test_optional_arrays(codec, T):
    a, b = make_pair(T + 5, 50)
    a_rows, b_rows = rows_of(a, 3), rows_of(b, 3)
    order = an_order(len(a_rows))
    full = compare_and_check(codec, a_rows, len(a), b_rows, len(b), PHASES[1], order, True, True)
    for order_, peer, counts in ((None, True, True), (order, False, True), (order, True, False), (None, False, False)):
        want = compare_and_check(codec, a_rows, len(a), b_rows, len(b), PHASES[2], order_, peer, counts)
        for f in ("pos", "end", "flags"):
            assert np.array_equal(want[0][f], full[0][f])
        if order_ is None:
            assert (want[0]["first"] == SEEK_NONE).all() and (want[0]["latest"] == SEEK_NONE).all()
    found = (full[0]["flags"] & SEEK_FOUND) != 0
    assert found.any() and (~found).any()
    assert np.array_equal(full[0]["first"][found], order[full[0]["pos"][found]])
    assert np.array_equal(full[0]["latest"][found], order[full[0]["end"][found] - 1])
    assert (full[0]["first"][~found] == SEEK_NONE).all() and (full[0]["latest"][~found] == SEEK_NONE).all()


# --------------------------------------------------------------------------
# 6. garbage in the offsets and the counts
# --------------------------------------------------------------------------
def test_garbage_offsets_stay_inside(codec, T):
    """Offsets that descend, lie beyond va, or are noise, and an object count
    beyond na: the rows may be wrong, but nothing is touched outside the write
    set and pos <= end <= va holds."""
    a, b = make_pair(T + 40, 60)
    a_rows, b_rows = rows_of(a, 6), rows_of(b, 6)
    na, va = len(a_rows), len(a)
    good, objects = objects_of(a_rows, va)
    rng = np.random.default_rng(61)
    descending = good.copy()
    descending[:objects + 1] = good[:objects + 1][::-1]
    beyond = good.copy()
    beyond[:objects + 1] += np.uint64(va)
    beyond[3] = M64
    noise = rng.integers(0, 1 << 63, na + 1, dtype=np.uint64)
    noise[::2] = rng.integers(0, na + 3, len(noise[::2]))
    zeros = np.zeros(na + 1, np.uint64)
    for j, (off, objs, valid) in enumerate(((descending, objects, va), (beyond, objects, va), (noise, na, va),
                                            (noise, M64, va + 100), (zeros, na, va), (good, objects, 3))):
        def body(fill):
            c = Call(codec, a_rows, valid, b_rows, len(b), fill, PHASES[j % 4], an_order(na), obj=(off, objs))
            assert c.run() == 0
            torch.cuda.synchronize()
            c.write_set()
            rows, peer, counts = c.results()
            v = min(valid, na)
            assert len(rows) == min(objs, na)
            assert (rows["pos"] <= rows["end"]).all() and (rows["end"] <= v).all()
            assert ((peer == SEEK_NONE) | (peer < len(b))).all()
            assert int(counts[0]) == min(objs, na) and counts[6] == counts[7] == 0
            assert int(counts[1:5].sum()) <= min(objs, na)

        guards.twice(body)


# --------------------------------------------------------------------------
# 7. refusals
# --------------------------------------------------------------------------
def test_refusals_store_nothing(codec, T):
    a, b = make_pair(T + 3, 70)
    a_rows, b_rows = rows_of(a, 2), rows_of(b, 2)
    order = an_order(len(a_rows))
    want = expected(a_rows, len(a), b_rows, len(b), order)

    def body(fill):
        c = Call(codec, a_rows, len(a), b_rows, len(b), fill, (1, 3), order)
        x = c.args()
        for kw in (dict(na=1 << 32), dict(nb=1 << 32), dict(na=M64), dict(nb=M64)):
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(valid_a=0), dict(valid_b=0), dict(obj_off=0), dict(objects=0),
                   dict(sorted_a=0), dict(sorted_b=0), dict(out=0), dict(work_bytes=c.work_bytes - 1),
                   dict(work_bytes=0), dict(work=0), dict(work=x["work"] + 128), dict(out=x["out"] + 2),
                   dict(peer=x["peer"] + 2), dict(order=x["order"] + 2), dict(counts=x["counts"] + 4),
                   dict(obj_off=x["obj_off"] + 4), dict(objects=x["objects"] + 4), dict(valid_a=x["valid_a"] + 4),
                   dict(valid_b=x["valid_b"] + 4)):
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run() == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)


# --------------------------------------------------------------------------
# 8. determinism
# --------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(codec, T, S):
    a, b = staged_pair(T, (S, S + 1))
    a_rows, b_rows = rows_of(a, 5), rows_of(b, 5)

    def body(fill):
        c = Call(codec, a_rows, len(a), b_rows, len(b), fill, (3, 1), an_order(len(a_rows)))
        seen = []
        for _ in range(2):
            assert c.run() == 0
            torch.cuda.synchronize()
            seen.append([guards.block_of(t).bytes().tobytes() for t in c.outs])
        assert seen[0] == seen[1]
        c.write_set()

    guards.twice(body)


# --------------------------------------------------------------------------
# 9. the chain: objects -> compare -> list -> fetch in a graph, against compare -> scan -> fetch on the host
# --------------------------------------------------------------------------
def chain_batch(n, objects=23):
    """Generator Small records of `objects` objects, no two versions alike."""
    rng = np.random.default_rng(100)
    oids = rng.integers(0, 256, (objects, 16), dtype=np.uint8)
    hb = gen_host_batch(101, "small", 0, n)
    hb.meta["object_id"] = oids[rng.integers(0, objects, n)]
    hb.meta["vid"] = rng.permutation(n) + 1
    hb.meta["pid"] = rng.integers(1, 4, n)
    return hb


def test_compare_list_fetch_chain_in_a_graph(codec):
    n = 200
    hb = chain_batch(n)
    dev = codec.torch_device
    enc = codec.marshal(hobj.DeviceBatch.from_host(hb, dev))
    rec_bytes = int(enc.out_off.view(torch.int64)[n].item())
    d1 = codec.decode(enc.out, enc.out_off, n, rec_bytes=rec_bytes)
    dk, dst = codec.keys(d1)
    dk, dst = dk[:29 * n], dst[:4 * n]
    order, col, valid = codec.sort_keys(dk, dst, n=n, want_sorted=True)
    col = col[:29 * n]
    # the peer holds about three records in five
    pick = np.flatnonzero(np.random.default_rng(102).random(n) < 0.6)
    nb = len(pick)
    ipick = torch.tensor(pick, device=dev)
    pk = dk.view(n, 29)[ipick].reshape(-1).contiguous()
    pst = dst.view(torch.int32)[ipick].contiguous().view(torch.uint8)
    _, col_b, valid_b = codec.sort_keys(pk, pst, n=nb, want_sorted=True)
    col_b = col_b[:29 * nb]
    cap = n
    torch.cuda.synchronize()
    va0, vb0 = int(valid.item()), int(valid_b.item())
    assert va0 == n and vb0 == nb

    def chain():  # nothing is read on the host in here
        obj_off, _, objects = codec.key_objects(dk, order, valid)
        rows, peer, counts = codec.compare_keys(col, order, valid, obj_off, objects, col_b, valid_b, want_peer=True)
        lrows, range_off, total, lkeys = codec.list_keys(col, order, valid, rows, cap, want_keys=True)
        values, val_off, val_total, status = codec.fetch_objects(lrows, total, cap, enc.out, enc.out_off, n, rec_bytes,
                                                                 rec_bytes)
        return objects, rows, peer, counts, lrows, total, lkeys, values, val_off, val_total, status

    chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = chain()
    objects, rows, peer, counts, lrows, total, lkeys, values, val_off, val_total, status = res

    sorted_keys = [bytes(r) for r in col.cpu().numpy().reshape(n, 29)]
    peer_keys = [bytes(r) for r in col_b.cpu().numpy().reshape(nb, 29)]
    host_order = order.cpu().numpy().view(np.uint32).tolist()
    off1 = hobj._to_host(enc.out_off, 8 * (n + 1), np.uint64).astype(np.int64)
    arena1 = hobj._to_host(enc.out, rec_bytes, np.uint8)
    records = [arena1[off1[i]:off1[i + 1]].tobytes() for i in range(n)]
    sent = []
    for va, vb in ((n, nb), (n - 37, nb // 2)):  # the valid counts lowered on the device between the replays
        valid.fill_(va)
        valid_b.fill_(vb)
        g.replay()
        torch.cuda.synchronize()
        a, b = sorted_keys[:va], peer_keys[:vb]
        cmp = hkeys.compare(a, b)
        visits = hkeys.scan(a, [(c.pos, c.end) for c in cmp])
        fetched = hkeys.fetch(records, visits, host_order)
        k = int(objects.item())
        assert k == len(cmp)
        got = rows.cpu().numpy().view(np.uint32)
        assert [(int(r[0]), int(r[1]), int(r[4])) for r in got[:k]] == [(c.pos, c.end, c.flags) for c in cmp]
        assert (got[k:] == 0).all()  # cleared rows: empty ranges to the list
        assert peer.cpu().numpy().view(np.uint32)[:k].tolist() == [SEEK_NONE if c.peer is None else c.peer for c in cmp]
        cnt = counts.cpu().numpy()
        assert cnt[0] == k and cnt[1:5].sum() == k
        t = int(total.item())
        lr = lrows.cpu().numpy().view(np.uint32)[:t]
        assert [(int(q), int(p)) for q, p in lr[:, :2]] == visits and 0 < t < va
        assert lkeys.cpu().numpy()[:29 * t].tobytes() == b"".join(a[p] for _, p in visits)
        off2 = val_off.cpu().numpy()
        assert int(val_total.item()) == off2[t] == sum(len(f) for f in fetched)
        assert (status.cpu().numpy()[:t] == OK).all()
        assert hobj._to_host(values, int(off2[t]), np.uint8).tobytes() == b"".join(fetched)
        sent.append(t)
    assert sent[0] != sent[1]
    # what was gathered decodes to the records the list named
    d2 = codec.decode(values, val_off, cap, rec_bytes=rec_bytes)
    meta1, info1, _, _, _, _ = d1.host()
    meta2, info2, _, _, _, _ = d2.host()
    r = lr[:, 2].astype(np.int64)
    assert (info2["meta_status"][:t] == OK).all()
    assert np.array_equal(meta2["object_id"][:t], meta1["object_id"][r]) and np.array_equal(meta2["vid"][:t],
                                                                                           meta1["vid"][r])
