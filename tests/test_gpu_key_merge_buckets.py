"""honu_key_merge_buckets on the GPU against numpy.

The expectation is built from keys.merge_buckets (the host statement) over
the two sides' buckets as the clamped offsets cut them. Where d_count_a is
unused the output is also compared bit for bit with Codec.merge_keys run
bucket by bucket on the same device: the per-bucket results, end to end, are
the output's first T rows. Every column, offset array and output is a guarded
view (tests/guards.py) under both fills, the key columns at byte phases 0, 1
and 3; the write set is exactly the 29 T bytes of the column, the 4 T of the
order (T = d_off_out[k]), the 8 (k + 1) of the offsets and the 8 k of the
counts, in outputs that hold na + nb rows. Sizes are in units of the tile T,
the param "merge_tile", and of the param "merge_buckets_stage".
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import keys as hkeys  # noqa: E402
from honu_amd import object as hobj  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
M32 = (1 << 32) - 1
PHASES = ((0, 0, 0), (1, 3, 1), (3, 1, 3), (0, 1, 3))  # (A's column, B's column, the output column)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 4096)
    yield c
    c.close()


def param(codec, name):
    v = L.C.c_int64(0)
    L.check(codec.lib.honu_ctx_get_param(codec.ctx, name, L.C.byref(v)), name.decode())
    return int(v.value)


@pytest.fixture(scope="module")
def T(codec):
    assert param(codec, b"merge_tile") == 1024
    return 1024


@pytest.fixture(scope="module")
def STAGE(codec):
    s = param(codec, b"merge_buckets_stage")
    assert 8 <= s < 1024
    return s


# --------------------------------------------------------------------------
# bucketed columns on the host, and what the call must write
# --------------------------------------------------------------------------
def random_keys(n, rng):
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def in_order(k):
    k = np.ascontiguousarray(k, np.uint8).reshape(-1, 29)
    return k[np.lexsort(k.T[::-1])] if len(k) else k


class BCol:
    """A bucketed column: parts[c] is bucket c's rows as they lie in the arena. The order holds
    distinct values that are not the row numbers, so that a mix-up of the two is seen."""

    def __init__(self, parts, count=None, off=None, order=None):
        parts = [np.ascontiguousarray(p, np.uint8).reshape(-1, 29) for p in parts]
        self.k = len(parts)
        self.S = np.concatenate(parts + [np.zeros((0, 29), np.uint8)])
        self.n = len(self.S)
        sizes = np.array([len(p) for p in parts], np.uint64)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64) if off is None else np.asarray(off, np.uint64)
        self.order = (np.arange(self.n, dtype=np.uint32) * 3 + 7) if order is None else np.asarray(order, np.uint32)
        self.count = None if count is None else np.asarray(count, np.uint64)

    def buckets(self):
        """Per bucket (first row, rows) as the clamped offsets cut them."""
        e = [min(int(x), self.n) for x in self.off[:self.k + 1]]
        return [(e[c], max(e[c + 1] - e[c], 0)) for c in range(self.k)]


def expected(a, b, base=None, b_base=0, ob=True):
    """(column, order, offsets, counts) from keys.merge_buckets."""
    ca, cb = a.buckets(), b.buckets()
    ka = [[a.S[r].tobytes() for r in range(f, f + n)] for f, n in ca]
    kb = [[b.S[r].tobytes() for r in range(f, f + n)] for f, n in cb]
    counts = None if a.count is None else [int(x) for x in a.count]
    merged = hkeys.merge_buckets(ka, kb, counts)
    rows, order = [], []
    for c, bucket in enumerate(merged):
        for key, side, i in bucket:
            rows.append(key)
            if side == 0:
                order.append(int(a.order[ca[c][0] + i]))
            else:
                g = cb[c][0] + i
                order.append(((int(b.order[g]) if ob else g) + (int(base[c]) if base is not None else b_base)) & M32)
    S = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 29)
    count = np.array([len(x) for x in merged], np.uint64)
    return S, np.array(order, np.uint32), np.concatenate([[0], np.cumsum(count)]).astype(np.uint64), count


def put(codec, a, phase, fill):
    """The bytes of `a` in a guarded block at a byte phase (an input)."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = guards.guarded(a.nbytes, phase=phase, fill=fill, device=codec.torch_device)
    if a.nbytes:
        t.copy_(torch.from_numpy(a.copy()).to(codec.torch_device))
    return t


class Call:
    """The guarded device arguments of one call. b_dev: B as device tensors (keys, order, offsets) with nb rows,
    honu_key_route's outputs as they stand."""

    def __init__(self, codec, a, b, fill, phases=(0, 0, 0), base=None, b_dev=None, nb=None):
        self.codec, self.a, self.b, self.k = codec, a, b, a.k
        self.na, self.nb = a.n, b.n if nb is None else nb
        self.n = self.na + self.nb
        self.inputs = []

        def inp(x, phase=0):
            t = put(codec, x, phase, fill)
            self.inputs.append((t, np.ascontiguousarray(x)))
            return t

        A = guards.address
        self.sa, self.oa, self.offa = A(inp(a.S, phases[0])), A(inp(a.order)), A(inp(a.off))
        self.ca = A(inp(a.count)) if a.count is not None else 0
        if b_dev is None:
            self.sb, self.ob, self.offb = A(inp(b.S, phases[1])), A(inp(b.order)), A(inp(b.off))
        else:
            self.b_dev = b_dev
            self.sb, self.ob, self.offb = (t.data_ptr() for t in b_dev)
        self.base = A(inp(np.asarray(base, np.uint32))) if base is not None else 0
        dev = codec.torch_device
        self.out = guards.guarded(29 * self.n, phase=phases[2], fill=fill, device=dev)
        self.order = guards.guarded(4 * self.n, fill=fill, device=dev)
        self.off = guards.guarded(8 * (self.k + 1), fill=fill, device=dev)
        self.count = guards.guarded(8 * self.k, fill=fill, device=dev)

    def args(self, b_base=0, with_order=True, ob=True, with_count=True, **kw):
        A = guards.address
        x = dict(ctx=self.codec.ctx, k=self.k, sa=self.sa, oa=self.oa, offa=self.offa, ca=self.ca, na=self.na,
                 sb=self.sb, ob=(self.ob if ob else 0) if isinstance(ob, bool) else ob, offb=self.offb, nb=self.nb, base=self.base, b_base=b_base,
                 out=A(self.out), order=A(self.order) if with_order else 0, off=A(self.off),
                 count=A(self.count) if with_count else 0)
        x.update(kw)
        return x

    def run(self, **kw):
        x = self.args(**kw)
        return self.codec.lib.honu_key_merge_buckets(
            x["ctx"], x["k"], x["sa"], x["oa"], x["offa"], x["ca"], x["na"], x["sb"], x["ob"], x["offb"], x["nb"],
            x["base"], x["b_base"], x["out"], x["order"], x["off"], x["count"], self.codec.stream)

    def outputs(self):
        return self.out, self.order, self.off, self.count

    def check(self, want, with_order=True, with_count=True):
        """The outputs against (column, order, offsets, counts) and the exact write set."""
        torch.cuda.synchronize()
        S, order, off, count = want
        t = len(S)
        assert t <= self.n
        got_off = guards.block_of(self.off).bytes().view(np.uint64)
        assert np.array_equal(got_off, off), (got_off[:8], off[:8])
        guards.assert_untouched(self.off, [(0, 8 * (self.k + 1))])
        if with_count:
            assert np.array_equal(guards.block_of(self.count).bytes().view(np.uint64), count)
        guards.assert_untouched(self.count, [(0, 8 * self.k)] if with_count else [])
        got = guards.block_of(self.out).bytes()[:29 * t].reshape(t, 29)
        bad = np.flatnonzero((got != S).any(axis=1))
        assert not len(bad), (len(bad), bad[:4], got[bad[:4]], S[bad[:4]])
        guards.assert_untouched(self.out, [(0, 29 * t)])  # nothing at or past row T
        if with_order:
            got = guards.block_of(self.order).bytes()[:4 * t].view(np.uint32)
            bad = np.flatnonzero(got != order)
            assert not len(bad), (len(bad), bad[:4], got[bad[:4]], order[bad[:4]])
        guards.assert_untouched(self.order, [(0, 4 * t)] if with_order else [])
        for tns, host in self.inputs:
            assert guards.block_of(tns).bytes().tobytes() == host.tobytes()
            guards.assert_untouched(tns, [(0, guards.block_of(tns).nbytes)])
        return guards.block_of(self.out).bytes()[:29 * t], guards.block_of(self.order).bytes()[:4 * t]


def per_bucket_merge_keys(codec, a, b, base, b_base, ob):
    """Codec.merge_keys bucket by bucket over the same columns on the same device, end to end: (column
    bytes, order bytes). Only without d_count_a and with offsets inside the arenas."""
    dev = codec.torch_device

    def up(x):  # (32 bytes more than the array: an empty column still has an address)
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        return torch.from_numpy(np.concatenate([raw, np.zeros(32, np.uint8)])).to(dev)

    sa, sb = up(a.S), up(b.S)
    oa = up(a.order).view(torch.int32)
    obt = up(b.order if ob else np.arange(b.n, dtype=np.uint32)).view(torch.int32)
    ca, cb = a.buckets(), b.buckets()
    va = up(np.array([n for _, n in ca] + [0], np.uint64)).view(torch.int64)
    vb = up(np.array([n for _, n in cb] + [0], np.uint64)).view(torch.int64)
    cols, orders = [], []
    for c in range(a.k):
        (fa, na), (fb, nb) = ca[c], cb[c]
        if na + nb == 0:
            continue
        bb = int(base[c]) if base is not None else b_base
        if na == 0 or nb == 0:  # (an empty tensor has no address to pass: the merge is the other side's rows)
            s = sb[29 * fb:29 * (fb + nb)] if na == 0 else sa[29 * fa:29 * (fa + na)]
            o = obt[fb:fb + nb] + (bb - (1 << 32) if bb >= 1 << 31 else bb) if na == 0 else oa[fa:fa + na]
        else:
            s, o, v = codec.merge_keys(sa[29 * fa:29 * (fa + na)], oa[fa:fa + na], va[c:c + 1],
                                       sb[29 * fb:29 * (fb + nb)], obt[fb:fb + nb], vb[c:c + 1], b_base=bb)
        cols.append(s)
        orders.append(o.contiguous().view(torch.uint8))
    torch.cuda.synchronize()
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    return torch.cat(cols + [empty]).cpu().numpy(), torch.cat(orders + [empty]).cpu().numpy()


def merge_and_check(codec, a, b, base=None, b_base=0, ob=True, phases=(0, 0, 0), per_bucket=None):
    want = expected(a, b, base, b_base, ob)
    plain = a.count is None and int(a.off[-1]) <= a.n and int(b.off[-1]) <= b.n
    peer = per_bucket_merge_keys(codec, a, b, base, b_base, ob) if (plain if per_bucket is None else per_bucket) else None

    def body(fill):
        c = Call(codec, a, b, fill, phases, base=base)
        assert c.run(b_base=b_base, ob=ob) == 0
        got = c.check(want)
        if peer is not None:
            assert got[0].tobytes() == peer[0].tobytes() and got[1].tobytes() == peer[1].tobytes()

    guards.twice(body)
    return want


def random_side(rng, sizes, pool=None):
    return BCol([in_order(random_keys(n, rng) if pool is None else pool[rng.integers(0, len(pool), n)]) for n in sizes])


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
NA = (0, 1, 2, "T-1", "T", "T+1")
NB = (0, 1, 63, "T", "3T+5")


def size_of(T, s):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[s] if isinstance(s, str) else s


@pytest.mark.parametrize("sa", NA)
def test_one_bucket_is_the_merge(codec, T, sa):
    """k = 1 with honu_key_merge's sizes, every na against every nb: the call equals honu_key_merge."""
    na = size_of(T, sa)
    for j, sb in enumerate(NB):
        nb = size_of(T, sb)
        rng = np.random.default_rng(9000 + 10 * na + j)
        pool = random_keys(max((na + nb) // 3, 1), rng)  # ties within and across the sides
        S, order, off, count = merge_and_check(codec, random_side(rng, [na], pool), random_side(rng, [nb], pool),
                                               b_base=5000, phases=PHASES[(NA.index(sa) + j) % len(PHASES)])
        assert off.tolist() == [0, na + nb] and count.tolist() == [na + nb]


def test_three_buckets_with_empty_ones(codec, T):
    """A bucket empty in A, one empty in B, one empty in both, in every position."""
    rng = np.random.default_rng(9101)
    for shift in range(3):
        sa = np.roll([0, 40, 0], shift)
        sb = np.roll([33, 0, 0], shift)
        S, order, off, count = merge_and_check(codec, random_side(rng, sa), random_side(rng, sb), base=[100, 200, 300],
                                               phases=PHASES[shift + 1])
        assert sorted(count.tolist()) == [0, 33, 40]
    pool = random_keys(20, rng)
    merge_and_check(codec, random_side(rng, [0, 2 * T + 9, 0, 50], pool), random_side(rng, [T + 1, 0, 0, 70], pool))


def test_a_long_bucket_between_two_short_ones(codec, T):
    """5000 + 3000 rows in the middle bucket: seven tile ends split inside one bucket, its diagonals local."""
    rng = np.random.default_rng(9102)
    pool = random_keys(900, rng)
    want = merge_and_check(codec, random_side(rng, [7, 5000, 3], pool), random_side(rng, [2, 3000, 9], pool),
                           base=[10, 20000, 40000], phases=PHASES[1])
    assert want[2].tolist() == [0, 9, 8009, 8021]


def test_bucket_ends_on_tile_ends(codec, T):
    """Buckets that end exactly at output rows 1024 and 2048."""
    rng = np.random.default_rng(9103)
    pool = random_keys(300, rng)
    want = merge_and_check(codec, random_side(rng, [600, 1000, 100], pool), random_side(rng, [T - 600, T - 1000, 50], pool),
                           b_base=1 << 20, phases=PHASES[2])
    assert want[2].tolist() == [0, T, 2 * T, 2 * T + 150]


def test_many_tiny_buckets(codec, T, STAGE):
    """k = 3000 with 0-2 rows a side: every tile holds more buckets than the stage, the slice is read from memory."""
    rng = np.random.default_rng(9104)
    k = 3000
    pool = random_keys(64, rng)
    a, b = random_side(rng, rng.integers(0, 3, k), pool), random_side(rng, rng.integers(0, 3, k), pool)
    want = merge_and_check(codec, a, b, base=rng.integers(0, 1 << 31, k), phases=PHASES[3])
    assert T / 4 > STAGE and (want[3] == 0).sum() > 100 and len(want[0]) > 2 * T


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_tile_at_the_stage(codec, T, STAGE, delta):
    """The first tile touches exactly stage - 1, stage and stage + 1 buckets (an empty one among them), the
    second tile one bucket."""
    s = STAGE + delta
    rng = np.random.default_rng(9105 + delta)
    tot = np.full(s, T // s)
    tot[:T - tot.sum()] += 1          # s buckets, T rows
    tot[1], tot[2] = 0, tot[1] + tot[2]  # one of them empty, inside the slice
    sa = rng.integers(0, tot + 1)
    pool = random_keys(40, rng)
    a = random_side(rng, list(sa) + [T + 30], pool)
    b = random_side(rng, list(tot - sa) + [70], pool)
    want = merge_and_check(codec, a, b, base=np.arange(s + 1) * 1000, phases=PHASES[delta + 1])
    assert want[2][s] == T and want[2][-1] == 2 * T + 100 and a.k == s + 1


def test_keys_descend_with_the_bucket(codec, T):
    """Bucket 0 holds the largest object IDs, the last bucket the smallest, and one key sits in A's bucket 1
    and in B's bucket 0: a compare that forgets the bucket puts rows into the wrong one."""
    rng = np.random.default_rng(9106)
    k = 4
    shared = random_keys(1, rng)
    shared[0, 1] = 0x80

    def side(with_shared_in):
        parts = []
        for c in range(k):
            rows = random_keys(90 + 7 * c, rng)
            rows[:, 1] = 0xE0 - 0x30 * c + rng.integers(0, 0x20, len(rows))  # byte 1: the object ID's first
            if c == with_shared_in:
                rows = np.concatenate([rows, shared, shared])
            parts.append(in_order(rows))
        return BCol(parts)

    a, b = side(1), side(0)
    S, order, off, count = merge_and_check(codec, a, b, base=[0, 1000, 2000, 3000], phases=PHASES[1])
    assert (np.diff(S[:, 1].astype(int)) < 0).any()  # the column as a whole is not sorted
    hits = np.flatnonzero((S == shared[0]).all(axis=1))
    assert len(hits) == 4 and (hits[:2] < off[1]).all() and (off[1] <= hits[2:]).all() and (hits[2:] < off[2]).all()


def test_all_keys_equal_inside_a_bucket(codec, T):
    """The tie rule over tiles: every A row of the bucket before every B row, each side in its order."""
    rng = np.random.default_rng(9107)
    key, other = random_keys(1, rng), random_keys(5, rng)
    a = BCol([in_order(other), np.tile(key, (T + T // 2, 1)), in_order(other[:2])])
    b = BCol([in_order(other[:3]), np.tile(key, (2 * T - 11, 1)), in_order(other)])
    S, order, off, count = merge_and_check(codec, a, b, b_base=1 << 24, phases=PHASES[2])
    mid = order[off[1]:off[2]]
    assert np.array_equal(mid, np.concatenate([a.order[5:5 + T + T // 2], b.order[3:3 + 2 * T - 11] + (1 << 24)]))


@pytest.mark.parametrize("byte", [28, 0, 16, 13, 14, 15, 12, 17])
def test_discriminating_byte(codec, T, byte):
    """Keys that differ only in one byte: the last, the first, the ObjectPrefix edge (16 / 17) and the
    overlap of the two 16-byte loads (13-15)."""
    rng = np.random.default_rng(9200 + byte)
    base = random_keys(1, rng)

    def part(n):
        rows = np.tile(base, (n, 1))
        rows[:, byte] = rng.choice(np.array([0, 1, 0x7E, 0x7F, 0x80, 0x81, 0xFE, 0xFF], np.uint8), n)
        return in_order(rows)

    merge_and_check(codec, BCol([part(T // 2 + 37), part(T)]), BCol([part(T // 2 + 5), part(90)]), base=[7, 70000],
                    phases=PHASES[byte % len(PHASES)])


def test_counts_and_clamped_offsets(codec, T):
    """d_count_a: a fifth of each bucket's rows invalid (arbitrary rows behind the valid ones), counts above a
    bucket's rows, and last offsets above na and nb: all clamped. The output is tight."""
    rng = np.random.default_rng(9108)
    pool = random_keys(500, rng)
    valid = np.array([700, 0, 1300, 40, 900])
    junk = valid // 4
    junk[3] = 0
    parts = [np.concatenate([in_order(pool[rng.integers(0, len(pool), v)]), random_keys(j, rng)]) for v, j in zip(valid, junk)]
    count = valid.copy()
    count[3] = 40 + 9          # above the bucket's rows
    count[1] = 1 << 50
    a = BCol(parts, count=count)
    b = random_side(rng, [300, 20, 0, 2 * T, 5], pool)
    want = merge_and_check(codec, a, b, base=[0, 5000, 10000, 20000, 30000], phases=PHASES[1])
    assert want[3].tolist() == (valid + np.array([300, 20, 0, 2 * T, 5])).tolist() and len(want[0]) < a.n + b.n
    # the same with the last offsets above the arenas
    a2 = BCol(parts, count=count, off=np.concatenate([a.off[:-1], [a.n + 77]]))
    b2 = BCol([b.S], off=np.concatenate([b.off[:-1], [1 << 40]]))
    b2.k = b.k
    assert all(np.array_equal(x, y) for x, y in zip(merge_and_check(codec, a2, b2, base=[0, 5000, 10000, 20000, 30000],
                                                                    phases=PHASES[2]), want))
    # and without counts: clamped offsets alone, every row valid
    a3 = BCol([in_order(p) for p in parts], off=a2.off)
    got = merge_and_check(codec, a3, b2, b_base=9, phases=PHASES[3])
    assert len(got[0]) == a.n + b.n
    # every count 0: B alone
    a4 = BCol(parts, count=np.zeros(5, np.uint64))
    got = merge_and_check(codec, a4, b, ob=False, b_base=3)
    assert np.array_equal(got[0], b.S) and np.array_equal(got[1], np.arange(b.n, dtype=np.uint32) + 3)


def test_b_from_a_route(codec, T):
    """B is what honu_key_route wrote, as it stands: d_keys_out, d_local, d_bucket_off, nb the route's m.
    Both tail classes are populated; their rows lie behind d_bucket_off[k] and are not merged."""
    rng = np.random.default_rng(9109)
    k, m = 3, 2 * T + 77
    table = in_order(np.pad(rng.integers(0, 256, (k, 16), dtype=np.uint8), ((0, 0), (0, 13))))[:, :16].copy()
    unknown = table[1].copy()
    unknown[15] ^= 1
    member = rng.integers(0, k + 1, m)
    ids = np.concatenate([table, unknown[None]])[member]
    pool = random_keys(400, rng)
    bkeys = pool[rng.integers(0, len(pool), m)]
    status = np.zeros(m, np.int32)
    status[rng.integers(0, 6, m) == 0] = 8
    dev = codec.torch_device
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_keys, d_status = up(bkeys), up(status)
    seq, _, _ = codec.sort_keys(d_keys, d_status, n=m)
    r = codec.route_keys(up(ids), m, up(table), k, status=d_status, seq=seq, keys=d_keys)
    torch.cuda.synchronize()
    boff = r.bucket_off.cpu().numpy().view(np.uint64)
    assert 0 < boff[1] < boff[2] < boff[k] < boff[k + 1] < m  # every bucket and both tails have rows
    routed = BCol([r.keys.cpu().numpy()], off=boff, order=r.local.cpu().numpy().view(np.uint32))
    routed.k = k
    counts = np.diff(boff[:k + 1].astype(np.int64))
    for c in range(k):  # the route left every bucket sorted, numbered from 0
        f, n = routed.buckets()[c]
        assert n == counts[c] and np.array_equal(routed.S[f:f + n], in_order(routed.S[f:f + n]))
        assert np.array_equal(routed.order[f:f + n], np.arange(n))
    a = random_side(rng, [T + 5, 300, 90], pool)
    base = [T + 5, 300, 90]  # the buckets' record counts: every bucket keeps its own numbering
    want = expected(a, routed, base=base)
    assert len(want[0]) == a.n + int(boff[k]) < a.n + m

    def body(fill):
        c = Call(codec, a, routed, fill, PHASES[1], base=base, b_dev=(r.keys, r.local, r.bucket_off), nb=m)
        assert c.run() == 0
        c.check(want)

    guards.twice(body)
    # one record numbering: d_order_b and d_base NULL, routed row g is record b_base + g
    want = expected(a, routed, b_base=a.n, ob=False)

    def body2(fill):
        c = Call(codec, a, routed, fill, PHASES[2], b_dev=(r.keys, r.local, r.bucket_off), nb=m)
        assert c.run(b_base=a.n, ob=False) == 0
        c.check(want)

    guards.twice(body2)


def test_empty_sides_and_no_buckets(codec, T):
    rng = np.random.default_rng(9110)
    sizes = [T + 9, 0, 70]
    full, none = random_side(rng, sizes), BCol([np.zeros((0, 29), np.uint8)] * 3)
    # na = 0: the first batch into an empty store; nb = 0; both
    want = merge_and_check(codec, none, full, base=[0, 0, 0])
    assert np.array_equal(want[0], full.S) and np.array_equal(want[1], full.order)
    want = merge_and_check(codec, full, none, b_base=5)
    assert np.array_equal(want[0], full.S) and np.array_equal(want[1], full.order)
    want = merge_and_check(codec, none, none)
    assert want[2].tolist() == [0, 0, 0, 0] and want[3].tolist() == [0, 0, 0]
    # k = 0: d_off_out[0] = 0 alone, whatever rows the arenas hold
    for na, nb, counted in ((0, 0, False), (50, 20, False), (50, 20, True), (0, 0, True)):
        a, b = BCol([random_keys(na, rng)]), BCol([random_keys(nb, rng)])
        a.k = b.k = 0
        a.off = b.off = np.zeros(1, np.uint64)
        if counted:
            a.count = np.zeros(0, np.uint64)  # (a pointer is given; it has no entry to read)
        want = merge_and_check(codec, a, b, per_bucket=False)
        assert len(want[0]) == 0 and want[2].tolist() == [0]


def test_orders(codec, T):
    """d_base per bucket against a scalar b_base, d_order_b NULL, and no order at all."""
    rng = np.random.default_rng(9111)
    pool = random_keys(150, rng)
    a, b = random_side(rng, [T - 3, 500, 8], pool), random_side(rng, [90, T + 1, 0], pool)
    per = merge_and_check(codec, a, b, base=[1000, 2000000, M32 - 5], phases=PHASES[1])
    one = merge_and_check(codec, a, b, b_base=4321, phases=PHASES[2])
    assert np.array_equal(per[0], one[0]) and not np.array_equal(per[1], one[1])
    plain = merge_and_check(codec, a, b, b_base=M32 - b.n, ob=False, phases=PHASES[3])
    assert np.array_equal(plain[0], one[0])
    merge_and_check(codec, a, b, base=[5, 6, 7], ob=False)
    want = expected(a, b)

    def body(fill):
        for given in (False, True):  # the input orders are ignored, given or not
            c = Call(codec, a, b, fill, PHASES[1])
            kw = {} if given else dict(oa=0, ob=False)
            assert c.run(with_order=False, with_count=given, **kw) == 0
            c.check(want, with_order=False, with_count=given)

    guards.twice(body)


def refill(codec, t, fill):
    """The view back to its pattern, so that what it holds afterwards is the replay's."""
    blk = guards.block_of(t)
    p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
    t.copy_(torch.from_numpy(p).to(codec.torch_device))


@pytest.mark.parametrize("counted", [False, True])
def test_graph_capture_and_another_batch(codec, T, counted):
    """One call captured and replayed; then another batch's rows and offsets (and other counts) written on
    the device into the same arrays, and the same graph replayed."""
    rng = np.random.default_rng(9112 + counted)
    pool = random_keys(300, rng)
    k = 4
    a1, b1 = random_side(rng, [T, 50, 0, 700], pool), random_side(rng, [300, 0, 20, T + 7], pool)
    # the second state has the same arena sizes, other buckets
    a2, b2 = random_side(rng, [10, T + 500, 240, 0], pool), random_side(rng, [T, 0, 300, 27], pool)
    assert a1.n == a2.n and b1.n == b2.n
    if counted:
        a1.count, a2.count = np.array([T, 50, 0, 650], np.uint64), np.array([10, T, 1 << 40, 0], np.uint64)
    base = [100, 200, 300, 400]
    dev = codec.torch_device

    def body(fill):
        c = Call(codec, a1, b1, fill, PHASES[2], base=base)
        assert c.run() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run() == 0
        for t in c.outputs():
            refill(codec, t, fill)
        g.replay()
        c.check(expected(a1, b1, base=base))
        for t in c.outputs():
            refill(codec, t, fill)
        new = [a2.S, a2.order, a2.off] + ([a2.count] if counted else []) + [b2.S, b2.order, b2.off]
        for j, x in enumerate(new):
            c.inputs[j][0].copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev))
            c.inputs[j] = (c.inputs[j][0], np.ascontiguousarray(x))
        g.replay()
        c.check(expected(a2, b2, base=base))

    guards.twice(body)


def test_refusals_store_nothing(codec, T):
    rng = np.random.default_rng(9113)
    a, b = random_side(rng, [300, 20]), random_side(rng, [70, 5])
    a.count = np.array([300, 20], np.uint64)
    want = expected(a, b, b_base=a.n)

    def body(fill):
        c = Call(codec, a, b, fill, (1, 3, 1), base=[1, 2])
        base = c.base
        c.base = 0
        A = guards.address
        for kw in (dict(na=(1 << 32) - b.n), dict(na=1 << 32), dict(nb=1 << 32), dict(na=(1 << 64) - 1),
                   dict(na=M32, nb=1), dict(k=(1 << 32) - 3), dict(k=1 << 40), dict(k=4096)):  # (k + 1 above max_records, with counts)
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(offa=0), dict(offb=0), dict(off=0), dict(sa=0), dict(sb=0), dict(out=0), dict(oa=0),
                   dict(b_base=(1 << 32) - b.n), dict(oa=c.oa + 2), dict(ob=c.ob + 2), dict(order=A(c.order) + 2),
                   dict(base=base + 2), dict(offa=c.offa + 4), dict(offb=c.offb + 4), dict(ca=c.ca + 4),
                   dict(off=A(c.off) + 4), dict(count=A(c.count) + 4)):
            assert c.run(**kw) == E_ARG, kw
        torch.cuda.synchronize()
        for t in c.outputs():
            guards.assert_untouched(t, [])
        # b_base + nb may pass 2^32 - 1 with d_base; d_order_a is not needed without d_order_out or without A rows
        assert c.run(base=base, b_base=M32) == 0
        assert c.run(oa=0, with_order=False) == 0
        assert c.run(b_base=a.n) == 0  # and the arguments were good
        c.check(want)

    guards.twice(body)
