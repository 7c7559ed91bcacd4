"""honu_key_route on the GPU against numpy.

The expectation is numpy's alone and never calls the library: the IDs and the
table's rows as pairs of big-endian 64-bit words ranked together, searchsorted
of the IDs' ranks in the table's, the test for equality, and a stable argsort
of the classes. Every input and output is a guarded view (tests/guards.py)
under both fills, d_ids at byte phases 0 and 1 with strides 16, 17 and 352,
the table, d_keys and d_keys_out at phases 0 and 1; the write set is exactly
d_bucket_off[0, k + 3), d_bucket_count[0, k + 2), d_rows[0, m), d_local[0, m),
d_keys_out[0, 29 m) and the d_bucket entries some position names, and the
inputs are unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import LIST_ROW_HEAD, SEEK_NONE  # noqa: E402

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
MAX_RECORDS = 4096
NONE = np.uint32(SEEK_NONE)
MS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4096)
STRIDES = (16, 17, 352)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, MAX_RECORDS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stage(codec):
    v = L.C.c_int64(0)
    assert codec.lib.honu_ctx_get_param(codec.ctx, b"route_stage", L.C.addressof(v)) == 0
    return int(v.value)


def table_sizes(stage):
    return (0, 1, 2, 255, 256, 257, stage - 1, stage, stage + 1, 3000)


# --------------------------------------------------------------------------
# inputs and expectations
# --------------------------------------------------------------------------
HIGH = np.array([0, 1, 1 << 8, 1 << 56, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)


def some_ids(n, rng):
    """n IDs (uint8[n, 16]) that share leading and trailing bytes often: few high words, and low words
    that are small, near the top or arbitrary; the all-0x00 and all-0xff IDs among them."""
    hi = np.where(rng.random(n) < 0.8, rng.choice(HIGH, n), rng.integers(0, 1 << 64, n, dtype=np.uint64))
    lo = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    small = rng.random(n) < 0.5
    lo[small] = rng.integers(0, 600, int(small.sum()), dtype=np.uint64)
    top = rng.random(n) < 0.1
    lo[top] = np.uint64((1 << 64) - 1) - rng.integers(0, 3, int(top.sum()), dtype=np.uint64)
    ids = np.stack([hi, lo], 1).astype(">u8").view(np.uint8).reshape(n, 16)
    if n > 1:
        ids[0], ids[1] = 0x00, 0xFF
    return ids


def pairs(ids):
    return np.ascontiguousarray(ids).reshape(-1, 16).view(">u8").astype(np.uint64).reshape(-1, 2)


def make_table(k, rng):
    """k distinct IDs in ascending bytes.Compare order."""
    rows = np.zeros((0, 16), np.uint8)
    while len(rows) < k:
        more = np.concatenate([rows, some_ids(2 * k + 8, rng)])
        _, first = np.unique(pairs(more), axis=0, return_index=True)
        rows = more[np.sort(first)]
    rows = rows[rng.permutation(len(rows))[:k]]
    order = np.lexsort((pairs(rows)[:, 1], pairs(rows)[:, 0]))
    return np.ascontiguousarray(rows[order])


def draw_ids(m, table, rng, known=0.7):
    """m IDs: rows of the table, rows with byte 15 or byte 0 one off, and others."""
    ids = some_ids(m, rng)
    k = len(table)
    if k and m:
        pick = rng.integers(0, k, m)
        how = rng.random(m)
        take = how < known + 0.2
        ids[take] = table[pick[take]]
        near = (how >= known) & take
        ids[near, 15] += 1
        ids[near & (how < known + 0.05), 0] -= 1
    return ids


def want(ids, table, status=None, seq=None, keys=None):
    """numpy's route."""
    m, k = len(ids), len(table)
    rank = np.zeros(0, np.int64)
    if m + k:
        rank = np.unique(np.concatenate([pairs(table), pairs(ids)]), axis=0, return_inverse=True)[1].reshape(-1)
    t, x = rank[:k], rank[k:]
    assert (np.diff(t) > 0).all()  # the table is ascending and distinct
    lb = np.searchsorted(t, x)
    found = (lb < k) & (np.append(t, -1)[lb] == x)
    seq = np.arange(m, dtype=np.int64) if seq is None else np.asarray(seq, np.uint32).astype(np.int64)
    named = seq < m
    i = np.where(named, seq, 0)
    ok = np.ones(m, bool) if status is None else np.asarray(status) == 0
    part = named & ok[i]
    cls = np.where(part, np.where(found[i], lb[i], k), k + 1).astype(np.int64)
    g = np.argsort(cls, kind="stable")
    w = {"m": m, "k": k}
    w["off"] = np.searchsorted(cls[g], np.arange(k + 3)).astype(np.uint64)
    w["count"] = np.diff(w["off"].astype(np.int64)).astype(np.uint64)
    c = cls[g]
    head = np.ones(m, bool)
    head[1:] = c[1:] != c[:-1]
    rec = np.where(named[g], seq[g], int(NONE))
    w["rows"] = np.stack([c, g, rec, np.where(head, LIST_ROW_HEAD, 0)], 1).astype(np.uint32)
    w["local"] = (np.arange(m) - w["off"].astype(np.int64)[c]).astype(np.uint32)
    if keys is not None:
        w["keys"] = np.where(named[g][:, None], keys.reshape(-1, 29)[i[g]], 0).astype(np.uint8).reshape(-1)
    w["named"] = np.unique(seq[named])
    bucket = np.full(m, NONE, np.uint32)
    sel = named & (cls < k)
    bucket[seq[sel]] = cls[sel]
    w["bucket"] = bucket
    w["cls"] = cls
    return w


def strided(ids, stride, rng):
    """The IDs at `stride` bytes from one another, arbitrary bytes between them, not a byte behind the last."""
    m = len(ids)
    buf = rng.integers(0, 256, stride * (m - 1) + 16 if m else 0, dtype=np.uint8)
    for j in range(16):
        buf[j::stride][:m] = ids[:, j]
    return buf


# --------------------------------------------------------------------------
# one guarded call
# --------------------------------------------------------------------------
def put(codec, a, phase, fill):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = guards.guarded(a.nbytes, phase=phase, fill=fill, device=codec.torch_device)
    if a.nbytes:
        t.copy_(torch.from_numpy(a.copy()).to(codec.torch_device))
    return t


def now(t, dtype=np.uint8):
    return guards.block_of(t).bytes().view(dtype)


class Call:
    def __init__(self, codec, ids, table, fill, status=None, seq=None, keys=None, stride=16, id_phase=0, phase=0,
                 seed=1):
        self.codec, self.m, self.k, self.stride = codec, len(ids), len(table), stride
        m, k, dev = self.m, self.k, codec.torch_device
        self.host = {"ids": strided(ids, stride, np.random.default_rng(seed)), "table": table}
        for name, a, dt in (("status", status, np.int32), ("seq", seq, np.uint32), ("keys", keys, np.uint8)):
            if a is not None:
                self.host[name] = np.asarray(a, dt)
        ph = {"ids": id_phase, "table": phase, "keys": phase}
        self.dev = {n: put(codec, a, ph.get(n, 0), fill) for n, a in self.host.items()}
        g = lambda nbytes, p=0: guards.guarded(nbytes, phase=p, fill=fill, device=dev)  # noqa: E731
        self.bucket, self.rows, self.local, self.keys_out = g(4 * m), g(16 * m), g(4 * m), g(29 * m, phase)
        self.off, self.count = g(8 * (k + 3)), g(8 * (k + 2))
        self.work_bytes = int(codec.lib.honu_key_route_workspace(m))
        self.work = g(self.work_bytes)
        self.outs = (self.bucket, self.rows, self.local, self.keys_out, self.off, self.count)

    def args(self, **kw):
        A, d = guards.address, self.dev
        x = dict(ctx=self.codec.ctx, ids=A(d["ids"]), id_stride=self.stride, status=A(d.get("status")), m=self.m,
                 seq=A(d.get("seq")), table=A(d["table"]), k=self.k, keys=A(d.get("keys")), bucket=A(self.bucket),
                 rows=A(self.rows), local=A(self.local), keys_out=A(self.keys_out) if "keys" in d else 0,
                 off=A(self.off), count=A(self.count), work=A(self.work), work_bytes=self.work_bytes)
        x.update(kw)
        return x

    def run(self, **kw):
        x = self.args(**kw)
        return self.codec.lib.honu_key_route(
            x["ctx"], x["ids"], x["id_stride"], x["status"], x["m"], x["seq"], x["table"], x["k"], x["keys"],
            x["bucket"], x["rows"], x["local"], x["keys_out"], x["off"], x["count"], x["work"], x["work_bytes"],
            self.codec.stream)

    def inputs_unchanged(self):
        for n, t in self.dev.items():
            assert guards.block_of(t).bytes().tobytes() == np.ascontiguousarray(self.host[n]).tobytes(), n
            guards.assert_untouched(t, [(0, guards.block_of(t).nbytes)])

    def nothing_stored(self):
        torch.cuda.synchronize()
        for t in self.outs + (self.work,):
            guards.assert_untouched(t, [])
        self.inputs_unchanged()

    def write_set(self, named, absent=()):
        """The write set alone (bounds): named, the records some position names."""
        torch.cuda.synchronize()
        m, k = self.m, self.k
        has = lambda n: n not in absent  # noqa: E731
        guards.assert_untouched(self.off, [(0, 8 * (k + 3))])
        guards.assert_untouched(self.count, [(0, 8 * (k + 2))])
        guards.assert_untouched(self.rows, [(0, 16 * m)] if has("rows") else [])
        guards.assert_untouched(self.local, [(0, 4 * m)] if has("local") else [])
        guards.assert_untouched(self.keys_out, [(0, 29 * m)] if "keys" in self.dev and has("keys_out") else [])
        guards.assert_untouched(self.bucket, [(4 * int(i), 4 * int(i) + 4) for i in named] if has("bucket") else [])
        guards.assert_untouched(self.work, [(0, self.work_bytes)])
        self.inputs_unchanged()

    def check(self, w, absent=()):
        """The outputs against numpy's route `w`, and the write set."""
        self.write_set(w["named"], absent)
        m = self.m

        def same(name, got, exp):
            bad = np.flatnonzero(got != exp)
            assert not len(bad), (name, m, self.k, len(bad), bad[:4], got[bad[:4]], exp[bad[:4]])

        same("bucket_off", now(self.off, np.uint64), w["off"])
        same("bucket_count", now(self.count, np.uint64), w["count"])
        if "rows" not in absent:
            same("rows", now(self.rows, np.uint32), w["rows"].reshape(-1))
        if "local" not in absent:
            same("local", now(self.local, np.uint32), w["local"])
        if "keys" in self.dev and "keys_out" not in absent:
            same("keys_out", now(self.keys_out), w["keys"])
        if "bucket" not in absent:
            same("bucket", now(self.bucket, np.uint32)[w["named"]], w["bucket"][w["named"]])


def route_and_check(codec, ids, table, status=None, seq=None, keys=None, stride=16, id_phase=0, phase=0, absent=(),
                    how=None):
    """One call under both fills against numpy. absent: the optional outputs passed as NULL; how: further
    arguments of the call to replace, 0 for a NULL pointer."""
    w = want(ids, table, status, seq, keys)
    how = how or {}

    def body(fill):
        c = Call(codec, ids, table, fill, status, seq, keys, stride, id_phase, phase)
        null = {n: 0 for n in absent}
        if "keys_out" in absent:
            null["keys"] = 0
        assert c.run(**null, **how) == 0
        c.check(w, absent)

    guards.twice(body)
    return w


def mixed(m, table, rng, bad=0.15):
    """(ids, status, keys): IDs of the table and others, some records not OK."""
    ids = draw_ids(m, table, rng)
    status = np.where(rng.random(m) < bad, rng.choice([1, 2, -1, 7], m), 0).astype(np.int32)
    keys = rng.integers(0, 256, 29 * m, dtype=np.uint8)
    return ids, status, keys


# --------------------------------------------------------------------------
# 1. shapes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_shapes(codec, stage, m):
    """Every m against every k: the staged and the unstaged table at the threshold, statuses mixed in, with
    and without a sequence, the strides and phases in turn."""
    rng = np.random.default_rng(1000 + m)
    tables = {k: make_table(k, rng) for k in table_sizes(stage)}
    for j, (k, table) in enumerate(tables.items()):
        ids, status, keys = mixed(m, table, rng)
        seq = rng.permutation(m).astype(np.uint32) if j % 2 else None
        w = route_and_check(codec, ids, table, status if j % 3 else None, seq, keys, stride=STRIDES[j % 3],
                            id_phase=j % 2, phase=(j // 2) % 2)
        assert int(w["off"][k + 2]) == m and int(w["count"].sum()) == m
        if m >= 255 and k >= 2:
            assert 0 < int(w["count"][:k].sum()) < m  # known and other records both


def test_both_forms_give_identical_classes(codec, stage):
    """One batch against a table of route_stage rows and the same table with one row more, a row above
    every ID of the batch: the classes of the staged search are those of the search in global memory."""
    rng = np.random.default_rng(7)
    table = make_table(stage + 1, rng)
    ids, status, _ = mixed(1025, table[:stage], rng)
    ids = ids[(pairs(ids) != pairs(table[stage:])[0]).any(1)]  # none is the last row
    a = route_and_check(codec, ids, table[:stage], stride=17, id_phase=1, phase=1)
    b = route_and_check(codec, ids, table, stride=17, id_phase=1, phase=1)
    moved = np.where(a["cls"] >= stage, a["cls"] + 1, a["cls"])
    assert np.array_equal(moved, b["cls"]) and 0 < (a["cls"] < stage).sum() < len(ids)


# --------------------------------------------------------------------------
# 2. distributions
# --------------------------------------------------------------------------
@pytest.mark.parametrize("how", ("one_bucket", "own_bucket", "gaps", "all_unknown", "all_skipped", "mixed"))
@pytest.mark.parametrize("k", (5, 1300, 3000))
def test_distributions(codec, stage, how, k):
    assert 1300 < stage < 3000  # a staged and an unstaged table
    m = 1025
    rng = np.random.default_rng(k + len(how))
    table = make_table(k, rng)
    status = None
    if how == "one_bucket":
        ids = np.repeat(table[k // 2][None], m, 0)
    elif how == "own_bucket":
        ids = table[rng.permutation(k)[:m]] if k >= m else table[np.arange(m) % k]
    elif how == "gaps":  # every third bucket full, the others empty
        ids = table[3 * rng.integers(0, (k + 2) // 3, m)]
    elif how == "all_unknown":
        ids = table[rng.integers(0, k, m)].copy()
        ids[:, 15] ^= 0x80  # (a row that becomes another row of the table is numpy's to tell)
    elif how == "all_skipped":
        ids, status = draw_ids(m, table, rng), np.full(m, 3, np.int32)
    else:
        ids, status, _ = mixed(m, table, rng, bad=0.3)
    keys = rng.integers(0, 256, 29 * len(ids), dtype=np.uint8)
    seq = rng.permutation(len(ids)).astype(np.uint32)
    w = route_and_check(codec, ids, table, status, seq, keys, stride=352, id_phase=1, phase=1)
    count = w["count"].astype(np.int64)
    if how == "one_bucket":
        assert count[k // 2] == m
    elif how == "own_bucket" and k >= m:
        assert count[:k].max() == 1 and count[:k].sum() == m
    elif how == "gaps":
        assert count[:k].sum() == m and count[1:k:3].sum() == 0 and count[2:k:3].sum() == 0
    elif how == "all_skipped":
        assert count[k + 1] == m and (w["bucket"] == NONE).all()
    elif how == "all_unknown":
        assert count[k] > m // 2
    elif how == "mixed":
        assert count[k] > 0 and count[k + 1] > 0 and count[:k].sum() > 0


# --------------------------------------------------------------------------
# 3. optional arguments
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    rng = np.random.default_rng(30)
    table = make_table(300, rng)
    ids, status, keys = mixed(1300, table, rng)
    return ids, table, status, rng.permutation(1300).astype(np.uint32), keys


@pytest.mark.parametrize("absent", (("bucket",), ("rows",), ("local",), ("keys_out",), ("bucket", "rows", "local", "keys_out")))
def test_each_optional_output_absent(codec, pool, absent):
    ids, table, status, seq, keys = pool
    route_and_check(codec, ids, table, status, seq, keys, stride=17, id_phase=1, phase=1, absent=absent)


@pytest.mark.parametrize("given", ("neither", "status", "seq"))
def test_optional_inputs(codec, pool, given):
    ids, table, status, seq, keys = pool
    route_and_check(codec, ids, table, status if given == "status" else None, seq if given == "seq" else None, None)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("id_phase", (0, 1))
@pytest.mark.parametrize("phase", (0, 1))
def test_phases_and_strides(codec, pool, stride, id_phase, phase):
    ids, table, status, seq, keys = pool
    route_and_check(codec, ids[:300], table, status[:300], None, keys[:29 * 300], stride=stride, id_phase=id_phase,
                    phase=phase)


def test_no_records(codec, pool):
    """m == 0: the offsets and counts alone, all zero; every other pointer may be NULL."""
    ids, table, *_ = pool
    empty = np.zeros((0, 16), np.uint8)
    for tab in (table, empty):
        w = route_and_check(codec, empty, tab, keys=np.zeros(0, np.uint8))
        assert not w["off"].any() and not w["count"].any()
        route_and_check(codec, empty, tab, absent=("bucket", "rows", "local"), how=dict(ids=0, work=0, work_bytes=0))
    route_and_check(codec, empty, empty, how=dict(ids=0, table=0))


def test_no_table(codec, pool):
    """k == 0: every record that takes part is of no known collection."""
    ids, _, status, seq, keys = pool
    w = route_and_check(codec, ids, np.zeros((0, 16), np.uint8), status, seq, keys, how=dict(table=0))
    assert int(w["count"][0]) == int((status == 0).sum()) and (w["bucket"] == NONE).all()


# --------------------------------------------------------------------------
# 4. garbage in: bounds only, through the guards
# --------------------------------------------------------------------------
def test_a_sequence_with_repeats_and_values_that_name_no_record(codec, pool):
    ids, table, status, seq, keys = pool
    m = len(ids)
    bad = seq.copy()
    bad[10:20] = bad[3]
    bad[40:45] = (m, m + 1, SEEK_NONE, 1 << 31, m + 4096)
    bad[-1] = m
    # what the contract says of such a sequence is still numpy's: a row per position, NONE for no record
    w = route_and_check(codec, ids, table, status, bad, keys, stride=17, id_phase=1, phase=1)
    assert int(w["count"][len(table) + 1]) >= 6 and (w["rows"][:, 2] == NONE).sum() == 6
    assert len(w["named"]) < m
    wild = np.random.default_rng(41).integers(0, 1 << 32, m, dtype=np.uint32)
    wild[::3] %= m
    route_and_check(codec, ids, table, status, wild, keys, stride=352)


@pytest.mark.parametrize("k", (300, 2500))
def test_a_table_out_of_order_and_with_repeats(codec, k):
    rng = np.random.default_rng(50 + k)
    table = make_table(k, rng)[rng.permutation(k)]
    table[rng.integers(0, k, k // 4)] = table[rng.integers(0, k, k // 4)]
    m = 2049
    ids, status, keys = mixed(m, table, rng)
    seq = rng.permutation(m).astype(np.uint32)

    def body(fill):
        c = Call(codec, ids, table, fill, status, seq, keys, 17, 1, 1)
        assert c.run() == 0
        c.write_set(np.arange(m))
        off, count = now(c.off, np.uint64), now(c.count, np.uint64)
        rows = now(c.rows, np.uint32).reshape(m, 4)
        # wrong classes perhaps, but a partition all the same
        assert int(off[k + 2]) == m and int(count.sum()) == m and (np.diff(off.astype(np.int64)) >= 0).all()
        assert (rows[:, 0] <= k + 1).all() and np.array_equal(np.sort(rows[:, 1]), np.arange(m))
        known = rows[rows[:, 0] < k]
        assert (table[known[:, 0]] == ids[known[:, 2]]).all()  # a class below k is a row that equals the ID

    guards.twice(body)


# --------------------------------------------------------------------------
# 5. refusals
# --------------------------------------------------------------------------
def test_refusals_store_nothing(codec, pool):
    ids, table, status, seq, keys = pool
    w = want(ids, table, status, seq, keys)

    def body(fill):
        c = Call(codec, ids, table, fill, status, seq, keys, 17, 1, 1)
        a = c.args()
        for kw in (dict(m=MAX_RECORDS + 1), dict(m=1 << 32), dict(m=(1 << 64) - 1), dict(k=(1 << 32) - 3),
                   dict(k=1 << 32), dict(k=(1 << 64) - 1), dict(m=MAX_RECORDS + 1, work_bytes=1 << 40)):
            assert c.run(**kw) == E_WORKSPACE, kw
        for kw in (dict(ctx=None), dict(off=0), dict(count=0), dict(ids=0), dict(id_stride=15), dict(id_stride=0),
                   dict(table=0), dict(keys=0), dict(keys_out=0), dict(work=0), dict(work=a["work"] + 128),
                   dict(work_bytes=c.work_bytes - 1), dict(work_bytes=0), dict(status=a["status"] + 2),
                   dict(seq=a["seq"] + 2), dict(bucket=a["bucket"] + 2), dict(local=a["local"] + 2),
                   dict(off=a["off"] + 4), dict(count=a["count"] + 4), dict(rows=a["rows"] + 8),
                   dict(rows=a["rows"] + 4)):
            assert c.run(**kw) == E_ARG, kw
        c.nothing_stored()
        assert c.run() == 0  # and the arguments were good
        c.check(w)

    guards.twice(body)


def test_a_context_takes_max_records(codec):
    rng = np.random.default_rng(60)
    table = make_table(40, rng)
    ids, status, keys = mixed(MAX_RECORDS, table, rng)
    route_and_check(codec, ids, table, status, None, keys)


def test_route_stage_param(codec, stage):
    assert stage == 2048
    assert codec.lib.honu_ctx_set_param(codec.ctx, b"route_stage", 512) == E_ARG


# --------------------------------------------------------------------------
# 6. graph
# --------------------------------------------------------------------------
def test_graph_replays_after_ids_statuses_and_table_changed(codec, pool):
    ids, table, status, seq, keys = pool
    rng = np.random.default_rng(70)
    table2 = make_table(len(table), rng)
    ids2, status2, _ = mixed(len(ids), table2, rng, bad=0.4)
    rounds = [(ids, status, table), (ids2, status, table), (ids2, status2, table2), (ids, status2, table2)]
    dev = codec.torch_device

    def refill(t, fill):
        blk = guards.block_of(t)
        p = guards.pattern(blk.start + blk.nbytes, fill)[blk.start:].copy()
        t.copy_(torch.from_numpy(p).to(dev))

    def body(fill):
        c = Call(codec, ids, table, fill, status, seq, keys, 17, 1, 1)
        assert c.run() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert c.run() == 0
        seen = []
        for x, st, tab in rounds:
            for t in c.outs:
                refill(t, fill)
            c.host["ids"] = strided(x, 17, np.random.default_rng(2))
            c.host["status"], c.host["table"] = st, tab
            for n in ("ids", "status", "table"):
                c.dev[n].copy_(torch.from_numpy(np.ascontiguousarray(c.host[n]).view(np.uint8).reshape(-1).copy()).to(dev))
            g.replay()
            w = want(x, tab, st, seq, keys)
            c.check(w)
            seen.append(w["count"].tobytes())
        assert len(set(seen)) == len(rounds)

    guards.twice(body)


# --------------------------------------------------------------------------
# 7. what the call is for: one sort and one route in place of a sort per collection
# --------------------------------------------------------------------------
def test_each_segment_is_the_sort_of_its_collection_alone(codec):
    m, k = 1025, 5
    rng = np.random.default_rng(80)
    dev = codec.torch_device
    table = make_table(k, rng)
    member = rng.integers(0, k, m)
    ids = table[member]
    objects = rng.integers(0, 256, (60, 29), dtype=np.uint8)  # few keys: many equal ones, within and across collections
    objects[:, 0] = 0x01
    keys = objects[rng.integers(0, 60, m)]
    status = np.where(rng.random(m) < 0.1, 5, 0).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_keys, d_status = up(keys), up(status)
    order, _, valid = codec.sort_keys(d_keys, d_status, n=m)
    r = codec.route_keys(up(ids), m, up(table), k, status=d_status, seq=order, keys=d_keys)
    torch.cuda.synchronize()
    assert int(valid.item()) == int((status == 0).sum())
    off = r.bucket_off.cpu().numpy()
    count = r.bucket_count.cpu().numpy()
    routed = r.keys.cpu().numpy().reshape(m, 29)
    rows = r.rows.cpu().numpy().view(np.uint32)
    local = r.local.cpu().numpy()
    assert off[k + 2] == m and off[k] == off[k + 1] == int(valid.item())  # no unknown collection here
    for c in range(k):
        own = np.flatnonzero(member == c)  # the collection's records in arrival order
        o2, s2, v2 = codec.sort_keys(up(keys[own]), up(status[own]), n=len(own), want_sorted=True)
        torch.cuda.synchronize()
        v = int(v2.item())
        assert v == count[c] == off[c + 1] - off[c] and v > 100
        alone = s2.cpu().numpy()[:29 * v].reshape(v, 29)
        assert routed[off[c]:off[c + 1]].tobytes() == alone.tobytes()
        # the same records under the rows, so equal keys stand in arrival order
        assert np.array_equal(rows[off[c]:off[c + 1], 2], own[o2.cpu().numpy()[:v]])
        assert np.array_equal(local[off[c]:off[c + 1]], np.arange(v))
    # the wrapper's outputs are the call's: against numpy as well
    w = want(ids, table, status, order.cpu().numpy().view(np.uint32), keys)
    assert np.array_equal(rows, w["rows"]) and np.array_equal(r.bucket.cpu().numpy().view(np.uint32), w["bucket"])
    assert np.array_equal(off.astype(np.uint64), w["off"]) and routed.reshape(-1).tobytes() == w["keys"].tobytes()
