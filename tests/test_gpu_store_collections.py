"""A store of three collections fed with mixed batches, on the GPU.

tests/store_collections.py takes every batch apart on the device with
honu_key_route and hands each collection's segment to an unchanged
store_gpu.Store. Each of three batches holds about 300 generator Small records
of three collections mixed together, records of a collection the store does not
have, one record that does not decode, and records that carry the key of an
earlier record of their collection. After every round each collection's
column, valid count, order and the record under every column row equal those
of a control Store that was given that collection's records alone, in arrival
order, through put_raw; honu_key_merge fed directly with the segment of
d_keys_out, d_local and d_bucket_count + c gives the same column; and the
unknown collection's records and the malformed record reach no store.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import HostBatch  # noqa: E402
from honu_amd.workload import gen_host_batch  # noqa: E402
from store_collections import CollectionStore, subset  # noqa: E402
from store_gpu import Store  # noqa: E402

MAX_RECORDS = 4096
K = 3
TABLE = np.array([[0x01] + [0x55] * 15, [0x01] + [0x55] * 14 + [0x56], [0xC0] + [0x00] * 15], np.uint8)
UNKNOWN = np.array([0x01] + [0x55] * 14 + [0x57], np.uint8)  # a neighbour of two rows; no bucket of that name


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, MAX_RECORDS)
    yield c
    c.close()


def h(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.reshape(-1).view(np.uint8).view(dtype)


def mixed_batch(seed, m):
    """(batch, member): record i is of collection member[i], 3 the unknown one."""
    rng = np.random.default_rng(seed)
    hb = gen_host_batch(seed, "small", 0, m)
    meta = hb.meta.copy()
    member = rng.integers(0, K + 1, m)
    member[rng.random(m) < 0.15] = K  # and more of the unknown collection
    meta["collection_id"] = np.concatenate([TABLE, UNKNOWN[None]])[member]
    for j in range(6):  # the key of an earlier record of the same collection
        own = np.flatnonzero(member == j % K)
        a, b = own[2 * j], own[2 * j + 9]
        for f in ("object_id", "vid", "pid"):
            meta[f][b] = meta[f][a]
    return HostBatch(meta, hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off), member


def records_by_row(store):
    """The record under every valid column row."""
    off, arena, order = h(store.rec_off), h(store.arena), h(store.order)
    v = int(store.valid.item())
    return [arena[int(off[r]):int(off[r + 1])].tobytes() for r in order[:v]]


def test_three_rounds_of_mixed_batches(codec):
    cs = CollectionStore(codec, TABLE)
    controls = [Store(codec) for _ in range(K)]
    to_control = [[] for _ in range(K)]  # per collection: the store's record index -> the control's
    reached = 0
    for seed, m in ((901, 300), (902, 333), (903, 257)):
        hb, member = mixed_batch(seed, m)
        spoiled = int(np.flatnonzero(member == 1)[5])  # a record of a known collection that will not decode
        R = cs.put(hb, spoil=[spoiled])
        torch.cuda.synchronize()
        st = h(R.key_status)
        assert st[spoiled] != 0 and (np.delete(st, spoiled) == 0).all()
        off, count = R.off, h(R.route.bucket_count)
        known = (member < K) & (np.arange(m) != spoiled)
        assert count[K] == int((member == K).sum()) > 20 and count[K + 1] == 1 and off[K] == int(known.sum())
        rows = h(R.route.rows).view(np.uint32)
        assert rows[off[K + 1], 2] == spoiled and set(rows[off[K]:off[K + 1], 2]) == set(np.flatnonzero(member == K))
        bucket = h(R.route.bucket).view(np.uint32)
        assert np.array_equal(bucket, np.where(known, member, 0xFFFFFFFF).astype(np.uint32))
        for c in range(K):
            idx = np.flatnonzero((member == c) & known)  # the collection's records alone, in arrival order
            ctl, store = controls[c], cs.stores[c]
            first_ctl = ctl.n
            ctl.put_raw(subset(hb, idx))
            (col0, order0, valid0, n0), first, fetched = R.segments[c]
            a, cnt = int(off[c]), int(count[c])
            assert cnt == len(idx) > 30 and first == n0 == first_ctl and (h(fetched) == 0).all()
            # the segment's rows name the collection's records, in key order; local counts them
            seg = rows[a:a + cnt]
            assert (seg[:, 0] == c).all() and sorted(seg[:, 2]) == idx.tolist()
            assert np.array_equal(h(R.route.local)[a:a + cnt], np.arange(cnt))
            place = {int(r): j for j, r in enumerate(idx)}
            to_control[c] += [first_ctl + place[int(r)] for r in seg[:, 2]]
            # the store against the control
            torch.cuda.synchronize()
            assert store.n == ctl.n == len(to_control[c])
            assert int(store.valid.item()) == int(ctl.valid.item()) == store.n
            assert h(store.col).tobytes() == h(ctl.col).tobytes()
            assert np.array_equal(np.asarray(to_control[c])[h(store.order)], h(ctl.order))
            assert records_by_row(store) == records_by_row(ctl)
            # honu_key_merge fed with the route's outputs as they stand
            seg_keys = R.route.keys[29 * a:29 * (a + cnt)]
            seg_local, seg_count = R.route.local[a:a + cnt], R.route.bucket_count[c:c + 1]
            if n0 == 0:  # nothing to merge into: the segment is the column
                assert h(seg_keys).tobytes() == h(store.col).tobytes() and int(seg_count.item()) == store.n
                assert np.array_equal(h(seg_local), h(store.order))
            else:
                col, order, valid = codec.merge_keys(col0, order0, valid0, seg_keys, seg_local, seg_count, b_base=n0)
                torch.cuda.synchronize()
                assert h(col).tobytes() == h(store.col).tobytes() and int(valid.item()) == store.n
                assert np.array_equal(h(order), h(store.order))
            # equal keys met: the column has fewer distinct rows than rows
            assert len(set(map(bytes, h(store.col).reshape(-1, 29)))) < store.n
        reached += int(known.sum())
        assert sum(s.n for s in cs.stores) == reached  # the unknown and the malformed records reached no store
