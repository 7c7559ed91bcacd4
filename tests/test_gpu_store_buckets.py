"""A store of three collections kept as one bucketed column, on the GPU.

tests/store_buckets.py writes every mixed batch with the chain sort -> route
-> honu_key_merge_buckets, nothing read on the host between the route and the
merge. The control is tests/store_collections.py's CollectionStore, an
unchanged store_gpu.Store per collection fed with k honu_key_merge calls after
a host read. Three batches of about 300 generator Small records of three
collections mixed together, with records of a collection the store does not
have, one record that does not decode and records that carry the key of an
earlier record of their collection (tests/test_gpu_store_collections.py's
batches). After every round each bucket's view equals the control's column and
order for that collection, honu_key_seek over each view finds every key put so
far, and before the last round a honu_key_delete over one view writes that
bucket's count, the next merge's d_count_a.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import SEEK_FOUND  # noqa: E402
from store_buckets import BucketStore  # noqa: E402
from store_collections import CollectionStore  # noqa: E402
from test_gpu_store_collections import K, MAX_RECORDS, TABLE, h, mixed_batch  # noqa: E402


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, MAX_RECORDS)
    yield c
    c.close()


def test_three_rounds_into_one_bucketed_column(codec):
    cs, bs = CollectionStore(codec, TABLE), BucketStore(codec, TABLE)
    put = [[] for _ in range(K)]  # per collection: every key put so far
    rounds = ((901, 300), (902, 333), (903, 257))
    count_a = None
    for rnd, (seed, m) in enumerate(rounds):
        hb, member = mixed_batch(seed, m)
        spoiled = int(np.flatnonzero(member == 1)[5])  # a record of a known collection that will not decode
        R = cs.put(hb, spoil=[spoiled])
        r = bs.put(hb, spoil=[spoiled], count_a=count_a)
        count_a = None
        torch.cuda.synchronize()
        off, count = h(bs.off), h(bs.count)
        known = (member < K) & (np.arange(m) != spoiled)
        batch_keys = h(R.keys).reshape(m, 29)
        assert h(r.bucket_off).tolist() == R.off.tolist()  # the same route
        assert off[0] == 0 and np.array_equal(np.diff(off), count)
        assert int(h(r.bucket_count)[K]) > 20  # the unknown collection's records reach no bucket
        for c in range(K):
            store = cs.stores[c]
            v = int(store.valid.item())
            assert count[c] == v > 30, (rnd, c, count[c], v)
            col, order, valid = bs.view(c, off)
            # the control keeps the rows a delete took out behind its valid rows; the bucketed column is tight
            assert h(col).tobytes() == h(store.col)[:29 * v].tobytes(), (rnd, c)
            assert np.array_equal(h(order), h(store.order)[:v]), (rnd, c)
            # every key put so far, less what the delete took, is found in the view
            put[c] += [bytes(x) for x in batch_keys[(member == c) & known]]
            probes = np.frombuffer(b"".join(put[c]), np.uint8)
            rows = h(codec.seek_keys(col, valid, bs.front._dev(probes), 29, order=order)).view(np.uint32)
            held = set(map(bytes, h(col).reshape(-1, 29)))
            found = (rows[:, 4] & SEEK_FOUND) != 0
            assert np.array_equal(found, np.array([x in held for x in put[c]])), (rnd, c)
            assert found.sum() >= len(put[c]) - 40 and (rnd < 2 or c != 1 or not found.all())
            assert (rows[found, 1] <= v).all()
        assert int(off[K]) == sum(int(s.valid.item()) for s in cs.stores)
        if rnd == 1:
            # a delete over one view: its rows that stay to the front of the view, its count to the count array
            c = 1
            col, order, valid = bs.view(c, off)
            gone = np.stack([np.frombuffer(x, np.uint8) for x in put[c][3:40:3]])  # whole keys: every row of one goes
            _, del_sorted, del_valid = codec.sort_keys(bs.front._dev(gone), None, n=len(gone), want_sorted=True)
            new_col, new_order, new_valid, _ = codec.delete_keys(col, order, valid, del_sorted[:29 * len(gone)], del_valid,
                                                                 probe_len=29)
            col.copy_(new_col)
            order.copy_(new_order)
            count_a = bs.count.clone()
            count_a[c:c + 1].copy_(new_valid)
            cs.stores[c].drop(gone, probe_len=29)
            torch.cuda.synchronize()
            assert 0 < int(count_a[c].item()) == int(cs.stores[c].valid.item()) < count[c]
