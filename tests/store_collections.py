"""A store of many collections over one Codec: the driver of
tests/test_gpu_store_collections.py. TEST INFRASTRUCTURE ONLY.

The reference store has one bbolt bucket per collection, named by the
collection ID (store.go:236-240, tx.go:112-120). Here a bucket is an unchanged
store_gpu.Store, one per row of the table of collections, and a mixed batch is
taken apart on the device by honu_key_route. One round:

  marshal -> decode -> keys -> sort (the batch's keys, once, as a whole)
  -> route (the decoded rows' collection IDs as they stand, the sort's order
     as the sequence, so every bucket's rows come out in key order)
  -> fetch (the routed rows; d_total = d_bucket_off + k: the rows of the known
     collections, bucket by bucket, in one CSR arena)
  -> per collection: decode of its segment -> Store._merge

One host read follows the route, of d_bucket_off: the segments' lengths are
host arguments of everything after it. The records of no known collection and
the records that did not decode are behind d_bucket_off[k] and reach no store.
"""
from collections import namedtuple

import numpy as np
import torch

from honu_amd.metadata import HostBatch
from store_gpu import Store

Routed = namedtuple("Routed", "route off key_status keys m segments")


def subset(hb: HostBatch, idx) -> HostBatch:
    """The records idx of a batch, in that order, as a batch of their own: the rows keep their offsets into the
    batch's tables, the payloads are gathered."""
    off = hb.payload_off.astype(np.int64)
    parts = [hb.payload[off[i]:off[i + 1]] for i in idx]
    new = np.zeros(len(idx) + 1, np.uint64)
    new[1:] = np.cumsum([len(p) for p in parts])
    payload = np.concatenate(parts + [np.zeros(1, np.uint8)])
    return HostBatch(hb.meta[np.asarray(idx, np.int64)].copy(), hb.var, hb.acl, hb.regions, payload, new)


class CollectionStore:
    def __init__(self, codec, table):
        """table: uint8[k, 16], the collections' IDs, ascending and distinct."""
        self.c, self.k = codec, len(table)
        self.front = Store(codec)  # its plumbing alone: uploads, the encode, the decode
        self.table = self.front._dev(table)
        self.stores = [Store(codec) for _ in range(self.k)]

    def put(self, hb: HostBatch, spoil=()) -> Routed:
        """One round over a mixed batch. spoil: records whose encoded bytes are overwritten before the decode."""
        c, k, f, m = self.c, self.k, self.front, len(hb.meta)
        b, _ = f._batch(hb)
        cap = f._room(hb)
        arena, sizes, out_off, _ = f._encode(b, cap)
        for i in spoil:  # (a test's own host read: where the record lies)
            a, e = int(out_off[i].item()), int(out_off[i + 1].item())
            arena[a:e] = 0xFF
        d = f._decode(arena, out_off, m, cap)
        keys, st = c.keys(d)
        keys, st = keys[:29 * m], st[:4 * m]
        order, _, _ = c.sort_keys(keys, st, n=m)
        r = c.route_keys(d.meta.data_ptr() + 112, m, self.table, k, id_stride=352, status=st, seq=order, keys=keys)
        # the routed rows of the known collections, fetched bucket by bucket: nothing read on the host so far
        values, val_off, _, status = c.fetch_objects(r.rows, r.bucket_off[k:k + 1], m, arena, out_off, m, cap, cap)
        off = r.bucket_off.cpu().numpy()  # the one host read that follows a route
        segments = []
        for j, store in enumerate(self.stores):
            a, cnt = int(off[j]), int(off[j + 1] - off[j])
            if cnt == 0:
                segments.append(None)
                continue
            store.acl_room += f.acl_room
            store.regions_room += f.regions_room
            seg_off = val_off[a:a + cnt + 1]
            dj = store._decode(values, seg_off, cnt, cap)
            kj, sj = c.keys(dj)
            kj, sj = kj[:29 * cnt], sj[:4 * cnt].view(torch.int32)
            before = (store.col, store.order, store.valid, store.n)
            base = seg_off[:1]
            first = store._merge(cnt, kj, sj, dj.info, values[int(base.item()):], None, seg_off - base)
            segments.append((before, first, status[a:a + cnt]))
        return Routed(r, off, st.view(torch.int32), keys, m, segments)
