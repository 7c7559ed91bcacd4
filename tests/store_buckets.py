"""A store of many collections as ONE bucketed column over one Codec: the driver
of tests/test_gpu_store_buckets.py. TEST INFRASTRUCTURE ONLY.

tests/store_collections.py keeps one store_gpu.Store per collection and reads
d_bucket_off on the host after every route, since honu_key_merge's nb and
pointers are host arguments. Here all k buckets' columns lie end to end in one
arena (sorted rows, order, k + 1 offsets, k counts) and a mixed batch is
written by one chain on one stream:

  marshal -> decode -> keys -> sort (the batch's keys, once, as a whole)
  -> route (the decoded rows' collection IDs, the sort's order as the sequence)
  -> merge_bucket_keys (the route's keys, local and bucket_off as they stand:
     the B side; d_base the buckets' record counts, so that every bucket keeps
     its own record numbering, as a Store per collection has it)

with nothing read on the host between the route and the merge: the arenas are
sized by na + nb, both host bounds. The buckets' record counts advance on the
device too (base += bucket_count[:k]).
"""
import torch

from store_gpu import Store


class BucketStore:
    def __init__(self, codec, table):
        """table: uint8[k, 16], the collections' IDs, ascending and distinct."""
        self.c, self.k = codec, len(table)
        self.front = Store(codec)  # its plumbing alone: uploads, the encode, the decode
        self.table = self.front._dev(table)
        dev = codec.torch_device
        self.col = torch.empty(0, dtype=torch.uint8, device=dev)
        self.order = torch.empty(0, dtype=torch.int32, device=dev)
        self.off = torch.zeros(self.k + 1, dtype=torch.int64, device=dev)
        self.count = torch.zeros(self.k, dtype=torch.int64, device=dev)
        self.base = torch.zeros(self.k, dtype=torch.int32, device=dev)  # records each bucket holds
        self.rows = 0  # a host bound on the arena's rows: the sum of the batches' sizes

    def put(self, hb, spoil=(), count_a=None):
        """One round over a mixed batch; returns the route. spoil: records whose encoded bytes are overwritten
        before the decode. count_a: the buckets' valid rows (int64[k] on the device), when deletes left some."""
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
        # nothing read on the host from here on
        res = c.merge_bucket_keys(k, self.col, self.order, self.off, r.keys, r.local, r.bucket_off, count_a=count_a,
                                  nb=m, base=self.base)
        self.base = self.base + r.bucket_count[:k].to(torch.int32)
        self.col, self.order, self.off, self.count = res.sorted, res.order, res.off, res.count
        self.rows += m
        return r

    def view(self, c, off):
        """Bucket c as (sorted column, order, valid count): an input of every per-bucket call. off: the offsets
        on the host (the caller's read)."""
        a, e = int(off[c]), int(off[c + 1])
        return self.col[29 * a:29 * e], self.order[a:e], self.count[c:c + 1]
