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
from collections import namedtuple

import numpy as np
import torch

from store_gpu import Shipped, Store
from store_reclaim import ReclaimStore

Routed = namedtuple("Routed", "route keys key_status fetch_status off bucket_off m")


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


class BucketView(ReclaimStore):
    """One bucket of a BucketRounds as a store_gpu.Store: col, order and valid are the bucket's view into the
    arena (d_sorted + 29 off[c], d_order + off[c], d_count + c), the record state (the unsorted keys and
    statuses, the honu_record_info rows, the CSR records arena, n) is the bucket's own, numbered d_local +
    d_base[c]. Store's read methods run over the view unchanged. The invariant they need, one row per
    record, holds by the recipe of include/honu_codec.h: a delete over the view is followed by reclaim()
    before the merge that squeezes the bucket."""

    def attach(self, col, order, count):
        self.col, self.order, self.valid, self.view_order = col, order, count, order
        assert col.numel() == 29 * self.n and order.numel() == self.n  # the view's rows equal the records

    def append(self, m, keys, info, arena, sizes):
        """Store._merge's bookkeeping for m routed records: every one of them is a valid row."""
        c = self.c
        self.keys = self._grown("keys", keys)
        self.key_status = self._grown("key_status", torch.zeros(4 * m, dtype=torch.uint8, device=keys.device)).view(torch.int32)
        self.info = self._grown("info", info)
        self.arena = self._grown("arena", arena)
        self.rec_size = self._grown("rec_size", self._dev(np.asarray(sizes, np.int64)))
        self.n, self.rec_bytes = self.n + m, self.rec_bytes + arena.numel()
        rec_off = c._empty(8 * (self.n + 1))
        c.scan(self.rec_size, self.n, rec_off)
        self.rec_off = rec_off[:8 * (self.n + 1)].view(torch.int64)

    def reclaim(self):
        """ReclaimStore.reclaim over the view: the new order goes back into the arena, whole (the rows behind
        the valid ones name no record any more), and the view shrinks to the kept rows until the next merge."""
        n, view_order, col = self.n, self.view_order, self.col
        self.order = view_order  # all n rows, as the call takes them
        R = self.c.reclaim_records(self.order, self.valid, n, self.arena, self.rec_off, n, self.rec_bytes,
                                   max(self.rec_bytes, 16), keys=self.keys, key_status=self.key_status, info=self.info)
        kept, total = torch.cat([R.kept, R.val_total]).cpu().tolist()  # the one host read
        view_order.copy_(R.order)
        sizes = (R.rec_off[1:kept + 1] - R.rec_off[:kept]).contiguous().view(torch.uint8)
        self.col, self.order = col[:29 * kept], view_order[:kept]
        self.n, self.rec_bytes, self.removed = kept, total, None
        self.rec_off = R.rec_off[:kept + 1]
        self._room_of = {"keys": (R.keys, 29 * kept), "key_status": (R.key_status.view(torch.uint8), 4 * kept),
                         "info": (R.info, 32 * kept), "arena": (R.values, total), "rec_size": (sizes, 8 * kept)}
        self.keys, self.key_status = R.keys[:29 * kept], R.key_status[:kept]
        self.info, self.arena, self.rec_size = R.info[:32 * kept], R.values[:total], sizes
        return kept, total, R.kept


class BucketRounds(BucketStore):
    """BucketStore with the buckets' record state: the driver of tests/test_gpu_store_bucket_rounds.py. The
    write chain is marshal -> decode -> keys -> sort -> route -> fetch of the routed rows (d_total =
    d_bucket_off + k) -> merge_bucket_keys (d_order_b = d_local, d_base the buckets' record counts), nothing
    read on the host between the route and the merge. One host read follows the merge, of d_off_out,
    d_bucket_off and the fetch's offsets: it splits the fetched records into the buckets' arenas, and view()
    needs it anyway. keep: the buckets whose record state is kept (default: all); d_info is given only over
    their views."""

    def __init__(self, codec, table, keep=None):
        super().__init__(codec, table)
        self.views = {c: BucketView(codec) for c in (range(self.k) if keep is None else keep)}
        self.host_off = np.zeros(self.k + 1, np.int64)

    def put(self, hb, spoil=(), counted=False):
        f, m = self.front, len(hb.meta)
        b, _ = f._batch(hb)
        cap = f._room(hb)
        arena, sizes, out_off, _ = f._encode(b, cap)
        for i in spoil:  # (a test's own host read: where the record lies)
            a, e = int(out_off[i].item()), int(out_off[i + 1].item())
            arena[a:e] = 0xFF
        return self.put_records(arena, out_off, m, cap, counted)

    def put_records(self, arena, out_off, m, cap, counted=False) -> Routed:
        """decode -> keys -> sort -> route -> fetch -> merge of m records in a CSR arena of cap bytes."""
        c, k, f = self.c, self.k, self.front
        d = f._decode(arena, out_off, m, cap)
        keys, st = c.keys(d)
        keys, st = keys[:29 * m], st[:4 * m]
        order, _, _ = c.sort_keys(keys, st, n=m)
        r = c.route_keys(d.meta.data_ptr() + 112, m, self.table, k, id_stride=352, status=st, seq=order, keys=keys)
        values, val_off, _, fetched = c.fetch_objects(r.rows, r.bucket_off[k:k + 1], m, arena, out_off, m, cap, cap)
        res = c.merge_bucket_keys(k, self.col, self.order, self.off, r.keys, r.local, r.bucket_off,
                                  count_a=self.count if counted else None, nb=m, base=self.base)
        self.base = self.base + r.bucket_count[:k].to(torch.int32)
        self.col, self.order, self.off, self.count = res.sorted, res.order, res.off, res.count
        self.rows += m
        # the one host read: where every bucket lies now, and where its new records lie in what was fetched
        host = torch.cat([res.off, r.bucket_off, val_off]).cpu().numpy()
        self.host_off, boff, voff = host[:k + 1], host[k + 1:2 * k + 4], host[2 * k + 4:]
        info = d.info[:32 * m].view(m, 32)
        for j, v in self.views.items():
            a, cnt = int(boff[j]), int(boff[j + 1] - boff[j])
            v.acl_room, v.regions_room = f.acl_room, f.regions_room  # what is stored is some of what arrived
            if cnt:
                records = r.rows[a:a + cnt, 2].long()
                v.append(cnt, r.keys[29 * a:29 * (a + cnt)], info[records].reshape(-1),
                         values[int(voff[a]):int(voff[a + cnt])], np.diff(voff[a:a + cnt + 1]))
            v.attach(*self.view(j, self.host_off))
        return Routed(r, keys, st.view(torch.int32), fetched, self.host_off, boff, m)

    def drop(self, j, prefixes=None, probe_len=17, superseded=False):
        """honu_key_delete over bucket j's view: the rows back into the view, the count into the count array."""
        c = self.c
        col, order, valid = self.view(j, self.host_off)
        del_sorted = del_valid = None
        if prefixes is not None:
            n = len(prefixes)
            _, del_sorted, del_valid = c.sort_keys(self.front._dev(prefixes), None, n=n, want_sorted=True)
            del_sorted = del_sorted[:29 * n]
        new_col, new_order, new_valid, removed = c.delete_keys(col, order, valid, del_sorted, del_valid, probe_len, superseded)
        col.copy_(new_col)
        order.copy_(new_order)
        valid.copy_(new_valid)
        if j in self.views:
            self.views[j].removed = removed
        return removed

    def reclaim(self, j):
        """honu_key_reclaim over bucket j's view and record state; d_base[j] is then `kept`."""
        kept, total, d_kept = self.views[j].reclaim()
        self.base[j:j + 1].copy_(d_kept.to(torch.int32))
        return kept, total

    def gather(self, peer: "BucketRounds"):
        """Per bucket compare -> list -> fetch against the peer's view: what to send, a Shipped each (None
        for a bucket that holds no record)."""
        c, out = self.c, []
        for j, v in self.views.items():
            if v.n == 0:
                out.append(None)
                continue
            pcol, _, pvalid = peer.view(j, peer.host_off)
            cmp = v.compare(pcol, pvalid)
            cap = v.n
            rows, _, total, keys = c.list_keys(v.col, v.order, v.valid, cmp.rows, cap, want_keys=True)
            val_cap = max(v.rec_bytes, 16)
            values, val_off, val_total, status = c.fetch_objects(rows, total, cap, v.arena, v.rec_off, v.n, v.rec_bytes,
                                                                 val_cap)
            out.append(Shipped(cmp, rows, total, keys, values, val_off, val_total, status, cap, None))
        return out

    def ship(self, peer: "BucketRounds", gathered, counted=True):
        """The buckets' shipments concatenated on the device into one batch of many collections mixed
        together, then decode -> keys -> sort -> route -> fetch -> merge on the peer. The batch crosses the
        wire as (values, offsets): the one host read is of each shipment's row and byte totals."""
        sent = [g for g in gathered if g is not None]
        totals = torch.cat([t for g in sent for t in (g.total, g.val_total)]).cpu().tolist()
        values, offsets, at = [], [], 0
        for g, t, nbytes in zip(sent, totals[0::2], totals[1::2]):
            values.append(g.values[:nbytes])
            offsets.append(g.val_off[:t] + at)
            at += nbytes
        m = sum(totals[0::2])
        if m == 0:
            return None
        offsets.append(torch.tensor([at], dtype=torch.int64, device=values[0].device))
        cap = max(at, 16)
        arena = peer.c._empty(cap)
        arena[:at].copy_(torch.cat(values))
        peer.front.acl_room += self.front.acl_room  # what is shipped is some of what is stored here
        peer.front.regions_room += self.front.regions_room
        return peer.put_records(arena, torch.cat(offsets), m, cap, counted)
