"""A store over one Codec that holds only device state: the driver of
tests/test_gpu_store_rounds.py. TEST INFRASTRUCTURE ONLY.

What a cgo caller would build from the honu_key_* calls, each output handed to
the next call as the header says it may be:

  column, order, valid   the sorted key column, as the last merge or delete wrote it
  keys, key_status       the unsorted key column of all batches, concatenated
  info                   their honu_record_info rows, concatenated (the key calls read
                         only `tombstone` there; data_off stays relative to its batch)
  arena, rec_size,       the records of all batches, one CSR arena: the sizes are kept,
  rec_off                and the offsets are their honu_exclusive_scan after every batch
  n                      the records so far

Invariant: the column has one row per record. Every batch is merged whole, its
invalid rows included, because d_info is indexed by record index and the calls
clamp such an index by n, the column's rows.

Within a batch nothing is read on the host between the first call and the
last. One host read follows a batch that brings records: its byte total, to
append its records to the arena, as a caller sizing its arena reads it. The
encoders need a 16-byte aligned arena, so each batch is encoded into a buffer
of its own and its bytes are appended. The plumbing is torch on the device:
buffers grow by device-to-device copies, and no offset needs a base added: the
running offsets are the library's own scan of the sizes. A shipped batch comes
as (values, offsets), what would cross the wire; the receiver's one host read is
of those offsets, whose last is the byte total.
"""
from collections import namedtuple

import numpy as np
import torch

from honu_amd import object as hobj
from honu_amd.metadata import HostBatch

NEXT_DELETE = 3

Wrote = namedtuple("Wrote", "rows keys key_status arena out_off enc_status decoded_keys decoded_status m first")
Put = namedtuple("Put", "arena out_off enc_status keys key_status m first")
Read = namedtuple("Read", "seeks rows range_off total keys values val_off val_total status decoded cap")
Listed = namedtuple("Listed", "rows range_off total unfiltered_total cap")
Compared = namedtuple("Compared", "rows peer counts objects")
Shipped = namedtuple("Shipped", "compared rows total keys values val_off val_total status cap first")


class Store:
    def __init__(self, codec: hobj.Codec):
        self.c = c = codec
        dev = c.torch_device
        self.col = torch.empty(0, dtype=torch.uint8, device=dev)
        self.order = torch.empty(0, dtype=torch.int32, device=dev)
        self.valid = self._dev(np.zeros(1, np.int64)).view(torch.int64)
        self.keys = torch.empty(0, dtype=torch.uint8, device=dev)
        self.key_status = torch.empty(0, dtype=torch.int32, device=dev)
        self.info = torch.empty(0, dtype=torch.uint8, device=dev)
        self.arena = torch.empty(0, dtype=torch.uint8, device=dev)
        self.rec_size = torch.empty(0, dtype=torch.uint8, device=dev)  # int64 per record, as bytes
        self.rec_off = self._dev(np.zeros(1, np.int64)).view(torch.int64)
        self.n = 0
        self.rec_bytes = 0
        self.acl_room = self.regions_room = 16  # bounds the host knows on the stored records' list entries
        self.removed = None
        self._room_of = {}  # a growing buffer's name -> (its allocation, the bytes in use)
        self._whole = self._dev(np.zeros((1, 29), np.uint8))

    # ---- plumbing ---------------------------------------------------------
    def _dev(self, a):
        a = np.ascontiguousarray(a)
        return hobj._dev_bytes(a, self.c.torch_device)[:a.nbytes]

    def _upload(self, *arrays):
        """Host arrays in ONE upload, since every copy from pageable memory costs a wait: their device
        views, 16-byte aligned and none empty (an unused table still gets an address)."""
        raw = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]
        room = [-(-max(r.size, 16) // 16) * 16 for r in raw]
        at = np.concatenate([[0], np.cumsum(room)])
        buf = np.zeros(int(at[-1]), np.uint8)
        for r, o in zip(raw, at):
            buf[o:o + r.size] = r
        t = hobj._dev_bytes(buf, self.c.torch_device)
        return [t[o:o + max(r.size, 16)] for r, o in zip(raw, at)]

    def _batch(self, hb: HostBatch, *more):
        """The encode input on the device, and `more` arrays with it."""
        meta, var, acl, regions, payload, payload_off, *rest = self._upload(
            hb.meta, hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off, *more)
        self.acl_room += len(hb.acl)
        self.regions_room += len(hb.regions)
        return hobj.DeviceBatch(meta, var, len(hb.var), acl, len(hb.acl), regions, len(hb.regions), payload,
                                payload_off, len(hb.meta)), rest

    def _decode(self, rec, rec_off, n, rec_bytes):
        return self.c.decode(rec, rec_off, n, acl_cap=self.acl_room, regions_cap=self.regions_room, rec_bytes=rec_bytes)

    def _encode(self, b: hobj.DeviceBatch, cap):
        c, m = self.c, b.n
        sizes, out_off, status, arena = c._empty(8 * m), c._empty(8 * (m + 1)), c._empty(4 * m), c._empty(cap)
        c.encode_sizes(b, sizes, status)
        c.scan(sizes, m, out_off)
        c.marshal_into(b, arena, cap, out_off, status)
        return arena, sizes[:8 * m], out_off[:8 * (m + 1)].view(torch.int64), status[:4 * m].view(torch.int32)

    def _grown(self, name, more):
        """The bytes of `more` appended to the growing buffer `name`: a device copy, and when the
        allocation is full a doubled one with the old bytes copied over. Returns the bytes in use."""
        buf, used = self._room_of.get(name, (None, 0))
        k = more.numel()
        if buf is None or used + k > buf.numel():
            new = self.c._empty(max(2 * (used + k), 1 << 12))
            if used:
                new[:used].copy_(buf[:used])
            buf = new
        buf[used:used + k].copy_(more)
        self._room_of[name] = (buf, used + k)
        return buf[:used + k]

    @staticmethod
    def _room(hb: HostBatch):
        """A bound on the batch's encoded bytes that the host knows: payloads, the variable bytes with their
        length prefixes, 18 bytes per ACL entry, 5 per region, and the fixed fields of a record."""
        return int(hb.payload_off[len(hb.meta)]) + len(hb.var) + 18 * len(hb.acl) + 5 * len(hb.regions) + 512 * len(hb.meta) + 16

    def _merge(self, m, keys, key_status, info, arena, sizes, offsets):
        """Sort the batch's keys, merge them whole into the column, then append the batch's state."""
        c = self.c
        order_b, sorted_b, valid_b = c.sort_keys(keys, key_status.view(torch.uint8), n=m, want_sorted=True)
        if self.n == 0:  # an empty store has no column to merge into: the first batch's sort is the column
            col, order, valid = sorted_b[:29 * m], order_b, valid_b
        else:
            col, order, valid = c.merge_keys(self.col, self.order, self.valid, sorted_b[:29 * m], order_b, valid_b,
                                             b_base=self.n)
        # the one host read: the batch's bytes
        if sizes is not None:
            total = int(offsets[m].item())
        else:  # a shipped batch has crossed the wire as (values, offsets): the receiver has the offsets
            off = offsets[:m + 1].cpu().numpy()
            total, sizes = int(off[m]), self._dev(np.diff(off))
        first = self.n
        self.col, self.order, self.valid = col, order, valid
        self.keys = self._grown("keys", keys[:29 * m])
        self.key_status = self._grown("key_status", key_status[:m].view(torch.uint8)).view(torch.int32)
        self.info = self._grown("info", info[:32 * m])
        self.arena = self._grown("arena", arena[:total])
        self.rec_size = self._grown("rec_size", sizes[:8 * m])
        self.n, self.rec_bytes = first + m, self.rec_bytes + total
        rec_off = c._empty(8 * (self.n + 1))
        c.scan(self.rec_size, self.n, rec_off)
        self.rec_off = rec_off[:8 * (self.n + 1)].view(torch.int64)
        assert self.col.numel() == 29 * self.n and self.order.numel() == self.n  # column rows equal records
        assert self.info.numel() == 32 * self.n and self.rec_off.numel() == self.n + 1
        return first

    def _info(self):
        return self.info if self.n else None

    # ---- writes -----------------------------------------------------------
    def write(self, op, requests, skip, pid, region, now, rows: HostBatch) -> Wrote:
        """next -> encode_sizes -> scan -> marshal_into -> decode -> keys -> sort over next's keys -> merge."""
        c, m = self.c, len(requests)
        if op == NEXT_DELETE:  # a tombstone is encoded with an empty payload
            rows = HostBatch(rows.meta, rows.var, rows.acl, rows.regions, np.zeros(1, np.uint8), np.zeros(m + 1, np.uint64))
        b, (d_req, d_skip) = self._batch(rows, requests, np.zeros(m, np.int32) if skip is None else np.asarray(skip, np.int32))
        cap = self._room(rows)
        out, keys, key_status = c.next_versions(self.col, self.valid, d_req, op, pid, region, now,
                                                order=self.order if self.n else None, info=self._info(),
                                                req_status=d_skip, meta=b.meta, m=m)
        arena, sizes, out_off, enc_status = self._encode(b, cap)
        d = self._decode(arena, out_off, m, cap)
        k2, st2 = c.keys(d)
        first = self._merge(m, keys, key_status, d.info, arena, sizes, out_off)
        return Wrote(out, keys, key_status, arena, out_off, enc_status, k2[:29 * m], st2[:4 * m].view(torch.int32), m, first)

    def put_raw(self, rows: HostBatch) -> Put:
        """marshal -> decode -> keys -> sort -> merge of already-versioned records."""
        c, m = self.c, len(rows.meta)
        b, _ = self._batch(rows)
        cap = self._room(rows)
        arena, sizes, out_off, enc_status = self._encode(b, cap)
        d = self._decode(arena, out_off, m, cap)
        k, st = c.keys(d)
        k, st = k[:29 * m], st[:4 * m].view(torch.int32)
        first = self._merge(m, k, st, d.info, arena, sizes, out_off)
        return Put(arena, out_off, enc_status, k, st, m, first)

    def _delete(self, del_sorted, del_valid, probe_len, superseded):
        self.col, self.order, self.valid, self.removed = self.c.delete_keys(
            self.col, self.order, self.valid, del_sorted, del_valid, probe_len, superseded)
        return self.removed

    def drop(self, prefixes, probe_len=17):
        k = len(prefixes)
        _, del_sorted, del_valid = self.c.sort_keys(self._dev(prefixes), None, n=k, want_sorted=True)
        return self._delete(del_sorted[:29 * k], del_valid, probe_len, False)

    def compact(self):
        return self._delete(None, None, 29, True)

    # ---- reads ------------------------------------------------------------
    def probes(self, rows):
        """Probe rows on the device. A caller uploads them once, before the calls they serve: an upload
        from pageable memory waits for the stream, and the reads are to follow one another, and a delete
        before them, with nothing in between."""
        return self._dev(rows)

    def seek(self, d_probes):
        return self.c.seek_keys(self.col, self.valid, d_probes, 17, order=self.order, info=self.info,
                                m=d_probes.numel() // 29)

    def objects(self):
        return self.c.key_objects(self.keys, self.order, self.valid)

    def retrieve(self, d_probes, seeks=None) -> Read:
        """seek (17) -> list (reverse, limit 1, info) -> filter (tombstones) -> fetch -> decode."""
        c, cap = self.c, d_probes.numel() // 29
        seeks = self.seek(d_probes) if seeks is None else seeks
        rows, range_off, total, keys = c.list_keys(self.col, self.order, self.valid, seeks, cap, limit=1, reverse=True,
                                                   info=self.info, want_keys=True)
        rows, range_off, total, keys = c.filter_rows(rows, range_off, total, cap, tombstones=True, keys=keys)
        val_cap = max(self.rec_bytes, 16)  # distinct probes fetch distinct records
        values, val_off, val_total, status = c.fetch_objects(rows, total, cap, self.arena, self.rec_off, self.n,
                                                             self.rec_bytes, val_cap)
        d = self._decode(values, val_off, cap, val_cap)
        return Read(seeks, rows, range_off, total, keys, values, val_off, val_total, status, d, cap)

    def versions(self, d_probes, deleted: bool, seeks=None, objects=None) -> Listed:
        """Versions, most recent first: FILTER_DELETED over key_objects' outputs (fresh ones unless the
        caller made them for this column), or FILTER_TOMBSTONE alone."""
        c, cap = self.c, self.n
        seeks = self.seek(d_probes) if seeks is None else seeks
        rows, range_off, total, _ = c.list_keys(self.col, self.order, self.valid, seeks, cap, reverse=True, info=self.info)
        if deleted:
            obj_off, latest, objects = self.objects() if objects is None else objects
            out = c.filter_rows(rows, range_off, total, cap, deleted=(self.valid, self.n, obj_off, latest, objects, self.info))
        else:
            out = c.filter_rows(rows, range_off, total, cap, tombstones=True)
        return Listed(out[0], out[1], out[2], total, cap)

    def latest_of_all(self, want_keys=False, objects=None):
        """LIST_LATEST over (0, valid): a seek of the empty probe is that range."""
        c, cap = self.c, self.n
        obj_off, _, objects = self.objects() if objects is None else objects
        whole = c.seek_keys(self.col, self.valid, self._whole, 0, m=1)
        rows, range_off, total, keys = c.list_keys(self.col, self.order, self.valid, whole, cap, latest=(obj_off, objects),
                                                   info=self.info, want_keys=want_keys)
        return rows, total, keys

    # ---- two replicas -----------------------------------------------------
    def compare(self, peer_col, peer_valid) -> Compared:
        obj_off, _, objects = self.objects()
        rows, peer, counts = self.c.compare_keys(self.col, self.order, self.valid, obj_off, objects, peer_col, peer_valid,
                                                 want_peer=True)
        return Compared(rows, peer, counts, objects)

    def ship_to(self, peer: "Store", cap=None, digest=None) -> Shipped:
        """key_objects -> compare -> list -> fetch here; decode -> keys -> sort -> merge on the peer. All cap
        rows are appended there: the rows past the list's total are empty records."""
        c = self.c
        cap = self.n if cap is None else cap
        cmp = self.compare(*(digest if digest is not None else (peer.col, peer.valid)))
        rows, _, total, keys = c.list_keys(self.col, self.order, self.valid, cmp.rows, cap, want_keys=True)
        val_cap = max(self.rec_bytes, 16)
        values, val_off, val_total, status = c.fetch_objects(rows, total, cap, self.arena, self.rec_off, self.n,
                                                             self.rec_bytes, val_cap)
        peer.acl_room += self.acl_room  # what is shipped is some of what is stored here
        peer.regions_room += self.regions_room
        d = peer._decode(values, val_off, cap, val_cap)
        k, st = peer.c.keys(d)
        k, st = k[:29 * cap], st[:4 * cap].view(torch.int32)
        first = peer._merge(cap, k, st, d.info, values, None, val_off)
        return Shipped(cmp, rows, total, keys, values, val_off, val_total, status, cap, first)
