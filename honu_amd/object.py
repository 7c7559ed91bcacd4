"""Host mirror of pkg/store/object over the gfx950 batch codec.

Reference API (pkg/store/object/object.go):
    Marshal(meta, data) (Object, error)            :24-45
    Object.StorageVersion() uint8                  :47-52
    Object.Key() (keys.Key, error)                 :57-64
    Object.Metadata() (*metadata.Metadata, error)  :66-83
    Object.Data() ([]byte, error)                  :85-99
    Object.Tombstone() bool                        :103-112
Errors are raised as the Python counterparts of the Go sentinels
(object/errors.go:6-7, lani/errors.go:6-10, io.EOF, io.ErrUnexpectedEOF);
inputs on which Go panics raise GoPanic.

Every codec operation runs on the GPU through the C ABI (Codec). The
per-record mirror functions are batches of one, kept for API parity; the batch
methods (Codec.marshal / Codec.decode) are the point of the library.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .metadata import (ACL_DTYPE, DELETE_SUPERSEDED, FETCH_LIVE, FILTER_DELETED, FILTER_TOMBSTONE, INFO_DTYPE,
                       LIST_LATEST, LIST_REVERSE, META_DTYPE, HostBatch, Metadata, pack_batch, unpack_row)

StorageVersion = 1  # object.go:14

# --------------------------------------------------------------------------
# status codes (include/honu_codec.h) and the Go sentinels they stand for
# --------------------------------------------------------------------------
OK, BAD_VERSION, MALFORMED, EOF, UNEXPECTED_EOF, NO_LENGTH, PARSE_BOOLEAN, PARSE_VARINT, \
    PANIC, CAPACITY, INPUT = range(11)


class HonuCodecError(Exception):
    status = -1


class ErrBadVersion(HonuCodecError):  # object/errors.go:6
    status = BAD_VERSION


class ErrMalformed(HonuCodecError):  # object/errors.go:7
    status = MALFORMED


class EOFError_(HonuCodecError):  # io.EOF
    status = EOF


class ErrUnexpectedEOF(HonuCodecError):  # io.ErrUnexpectedEOF
    status = UNEXPECTED_EOF


class ErrNoLength(HonuCodecError):  # lani/errors.go:8
    status = NO_LENGTH


class ErrParseBoolean(HonuCodecError):  # lani/errors.go:9
    status = PARSE_BOOLEAN


class ErrParseVarInt(HonuCodecError):  # lani/errors.go:10
    status = PARSE_VARINT


class GoPanic(HonuCodecError):  # the reference panics on this input
    status = PANIC


class ErrCapacity(HonuCodecError):
    status = CAPACITY


class ErrInput(HonuCodecError):
    status = INPUT


_ERRORS = {c.status: c for c in (ErrBadVersion, ErrMalformed, EOFError_, ErrUnexpectedEOF,
                                 ErrNoLength, ErrParseBoolean, ErrParseVarInt, GoPanic,
                                 ErrCapacity, ErrInput)}


def raise_status(st: int):
    if st != OK:
        raise _ERRORS.get(int(st), HonuCodecError)(f"status {int(st)}")


# --------------------------------------------------------------------------
# device plumbing (torch is used for device memory and streams only)
# --------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dev_bytes(a: np.ndarray, device):
    torch = _torch()
    a = np.ascontiguousarray(a)
    t = torch.empty(max(a.nbytes, 16), dtype=torch.uint8, device=device)
    if a.nbytes:
        src = a.view(np.uint8).reshape(-1)
        if not src.flags.writeable:
            src = src.copy()
        t[: a.nbytes].copy_(torch.from_numpy(src))
    return t


def _to_host(t, nbytes: int, dtype) -> np.ndarray:
    raw = t[:nbytes].cpu().numpy() if nbytes else np.zeros(0, np.uint8)
    return raw.view(dtype)


@dataclass
class DeviceBatch:
    """Encode input on the device, C layout (rows + arenas + CSR payload)."""
    meta: object
    var: object
    var_len: int
    acl: object
    acl_len: int
    regions: object
    regions_len: int
    payload: object
    payload_off: object
    n: int

    @classmethod
    def from_host(cls, hb: HostBatch, device="cuda"):
        return cls(_dev_bytes(hb.meta, device), _dev_bytes(hb.var, device), len(hb.var),
                   _dev_bytes(hb.acl, device), len(hb.acl), _dev_bytes(hb.regions, device),
                   len(hb.regions), _dev_bytes(hb.payload, device),
                   _dev_bytes(hb.payload_off, device), len(hb.meta))


@dataclass
class EncodeResult:
    out: object        # device uint8 records arena
    out_off: object    # device uint64[n+1]
    status: object     # device int32[n]
    n: int

    def host(self):
        total = int(self.out_off.view(_torch().int64)[self.n].item())
        off = _to_host(self.out_off, 8 * (self.n + 1), np.uint64)
        st = _to_host(self.status, 4 * self.n, np.int32)
        return _to_host(self.out, total, np.uint8), off, st


@dataclass
class DecodeResult:
    meta: object       # device honu_meta[n]
    info: object       # device honu_record_info[n]
    acl: object        # device honu_acl table
    regions: object    # device uint32 table
    data: object       # device data arena or None (zero copy)
    totals: object     # device u64[3]: ACL entries, regions, data bytes
    n: int

    def host(self):
        tot = _to_host(self.totals, 24, np.uint64)
        meta = _to_host(self.meta, 352 * self.n, META_DTYPE)
        info = _to_host(self.info, 32 * self.n, INFO_DTYPE)
        acl = _to_host(self.acl, 20 * int(tot[0]), ACL_DTYPE)
        reg = _to_host(self.regions, 4 * int(tot[1]), np.uint32)
        data = _to_host(self.data, int(tot[2]), np.uint8) if self.data is not None else None
        return meta, info, acl, reg, data, tot


class Codec:
    """A device context of the batch codec (one per GPU / stream family)."""

    def __init__(self, device: int = 0, max_records: int = 1 << 16):
        torch = _torch()
        self.lib = _lib.load()
        self.device = device
        self.torch_device = torch.device("cuda", device)
        err = _lib.I32(0)
        torch.cuda.set_device(device)
        self.ctx = self.lib.honu_ctx_create(device, max_records, _lib.C.byref(err))
        if not self.ctx:
            _lib.check(err.value or -4, "honu_ctx_create")
        self.max_records = max_records

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.honu_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return _torch().cuda.current_stream(self.torch_device).cuda_stream

    def _empty(self, nbytes: int):
        torch = _torch()
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.torch_device)

    # ---- encode ---------------------------------------------------------
    def encode_sizes(self, b: DeviceBatch, sizes, status):
        _lib.check(self.lib.honu_encode_sizes(
            self.ctx, _lib.ptr(b.meta), b.var_len, _lib.ptr(b.acl), b.acl_len,
            _lib.ptr(b.regions), b.regions_len, _lib.ptr(b.payload_off), b.n, _lib.ptr(sizes),
            _lib.ptr(status), self.stream), "honu_encode_sizes")

    def scan(self, inp, n, out):
        _lib.check(self.lib.honu_exclusive_scan(self.ctx, _lib.ptr(inp), n, _lib.ptr(out),
                                                self.stream), "honu_exclusive_scan")

    def encode(self, b: DeviceBatch, out, out_cap, out_off, status):
        _lib.check(self.lib.honu_encode(
            self.ctx, _lib.ptr(b.meta), _lib.ptr(b.var), b.var_len, _lib.ptr(b.acl), b.acl_len,
            _lib.ptr(b.regions), b.regions_len, _lib.ptr(b.payload), _lib.ptr(b.payload_off),
            b.n, _lib.ptr(out), out_cap, _lib.ptr(out_off), _lib.ptr(status), self.stream),
            "honu_encode")

    def marshal(self, b: DeviceBatch) -> EncodeResult:
        """object.Marshal over the batch; sizes the output arena (one sync)."""
        out_off = self._empty(8 * (b.n + 1))
        status = self._empty(4 * b.n)
        self.encode_sizes(b, out_off, status)
        self.scan(out_off, b.n, out_off)
        total = int(out_off.view(_torch().int64)[b.n].item())
        out = self._empty(total)
        self.marshal_into(b, out, total, out_off, status)
        return EncodeResult(out, out_off, status, b.n)

    def marshal_into(self, b: DeviceBatch, out, out_cap, out_off, status):
        """honu_marshal_batch into a caller-sized arena: the single-launch
        size/offset/header/tail kernel + the payload copy (record_variant 0),
        or the split phases."""
        _lib.check(self.lib.honu_marshal_batch(
            self.ctx, _lib.ptr(b.meta), _lib.ptr(b.var), b.var_len, _lib.ptr(b.acl), b.acl_len,
            _lib.ptr(b.regions), b.regions_len, _lib.ptr(b.payload), _lib.ptr(b.payload_off),
            b.n, _lib.ptr(out), out_cap, _lib.ptr(out_off), _lib.ptr(status), self.stream),
            "honu_marshal_batch")

    # ---- decode ---------------------------------------------------------
    def decode(self, rec, rec_off, n: int, materialize: bool = False,
               acl_cap: Optional[int] = None, regions_cap: Optional[int] = None,
               data_cap: Optional[int] = None, rec_bytes: Optional[int] = None) -> DecodeResult:
        """Object.Metadata() + Object.Data() over a CSR batch of records."""
        if rec_bytes is None:
            rec_bytes = int(rec_off.view(_torch().int64)[n].item())
        # every ACL entry / region takes >= 1 byte of its record
        acl_cap = rec_bytes if acl_cap is None else acl_cap
        regions_cap = rec_bytes if regions_cap is None else regions_cap
        meta = self._empty(352 * n)
        info = self._empty(32 * n)
        acl = self._empty(20 * acl_cap)
        reg = self._empty(4 * regions_cap)
        totals = self._empty(32)
        data = None
        if materialize:
            data_cap = rec_bytes + 16 * n if data_cap is None else data_cap
            data = self._empty(data_cap)
        _lib.check(self.lib.honu_decode_batch(
            self.ctx, _lib.ptr(rec), _lib.ptr(rec_off), n, _lib.ptr(meta), _lib.ptr(info),
            _lib.ptr(acl), acl_cap, _lib.ptr(reg), regions_cap, _lib.ptr(data),
            data_cap or 0, _lib.ptr(totals), self.stream), "honu_decode_batch")
        return DecodeResult(meta, info, acl, reg, data, totals, n)

    def keys(self, d: DecodeResult):
        keys = self._empty(29 * d.n)
        st = self._empty(4 * d.n)
        _lib.check(self.lib.honu_decode_keys(self.ctx, _lib.ptr(d.meta), _lib.ptr(d.info), d.n,
                                             _lib.ptr(keys), _lib.ptr(st), self.stream),
                   "honu_decode_keys")
        return keys, st

    # ---- key order ------------------------------------------------------
    def sort_workspace(self, n: int):
        """The workspace of sort_keys / key_objects for n keys (honu_sort_keys_workspace)."""
        nbytes = int(self.lib.honu_sort_keys_workspace(n))
        return self._empty(nbytes), nbytes

    def sort_keys(self, keys, key_status=None, n: Optional[int] = None, want_sorted: bool = False):
        """sort.Sort(keys.Keys) (keys/keys.go:126-130), stable, over the device
        key column of Codec.keys: (order, n record indices as an int32 view of
        the uint32 column; sorted column or None; valid count, one int64), all
        on the device. Keys whose status is not OK follow the valid ones, in
        index order."""
        if n is None:
            n = keys.numel() // 29
        order = self._empty(4 * n)
        out = self._empty(29 * n) if want_sorted else None
        valid = self._empty(8)
        work, work_bytes = self.sort_workspace(n)
        _lib.check(self.lib.honu_sort_keys(
            self.ctx, _lib.ptr(keys), _lib.ptr(key_status), n, _lib.ptr(order), _lib.ptr(out),
            _lib.ptr(valid), _lib.ptr(work), work_bytes, self.stream), "honu_sort_keys")
        return order[:4 * n].view(_torch().int32), out, valid[:8].view(_torch().int64)

    def key_objects(self, keys, order, valid):
        """The objects of a sorted column (keys.go:73-92) from sort_keys' order
        and valid count, which stay on the device: (offsets uint64[n+1] of
        which objects + 1 are set, latest record index per object uint32[n] of
        which `objects` are set, object count uint64[1])."""
        n = order.numel()
        obj_off = self._empty(8 * (n + 1))
        latest = self._empty(4 * n)
        objects = self._empty(8)
        work, work_bytes = self.sort_workspace(n)
        _lib.check(self.lib.honu_key_objects(
            self.ctx, _lib.ptr(keys), _lib.ptr(order), _lib.ptr(valid), n, _lib.ptr(obj_off),
            _lib.ptr(latest), _lib.ptr(objects), _lib.ptr(work), work_bytes, self.stream),
            "honu_key_objects")
        torch = _torch()
        return (obj_off[:8 * (n + 1)].view(torch.int64), latest[:4 * n].view(torch.int32),
                objects[:8].view(torch.int64))

    def seek_keys(self, sorted_keys, valid, probes, probe_len: int = 29, probe_status=None, order=None,
                  info=None, m: Optional[int] = None):
        """Cursor.Seek (iterator/cursor.go:44-55) of m probes (the first
        probe_len bytes of each 29-byte row of `probes`) over sort_keys'
        sorted column and valid count, which stay on the device: the
        honu_seek rows (metadata.SEEK_DTYPE: pos, end, first, latest, flags)
        as an int32 view of shape (m, 5), on the device. `order` (sort_keys')
        enables first / latest, `info` (the decode's record info) the LIVE
        flags; probes whose status is not OK are SKIPPED."""
        n = sorted_keys.numel() // 29
        if m is None:
            m = probes.numel() // 29
        out = self._empty(20 * m)
        _lib.check(self.lib.honu_key_seek(
            self.ctx, _lib.ptr(sorted_keys), _lib.ptr(valid), n, _lib.ptr(probes), _lib.ptr(probe_status),
            probe_len, m, _lib.ptr(order), _lib.ptr(info), _lib.ptr(out), self.stream), "honu_key_seek")
        return out[:20 * m].view(_torch().int32).view(m, 5)

    def merge_keys(self, sorted_a, order_a, valid_a, sorted_b, order_b, valid_b, b_base: Optional[int] = None):
        """A batch of Puts into the sorted column (store.go:232, 395, 530):
        the stable merge of two of sort_keys' outputs (sorted column, order,
        valid count, all on the device), A first on equal keys, with b_base
        (default: A's row count) added to B's record indices. Returns (sorted
        column, order as an int32 view or None when either input order is
        None, valid count as one int64), on the device: what sort_keys returns
        for the concatenated columns, so it feeds seek_keys, key_objects and
        a further merge_keys."""
        na, nb = sorted_a.numel() // 29, sorted_b.numel() // 29
        if b_base is None:
            b_base = na
        with_order = order_a is not None and order_b is not None
        out = self._empty(29 * (na + nb))
        order = self._empty(4 * (na + nb)) if with_order else None
        valid = self._empty(8)
        _lib.check(self.lib.honu_key_merge(
            self.ctx, _lib.ptr(sorted_a), _lib.ptr(order_a) if with_order else 0, _lib.ptr(valid_a), na,
            _lib.ptr(sorted_b), _lib.ptr(order_b) if with_order else 0, _lib.ptr(valid_b), nb, b_base,
            _lib.ptr(out), _lib.ptr(order), _lib.ptr(valid), self.stream), "honu_key_merge")
        torch = _torch()
        return (out[:29 * (na + nb)], order[:4 * (na + nb)].view(torch.int32) if with_order else None,
                valid[:8].view(torch.int64))

    def delete_workspace(self, n: int):
        """The workspace of delete_keys for a column of n rows (honu_key_delete_workspace)."""
        nbytes = int(self.lib.honu_key_delete_workspace(n))
        return self._empty(nbytes), nbytes

    def delete_keys(self, sorted_keys, order, valid, del_sorted, del_valid, probe_len: int = 29,
                    superseded: bool = False):
        """A batch of Deletes from the sorted column (the loop of Store.Drop,
        store.go:378-383, and its DeleteBucket, store.go:399-404): every valid
        row whose first probe_len bytes equal those of a valid row of
        del_sorted (sort_keys' sorted column and valid count over the keys to
        delete; None, None for no list) goes, and with `superseded` every row
        that the next valid row repeats (a Put replaced it). Returns (sorted
        column, order as an int32 view or None when `order` is None, valid
        count, removed count, both one int64), on the device: the rows that
        stay in [0, valid), the rows that went in [valid, valid + removed),
        then the invalid tail, so it feeds seek_keys, key_objects, merge_keys
        and a further delete_keys."""
        n = sorted_keys.numel() // 29
        m = 0 if del_sorted is None else del_sorted.numel() // 29
        out = self._empty(29 * n)
        order_out = self._empty(4 * n) if order is not None else None
        valid_out, removed = self._empty(8), self._empty(8)
        work, work_bytes = self.delete_workspace(n)
        _lib.check(self.lib.honu_key_delete(
            self.ctx, _lib.ptr(sorted_keys), _lib.ptr(order), _lib.ptr(valid), n, _lib.ptr(del_sorted) if m else 0,
            _lib.ptr(del_valid) if m else 0, m, probe_len, DELETE_SUPERSEDED if superseded else 0, _lib.ptr(out),
            _lib.ptr(order_out), _lib.ptr(valid_out), _lib.ptr(removed), _lib.ptr(work), work_bytes, self.stream),
            "honu_key_delete")
        torch = _torch()
        return (out[:29 * n], order_out[:4 * n].view(torch.int32) if order is not None else None,
                valid_out[:8].view(torch.int64), removed[:8].view(torch.int64))

    def list_keys(self, sorted_keys, order, valid, ranges, cap: int, limit: int = 0, reverse: bool = False,
                  latest=None, info=None, want_keys: bool = False):
        """A batch of cursor walks (Cursor.Next / Prev, iterator/cursor.go:57-89;
        List, Versions, Retrieve, collection.go:32-35, 97-110; the loop of
        store.go:379) over `ranges`, seek_keys' rows, which stay on the
        device: every row a cursor walking [pos, end) of each range would
        visit, packed, the ranges in order; `reverse` walks from end - 1 down,
        `limit` (not 0) stops each walk after that many rows, `latest`
        ((obj_off, objects) of key_objects) keeps one row per object, its last.
        Returns (rows: honu_list_row as an int32 view of shape (cap, 4), range,
        pos, record, flags (metadata.LIST_ROW_DTYPE), of which min(total, cap)
        are written; range_off: int64[m + 1], the rows before each range and
        the total; total: one int64; keys: 29 bytes per row when `want_keys`,
        else None), all on the device. A caller that reads total > cap calls
        again with more room. `order` (or None) gives the record indices,
        `info` (the decode's record info; needs `order`) the TOMBSTONE flag."""
        n = sorted_keys.numel() // 29
        m = ranges.numel() * ranges.element_size() // 20
        flags = (LIST_REVERSE if reverse else 0) | (LIST_LATEST if latest is not None else 0)
        obj_off, objects = latest if latest is not None else (None, None)
        rows = self._empty(16 * cap)
        range_off, total = self._empty(8 * (m + 1)), self._empty(8)
        keys = self._empty(29 * cap) if want_keys else None
        _lib.check(self.lib.honu_key_list(
            self.ctx, _lib.ptr(sorted_keys), _lib.ptr(order), _lib.ptr(valid), n, _lib.ptr(ranges), m, limit, flags,
            _lib.ptr(obj_off), _lib.ptr(objects), _lib.ptr(info), _lib.ptr(range_off), _lib.ptr(rows), _lib.ptr(keys),
            cap, _lib.ptr(total), self.stream), "honu_key_list")
        torch = _torch()
        return (rows[:16 * cap].view(torch.int32).view(cap, 4), range_off[:8 * (m + 1)].view(torch.int64),
                total[:8].view(torch.int64), keys[:29 * cap] if want_keys else None)

    def fetch_objects(self, rows, total, cap: int, rec, rec_off, nrec: int, rec_bytes: int, val_cap: int,
                      live: bool = False):
        """Cursor.Object() (iterator/cursor.go:31-38: make + copy of the value
        under the cursor) for the rows of list_keys, which stay on the device
        with their total: the records they name, out of the CSR arena (rec,
        rec_off uint64[nrec + 1], rec_bytes readable bytes), packed into a CSR
        arena of val_cap bytes. Returns (values: uint8[val_cap]; val_off:
        int64[cap + 1], where each row's value starts and the bytes they all
        need; val_total: one int64, the same need; status: int32[cap], of
        which min(total, cap) are written, INPUT for a row whose record index
        or offsets are out of range), all on the device: the (rec, rec_off,
        n = cap) of Codec.decode. The rows with val_off[g + 1] <= val_cap are
        copied, a prefix; a caller that reads val_total > val_cap calls again
        with more room (val_cap 0 only sizes). With `live`, a row flagged
        LIST_ROW_TOMBSTONE fetches nothing and stays in place, an empty
        value."""
        values = self._empty(val_cap) if val_cap else None
        val_off, val_total, status = self._empty(8 * (cap + 1)), self._empty(8), self._empty(4 * cap)
        _lib.check(self.lib.honu_key_fetch(
            self.ctx, _lib.ptr(rows), _lib.ptr(total), cap, _lib.ptr(rec), _lib.ptr(rec_off), nrec, rec_bytes,
            FETCH_LIVE if live else 0, _lib.ptr(val_off), _lib.ptr(status), _lib.ptr(values), val_cap,
            _lib.ptr(val_total), self.stream), "honu_key_fetch")
        torch = _torch()
        return (values[:val_cap] if val_cap else None, val_off[:8 * (cap + 1)].view(torch.int64),
                val_total[:8].view(torch.int64), status[:4 * cap].view(torch.int32))

    def filter_workspace(self, cap: int):
        """The workspace of filter_rows for a list of cap rows (honu_key_filter_workspace)."""
        nbytes = int(self.lib.honu_key_filter_workspace(cap))
        return self._empty(nbytes), nbytes

    def filter_rows(self, rows, range_off, total, cap: int, tombstones: bool = False, deleted=None, keys=None):
        """The live-object filter over the rows of list_keys, which stay on
        the device with their offsets and total: an object deleted with a
        tombstone version "will not be returned in list queries or retrieval"
        (collection.go:132-134; Retrieve: "not found", collection.go:97-101).
        With `tombstones` a row flagged LIST_ROW_TOMBSTONE goes (the list was
        made with `info`); with `deleted` ((valid, n, obj_off, latest, objects,
        info): the column's valid count and rows, key_objects' outputs and the
        decode's record info) every row of an object whose latest version is a
        tombstone goes, wherever that version lies; with neither the list is
        copied. Returns (rows, range_off, total, keys) in the forms list_keys
        returns them, on the device: the rows that stay, in order, of which
        `total` are written, the rows kept before each range and their total,
        HEAD on the first kept row of each range, and the kept rows' keys when
        `keys` (list_keys' keys) is given, else None. The result passes
        straight to fetch_objects; a range that comes out empty is Retrieve's
        "not found"."""
        m = range_off.numel() * range_off.element_size() // 8 - 1
        flags = (FILTER_TOMBSTONE if tombstones else 0) | (FILTER_DELETED if deleted is not None else 0)
        valid, n, obj_off, latest, objects, info = deleted if deleted is not None else (None, 0, None, None, None, None)
        rows_out = self._empty(16 * cap)
        range_off_out, total_out = self._empty(8 * (m + 1)), self._empty(8)
        keys_out = self._empty(29 * cap) if keys is not None else None
        work, work_bytes = self.filter_workspace(cap)
        _lib.check(self.lib.honu_key_filter(
            self.ctx, _lib.ptr(rows), _lib.ptr(keys), _lib.ptr(range_off), m, _lib.ptr(total), cap, flags,
            _lib.ptr(valid), n, _lib.ptr(obj_off), _lib.ptr(latest), _lib.ptr(objects), _lib.ptr(info),
            _lib.ptr(rows_out), _lib.ptr(keys_out), _lib.ptr(range_off_out), _lib.ptr(total_out), _lib.ptr(work),
            work_bytes, self.stream), "honu_key_filter")
        torch = _torch()
        return (rows_out[:16 * cap].view(torch.int32).view(cap, 4), range_off_out[:8 * (m + 1)].view(torch.int64),
                total_out[:8].view(torch.int64), keys_out[:29 * cap] if keys is not None else None)

    def next_workspace(self, m: int):
        """The workspace of next_versions for m requests (honu_key_next_workspace)."""
        nbytes = int(self.lib.honu_key_next_workspace(m))
        return self._empty(nbytes), nbytes

    def next_versions(self, sorted_keys, valid, requests, op: int, pid: int, region: int = 0, now: int = 0,
                      order=None, info=None, req_status=None, meta=None, m: Optional[int] = None):
        """The version each of a batch of writes writes (pid.Next of the
        stored latest version, lamport/pid.go:10-15, as Tombstone() uses it,
        metadata/collection.go:56-63; Collection.Create, Update, Merge,
        Delete, collection.go:75-137, whose bodies are stubs upstream and
        whose doc comments `op` carries out: metadata.NEXT_CREATE ..
        NEXT_DELETE), for m requests (the first 17 bytes of each 29-byte row
        of `requests`) over sort_keys' sorted column and valid count, which
        stay on the device; keys.next is the host statement. `order`
        (sort_keys') gives parent_record, `info` (the decode's record info;
        needs `order`) lets a stored tombstone say "not found"; requests whose
        status is not OK are SKIPPED. `meta` (m honu_meta rows on the device)
        is stamped in place with the assigned version, parent, tombstone,
        `region`, the ObjectID and `now` as the timestamps. Returns (rows:
        honu_next as a uint8 view of shape (m, 32), metadata.NEXT_DTYPE;
        keys: 29 bytes per request; key_status: int32[m], OK on assigned
        rows), on the device: keys and key_status are sort_keys' input as they
        stand, and its output merge_keys'."""
        n = sorted_keys.numel() // 29
        if m is None:
            m = requests.numel() // 29
        out, keys, key_status = self._empty(32 * m), self._empty(29 * m), self._empty(4 * m)
        work, work_bytes = self.next_workspace(m)
        _lib.check(self.lib.honu_key_next(
            self.ctx, _lib.ptr(sorted_keys), _lib.ptr(valid), n, _lib.ptr(order), _lib.ptr(info), _lib.ptr(requests),
            _lib.ptr(req_status), m, op, pid, region, now, _lib.ptr(out), _lib.ptr(keys), _lib.ptr(key_status),
            _lib.ptr(meta), _lib.ptr(work), work_bytes, self.stream), "honu_key_next")
        return out[:32 * m].view(m, 32), keys[:29 * m], key_status[:4 * m].view(_torch().int32)

    def compare_workspace(self, na: int):
        """The workspace of compare_keys for a local column of na rows (honu_key_compare_workspace)."""
        nbytes = int(self.lib.honu_key_compare_workspace(na))
        return self._empty(nbytes), nbytes

    def compare_keys(self, sorted_a, order_a, valid_a, obj_off_a, objects_a, sorted_b, valid_b,
                     want_peer: bool = False, want_counts: bool = True):
        """The versions of two sorted columns compared object by object: what
        two replicas decide when they meet under "latest writer wins"
        (lamport/scalar.go:15-24; lamport.Compare, scalar.go:47-78, which is
        bytes.Compare of two keys of one object, keys/keys.go:35-36). A is the
        local column (sort_keys' / merge_keys' sorted column, order or None,
        valid count) with key_objects' (obj_off, objects) over it, B the
        peer's sorted column and valid count, whole or a digest of one key per
        object; all stay on the device. keys.compare is the host statement.
        Returns (rows: honu_seek as an int32 view of shape (na, 5), of which
        `objects` are written: [pos, end) the versions of the object the peer
        is behind by, first / latest their record indices, flags SEEK_FOUND and
        metadata.CMP_*; peer: int32[na], the peer's latest row of each object
        or SEEK_NONE, with `want_peer`, else None; counts: int64[8],
        metadata.CMP_COUNTS_DTYPE, with `want_counts`, else None). The rows are
        list_keys' `ranges` as they stand: compare -> list -> fetch gathers
        what to send. The call writes `objects` rows and the host does not
        know that count, so the rows are cleared first: the rows from
        `objects` on are empty ranges to list_keys. The objects only the peer
        has are the only-mine rows of the call with the sides exchanged."""
        na, nb = sorted_a.numel() // 29, sorted_b.numel() // 29
        out = self._empty(20 * na).zero_()
        peer = self._empty(4 * na) if want_peer else None
        counts = self._empty(64) if want_counts else None
        work, work_bytes = self.compare_workspace(na)
        _lib.check(self.lib.honu_key_compare(
            self.ctx, _lib.ptr(sorted_a), _lib.ptr(order_a), _lib.ptr(valid_a), na, _lib.ptr(obj_off_a),
            _lib.ptr(objects_a), _lib.ptr(sorted_b), _lib.ptr(valid_b), nb, _lib.ptr(out), _lib.ptr(peer),
            _lib.ptr(counts), _lib.ptr(work), work_bytes, self.stream), "honu_key_compare")
        torch = _torch()
        return (out[:20 * na].view(torch.int32).view(na, 5), peer[:4 * na].view(torch.int32) if want_peer else None,
                counts[:64].view(torch.int64) if want_counts else None)

    def reclaim_workspace(self, nrec: int):
        """The workspace of reclaim_records for nrec records (honu_key_reclaim_workspace)."""
        nbytes = int(self.lib.honu_key_reclaim_workspace(nrec))
        return self._empty(nbytes), nbytes

    def reclaim_records(self, order, valid, n: int, rec, rec_off, nrec: int, rec_bytes: int, val_cap: int,
                        keys=None, key_status=None, info=None, want_remap: bool = False) -> "ReclaimResult":
        """The space a Drop frees (store.go:314-322, 399-404): the records
        arena (rec, rec_off uint64[nrec + 1], rec_bytes readable bytes) and
        the per-record arrays beside it (`keys` 29 bytes, `key_status` int32,
        `info` honu_record_info per record; each optional) compacted to the
        records that the first min(valid, n) entries of `order` name (the
        order and valid count of sort_keys, merge_keys or delete_keys),
        renumbered in ascending old index, and the order rewritten to the new
        indices. keys.reclaim is the host statement. Returns a ReclaimResult
        of device tensors; nothing is read on the host. The records with
        rec_off[j + 1] <= val_cap are copied, a prefix; a caller that reads
        val_total > val_cap calls again with more room (val_cap 0 only sizes).
        The new state has kept records and kept column rows: the caller reads
        `kept` once, for the b_base of its next merge_keys."""
        order_out = self._empty(4 * n)
        remap = self._empty(4 * nrec) if want_remap else None
        source, status = self._empty(4 * nrec), self._empty(4 * nrec)
        keys_out = self._empty(29 * nrec) if keys is not None else None
        key_status_out = self._empty(4 * nrec) if key_status is not None else None
        info_out = self._empty(32 * nrec) if info is not None else None
        off_out = self._empty(8 * (nrec + 1))
        values = self._empty(val_cap) if val_cap else None
        kept, val_total = self._empty(8), self._empty(8)
        work, work_bytes = self.reclaim_workspace(nrec)
        _lib.check(self.lib.honu_key_reclaim(
            self.ctx, _lib.ptr(order), _lib.ptr(valid), n, _lib.ptr(keys), _lib.ptr(key_status), _lib.ptr(info),
            _lib.ptr(rec), _lib.ptr(rec_off), nrec, rec_bytes, 0, _lib.ptr(order_out), _lib.ptr(remap),
            _lib.ptr(source), _lib.ptr(keys_out), _lib.ptr(key_status_out), _lib.ptr(info_out), _lib.ptr(off_out),
            _lib.ptr(status), _lib.ptr(values), val_cap, _lib.ptr(kept), _lib.ptr(val_total), _lib.ptr(work),
            work_bytes, self.stream), "honu_key_reclaim")
        torch = _torch()
        i32 = lambda t, k: t[:4 * k].view(torch.int32)  # noqa: E731
        return ReclaimResult(
            order=i32(order_out, n), remap=i32(remap, nrec) if want_remap else None, source=i32(source, nrec),
            values=values[:val_cap] if val_cap else None, rec_off=off_out[:8 * (nrec + 1)].view(torch.int64),
            kept=kept[:8].view(torch.int64), val_total=val_total[:8].view(torch.int64), status=i32(status, nrec),
            keys=keys_out[:29 * nrec] if keys is not None else None,
            key_status=i32(key_status_out, nrec) if key_status is not None else None,
            info=info_out[:32 * nrec] if info is not None else None)

    def route_workspace(self, m: int):
        """The workspace of route_keys for a batch of m positions (honu_key_route_workspace)."""
        nbytes = int(self.lib.honu_key_route_workspace(m))
        return self._empty(nbytes), nbytes

    def route_keys(self, ids, m: int, table, k: int, id_stride: int = 16, status=None, seq=None, keys=None,
                   want_bucket: bool = True, want_rows: bool = True, want_local: bool = True) -> "RouteResult":
        """A batch taken apart by collection: one bbolt bucket per collection
        ID (store.go:236-240; tx.go:112-120, 141-158; collection.go:86).
        Record i's collection ID is the 16 bytes at `ids` + id_stride * i (a
        uint8 tensor, or a device address: codec's decoded rows with
        `dec.meta.data_ptr() + 112` and stride 352); `table` is the store's k
        collection IDs, 16-byte rows, ascending and distinct; `status` (int32
        per record) leaves out the records that are not OK; `seq` (sort_keys'
        order of the batch's keys) is the sequence the partition keeps, so
        that every bucket's rows come out in key order; `keys` (29 bytes per
        record) are gathered by output row. keys.route is the host statement.
        Returns a RouteResult of device tensors; nothing is read on the host.
        The caller reads bucket_off once, for the nb and the segments of its
        merge_keys calls; bucket_off[k:] is fetch_objects' `total` as it
        stands."""
        bucket = self._empty(4 * m) if want_bucket else None
        rows = self._empty(16 * m) if want_rows else None
        local = self._empty(4 * m) if want_local else None
        keys_out = self._empty(29 * m) if keys is not None else None
        off, count = self._empty(8 * (k + 3)), self._empty(8 * (k + 2))
        work, work_bytes = self.route_workspace(m)
        _lib.check(self.lib.honu_key_route(
            self.ctx, _lib.ptr(ids), id_stride, _lib.ptr(status), m, _lib.ptr(seq), _lib.ptr(table), k, _lib.ptr(keys),
            _lib.ptr(bucket), _lib.ptr(rows), _lib.ptr(local), _lib.ptr(keys_out), _lib.ptr(off), _lib.ptr(count),
            _lib.ptr(work), work_bytes, self.stream), "honu_key_route")
        torch = _torch()
        i32 = lambda t: t[:4 * m].view(torch.int32)  # noqa: E731
        return RouteResult(
            bucket=i32(bucket) if want_bucket else None,
            rows=rows[:16 * m].view(torch.int32).view(m, 4) if want_rows else None,
            local=i32(local) if want_local else None, keys=keys_out[:29 * m] if keys is not None else None,
            bucket_off=off[:8 * (k + 3)].view(torch.int64), bucket_count=count[:8 * (k + 2)].view(torch.int64))


    def merge_bucket_keys(self, k: int, sorted_a, order_a, off_a, sorted_b, order_b, off_b, count_a=None,
                          nb: Optional[int] = None, base=None, b_base: int = 0,
                          want_count: bool = True) -> "BucketsResult":
        """A routed batch of Puts into every collection's bucket at once
        (store.go:232-240, 395, 530; tx.go:112-120). A and B are bucketed
        columns on the device: k buckets' sorted 29-byte rows end to end
        (`sorted_a`, `sorted_b`), one int32 record index per row (`order_a`,
        `order_b`, or None), and k + 1 int64 offsets (`off_a`, `off_b`);
        `count_a` (int64[k], optional) gives a bucket's valid rows.
        route_keys' outputs are B as they stand: keys, local (or None),
        bucket_off, with `nb` = the route's m (default: sorted_b's rows). B's
        row g of bucket c gets (order_b[g], or g) + (base[c], int32[k] on the
        device, or the scalar b_base). keys.merge_buckets is the host
        statement. Returns a BucketsResult of device tensors sized by na + nb;
        nothing is read on the host: the rows behind off[k] are not written.
        The order is None unless order_a is given (or A has no rows)."""
        na = sorted_a.numel() // 29 if sorted_a is not None else 0
        if nb is None:
            nb = sorted_b.numel() // 29 if sorted_b is not None else 0
        with_order = order_a is not None or na == 0
        out = self._empty(29 * (na + nb))
        order = self._empty(4 * (na + nb)) if with_order else None
        off = self._empty(8 * (k + 1))
        count = self._empty(8 * k) if want_count else None
        _lib.check(self.lib.honu_key_merge_buckets(
            self.ctx, k, _lib.ptr(sorted_a), _lib.ptr(order_a), _lib.ptr(off_a), _lib.ptr(count_a), na,
            _lib.ptr(sorted_b), _lib.ptr(order_b), _lib.ptr(off_b), nb, _lib.ptr(base), b_base, _lib.ptr(out),
            _lib.ptr(order), _lib.ptr(off), _lib.ptr(count), self.stream), "honu_key_merge_buckets")
        torch = _torch()
        return BucketsResult(
            sorted=out[:29 * (na + nb)], order=order[:4 * (na + nb)].view(torch.int32) if with_order else None,
            off=off[:8 * (k + 1)].view(torch.int64), count=count[:8 * k].view(torch.int64) if want_count else None)


@dataclass
class BucketsResult:
    """What Codec.merge_bucket_keys returns, all on the device: a bucketed
    column, bucket c the rows [off[c], off[c + 1])."""
    sorted: object  # uint8[29 (na + nb)]: the first off[k] rows are written
    order: object   # int32[na + nb] or None
    off: object     # int64[k + 1]
    count: object   # int64[k] or None: the rows of each bucket


@dataclass
class RouteResult:
    """What Codec.route_keys returns, all on the device. Class c < k is row c
    of the table, k the records of no known collection, k + 1 the positions
    that do not take part."""
    bucket: object        # int32[m] or None: per record its table row, SEEK_NONE (-1) for none
    rows: object          # int32[m, 4] or None: honu_list_row (range = class, pos, record, flags), by output row
    local: object         # int32[m] or None: the output row's index inside its class
    keys: object          # uint8[29 m] or None: the keys by output row
    bucket_off: object    # int64[k + 3]: the first output row of each class, then m
    bucket_count: object  # int64[k + 2]


@dataclass
class ReclaimResult:
    """What Codec.reclaim_records returns, all on the device. The first `kept`
    entries of source, status and the gathered arrays are written; order holds
    n entries, remap nrec, rec_off nrec + 1 (flat at val_total from kept on)."""
    order: object       # int32[n]: the new record index of each valid row, SEEK_NONE (-1) elsewhere
    remap: object       # int32[nrec] or None: old index -> new index or SEEK_NONE
    source: object      # int32[nrec]: new index -> old index
    values: object      # uint8[val_cap] or None: the new arena
    rec_off: object     # int64[nrec + 1]: the new offsets
    kept: object        # int64[1]
    val_total: object   # int64[1]: the bytes the kept records need
    status: object      # int32[nrec]: OK, or INPUT for a record whose offsets are out of order or of the arena
    keys: object        # uint8[29 nrec] or None
    key_status: object  # int32[nrec] or None
    info: object        # uint8[32 nrec] or None: honu_record_info rows, verbatim


_default: Optional[Codec] = None


def default_codec() -> Codec:
    global _default
    if _default is None:
        _default = Codec(0, 1 << 16)
    return _default


# --------------------------------------------------------------------------
# batch helpers on host values
# --------------------------------------------------------------------------
def marshal_batch(metas: Sequence[Optional[Metadata]], datas: Sequence[Optional[bytes]],
                  codec: Optional[Codec] = None):
    """[object.Marshal(m, d) ...] -> (list of Object | exception)."""
    codec = codec or default_codec()
    hb = pack_batch(metas, datas)
    res = codec.marshal(DeviceBatch.from_host(hb, codec.torch_device))
    out, off, st = res.host()
    objs: List[object] = []
    for i in range(len(metas)):
        if st[i] != OK:
            objs.append(_ERRORS.get(int(st[i]), HonuCodecError)(f"status {int(st[i])}"))
        else:
            objs.append(Object(bytes(out[int(off[i]):int(off[i + 1])])))
    return objs


def decode_batch(objs: Sequence[bytes], codec: Optional[Codec] = None):
    """[(meta|exc, data|exc, tombstone)] for each object, decoded on the GPU."""
    codec = codec or default_codec()
    n = len(objs)
    off = np.zeros(n + 1, np.uint64)
    buf = bytearray()
    for i, o in enumerate(objs):
        off[i] = len(buf)
        buf.extend(o)
    off[n] = len(buf)
    arena = np.frombuffer(bytes(buf) or b"\0", np.uint8)
    rec = _dev_bytes(arena, codec.torch_device)
    rec_off = _dev_bytes(off, codec.torch_device)
    d = codec.decode(rec, rec_off, n, rec_bytes=len(buf))
    meta, info, acl, reg, _, _ = d.host()
    out = []
    for i in range(n):
        ms, ds = int(info[i]["meta_status"]), int(info[i]["data_status"])
        m = unpack_row(meta[i], arena, acl, reg) if ms == OK else _ERRORS.get(ms, HonuCodecError)()
        if ds == OK:
            ln = int(info[i]["data_len"])
            o = int(info[i]["data_off"])
            data = bytes(arena[o:o + ln]) if ln else None
        else:
            data = _ERRORS.get(ds, HonuCodecError)()
        out.append((m, data, bool(info[i]["tombstone"])))
    return out


# --------------------------------------------------------------------------
# per-record mirror of the reference API
# --------------------------------------------------------------------------
def Marshal(meta: Optional[Metadata], data: Optional[bytes]) -> "Object":
    (r,) = marshal_batch([meta], [data])
    if isinstance(r, Exception):
        raise r
    return r


class Object(bytes):
    """object.Object: the encoded record bytes."""

    def StorageVersion(self) -> int:  # object.go:47-52
        return self[0] if len(self) else 0

    def _decoded(self):
        return decode_batch([bytes(self)])[0]

    def Metadata(self) -> Metadata:  # object.go:66-83
        m, _, _ = self._decoded()
        if isinstance(m, Exception):
            raise m
        return m

    def Data(self) -> Optional[bytes]:  # object.go:85-99
        _, d, _ = self._decoded()
        if isinstance(d, Exception):
            raise d
        return d

    def Tombstone(self) -> bool:  # object.go:103-112
        return self._decoded()[2]

    def Key(self) -> bytes:  # object.go:57-64 -> keys.New (keys/keys.go:42-51)
        codec = default_codec()
        arena = np.frombuffer(bytes(self) or b"\0", np.uint8)
        rec = _dev_bytes(arena, codec.torch_device)
        rec_off = _dev_bytes(np.array([0, len(self)], np.uint64), codec.torch_device)
        d = codec.decode(rec, rec_off, 1, rec_bytes=len(self))
        keys, st = codec.keys(d)
        s = int(_to_host(st, 4, np.int32)[0])
        raise_status(s)
        return bytes(_to_host(keys, 29, np.uint8))
