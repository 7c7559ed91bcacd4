"""Device side of the write-set and placement tests: inputs placed at a chosen
address phase, guarded outputs, the encode and decode calls through the C
ABI, and the checks every such test ends with (the allowed ranges equal the
oracle's bytes; everything else still holds the guard pattern)."""
import ctypes

import numpy as np
import torch

import guards
from bounds_batches import ok_ranges
from honu_amd import object as hobj
from honu_amd.metadata import ACL_INPLACE, INFO_DTYPE, META_DTYPE, REGIONS_INPLACE

L = hobj._lib
E_ARG, E_WORKSPACE = -1, -2
ERR_CAPACITY, ERR_INPUT = 9, 10
PATHS = ("plain", "units", "marshal")


def placed(a, dev, phase=0):
    """The bytes of `a` on the device, starting `phase` bytes past a 256-byte
    boundary (an input: its guard bands are only there to place it)."""
    a = np.ascontiguousarray(a)
    src = a.view(np.uint8).reshape(-1)
    t = guards.guarded(len(src), phase=phase, device=dev)
    if len(src):
        t.copy_(torch.from_numpy(src.copy()))
    return t


def ptr(t) -> int:
    """The device address of a guarded view (0 for None); an empty view's too,
    for which torch reports none."""
    return guards.address(t)


def out_buf(nbytes, dev, fill, phase=0):
    return guards.guarded(nbytes, phase=phase, fill=fill, device=dev)


def got(t, dtype=np.uint8):
    """A guarded view's bytes now, on the host."""
    return guards.block_of(t).bytes().view(dtype)


def set_param(c, name, value):
    """Set a context param; False when the library refuses the value."""
    return c.lib.honu_ctx_set_param(c.ctx, name.encode(), int(value)) == 0


def get_param(c, name):
    v = ctypes.c_int64(-1)
    L.check(c.lib.honu_ctx_get_param(c.ctx, name.encode(), ctypes.byref(v)), "get_param")
    return v.value


# --------------------------------------------------------------------------
# encode
# --------------------------------------------------------------------------
class EncIn:
    """A HostBatch on the device, each arena at its own phase; rows [k, n)
    are passed as d_meta + k and d_payload_off + k."""

    def __init__(self, hb, dev, payload=0, var=0, tables=0, k=0):
        self.n = len(hb.meta) - k
        self.t = dict(meta=placed(hb.meta, dev), var=placed(hb.var, dev, var),
                      acl=placed(hb.acl, dev, tables), reg=placed(hb.regions, dev, tables),
                      payload=placed(hb.payload, dev, payload), payload_off=placed(hb.payload_off, dev))
        p = {name: ptr(t) for name, t in self.t.items()}
        self.meta, self.payload_off = p["meta"] + 352 * k, p["payload_off"] + 8 * k
        self.var, self.acl, self.reg, self.payload = p["var"], p["acl"], p["reg"], p["payload"]
        self.var_len, self.acl_len, self.reg_len = len(hb.var), len(hb.acl), len(hb.regions)


def encode_sizes(c, x, out_off, status):
    """The size pass and the scan (in place): d_out_off and d_status."""
    L.check(c.lib.honu_encode_sizes(c.ctx, x.meta, x.var_len, x.acl, x.acl_len, x.reg, x.reg_len,
                                    x.payload_off, x.n, ptr(out_off), ptr(status), c.stream), "sizes")
    L.check(c.lib.honu_exclusive_scan(c.ctx, ptr(out_off), x.n, ptr(out_off), c.stream), "scan")


def encode_call(c, path, x, out, out_cap, out_off, status, streams=None):
    """One encode by `path`: the plain pair, the units pair (both need
    d_out_off and d_status filled) or honu_marshal_batch. streams: the records
    call and the payload call each on its own stream. Returns the calls'
    return codes."""
    s1, s2 = (c.stream, c.stream) if streams is None else (s.cuda_stream for s in streams)
    po, pf, ps = ptr(out), ptr(out_off), ptr(status)
    lib = c.lib
    if path == "marshal":
        return [lib.honu_marshal_batch(c.ctx, x.meta, x.var, x.var_len, x.acl, x.acl_len, x.reg, x.reg_len,
                                       x.payload, x.payload_off, x.n, po, out_cap, pf, ps, s1)]
    if path == "plain":
        return [lib.honu_encode_records(c.ctx, x.meta, x.var, x.acl, x.reg, x.payload_off, x.n, po, out_cap,
                                        pf, ps, s1),
                lib.honu_encode_payloads(c.ctx, x.payload, x.payload_off, x.n, po, out_cap, pf, ps, s2)]
    assert path == "units"
    return [lib.honu_encode_records_units(c.ctx, x.meta, x.var, x.acl, x.reg, x.payload, x.payload_off, x.n,
                                          po, out_cap, pf, ps, s1),
            lib.honu_encode_payloads_units(c.ctx, x.payload, x.payload_off, x.n, po, out_cap, pf, ps, s2)]


def check_encode(out, out_off, status, oout, ooff, ost):
    """After an encode: offsets and statuses are the oracle's, every completed
    record holds the oracle's bytes, and nothing else was stored anywhere."""
    n = len(ost)
    assert np.array_equal(got(out_off, np.uint64), ooff)
    assert np.array_equal(got(status, np.int32), ost)
    allowed = ok_ranges(ooff, ost)
    g = got(out)
    bad = [(a, b) for a, b in allowed if g[a:b].tobytes() != oout[a:b].tobytes()]
    if bad:
        a, b = bad[0]
        d = np.flatnonzero(g[a:b] != oout[a:b])
        raise AssertionError(f"{len(bad)} record(s) differ from the oracle; the first, [{a}, {b}), at its "
                             f"bytes {int(d[0])}..{int(d[-1])} ({len(d)} bytes)")
    guards.assert_untouched(out, allowed)
    guards.assert_untouched(out_off, [(0, 8 * (n + 1))])
    guards.assert_untouched(status, [(0, 4 * n)])


def run_encode(c, hb, path, oracle_out, fill, out_phase=0, k=0, **phases):
    """A whole encode of rows [k, n) of `hb` into guarded outputs, checked."""
    oout, ooff, ost = oracle_out
    dev = c.torch_device
    x = EncIn(hb, dev, k=k, **phases)
    out = out_buf(int(ooff[-1]), dev, fill, out_phase)
    out_off, status = out_buf(8 * (x.n + 1), dev, fill), out_buf(4 * x.n, dev, fill)
    if path != "marshal":
        encode_sizes(c, x, out_off, status)
    assert encode_call(c, path, x, out, int(ooff[-1]), out_off, status) == [0] * (1 if path == "marshal" else 2)
    torch.cuda.synchronize()
    check_encode(out, out_off, status, oout, ooff, ost)


# --------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------
class DecOut:
    """Guarded outputs of one honu_decode_batch: tables and data arena sized
    by what the batch needs (`tot`, the oracle's totals), each at its phase."""

    def __init__(self, n, tot, dev, fill, materialize, meta=0, info=0, tables=0, data=0):
        self.n, self.need = n, [int(v) for v in tot]
        self.meta, self.info = out_buf(352 * n, dev, fill, meta), out_buf(32 * n, dev, fill, info)
        self.tot = out_buf(24, dev, fill)
        self.acl, self.reg = out_buf(20 * self.need[0], dev, fill, tables), out_buf(4 * self.need[1], dev, fill, tables)
        self.data = out_buf(self.need[2], dev, fill, data) if materialize else None


def decode_call(c, d_rec, d_off, o, acl_cap=None, regions_cap=None, data_cap=None):
    """honu_decode_batch into `o`; d_rec / d_off: device addresses."""
    acl_cap = o.need[0] if acl_cap is None else acl_cap
    regions_cap = o.need[1] if regions_cap is None else regions_cap
    data_cap = (o.need[2] if data_cap is None else data_cap) if o.data is not None else 0
    return c.lib.honu_decode_batch(c.ctx, d_rec, d_off, o.n, ptr(o.meta), ptr(o.info), ptr(o.acl), acl_cap,
                                   ptr(o.reg), regions_cap, ptr(o.data), data_cap, ptr(o.tot), c.stream)


def table_ranges(ometa, oinfo):
    """The ACL and region table entries (byte ranges) of the records that fit."""
    acl, reg = [], []
    for i in np.flatnonzero(oinfo["meta_status"] == 0):
        m = ometa[i]
        pr = int(m["present"])
        if int(m["acl_count"]) and not pr & ACL_INPLACE:
            acl.append((20 * int(m["acl_off"]), 20 * (int(m["acl_off"]) + int(m["acl_count"]))))
        if int(m["regions_count"]) and not pr & REGIONS_INPLACE:
            reg.append((4 * int(m["regions_off"]), 4 * (int(m["regions_off"]) + int(m["regions_count"]))))
    return acl, reg


def data_ranges(oinfo):
    ok = (oinfo["data_status"] == 0) & (oinfo["data_len"] > 0)
    return [(int(o), int(o + ln)) for o, ln in zip(oinfo["data_off"][ok], oinfo["data_len"][ok])]


def _same(name, g, o, ranges):
    for a, b in ranges:
        assert g[a:b].tobytes() == o[a:b].tobytes(), f"{name} bytes [{a}, {b}) differ from the oracle's"


def check_decode(o, oracle_out):
    """After a decode: rows, infos and totals are the oracle's byte for byte,
    the table entries of the records that fit and the payloads it reports too,
    and nothing else was stored anywhere (no table entry of a record that did
    not fit, nothing at or past a capacity, no byte of the data arena's
    alignment gaps or behind its last payload, no row n, totals of 24 bytes)."""
    ometa, oinfo, oacl, oreg, odata, otot = oracle_out
    n = o.n
    assert np.array_equal(got(o.tot, np.uint64), otot)
    info, meta = got(o.info, INFO_DTYPE), got(o.meta, META_DTYPE)
    for f in INFO_DTYPE.names:
        assert np.array_equal(info[f], oinfo[f]), (f, np.flatnonzero(info[f] != oinfo[f])[:8])
    assert info.tobytes() == oinfo.tobytes()
    bad = [i for i in range(n) if meta[i].tobytes() != ometa[i].tobytes()]
    assert not bad, (bad[:5], meta[bad[0]], ometa[bad[0]])
    acl_r, reg_r = table_ranges(ometa, oinfo)
    _same("ACL table", got(o.acl), oacl.view(np.uint8), acl_r)
    _same("region table", got(o.reg), oreg.view(np.uint8), reg_r)
    guards.assert_untouched(o.meta, [(0, 352 * n)])
    guards.assert_untouched(o.info, [(0, 32 * n)])
    guards.assert_untouched(o.tot, [(0, 24)])
    guards.assert_untouched(o.acl, acl_r)
    guards.assert_untouched(o.reg, reg_r)
    if o.data is not None:
        dr = data_ranges(oinfo)
        _same("data arena", got(o.data), odata, dr)
        guards.assert_untouched(o.data, dr)


# --------------------------------------------------------------------------
# system objects
# --------------------------------------------------------------------------
class SysIn:
    """A SystemHostBatch on the device, each arena at its own phase."""

    def __init__(self, sb, dev, var=0, lists=4, index=8, rows=0):
        self.n = len(sb.rows)
        self.t = dict(rows=placed(sb.rows, dev, rows), var=placed(sb.var, dev, var), acl=placed(sb.acl, dev, lists),
                      reg=placed(sb.regions, dev, lists), idx=placed(sb.index, dev, index))
        self.rows, self.var, self.acl, self.reg, self.idx = (ptr(self.t[k]) for k in ("rows", "var", "acl", "reg", "idx"))
        self.var_len, self.acl_len, self.reg_len, self.idx_len = len(sb.var), len(sb.acl), len(sb.regions), len(sb.index)


def system_sizes(c, x, sizes, status):
    """honu_system_sizes; sizes / status: guarded views or device addresses."""
    a = lambda t: t if isinstance(t, int) else ptr(t)  # noqa: E731
    return c.lib.honu_system_sizes(c.ctx, x.rows, x.var_len, x.acl, x.acl_len, x.reg, x.reg_len, x.idx, x.idx_len,
                                   x.n, a(sizes), a(status), c.stream)


def system_encode(c, route, x, out, out_cap, out_off, status):
    """One MarshalSystem of the batch by `route`: "calls" (sizes, the scan in
    place, encode) or "marshal" (honu_system_marshal_batch). Returns the
    calls' return codes."""
    po, pf, ps = ptr(out), ptr(out_off), ptr(status)
    lib = c.lib
    if route == "marshal":
        return [lib.honu_system_marshal_batch(c.ctx, x.rows, x.var, x.var_len, x.acl, x.acl_len, x.reg, x.reg_len,
                                              x.idx, x.idx_len, x.n, po, out_cap, pf, ps, c.stream)]
    assert route == "calls"
    return [system_sizes(c, x, out_off, status), lib.honu_exclusive_scan(c.ctx, pf, x.n, pf, c.stream),
            lib.honu_system_encode(c.ctx, x.rows, x.var, x.acl, x.reg, x.idx, x.n, po, out_cap, pf, ps, c.stream)]


class SysOut:
    """Guarded outputs of one system decode: rows, statuses, totals and the
    three tables, allocated at exactly `tot` entries (the oracle's totals)."""

    def __init__(self, n, tot, dev, fill, rows=0, lists=4, index=8):
        self.n, self.need = n, [int(v) for v in tot]
        self.rows, self.status = out_buf(368 * n, dev, fill, rows), out_buf(4 * n, dev, fill)
        self.tot = out_buf(24, dev, fill)
        self.acl, self.reg = out_buf(20 * self.need[0], dev, fill, lists), out_buf(4 * self.need[1], dev, fill, lists)
        self.idx = out_buf(112 * self.need[2], dev, fill, index)

    def all(self):
        return (self.rows, self.status, self.tot, self.acl, self.reg, self.idx)


def system_decode(c, headless, d_rec, d_off, o, acl_cap=None, regions_cap=None, index_cap=None, totals=True):
    """honu_system_decode_batch / honu_collection_decode_batch into `o`; a
    capacity of 0 passes a NULL table."""
    caps = [need if cap is None else cap for need, cap in zip(o.need, (acl_cap, regions_cap, index_cap))]
    tabs = [ptr(t) if cap else 0 for t, cap in zip((o.acl, o.reg, o.idx), caps)]
    fn = c.lib.honu_collection_decode_batch if headless else c.lib.honu_system_decode_batch
    return fn(c.ctx, d_rec, d_off, o.n, ptr(o.rows), ptr(o.status), tabs[0], caps[0], tabs[1], caps[1], tabs[2],
              caps[2], ptr(o.tot) if totals else 0, c.stream)


def system_table_ranges(orows, ost):
    """The byte ranges of the three tables that the rows with status 0 own."""
    acl, reg, idx = [], [], []
    for i in np.flatnonzero(ost == 0):
        r = orows[i]
        for out, f, size in ((acl, "acl", 20), (reg, "regions", 4), (idx, "index", 112)):
            o, k = int(r[f + "_off"]), int(r[f + "_count"])
            if k:
                out.append((size * o, size * (o + k)))
    return acl, reg, idx


def check_system_decode(o, oracle_out, totals=True):
    """After a system decode: rows, statuses and totals are the oracle's byte
    for byte, the table entries of the rows with status 0 too, and nothing
    else was stored anywhere."""
    orows, ost, oacl, oreg, oidx, otot = oracle_out
    n = o.n
    if totals:
        assert np.array_equal(got(o.tot, np.uint64), otot)
    st = got(o.status, np.int32)
    assert np.array_equal(st, ost), [(int(i), int(st[i]), int(ost[i])) for i in np.flatnonzero(st != ost)[:8]]
    rows = got(o.rows).reshape(n, 368)
    want = np.ascontiguousarray(orows).view(np.uint8).reshape(n, 368)
    bad = np.flatnonzero((rows != want).any(axis=1))
    assert not len(bad), (bad[:5], np.flatnonzero(rows[bad[0]] != want[bad[0]]))
    ranges = system_table_ranges(orows, ost)
    for name, t, ot, r in zip(("ACL", "region", "index"), (o.acl, o.reg, o.idx), (oacl, oreg, oidx), ranges):
        assert all(b <= block_len(t) for _, b in r), name
        _same(name + " table", got(t), np.ascontiguousarray(ot).view(np.uint8).reshape(-1), r)
        guards.assert_untouched(t, r)
    guards.assert_untouched(o.rows, [(0, 368 * n)])
    guards.assert_untouched(o.status, [(0, 4 * n)])
    guards.assert_untouched(o.tot, [(0, 24)] if totals else [])


def block_len(t) -> int:
    return guards.block_of(t).nbytes
