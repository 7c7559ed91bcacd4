"""Write sets of the codec's calls (include/honu_codec.h, Conventions: "What
a call stores, to the byte"). Every output of every call here is a guarded
buffer (tests/guards.py) and every test body runs under two complementary
fills: after the call the bytes inside the ranges the call owns equal the
oracle's, and every other byte of the buffer and of the guard bands in front
of and behind it still holds its pattern. So an output cannot be right by what
the allocator left in it, a writer that reaches into a neighbouring record
(whose own writer would normally overwrite the stray byte later) is seen in
the skipped neighbour's range, and a store past an arena's end or at or past
a capacity is seen in the guard band. Bit-exact throughout.

tests/test_guards.py shows, on the CPU, that these checks catch a one-byte
overshoot, a tail rounded up to 16 bytes, a store into a skipped range, a
store before the view and an unwritten interior byte.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from bounds_batches import ENCODE_BATCHES, decode_batch, encode_batch, ok_ranges  # noqa: E402
from bounds_gpu import (E_WORKSPACE, ERR_CAPACITY, ERR_INPUT, PATHS, DecOut, EncIn, L, check_decode,  # noqa: E402
                        check_encode, decode_call, encode_call, encode_sizes, get_param, got, out_buf, placed, ptr,
                        run_encode, set_param)
from honu_amd import object as hobj  # noqa: E402
from honu_amd.metadata import INFO_DTYPE  # noqa: E402


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 4096)
    c.defaults = {k: get_param(c, k) for k in ("copy_blocks", "encode_fork", "record_variant", "acl_inplace",
                                               "regions_inplace")}
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(codec):
    yield
    for k, v in codec.defaults.items():
        assert set_param(codec, k, v)


_oracle_cache = {}


def oracle_encode(oracle_lib, name):
    if name not in _oracle_cache:
        _oracle_cache[name] = oracle_lib.marshal_batch(encode_batch(name))
    return _oracle_cache[name]


def param_or_skip(c, name, value):
    if not set_param(c, name, value):
        pytest.skip(f"the library refuses {name} = {value}")


# --------------------------------------------------------------------------
# encode
# --------------------------------------------------------------------------
def _geometries(name):
    # steal / two_class: copy_blocks at its default (8192 waves: ranges of a
    # few hundred bytes, many empty, tails of 16 bytes or none) and at 1 (16
    # waves, four of them streaming in the two-class launch: long ranges and
    # tails): both ends of range() and cut() in copy.hip
    return ["default", 1] if name in ("steal", "two_class") else ["default"]


@pytest.mark.parametrize("fork", [0, 1], ids=["lists_after", "lists_fork"])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,copy_blocks", [(b, g) for b in ENCODE_BATCHES for g in _geometries(b)])
def test_encode_write_set(codec, oracle_lib, name, copy_blocks, path, fork):
    """The three writers of a record (lane encoder: header, tail, partial
    end chunks and units; ACL list kernel: whole 16-byte chunks, placed by the
    lane encoder or, forked, by itself; payload copy: the units between) fill
    exactly the records' ranges."""
    hb = encode_batch(name)
    ora = oracle_encode(oracle_lib, name)
    if name == "two_class":  # both copy classes: the launch's average is what picks them
        assert int(hb.payload_off[-1]) // len(hb.meta) >= 64 << 10
    if name == "steal":
        assert int(hb.payload_off[-1]) // len(hb.meta) >= 16 << 10
    param_or_skip(codec, "encode_fork", fork)
    if copy_blocks != "default":
        param_or_skip(codec, "copy_blocks", copy_blocks)
    guards.twice(lambda fill: run_encode(codec, hb, path, ora, fill))


@pytest.mark.parametrize("fork", [0, 1], ids=["lists_after", "lists_fork"])
@pytest.mark.parametrize("pair", ["plain", "units"])
@pytest.mark.parametrize("chosen", ["none", "every_third", "all_but_one"])
@pytest.mark.parametrize("name", ENCODE_BATCHES)
def test_encode_skipped_neighbours(codec, oracle_lib, name, chosen, pair, fork):
    """Records whose status is not HONU_OK on entry are skipped: with
    d_out_off from the oracle and the size pass's d_status, a chosen set of
    records is marked HONU_ERR_INPUT while their ranges stay non-empty. Every
    skipped range and both ends of the arena keep the pattern, the records
    left OK equal the oracle's: a writer that reaches into its neighbour has
    nobody to clean up after it here."""
    hb = encode_batch(name)
    oout, ooff, ost = oracle_encode(oracle_lib, name)
    n = len(ost)
    param_or_skip(codec, "encode_fork", fork)
    dev = codec.torch_device
    x = EncIn(hb, dev)
    sizes, st0 = out_buf(8 * (n + 1), dev, 0), out_buf(4 * n, dev, 0)
    encode_sizes(codec, x, sizes, st0)
    torch.cuda.synchronize()
    status = got(st0, np.int32).copy()
    assert np.array_equal(status, ost) and np.array_equal(got(sizes, np.uint64), ooff)
    skip = {"none": np.zeros(n, bool), "every_third": np.arange(n) % 3 == 1,
            "all_but_one": np.arange(n) != n // 2}[chosen]
    skip &= status == 0
    assert (status[~skip] == 0).any() and (np.diff(ooff.astype(np.int64))[skip] > 0).all()
    status[skip] = ERR_INPUT
    d_off = placed(ooff, dev)

    def body(fill):
        out, d_st = out_buf(int(ooff[-1]), dev, fill), out_buf(4 * n, dev, fill)
        d_st.copy_(torch.from_numpy(status.view(np.uint8).copy()))
        assert encode_call(codec, pair, x, out, int(ooff[-1]), d_off, d_st) == [0, 0]
        torch.cuda.synchronize()
        assert np.array_equal(got(d_st, np.int32), status)
        g = got(out)
        for a, b in ok_ranges(ooff, status):
            assert g[a:b].tobytes() == oout[a:b].tobytes(), (a, b)
        guards.assert_untouched(out, ok_ranges(ooff, status))
        guards.assert_untouched(d_st, [(0, 4 * n)])
    guards.twice(body)


def _cap_record(hb, oout, ooff, ost):
    """A record in the batch's middle with an all-present ACL list of two or
    more entries and a payload of 80 bytes or more, and where in the arena its
    header, payload, tail and list lie."""
    from fixtures import py_uvarint
    for j in range(64, len(ost)):
        m = hb.meta[j]
        a0, na = int(m["acl_off"]), int(m["acl_count"])
        dlen = int(hb.payload_off[j + 1] - hb.payload_off[j])
        if ost[j] or na < 2 or dlen < 80 or not hb.acl["present"][a0:a0 + na].all():
            continue
        beg, end = int(ooff[j]), int(ooff[j + 1])
        hdr = 1 + len(py_uvarint(dlen))
        first = bytes([1]) + hb.acl["client_id"][a0].tobytes() + bytes([int(hb.acl["permissions"][a0])])
        lst = beg + oout[beg:end].tobytes().index(first, hdr + dlen)
        return dict(header=beg + 1, payload=beg + hdr + dlen // 2, tail=beg + hdr + dlen + 3,
                    acl_list=lst + 18 + 7, record_end=end)
    raise AssertionError("no such record in the batch")


@pytest.mark.parametrize("fork", [0, 1], ids=["lists_after", "lists_fork"])
@pytest.mark.parametrize("pair", ["plain", "units"])
@pytest.mark.parametrize("where", ["header", "payload", "tail", "acl_list", "record_end"])
def test_encode_out_cap(codec, oracle_lib, where, pair, fork):
    """out_cap inside a record's header, payload, tail and ACL list, and
    exactly at a record's end; the records call and the payload call each on
    its own stream (the payload copy repeats the capacity check, it cannot see
    the lane encoder's verdict). Statuses equal the oracle's under the same
    out_cap, nothing is stored at or past the first failed record's start,
    the records before it are exact."""
    hb = encode_batch("units")
    full = oracle_encode(oracle_lib, "units")
    cap = _cap_record(hb, *full)[where]
    oout, ooff, ost = oracle_lib.marshal_batch(hb, out_cap=cap)
    n = len(ost)
    assert (ost == ERR_CAPACITY).any() and (ost[:64] == 0).sum() > 60
    param_or_skip(codec, "encode_fork", fork)
    dev = codec.torch_device
    x = EncIn(hb, dev)
    streams = (torch.cuda.Stream(), torch.cuda.Stream())

    def body(fill):
        out = out_buf(int(ooff[-1]), dev, fill)
        out_off, status = out_buf(8 * (n + 1), dev, fill), out_buf(4 * n, dev, fill)
        encode_sizes(codec, x, out_off, status)
        torch.cuda.synchronize()
        assert encode_call(codec, pair, x, out, cap, out_off, status, streams) == [0, 0]
        torch.cuda.synchronize()
        first = min(int(ooff[i]) for i in range(n) if ost[i] == ERR_CAPACITY)
        assert all(b <= first for _, b in ok_ranges(ooff, ost)) and first <= cap
        check_encode(out, out_off, status, oout, ooff, ost)
    guards.twice(body)


# --------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------
FORMS = {"lists_inplace": (1, 1), "lists_table": (0, 0)}


def _decode_setup(codec, rv, form):
    param_or_skip(codec, "record_variant", rv)
    acl_ip, reg_ip = FORMS[form]
    param_or_skip(codec, "acl_inplace", acl_ip)
    param_or_skip(codec, "regions_inplace", reg_ip)
    return bool(acl_ip), bool(reg_ip)


@pytest.mark.parametrize("materialize", [False, True], ids=["zero_copy", "materialize"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rv", [5, 6], ids=["split", "fused"])
def test_decode_write_set(codec, oracle_lib, rv, form, materialize):
    """honu_decode_batch: 352 n bytes of rows, 32 n of infos, 24 of totals,
    the table entries of the records' lists, and in the data arena exactly
    the payloads' bytes — not its 16-byte alignment gaps, nothing behind the
    last payload. Then honu_decode_keys on the rows: 29 n and 4 n bytes."""
    rec, off = decode_batch()
    n = len(off) - 1
    ip = _decode_setup(codec, rv, form)
    ora = oracle_lib.decode_batch(rec, off, materialize, *ip)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    keys = [oracle_lib.key(ora[0][i:i + 1], int(ora[1][i]["meta_status"])) for i in range(n)]

    def body(fill):
        o = DecOut(n, ora[5], dev, fill, materialize)
        assert decode_call(codec, ptr(d_rec), ptr(d_off), o) == 0
        k, kst = out_buf(29 * n, dev, fill), out_buf(4 * n, dev, fill)
        L.check(codec.lib.honu_decode_keys(codec.ctx, ptr(o.meta), ptr(o.info), n, ptr(k), ptr(kst),
                                           codec.stream), "keys")
        torch.cuda.synchronize()
        check_decode(o, ora)
        gk, gst = got(k).reshape(n, 29), got(kst, np.int32)
        for i, (st, key) in enumerate(keys):
            assert st == gst[i] and (st != 0 or key == gk[i].tobytes()), i
        guards.assert_untouched(kst, [(0, 4 * n)])
        # (a record without a key leaves its 29 bytes alone or not: unspecified)
        guards.assert_untouched(k, [(0, 29 * n)])
    guards.twice(body)
    if form == "lists_table":  # the batch exercises the tables
        assert int(ora[5][0]) > 1000 and int(ora[5][1]) > 100


def test_decode_headers_and_data_write_set(codec, oracle_lib):
    """honu_decode_headers (32 n bytes of infos) and honu_decode_data (infos,
    8 bytes of totals, the payloads' bytes of the data arena)."""
    rec, off = decode_batch()
    n = len(off) - 1
    _, oinfo, _, _, _, _ = oracle_lib.decode_batch(rec, off, False)
    _, minfo, _, _, mdata, mtot = oracle_lib.decode_batch(rec, off, True)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    fields = ("data_off", "data_len", "data_status", "storage_version", "tombstone")

    def body(fill):
        info = out_buf(32 * n, dev, fill)
        L.check(codec.lib.honu_decode_headers(codec.ctx, ptr(d_rec), ptr(d_off), n, ptr(info), codec.stream),
                "headers")
        info2, data, tot = out_buf(32 * n, dev, fill), out_buf(int(mtot[2]), dev, fill), out_buf(8, dev, fill)
        L.check(codec.lib.honu_decode_data(codec.ctx, ptr(d_rec), ptr(d_off), n, ptr(info2), ptr(data),
                                           int(mtot[2]), ptr(tot), codec.stream), "decode_data")
        torch.cuda.synchronize()
        for g, o in ((got(info, INFO_DTYPE), oinfo), (got(info2, INFO_DTYPE), minfo)):
            for f in fields:
                assert np.array_equal(g[f], o[f]), f
            assert (g["meta_status"] == 11).all()
        assert int(got(tot, np.uint64)[0]) == int(mtot[2])
        ranges = [(int(o), int(o + ln)) for o, ln in zip(minfo["data_off"], minfo["data_len"]) if ln]
        gd = got(data)
        for a, b in ranges:
            assert gd[a:b].tobytes() == mdata[a:b].tobytes(), (a, b)
        guards.assert_untouched(info, [(0, 32 * n)])
        guards.assert_untouched(info2, [(0, 32 * n)])
        guards.assert_untouched(tot, [(0, 8)])
        guards.assert_untouched(data, ranges)
    guards.twice(body)


def _caps(ora):
    """(acl_cap, regions_cap, data_cap) settings around what the batch needs."""
    need_a, need_r, _ = (int(v) for v in ora[5])
    info = ora[1]
    last = int(np.flatnonzero(info["data_len"] > 0)[-1])
    end = int(info["data_off"][last] + info["data_len"][last])
    out = [dict(acl_cap=c) for c in (need_a, need_a - 1, need_a // 2, 0)]
    out += [dict(regions_cap=c) for c in (need_r, need_r - 1, need_r // 2, 0)]
    out += [dict(data_cap=c) for c in (end, end - 1, int(info["data_off"][last]))]
    out += [dict(acl_cap=need_a // 2, regions_cap=need_r // 3, data_cap=end // 2)]
    return out


@pytest.mark.parametrize("rv", [5, 6], ids=["split", "fused"])
def test_decode_capacity_parity(codec, oracle_lib, rv):
    """acl_cap and regions_cap at exact need, need - 1, half and 0, data_cap
    at exact need, need - 1 and the last payload's offset, against the oracle
    under the same capacities: infos, the rows' list offsets and totals byte
    for byte, the table entries of the records that fit, the payloads that
    fit, and nothing stored at or past a capacity (for capacity 0 the table
    is still a guarded buffer, never NULL: a stray store is reported, it does
    not fault)."""
    rec, off = decode_batch()
    n = len(off) - 1
    ip = _decode_setup(codec, rv, "lists_table")
    full = oracle_lib.decode_batch(rec, off, True, *ip)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    for caps in _caps(full):
        ora = oracle_lib.decode_batch(rec, off, True, *ip, **caps)
        assert np.array_equal(ora[5], full[5])  # totals: what the batch needs

        def body(fill):
            o = DecOut(n, full[5], dev, fill, True)
            assert decode_call(codec, ptr(d_rec), ptr(d_off), o, **caps) == 0
            torch.cuda.synchronize()
            try:
                check_decode(o, ora)
            except AssertionError as e:
                raise AssertionError(f"under {caps}: {e}") from e
        guards.twice(body)


# --------------------------------------------------------------------------
# honu_exclusive_scan
# --------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 66 * 4096 + 1]


def _scan_values(kind, n):
    rng = np.random.default_rng(n + 1)
    if kind == "zeros":
        return np.zeros(n, np.uint64)
    if kind == "ones":
        return np.ones(n, np.uint64)
    if kind == "random":  # below 2^28: the largest size's total is 2^45
        return rng.integers(0, 1 << 28, n, dtype=np.uint64)
    if kind == "wrap":  # any uint64: the sum wraps modulo 2^64, as numpy's does
        return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    v = np.zeros(n, np.uint64)  # "big": prefixes cross 2^32 inside a tile and between tiles, and reach 2^42
    if n:
        v[rng.integers(0, n, min(4, n))] = 1 << 40
        v[:: max(1, n // 3)] += np.uint64(1 << 31)
    return v


@pytest.fixture(scope="module")
def scan_codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 66 * 4096 + 1)
    yield c
    c.close()


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("kind", ["zeros", "ones", "random", "big", "wrap"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan(scan_codec, n, kind, in_place):
    """honu_exclusive_scan against numpy.cumsum in uint64, written to a
    guarded buffer of 8 (n + 1) bytes: no row, one row, sizes around a wave,
    a workgroup and the 4096-row tile, several tiles, and more tiles than one
    look-back window of 64; prefixes that cross 2^32 inside a tile and between
    tiles and reach 2^42 ("big"), totals past the 43 value bits of a
    look-back word ("random" at the largest size: 2^45; the tile sums travel
    as three limbs) and sums that wrap modulo 2^64 ("wrap"). With whole sums
    in the 43-bit words, "random" at 66 * 4096 + 1 rows was wrong from row
    110592 or 159744 on (which tile first reads a truncated word depends on
    timing) and "wrap" from the second tile on at every size above 4096."""
    c = scan_codec
    dev = c.torch_device
    v = _scan_values(kind, n)
    want = np.zeros(n + 1, np.uint64)
    want[1:] = np.cumsum(v, dtype=np.uint64)
    if kind == "big" and n > 4:
        assert 1 << 40 <= int(want[-1]) < 1 << 43 and (np.diff(want >> np.uint64(32)) > 0).any()
    if kind == "random" and n == SCAN_SIZES[-1]:
        assert int(want[-1]) > 1 << 44
    d_in = placed(v, dev)

    def body(fill):
        out = out_buf(8 * (n + 1), dev, fill)
        src = out if in_place else d_in
        if in_place and n:
            out[:8 * n].copy_(d_in)
        L.check(c.lib.honu_exclusive_scan(c.ctx, ptr(src), n, ptr(out), c.stream), "scan")
        torch.cuda.synchronize()
        g = got(out, np.uint64)
        assert np.array_equal(g, want), np.flatnonzero(g != want)[:8]
        guards.assert_untouched(out, [(0, 8 * (n + 1))])
        if not in_place:
            assert np.array_equal(got(d_in, np.uint64), v)  # the input is only read
    guards.twice(body)


def test_exclusive_scan_refuses_more_than_max_records():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 4096)
    try:
        dev = c.torch_device
        n = 4097
        d_in = placed(np.ones(n, np.uint64), dev)

        def body(fill):
            out = out_buf(8 * (n + 1), dev, fill)
            assert c.lib.honu_exclusive_scan(c.ctx, ptr(d_in), n, ptr(out), c.stream) == E_WORKSPACE
            torch.cuda.synchronize()
            guards.assert_untouched(out, [])
        guards.twice(body)
    finally:
        c.close()
