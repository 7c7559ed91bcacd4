"""Write sets, capacities and input errors of the system-object calls
(honu_system_sizes / _encode / _marshal_batch, honu_system_decode_batch,
honu_collection_decode_batch), through the C ABI as test_gpu_bounds.py does
it for the record codec: every output is a guarded buffer under two
complementary fills, the allowed ranges equal the oracle's bytes (the oracle
itself is judged in test_system_bounds_host.py), everything else keeps its
pattern. Bit-exact throughout."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
import system_batches as sb  # noqa: E402
from bounds_batches import ok_ranges  # noqa: E402
from bounds_gpu import (E_ARG, E_WORKSPACE, ERR_CAPACITY, ERR_INPUT, SysIn, SysOut, check_encode,  # noqa: E402
                        check_system_decode, got, out_buf, placed, ptr, system_decode, system_encode, system_sizes)
from honu_amd import object as hobj  # noqa: E402
from honu_amd.system import COLLECTION_DTYPE, normalize_collection, pack_system_batch, unpack_collection  # noqa: E402

ROUTES = ("calls", "marshal")


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 8192)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_codec():
    """A context of max_records = 1024."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 1024)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def edge_batch():
    """The edge set cycled to 257 rows (two workgroups), packed."""
    return pack_system_batch(sb.encode_cap_batch())


_cache = {}


def oracle_encode(oracle_lib):
    if "enc" not in _cache:
        _cache["enc"] = oracle_lib.system_marshal_batch(edge_batch())
    return _cache["enc"]


def decode_case(oracle_lib, headless, n):
    """(rec, off, the oracle's decode) of batch_of(edge_records, n)."""
    key = ("dec", headless, n)
    if key not in _cache:
        rec, off = sb.arena(sb.batch_of(sb.edge_records(oracle_lib, headless), n, headless))
        _cache[key] = (rec, off, oracle_lib.system_decode_batch(rec, off, headless))
    return _cache[key]


def enc_outputs(n, total, dev, fill, out_phase=0):
    return out_buf(total, dev, fill, out_phase), out_buf(8 * (n + 1), dev, fill), out_buf(4 * n, dev, fill)


# --------------------------------------------------------------------------
# encode
# --------------------------------------------------------------------------
@pytest.mark.parametrize("out_phase", [0, 16])
@pytest.mark.parametrize("var_phase", [0, 1, 7, 15])
@pytest.mark.parametrize("route", ROUTES)
def test_encode_write_set(codec, oracle_lib, route, var_phase, out_phase):
    """Both routes store exactly the records' ranges, 8 (n + 1) bytes of
    offsets and 4 n of statuses, wherever the var arena (any byte phase: run()
    loads aligned blocks around it), the tables and the output arena lie."""
    hb = edge_batch()
    oout, ooff, ost = oracle_encode(oracle_lib)
    dev = codec.torch_device
    x = SysIn(hb, dev, var=var_phase)

    def body(fill):
        out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, fill, out_phase)
        rc = system_encode(codec, route, x, out, int(ooff[-1]), out_off, status)
        torch.cuda.synchronize()
        assert rc == [0] * len(rc)
        check_encode(out, out_off, status, oout, ooff, ost)
    guards.twice(body)


def test_encode_routes_agree_and_null_status(codec, oracle_lib):
    """The two routes leave identical arenas (guard bytes included), and
    honu_system_sizes with d_status = NULL gives the same sizes."""
    hb = edge_batch()
    oout, ooff, ost = oracle_encode(oracle_lib)
    dev = codec.torch_device
    x = SysIn(hb, dev)

    def body(fill):
        blocks = []
        for route in ROUTES:
            out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, fill)
            assert set(system_encode(codec, route, x, out, int(ooff[-1]), out_off, status)) == {0}
            blocks.append((out, out_off, status))
        sizes = out_buf(8 * x.n, dev, fill)
        assert system_sizes(codec, x, sizes, 0) == 0
        torch.cuda.synchronize()
        for a, b in zip(*blocks):
            assert guards.block_of(a).host().tobytes() == guards.block_of(b).host().tobytes()
        assert np.array_equal(got(sizes, np.uint64), np.diff(ooff))
        guards.assert_untouched(sizes, [(0, 8 * x.n)])
    guards.twice(body)


@pytest.mark.parametrize("route", ROUTES)
def test_encode_input_errors(codec, oracle_lib, route):
    """One defect per row (system_batches.input_error_batch): statuses and
    offsets are the oracle's, refused rows have size 0, their neighbours hold
    the oracle's bytes, nothing else is stored."""
    hb, want = sb.input_error_batch()
    oout, ooff, ost = oracle_lib.system_marshal_batch(hb)
    assert ost.tolist() == want and want.count(ERR_INPUT) == 20
    dev = codec.torch_device
    x = SysIn(hb, dev, var=7)

    def body(fill):
        out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, fill)
        rc = system_encode(codec, route, x, out, int(ooff[-1]), out_off, status)
        torch.cuda.synchronize()
        assert rc == [0] * len(rc)
        check_encode(out, out_off, status, oout, ooff, ost)
        size = np.diff(got(out_off, np.uint64).astype(np.int64))
        assert (size[ost != 0] == 0).all()
    guards.twice(body)


@pytest.mark.parametrize("chosen", ["every_third", "all_but_one"])
def test_encode_skipped_rows(codec, oracle_lib, chosen):
    """Rows whose status is not HONU_OK on entry are skipped: their ranges
    keep the pattern, the others hold the oracle's bytes."""
    hb = edge_batch()
    oout, ooff, ost = oracle_encode(oracle_lib)
    n = len(ost)
    skip = {"every_third": np.arange(n) % 3 == 1, "all_but_one": np.arange(n) != n // 2}[chosen]
    status = np.where(skip, ERR_INPUT, 0).astype(np.int32)
    dev = codec.torch_device
    x = SysIn(hb, dev)
    d_off = placed(ooff, dev)

    def body(fill):
        out, d_st = out_buf(int(ooff[-1]), dev, fill), out_buf(4 * n, dev, fill)
        d_st.copy_(torch.from_numpy(status.view(np.uint8).copy()))
        assert codec.lib.honu_system_encode(codec.ctx, x.rows, x.var, x.acl, x.reg, x.idx, n, ptr(out), int(ooff[-1]),
                                            ptr(d_off), ptr(d_st), codec.stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(got(d_st, np.int32), status)
        g = got(out)
        allowed = ok_ranges(ooff, status)
        for a, b in allowed:
            assert g[a:b].tobytes() == oout[a:b].tobytes(), (a, b)
        guards.assert_untouched(out, allowed)
        guards.assert_untouched(d_st, [(0, 4 * n)])
        assert np.array_equal(got(d_off, np.uint64), ooff)
    guards.twice(body)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("where", ["id", "name", "acl_list", "record_end", "zero"])
def test_encode_out_cap(codec, oracle_lib, where, route):
    """out_cap inside a mid-batch record's ID, name and ACL list, exactly at
    a record's end and at 0: statuses are the oracle's under the same out_cap,
    and no byte at or past the first failed record's start is written (the
    arena is allocated at full size, so the guard check sees it)."""
    hb = edge_batch()
    full = oracle_encode(oracle_lib)
    cap = sb.out_caps(hb, full[1], full[2], full[0])[where]
    oout, ooff, ost = oracle_lib.system_marshal_batch(hb, out_cap=cap)
    assert (ost == ERR_CAPACITY).any() and set(ost.tolist()) <= {0, ERR_CAPACITY}
    dev = codec.torch_device
    x = SysIn(hb, dev)

    def body(fill):
        out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, fill)
        rc = system_encode(codec, route, x, out, cap, out_off, status)
        torch.cuda.synchronize()
        assert rc == [0] * len(rc)
        assert all(b <= cap for _, b in ok_ranges(ooff, ost))
        check_encode(out, out_off, status, oout, ooff, ost)
    guards.twice(body)


def _refused(rc, want, outputs):
    torch.cuda.synchronize()
    assert rc == want, rc
    for t in outputs:
        guards.assert_untouched(t, [])


def test_encode_refusals(codec, small_codec, oracle_lib):
    """Each refused call returns HONU_E_ARG (HONU_E_WORKSPACE for n above
    max_records) before anything is launched: every output keeps its
    pattern."""
    hb = edge_batch()
    _, ooff, _ = oracle_encode(oracle_lib)
    dev = codec.torch_device
    x = SysIn(hb, dev)
    total, n = int(ooff[-1]), x.n
    big_hb = pack_system_batch(sb.cycled(sb.edge_collections()[:9], 1025))
    big, big_total = SysIn(big_hb, dev), int(oracle_lib.system_marshal_batch(big_hb)[1][-1])
    lib = codec.lib

    def body(fill):
        outs = enc_outputs(n, total, dev, fill)
        out, off, st = (ptr(t) for t in outs)

        def sizes(ctx=codec.ctx, rows=x.rows, acl=x.acl, reg=x.reg, idx=x.idx, d_sizes=off, d_status=st):
            return lib.honu_system_sizes(ctx, rows, x.var_len, acl, x.acl_len, reg, x.reg_len, idx, x.idx_len, n,
                                         d_sizes, d_status, codec.stream)

        def encode(ctx=codec.ctx, rows=x.rows, acl=x.acl, reg=x.reg, idx=x.idx, d_out=out, d_off=off, d_status=st):
            return lib.honu_system_encode(ctx, rows, x.var, acl, reg, idx, n, d_out, total, d_off, d_status,
                                          codec.stream)

        def marshal(ctx=codec.ctx, rows=x.rows, acl=x.acl, reg=x.reg, idx=x.idx, d_out=out, d_off=off, d_status=st):
            return lib.honu_system_marshal_batch(ctx, rows, x.var, x.var_len, acl, x.acl_len, reg, x.reg_len, idx,
                                                 x.idx_len, n, d_out, total, d_off, d_status, codec.stream)
        tables = [dict(acl=x.acl + 2), dict(reg=x.reg + 2), dict(idx=x.idx + 4)]
        for fn, bad in ((sizes, [dict(ctx=0), dict(rows=0), dict(d_sizes=0), dict(rows=x.rows + 8)] + tables),
                        (encode, [dict(ctx=0), dict(rows=0), dict(d_out=0), dict(d_off=0), dict(d_status=0),
                                  dict(rows=x.rows + 8), dict(d_out=out + 8)] + tables),
                        (marshal, [dict(ctx=0), dict(rows=0), dict(d_out=0), dict(d_off=0), dict(d_status=0),
                                   dict(rows=x.rows + 8), dict(d_out=out + 8)] + tables)):
            for kw in bad:
                _refused((fn.__name__, kw, fn(**kw)), (fn.__name__, kw, E_ARG), outs)
        c = small_codec
        outs = enc_outputs(1025, big_total, dev, fill)  # (of the batch's own size)
        out, off, st = (ptr(t) for t in outs)
        rc = c.lib.honu_system_marshal_batch(c.ctx, big.rows, big.var, big.var_len, big.acl, big.acl_len, big.reg,
                                             big.reg_len, big.idx, big.idx_len, 1025, out, big_total, off, st, c.stream)
        _refused(rc, E_WORKSPACE, outs)
    guards.twice(body)


def test_encode_no_rows(codec):
    """n = 0 succeeds through every entry point; the scan and the one-call
    form leave d_out_off[0] == 0 and nothing else."""
    dev = codec.torch_device
    x = SysIn(pack_system_batch([]), dev)
    assert x.n == 0

    def body(fill):
        for route in ROUTES:
            out, out_off, status = enc_outputs(0, 0, dev, fill)
            rc = system_encode(codec, route, x, out, 0, out_off, status)
            torch.cuda.synchronize()
            assert rc == [0] * len(rc)
            assert got(out_off, np.uint64).tolist() == [0]
            guards.assert_untouched(out_off, [(0, 8)])
            guards.assert_untouched(out, [])
            guards.assert_untouched(status, [])
    guards.twice(body)


# --------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------
ENTRY = pytest.mark.parametrize("headless", [False, True], ids=["system", "collection"])


@pytest.mark.parametrize("phase", [0, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 2049])
@ENTRY
def test_decode_write_set(codec, oracle_lib, headless, n, phase):
    """368 n bytes of rows, 4 n of statuses, 24 of totals and the table
    entries of the rows that decode, in tables of exactly the oracle's totals;
    n around a workgroup and around the 1024-row tile of the three-column
    scan, with a row of all three lists on either side of the tile's edge."""
    rec, off, ora = decode_case(oracle_lib, headless, n)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev, phase), placed(off, dev)
    if n >= 1025:
        assert all(int(ora[0][i][f]) for i in (1023, 1024) for f in ("acl_count", "regions_count", "index_count"))

    def body(fill):
        o = SysOut(n, ora[5], dev, fill, rows=phase)
        rc = system_decode(codec, headless, ptr(d_rec), ptr(d_off), o)
        torch.cuda.synchronize()
        assert rc == 0
        check_system_decode(o, ora)
    guards.twice(body)


@ENTRY
def test_decode_without_totals_and_without_rows(codec, oracle_lib, headless):
    """d_totals = NULL gives the same rows and tables; n = 0 writes zero
    totals and nothing else."""
    n = 257
    rec, off, ora = decode_case(oracle_lib, headless, n)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)

    def body(fill):
        o = SysOut(n, ora[5], dev, fill)
        rc = system_decode(codec, headless, ptr(d_rec), ptr(d_off), o, totals=False)
        torch.cuda.synchronize()
        assert rc == 0
        check_system_decode(o, ora, totals=False)
        e = SysOut(0, (4, 4, 4), dev, fill)
        rc = system_decode(codec, headless, ptr(d_rec), ptr(d_off), e)
        torch.cuda.synchronize()
        assert rc == 0 and got(e.tot, np.uint64).tolist() == [0, 0, 0]
        guards.assert_untouched(e.tot, [(0, 24)])
        for t in (e.rows, e.status, e.acl, e.reg, e.idx):
            guards.assert_untouched(t, [])
    guards.twice(body)


@ENTRY
def test_decode_capacities(codec, oracle_lib, headless):
    """Each table's capacity alone at need, need - 1, inside a mid-batch
    row's list, half and 0 (with a NULL table), and all three at 0: statuses,
    whole rows (those of the rows that do not fit included) and totals are
    the oracle's under the same capacities, the entries of the rows with
    status 0 too, nothing is stored for a row with status 9 and nothing at or
    past a capacity. The call returns HONU_OK: a capacity shows in the
    statuses and the totals (include/honu_codec.h)."""
    rec, off = sb.cap_batch(oracle_lib, headless)
    n = len(off) - 1
    full = oracle_lib.system_decode_batch(rec, off, headless)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    for caps in sb.decode_caps(full):
        ora = oracle_lib.system_decode_batch(rec, off, headless, **caps)
        assert np.array_equal(ora[5], full[5])
        assert (ora[1] == ERR_CAPACITY).any() == any(c < int(t) for c, t in zip(
            (caps.get(k, 1 << 62) for k in ("acl_cap", "regions_cap", "index_cap")), full[5]))

        def body(fill):
            o = SysOut(n, full[5], dev, fill)
            rc = system_decode(codec, headless, ptr(d_rec), ptr(d_off), o, **caps)
            torch.cuda.synchronize()
            assert rc == 0
            try:
                check_system_decode(o, ora)
            except AssertionError as e:
                raise AssertionError(f"under {caps}: {e}") from e
        guards.twice(body)


def test_scan_state_reuse(codec, oracle_lib):
    """The three-column scan of the decodes and the one-column scan of
    honu_system_marshal_batch and honu_exclusive_scan share the context's
    look-back state: a decode of 2049 rows, a marshal of 1025, a headless
    decode of 257 and a scan of 4097 ones on one stream with no
    synchronisation in between each give what they give alone."""
    dev = codec.torch_device
    rec1, off1, ora1 = decode_case(oracle_lib, False, 2049)
    rec3, off3, ora3 = decode_case(oracle_lib, True, 257)
    hb = pack_system_batch(sb.cycled(sb.edge_collections(), 1025))
    oout, ooff, ost = oracle_lib.system_marshal_batch(hb)
    ones = np.ones(4097, np.uint64)

    def body(fill):
        d1, f1, d3, f3 = placed(rec1, dev), placed(off1, dev), placed(rec3, dev), placed(off3, dev)
        x, d_ones = SysIn(hb, dev), placed(ones, dev)
        o1, o3 = SysOut(2049, ora1[5], dev, fill), SysOut(257, ora3[5], dev, fill)
        out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, fill)
        scan = out_buf(8 * 4098, dev, fill)
        torch.cuda.synchronize()
        rc = [system_decode(codec, False, ptr(d1), ptr(f1), o1)]
        rc += system_encode(codec, "marshal", x, out, int(ooff[-1]), out_off, status)
        rc += [system_decode(codec, True, ptr(d3), ptr(f3), o3),
               codec.lib.honu_exclusive_scan(codec.ctx, ptr(d_ones), 4097, ptr(scan), codec.stream)]
        torch.cuda.synchronize()
        assert rc == [0, 0, 0, 0]
        check_system_decode(o1, ora1)
        check_encode(out, out_off, status, oout, ooff, ost)
        check_system_decode(o3, ora3)
        assert np.array_equal(got(scan, np.uint64), np.arange(4098, dtype=np.uint64))
        guards.assert_untouched(scan, [(0, 8 * 4098)])
    guards.twice(body)


@ENTRY
def test_decode_limits(small_codec, oracle_lib, headless):
    """A context of max_records = 1024 decodes n = 1024 and refuses
    n = 1025 with HONU_E_WORKSPACE, every output untouched."""
    c = small_codec
    dev = c.torch_device
    rec, off, ora = decode_case(oracle_lib, headless, 1024)
    rec5, off5, ora5 = decode_case(oracle_lib, headless, 1025)
    d_rec, d_off, d_rec5, d_off5 = (placed(a, dev) for a in (rec, off, rec5, off5))

    def body(fill):
        o = SysOut(1024, ora[5], dev, fill)
        rc = system_decode(c, headless, ptr(d_rec), ptr(d_off), o)
        torch.cuda.synchronize()
        assert rc == 0
        check_system_decode(o, ora)
        o5 = SysOut(1025, ora5[5], dev, fill)
        _refused(system_decode(c, headless, ptr(d_rec5), ptr(d_off5), o5), E_WORKSPACE, o5.all())
    guards.twice(body)


@ENTRY
def test_decode_refusals(codec, oracle_lib, headless):
    """HONU_E_ARG before anything is launched: null pointers, a capacity
    with a NULL table, misaligned rows and tables, and a records arena that
    is not 16-byte aligned (only the refusal is tested: the decoder must
    never run on one, its aligned loads could leave mapped memory)."""
    n = 257
    rec, off, ora = decode_case(oracle_lib, headless, n)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    fn = codec.lib.honu_collection_decode_batch if headless else codec.lib.honu_system_decode_batch

    def body(fill):
        o = SysOut(n, ora[5], dev, fill)
        good = dict(d_rec=ptr(d_rec), d_off=ptr(d_off), rows=ptr(o.rows), status=ptr(o.status), acl=ptr(o.acl),
                    reg=ptr(o.reg), idx=ptr(o.idx))

        def call(**kw):
            a = {**good, **kw}
            return fn(codec.ctx if "ctx" not in kw else kw["ctx"], a["d_rec"], a["d_off"], n, a["rows"], a["status"],
                      a["acl"], o.need[0], a["reg"], o.need[1], a["idx"], o.need[2], ptr(o.tot), codec.stream)
        assert min(o.need) > 0
        bad = [dict(ctx=0), dict(d_rec=0), dict(d_off=0), dict(rows=0), dict(status=0), dict(acl=0), dict(reg=0),
               dict(idx=0), dict(rows=good["rows"] + 8), dict(acl=good["acl"] + 2), dict(reg=good["reg"] + 2),
               dict(idx=good["idx"] + 4), dict(d_rec=good["d_rec"] + 1), dict(d_rec=good["d_rec"] + 8)]
        for kw in bad:
            _refused((kw, call(**kw)), (kw, E_ARG), o.all())
    guards.twice(body)


def test_round_trip(codec, oracle_lib):
    """UnmarshalSystem on the GPU of MarshalSystem on the GPU gives every
    edge collection back."""
    cols = sb.edge_collections()
    hb = pack_system_batch(cols)
    oout, ooff, ost = oracle_lib.system_marshal_batch(hb)
    ora = oracle_lib.system_decode_batch(oout, ooff)
    dev = codec.torch_device
    x = SysIn(hb, dev)
    out, out_off, status = enc_outputs(x.n, int(ooff[-1]), dev, 0)
    assert system_encode(codec, "marshal", x, out, int(ooff[-1]), out_off, status) == [0]
    o = SysOut(x.n, ora[5], dev, 0)
    assert system_decode(codec, False, ptr(out), ptr(out_off), o) == 0
    torch.cuda.synchronize()
    assert not got(status, np.int32).any() and not got(o.status, np.int32).any()
    arena, rows = got(out), got(o.rows, COLLECTION_DTYPE)
    acl, reg, idx = got(o.acl, ora[2].dtype), got(o.reg, np.uint32), got(o.idx, ora[4].dtype)
    for i, c in enumerate(cols):
        assert unpack_collection(rows[i], arena, acl, reg, idx) == normalize_collection(c), i
