"""Placement: where an arena lies must not matter. The kernels count 64-byte
payload units and 16-byte ACL chunks on absolute addresses and decode windows
on offsets from d_rec; with every arena on a 256-byte boundary (what an
allocator hands out) the two agree, so a phase that switched from one to the
other would produce the same bytes. Here every arena is displaced by the
steps its alignment rule allows (include/honu_codec.h: 16 bytes for the
records arena, the data arena and rows, 4 for the tables, none for the payload
and var arenas), sub-batches are passed as d_meta + k / d_rec_off + k, and
what the rule forbids is refused before anything is launched. The expected
output is the oracle's and does not depend on placement (spans and in-place
lists are offsets from d_rec); outputs are guarded (tests/guards.py), so the
write-set checks of test_gpu_bounds.py apply to every placement too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guards  # noqa: E402
from bounds_batches import decode_batch, encode_batch, slice_batch  # noqa: E402
from bounds_gpu import (E_ARG, PATHS, DecOut, EncIn, L, check_decode, decode_call,  # noqa: E402
                        encode_sizes, get_param, got, out_buf, placed, ptr, run_encode, set_param)
from honu_amd import object as hobj  # noqa: E402

OUT_PHASES = list(range(0, 128, 16))  # records arena, data arena, rows
PAYLOAD_PHASES = [0, 1, 3, 8, 15, 17, 63]
VAR_PHASES = [0, 1, 7]
TABLE_PHASES = [0, 4, 8, 12]
INFO_PHASES = [0, 8]
KEY_PHASES = [0, 1, 13]
SUB_BATCHES = [1, 63, 64, 65]
FORMS = {"lists_inplace": (1, 1), "lists_table": (0, 0)}


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hobj.Codec(0, 4096)
    c.defaults = {k: get_param(c, k) for k in ("record_variant", "acl_inplace", "regions_inplace")}
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(codec):
    yield
    for k, v in codec.defaults.items():
        assert set_param(codec, k, v)


def _decode_setup(codec, rv, form):
    for name, v in zip(("record_variant", "acl_inplace", "regions_inplace"), (rv,) + FORMS[form]):
        if not set_param(codec, name, v):
            pytest.skip(f"the library refuses {name} = {v}")
    return tuple(bool(v) for v in FORMS[form])


_oracle_cache = {}


def oracle_encode(oracle_lib, name, k=0):
    if (name, k) not in _oracle_cache:
        _oracle_cache[name, k] = oracle_lib.marshal_batch(slice_batch(encode_batch(name), k))
    return _oracle_cache[name, k]


# --------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["units", "edges", "two_class"])
def test_encode_displaced(codec, oracle_lib, name, path):
    """d_out at every multiple of 16 in [0, 128), with d_payload, d_var and
    the tables displaced round-robin by the steps their rules allow."""
    hb = encode_batch(name)
    ora = oracle_encode(oracle_lib, name)
    for c, out_phase in enumerate(OUT_PHASES):
        ph = dict(payload=PAYLOAD_PHASES[c % 7], var=VAR_PHASES[c % 3], tables=TABLE_PHASES[c % 4])
        try:
            guards.twice(lambda fill: run_encode(codec, hb, path, ora, fill, out_phase=out_phase, **ph))
        except AssertionError as e:
            raise AssertionError(f"d_out + {out_phase}, {ph}: {e}") from e


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rv", [5, 6], ids=["split", "fused"])
def test_decode_displaced(codec, oracle_lib, rv, form):
    """Materialising honu_decode_batch + honu_decode_keys with d_rec at every
    multiple of 16 in [0, 128), d_data likewise in the opposite order, d_meta
    by multiples of 16, d_info by {0, 8}, the tables by {0, 4, 8, 12} and the
    keys by {0, 1, 13}."""
    rec, off = decode_batch()
    n = len(off) - 1
    ip = _decode_setup(codec, rv, form)
    ora = oracle_lib.decode_batch(rec, off, True, *ip)
    keys = [oracle_lib.key(ora[0][i:i + 1], int(ora[1][i]["meta_status"])) for i in range(n)]
    dev = codec.torch_device
    d_off = placed(off, dev)
    for c, rec_phase in enumerate(OUT_PHASES):
        ph = dict(data=OUT_PHASES[-1 - c], meta=OUT_PHASES[(3 * c) % 8], info=INFO_PHASES[c % 2],
                  tables=TABLE_PHASES[c % 4])
        d_rec = placed(rec, dev, rec_phase)

        def body(fill):
            o = DecOut(n, ora[5], dev, fill, True, **ph)
            assert decode_call(codec, ptr(d_rec), ptr(d_off), o) == 0
            k, kst = out_buf(29 * n, dev, fill, KEY_PHASES[c % 3]), out_buf(4 * n, dev, fill)
            L.check(codec.lib.honu_decode_keys(codec.ctx, ptr(o.meta), ptr(o.info), n, ptr(k), ptr(kst),
                                               codec.stream), "keys")
            torch.cuda.synchronize()
            check_decode(o, ora)
            gk, gst = got(k).reshape(n, 29), got(kst, np.int32)
            for i, (st, key) in enumerate(keys):
                assert st == gst[i] and (st != 0 or key == gk[i].tobytes()), i
            guards.assert_untouched(k, [(0, 29 * n)])
            guards.assert_untouched(kst, [(0, 4 * n)])
        try:
            guards.twice(body)
        except AssertionError as e:
            raise AssertionError(f"d_rec + {rec_phase}, keys + {KEY_PHASES[c % 3]}, {ph}: {e}") from e


@pytest.mark.parametrize("k", SUB_BATCHES)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rv", [5, 6], ids=["split", "fused"])
def test_decode_sub_batch(codec, oracle_lib, rv, form, k):
    """Records [k, n) of one arena, passed as d_rec_off + k: the first record
    no longer starts at d_rec, nor on a 16-byte boundary."""
    rec, off = decode_batch()
    n = len(off) - 1 - k
    ip = _decode_setup(codec, rv, form)
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev), placed(off, dev)
    for materialize in (False, True):
        ora = oracle_lib.decode_batch(rec, off[k:], materialize, *ip)

        def body(fill):
            o = DecOut(n, ora[5], dev, fill, materialize)
            assert decode_call(codec, ptr(d_rec), ptr(d_off) + 8 * k, o) == 0
            torch.cuda.synchronize()
            check_decode(o, ora)
        guards.twice(body)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,k", [(b, k) for b in ("units", "edges", "two_class") for k in SUB_BATCHES
                                    if k < len(encode_batch(b).meta)])
def test_encode_sub_batch(codec, oracle_lib, name, path, k):
    """Rows [k, n) passed as d_meta + k and d_payload_off + k: the payload
    copy's logical space starts at payload_off[k], not 0 (EncodeSegments::lo).
    (two_class has 64 rows: k = 1 and 63, the latter a batch of one row.)"""
    hb = encode_batch(name)
    assert int(hb.payload_off[k]) > 0  # (the batches' first payload is not empty)
    guards.twice(lambda fill: run_encode(codec, hb, path, oracle_encode(oracle_lib, name, k), fill, k=k))


# --------------------------------------------------------------------------
def test_alignment_refusals_encode(codec, oracle_lib):
    """A records arena or a row array off by 8 and a table off by 2 are
    refused with HONU_E_ARG before anything is launched: no output byte
    changes."""
    hb = encode_batch("units")
    oout, ooff, ost = oracle_encode(oracle_lib, "units")
    n, total = len(ost), int(ooff[-1])
    dev = codec.torch_device
    x = EncIn(hb, dev)
    good_off, good_st = out_buf(8 * (n + 1), dev, 0), out_buf(4 * n, dev, 0)
    encode_sizes(codec, x, good_off, good_st)
    torch.cuda.synchronize()

    def body(fill):
        for what in ("out", "meta", "acl", "regions"):
            for path in PATHS:
                out = out_buf(total + 16, dev, fill)
                out_off, status = out_buf(8 * (n + 1), dev, fill), out_buf(4 * n, dev, fill)
                if path != "marshal":  # the pairs read d_out_off and d_status: the size pass's
                    out_off.copy_(good_off)
                    status.copy_(good_st)
                y = EncIn.__new__(EncIn)
                y.__dict__.update(x.__dict__)
                po = ptr(out)
                if what == "out":
                    po += 8
                elif what == "meta":
                    y.meta += 8
                elif what == "acl":
                    y.acl += 2
                else:
                    y.reg += 2
                before_off, before_st = got(out_off).copy(), got(status).copy()
                lib, a = codec.lib, (codec.ctx,)
                if path == "marshal":
                    rcs = [lib.honu_marshal_batch(*a, y.meta, y.var, y.var_len, y.acl, y.acl_len, y.reg, y.reg_len,
                                                  y.payload, y.payload_off, n, po, total, ptr(out_off), ptr(status),
                                                  codec.stream)]
                elif path == "plain":
                    rcs = [lib.honu_encode_records(*a, y.meta, y.var, y.acl, y.reg, y.payload_off, n, po, total,
                                                   ptr(out_off), ptr(status), codec.stream)]
                    if what == "out":
                        rcs.append(lib.honu_encode_payloads(*a, y.payload, y.payload_off, n, po, total,
                                                            ptr(out_off), ptr(status), codec.stream))
                else:
                    rcs = [lib.honu_encode_records_units(*a, y.meta, y.var, y.acl, y.reg, y.payload, y.payload_off,
                                                         n, po, total, ptr(out_off), ptr(status), codec.stream)]
                    if what == "out":
                        rcs.append(lib.honu_encode_payloads_units(*a, y.payload, y.payload_off, n, po, total,
                                                                  ptr(out_off), ptr(status), codec.stream))
                assert rcs == [E_ARG] * len(rcs), (what, path, rcs)
                torch.cuda.synchronize()
                guards.assert_untouched(out, [])
                assert got(out_off).tobytes() == before_off.tobytes()
                assert got(status).tobytes() == before_st.tobytes()
        # the size pass alone: rows off by 8, a table off by 2
        for what in ("meta", "acl", "regions"):
            sizes, status = out_buf(8 * (n + 1), dev, fill), out_buf(4 * n, dev, fill)
            m, acl, reg = x.meta + 8 * (what == "meta"), x.acl + 2 * (what == "acl"), x.reg + 2 * (what == "regions")
            assert codec.lib.honu_encode_sizes(codec.ctx, m, x.var_len, acl, x.acl_len, reg, x.reg_len, x.payload_off,
                                               n, ptr(sizes), ptr(status), codec.stream) == E_ARG, what
            torch.cuda.synchronize()
            guards.assert_untouched(sizes, [])
            guards.assert_untouched(status, [])
    guards.twice(body)


@pytest.mark.parametrize("rv", [5, 6], ids=["split", "fused"])
def test_alignment_refusals_decode(codec, oracle_lib, rv):
    """A records arena, data arena or row array off by 8 and a table off by 2
    are refused with HONU_E_ARG before anything is launched (the split decode
    used to check the tables and the data arena only after its parse had
    stored the rows)."""
    rec, off = decode_batch()
    n = len(off) - 1
    ip = _decode_setup(codec, rv, "lists_table")
    tot = oracle_lib.decode_batch(rec, off, True, *ip)[5]
    dev = codec.torch_device
    d_rec, d_off = placed(rec, dev, 0), placed(off, dev)

    def body(fill):
        for what in ("rec", "data", "meta", "acl", "regions"):
            o = DecOut(n, [int(v) + 16 for v in tot], dev, fill, True)
            p = dict(rec=ptr(d_rec), meta=ptr(o.meta), acl=ptr(o.acl), regions=ptr(o.reg), data=ptr(o.data))
            p[what] += 2 if what in ("acl", "regions") else 8
            rc = codec.lib.honu_decode_batch(codec.ctx, p["rec"], ptr(d_off), n, p["meta"], ptr(o.info), p["acl"],
                                             int(tot[0]), p["regions"], int(tot[1]), p["data"], int(tot[2]),
                                             ptr(o.tot), codec.stream)
            assert rc == E_ARG, (what, rc)
            torch.cuda.synchronize()
            for t in (o.meta, o.info, o.tot, o.acl, o.reg, o.data):
                guards.assert_untouched(t, [])
    guards.twice(body)
