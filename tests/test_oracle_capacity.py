"""The oracle under capacities (oracle.decode_batch / marshal_batch with
acl_cap, regions_cap, data_cap, out_cap): the reference the GPU capacity
parity tests compare with (test_gpu_bounds.py). On a batch whose lists and
payloads straddle each capacity: HONU_ERR_CAPACITY falls exactly on the
records whose running offset plus count exceeds the capacity (a record with
no entries too, once the running offset has passed it), totals report what
the batch needs, failed payloads have data_off == data_len == 0, and nothing
is stored at or past a capacity."""
import numpy as np
import pytest

from bounds_batches import decode_batch, encode_batch

CAPACITY = 9


@pytest.fixture(scope="module")
def full(oracle_lib):
    """The batch decoded without capacities, every list in its table."""
    rec, off = decode_batch()
    meta, info, acl, reg, data, tot = oracle_lib.decode_batch(rec, off, True, False, False)
    assert (info["meta_status"] == 0).all() and (info["data_status"] == 0).all()
    na, nr = meta["acl_count"].astype(np.int64), meta["regions_count"].astype(np.int64)
    assert int(na.sum()) == int(tot[0]) > 1000 and int(nr.sum()) == int(tot[1]) > 100
    return dict(rec=rec, off=off, meta=meta, info=info, acl=acl, reg=reg, data=data, tot=tot, na=na, nr=nr,
                ao=np.cumsum(na) - na, ro=np.cumsum(nr) - nr)


def _poison(a, oracle_lib):
    return (a.view(np.uint8) == oracle_lib.POISON).all()


@pytest.mark.parametrize("which", ["acl", "regions", "both"])
@pytest.mark.parametrize("cap", ["need", "need-1", "half", "0"])
def test_table_capacities(oracle_lib, full, which, cap):
    f = full
    need_a, need_r = int(f["tot"][0]), int(f["tot"][1])
    pick = lambda need: {"need": need, "need-1": need - 1, "half": need // 2, "0": 0}[cap]  # noqa: E731
    acl_cap = pick(need_a) if which in ("acl", "both") else need_a
    reg_cap = pick(need_r) if which in ("regions", "both") else need_r
    meta, info, acl, reg, data, tot = oracle_lib.decode_batch(
        f["rec"], f["off"], False, False, False, acl_cap=acl_cap, regions_cap=reg_cap)
    fails = (f["ao"] + f["na"] > acl_cap) | (f["ro"] + f["nr"] > reg_cap)
    assert np.array_equal(info["meta_status"] == CAPACITY, fails)
    assert (info["meta_status"][~fails] == 0).all()
    assert fails.any() == (cap != "need")
    if cap in ("half", "0"):  # a record without entries fails too behind the capacity
        empty = (f["na"] == 0) & (f["nr"] == 0)
        assert (empty & fails).any() and (cap == "0" or (empty & ~fails).any())
    # totals: what the batch needs (the data bytes too, in a zero-copy call)
    assert np.array_equal(tot, f["tot"])
    # the rows keep the offsets the lists would have had
    assert np.array_equal(meta["acl_off"], f["meta"]["acl_off"])
    assert np.array_equal(meta["regions_off"], f["meta"]["regions_off"])
    # the untrimmed tables: entries of the records that fit, nothing at or past a capacity
    assert len(acl) > max(acl_cap, need_a - 1) and len(reg) > max(reg_cap, need_r - 1)
    assert _poison(acl[acl_cap:], oracle_lib) and _poison(reg[reg_cap:], oracle_lib)
    for i in np.flatnonzero(~fails):
        a, r = int(f["ao"][i]), int(f["ro"][i])
        assert acl[a:a + int(f["na"][i])].tobytes() == f["acl"][a:a + int(f["na"][i])].tobytes(), i
        assert reg[r:r + int(f["nr"][i])].tobytes() == f["reg"][r:r + int(f["nr"][i])].tobytes(), i


@pytest.mark.parametrize("cap", ["need", "need-1", "last", "half"])
def test_data_capacity(oracle_lib, full, cap):
    f = full
    oinfo = f["info"]
    have = np.flatnonzero(oinfo["data_len"] > 0)
    last = int(have[-1])
    need = int(oinfo["data_off"][last] + oinfo["data_len"][last])  # the last payload's end
    assert int(f["tot"][2]) == (need + 15) // 16 * 16
    data_cap = {"need": need, "need-1": need - 1, "last": int(oinfo["data_off"][last]), "half": need // 2}[cap]
    meta, info, acl, reg, data, tot = oracle_lib.decode_batch(f["rec"], f["off"], True, False, False,
                                                              data_cap=data_cap)
    fails = (oinfo["data_len"] > 0) & (oinfo["data_off"] + oinfo["data_len"] > data_cap)
    assert np.array_equal(info["data_status"] == CAPACITY, fails)
    assert fails.sum() == {"need": 0, "need-1": 1, "last": 1}.get(cap, fails.sum()) and (cap != "half" or fails.sum() > 1)
    assert (info["data_off"][fails] == 0).all() and (info["data_len"][fails] == 0).all()
    assert np.array_equal(info["data_off"][~fails], oinfo["data_off"][~fails])
    assert np.array_equal(info["data_len"][~fails], oinfo["data_len"][~fails])
    assert np.array_equal(tot, f["tot"]) and (info["meta_status"] == 0).all()
    assert len(data) > data_cap and _poison(data[data_cap:], oracle_lib)
    written = np.zeros(len(data), bool)
    for i in np.flatnonzero(~fails & (oinfo["data_len"] > 0)):
        o, ln = int(oinfo["data_off"][i]), int(oinfo["data_len"][i])
        assert data[o:o + ln].tobytes() == f["data"][o:o + ln].tobytes(), i
        written[o:o + ln] = True
    assert _poison(data[~written], oracle_lib)  # the alignment gaps and failed payloads' places too


def test_defaults_unchanged(oracle_lib, full):
    f = full
    meta, info, acl, reg, data, tot = oracle_lib.decode_batch(f["rec"], f["off"], True, False, False)
    assert len(acl) == int(tot[0]) and len(reg) == int(tot[1]) and len(data) == int(tot[2])
    with pytest.raises(ValueError):
        oracle_lib.decode_batch(f["rec"], f["off"], False, data_cap=16)
    hb = encode_batch("units")
    out, off, st = oracle_lib.marshal_batch(hb)
    assert len(out) == int(off[-1])
    out2, off2, st2 = oracle_lib.marshal_batch(hb, out_cap=int(off[-1]))
    assert out2.tobytes() == out.tobytes() and np.array_equal(st, st2) and np.array_equal(off, off2)


@pytest.mark.parametrize("where", ["start", "inside", "end-1", "end", "0"])
def test_out_capacity(oracle_lib, where):
    hb = encode_batch("units")
    out, off, st = oracle_lib.marshal_batch(hb)
    assert sorted(set(st.tolist())) == [0, 8]  # two nil metas: HONU_ERR_PANIC, empty ranges
    j = 100
    b, e = int(off[j]), int(off[j + 1])
    cap = {"start": b, "inside": (b + e) // 2, "end-1": e - 1, "end": e, "0": 0}[where]
    cout, coff, cst = oracle_lib.marshal_batch(hb, out_cap=cap)
    assert np.array_equal(coff, off) and len(cout) == int(off[-1])  # offsets: what the batch needs
    fails = (st == 0) & (off[1:] > cap)
    assert np.array_equal(cst == CAPACITY, fails) and np.array_equal(cst[~fails], st[~fails])
    first = int(off[np.flatnonzero(fails)[0]]) if fails.any() else int(off[-1])
    assert first == {"start": b, "inside": b, "end-1": b, "end": e, "0": 0}[where]
    assert cout[:first].tobytes() == out[:first].tobytes()
    assert _poison(cout[first:], oracle_lib)
