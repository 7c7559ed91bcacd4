"""keys.reclaim, the host statement of honu_key_reclaim (the space a Drop
frees, store.go:314-322, 399-404), against expectations written out by hand
over the ten-key fixture of tests/test_key_fetch_host.py; its agreement with
the route through scan and fetch; delete and compact followed by a reclaim;
and the entry point's presence, workspace function and first refusal, which
need no device."""
from honu_amd import _lib, keys
from honu_amd.metadata import SEEK_NONE
from test_key_fetch_host import A, ORDER, VALUES

E_ARG = -1
NONE = SEEK_NONE


def test_valid_10_keeps_everything_as_it_is():
    order_out, remap, source, values_out, k, s, i = keys.reclaim(ORDER, 10, VALUES)
    assert order_out == ORDER and remap == list(range(10)) and source == list(range(10))
    assert values_out == VALUES and (k, s, i) == (None, None, None)


def test_valid_6_frees_the_records_of_the_tail():
    """Rows 0..5 name records 3, 7, 0, 9, 1, 8: those stay, in ascending old index."""
    statuses = [10 * r for r in range(10)]
    info = [("info", r) for r in range(10)]
    order_out, remap, source, values_out, keys_out, statuses_out, info_out = keys.reclaim(
        ORDER, 6, VALUES, keys=[bytes([100 + r]) for r in range(10)], statuses=statuses, info=info)
    assert source == [0, 1, 3, 7, 8, 9]
    assert remap == [0, 1, NONE, 2, NONE, NONE, NONE, 3, 4, 5]
    assert order_out == [2, 3, 0, 5, 1, 4, NONE, NONE, NONE, NONE]
    assert values_out == [b"zero", b"", b"three" * 40, b"seven", b"eight", b"nine"]
    assert keys_out == [bytes([100 + r]) for r in source]
    assert statuses_out == [0, 10, 30, 70, 80, 90] and info_out == [("info", r) for r in source]


def test_valid_0_frees_everything():
    order_out, remap, source, values_out, *_ = keys.reclaim(ORDER, 0, VALUES)
    assert order_out == [NONE] * 10 and remap == [NONE] * 10 and source == [] and values_out == []


def test_a_repeated_index_keeps_its_record_once():
    order = [3, 3, 0] + ORDER[3:]
    order_out, remap, source, values_out, *_ = keys.reclaim(order, 3, VALUES)
    assert source == [0, 3] and order_out == [1, 1, 0] + [NONE] * 7
    assert remap == [0, NONE, NONE, 1] + [NONE] * 6 and values_out == [b"zero", b"three" * 40]


def test_an_index_that_names_no_record():
    order = [3, len(VALUES), 0xFFFFFFFF, 9] + ORDER[4:]
    order_out, remap, source, values_out, *_ = keys.reclaim(order, 4, VALUES)
    assert source == [3, 9] and order_out == [0, NONE, NONE, 1] + [NONE] * 6
    assert values_out == [b"three" * 40, b"nine"]
    assert [j for j in remap if j != NONE] == [0, 1] and remap[3] == 0 and remap[9] == 1


def test_valid_above_n_is_clamped():
    assert keys.reclaim(ORDER, 99, VALUES) == keys.reclaim(ORDER, 10, VALUES)
    assert keys.reclaim(ORDER, 1 << 63, VALUES)[2] == list(range(10))


def test_values_are_copies():
    mutable = [bytearray(v) for v in VALUES]
    values_out = keys.reclaim(ORDER, 10, mutable)[3]
    mutable[0][0] = 0
    assert values_out[0] == b"zero" and type(values_out[0]) is bytes


# arrival order: six records over three keys
K = [b"b", b"a", b"b", b"c", b"a", b"b"]


def column(arrivals):
    """(sorted keys, order): sort_keys' stable order of the arrivals."""
    order = sorted(range(len(arrivals)), key=lambda r: (arrivals[r], r))
    return [arrivals[r] for r in order], order


def test_equal_keys_keep_ascending_indices():
    col, order = column(K)
    assert col == [b"a", b"a", b"b", b"b", b"b", b"c"] and order == [1, 4, 0, 2, 5, 3]
    # the first b (record 0) goes: its row leaves the valid rows
    kept_order, tail = [1, 4, 2, 5, 3], [0]
    order_out, remap, source, *_ = keys.reclaim(kept_order + tail, 5, K)
    assert source == [1, 2, 3, 4, 5] and order_out == [0, 3, 1, 4, 2, NONE]
    kept_col = [K[r] for r in kept_order]
    for p in range(4):
        if kept_col[p] == kept_col[p + 1]:
            assert order_out[p] < order_out[p + 1]  # the later arrival still has the higher index


def test_reclaim_agrees_with_scan_and_fetch():
    """What the calls before offered: a listing of the valid rows, fetched."""
    for valid in (10, 6, 1, 0):
        order_out, _, _, values_out, *_ = keys.reclaim(ORDER, valid, VALUES)
        route = keys.fetch(VALUES, keys.scan(A, [(0, valid)]), ORDER)
        assert len(route) == valid
        for p in range(valid):
            assert values_out[order_out[p]] == route[p]


def split(col, order, gone):
    """A stable compaction of (col, order) by the rows' gone flags: (kept keys, order as delete writes it)."""
    kept = [p for p in range(len(col)) if not gone[p]]
    removed = [p for p in range(len(col)) if gone[p]]
    return [col[p] for p in kept], [order[p] for p in kept] + [order[p] for p in removed]


def reads(col, order, values, probes):
    """seek -> scan -> fetch of every probe, and the latest version of every range."""
    ranges = [keys.seek(col, q) for q in probes]
    walk = keys.scan(col, ranges)
    last = keys.scan(col, ranges, reverse=True, limit=1)
    return ranges, walk, keys.fetch(values, walk, order), keys.fetch(values, last, order)


def test_delete_and_compact_then_reclaim_read_the_same():
    arrivals = [b"b1", b"a1", b"b1", b"c1", b"a2", b"b1", b"c2", b"a1", b"d1"]
    values = [b"v%d" % r * (r + 1) for r in range(len(arrivals))]
    col, order = column(arrivals)
    probes = [b"a", b"b", b"b1", b"c", b"c2", b"d", b"e", b""]
    for name in ("delete", "compact"):
        if name == "delete":
            kept, removed = keys.delete(col, [b"c", b"a2"])
            gone = [k.startswith(b"c") or k.startswith(b"a2") for k in col]
        else:
            kept, removed = keys.compact(col)
            gone = [p + 1 < len(col) and col[p + 1] == col[p] for p in range(len(col))]
        kept2, order2 = split(col, order, gone)
        assert kept2 == kept and len(removed) == sum(gone) > 0
        v = len(kept)
        before = reads(kept, order2[:v], values, probes)
        order_out, remap, source, values_out, keys_out, *_ = keys.reclaim(order2, v, values, keys=arrivals)
        assert len(values_out) == v == len(source) and order_out[v:] == [NONE] * len(removed)
        assert sorted(order_out[:v]) == list(range(v))
        assert [keys_out[j] for j in order_out[:v]] == kept  # the rows stand, the records moved under them
        assert reads(kept, order_out[:v], values_out, probes) == before
        # and a second reclaim frees nothing
        again = keys.reclaim(order_out[:v], v, values_out, keys=keys_out)
        assert again[0] == order_out[:v] and again[3] == values_out and again[4] == keys_out


def test_docstrings_cite_the_store():
    assert "store.go:314-322" in keys.reclaim.__doc__ and "honu_key_reclaim" in keys.reclaim.__doc__


def test_library_exports_the_entry_point():
    assert {"honu_key_reclaim", "honu_key_reclaim_workspace"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "honu_key_reclaim") and hasattr(lib, "honu_key_reclaim_workspace")


def test_workspace_function():
    lib = _lib.load()
    assert lib.honu_key_reclaim_workspace(0) == 0
    last = 0
    for n in range(1, 5001):
        w = int(lib.honu_key_reclaim_workspace(n))
        assert w % 256 == 0 and last <= w < 8 * n + (1 << 20) and w > 0, n
        last = w
    for n in (1 << 20, (1 << 32) - 1):
        assert int(lib.honu_key_reclaim_workspace(n)) <= 8 * n + (1 << 20)


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_reclaim(None, *([0] * 25), None) == E_ARG
