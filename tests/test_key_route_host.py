"""keys.route, the host statement of honu_key_route (a mixed batch taken
apart by its collections' buckets: store.go:236-240, tx.go:112-120, 141-158,
collection.go:86), against expectations written out by hand over a ten-record
fixture: three collections, one record of a collection the store does not
have, one record whose status is not OK. With `seq` a key sort of the batch,
every segment is keys.sort of that collection's keys alone. And the entry
points' presence, the workspace function's properties and the first refusal,
which need no device."""
from honu_amd import _lib, keys
from honu_amd.metadata import LIST_ROW_HEAD, SEEK_NONE, Scalar

E_ARG = -1
NONE = SEEK_NONE
H = LIST_ROW_HEAD

CA, CB, CC = bytes([0x10]) * 16, bytes([0x20]) * 16, bytes([0x30]) * 16
CX = bytes([0x25]) * 16  # between CB and CC: no bucket of that name
TABLE = [CA, CB, CC]
IDS = [CB, CA, CC, CA, CX, CB, CA, CC, CB, CA]
STATUS = [0, 0, 0, 0, 0, 0, 7, 0, 0, 0]  # record 6 is not OK


def key(obj, vid):
    return keys.new(bytes([obj]) * 16, Scalar(PID=1, VID=vid))


# records 0 and 5 carry one key (both of CB); records 3 and 9 are two versions of one object (of CA)
KEYS = [key(5, 1), key(9, 1), key(1, 1), key(2, 1), key(7, 1), key(5, 1), key(0, 1), key(8, 1), key(3, 1), key(2, 2)]
# honu_sort_keys' order of KEYS under STATUS: ascending keys, equal keys in arrival order, record 6 behind them
SEQ = [2, 3, 9, 8, 0, 5, 4, 7, 1, 6]


def test_the_fixture_s_sequence_is_a_key_sort():
    ok = [i for i in range(10) if STATUS[i] == 0]
    assert SEQ == sorted(ok, key=lambda i: (KEYS[i], i)) + [6]
    assert [KEYS[i] for i in SEQ[:9]] == keys.sort(KEYS[i] for i in ok)


def test_arrival_order():
    r = keys.route(IDS, TABLE, statuses=STATUS)
    assert r.buckets == [1, 0, 2, 0, NONE, 1, NONE, 2, 1, 0]
    assert r.offsets == [0, 3, 6, 8, 9, 10] and r.counts == [3, 3, 2, 1, 1]
    assert r.rows == [(0, 1, 1, H), (0, 3, 3, 0), (0, 9, 9, 0), (1, 0, 0, H), (1, 5, 5, 0), (1, 8, 8, 0),
                      (2, 2, 2, H), (2, 7, 7, 0), (3, 4, 4, H), (4, 6, 6, H)]
    assert r.local == [0, 1, 2, 0, 1, 2, 0, 1, 0, 0] and r.keys is None


def test_without_statuses_every_record_takes_part():
    r = keys.route(IDS, TABLE)
    assert r.buckets == [1, 0, 2, 0, NONE, 1, 0, 2, 1, 0]
    assert r.offsets == [0, 4, 7, 9, 10, 10] and r.counts == [4, 3, 2, 1, 0]
    assert [row[1] for row in r.rows] == [1, 3, 6, 9, 0, 5, 8, 2, 7, 4]
    assert [row[3] for row in r.rows] == [H, 0, 0, 0, H, 0, 0, H, 0, H]  # the empty class has no head


def test_key_order():
    r = keys.route(IDS, TABLE, statuses=STATUS, seq=SEQ, keys=KEYS)
    assert r.buckets == [1, 0, 2, 0, NONE, 1, NONE, 2, 1, 0]  # by record: the sequence does not matter
    assert r.offsets == [0, 3, 6, 8, 9, 10] and r.counts == [3, 3, 2, 1, 1]
    assert r.rows == [(0, 1, 3, H), (0, 2, 9, 0), (0, 8, 1, 0), (1, 3, 8, H), (1, 4, 0, 0), (1, 5, 5, 0),
                      (2, 0, 2, H), (2, 7, 7, 0), (3, 6, 4, H), (4, 9, 6, H)]
    assert r.local == [0, 1, 2, 0, 1, 2, 0, 1, 0, 0]
    assert r.keys == [KEYS[row[2]] for row in r.rows]


def test_every_segment_is_the_sort_of_its_collection_alone():
    r = keys.route(IDS, TABLE, statuses=STATUS, seq=SEQ, keys=KEYS)
    for c, name in enumerate(TABLE):
        own = [i for i in range(10) if IDS[i] == name and STATUS[i] == 0]  # arrival order
        a, b = r.offsets[c], r.offsets[c + 1]
        assert r.keys[a:b] == keys.sort(KEYS[i] for i in own) and b - a == r.counts[c] == len(own)
        # equal keys in arrival order, as a stable sort of the collection's records leaves them
        assert [row[2] for row in r.rows[a:b]] == sorted(own, key=lambda i: (KEYS[i], i))
        # and so the B side of a merge as it stands: merged into a column it gives the sort of both
        column = keys.sort([key(4, 1), key(2, 1), key(6, 3)])
        assert keys.merge(column, r.keys[a:b]) == keys.sort(column + [KEYS[i] for i in own])
    assert [row[2] for row in r.rows[r.offsets[3]:r.offsets[4]]] == [4]  # the unknown collection's record
    assert [row[2] for row in r.rows[r.offsets[4]:]] == [6]             # the record that is not OK


def test_a_sequence_value_that_names_no_record():
    r = keys.route(IDS[:3], TABLE, seq=[0, 10, 1], keys=KEYS[:3])
    assert r.rows == [(0, 2, 1, H), (1, 0, 0, H), (4, 1, NONE, H)]
    assert r.keys == [KEYS[1], KEYS[0], bytes(29)] and r.buckets == [1, 0, None]
    assert r.offsets == [0, 1, 2, 2, 2, 3] and r.counts == [1, 1, 0, 0, 1] and r.local == [0, 0, 0]
    assert keys.route(IDS[:3], TABLE, seq=[-1, 3, 1 << 32]).counts == [0, 0, 0, 0, 3]


def test_a_repeated_sequence_value_gives_a_row_each():
    r = keys.route(IDS[:3], TABLE, seq=[1, 1, 1])
    assert r.rows == [(0, 0, 1, H), (0, 1, 1, 0), (0, 2, 1, 0)] and r.buckets == [None, 0, None]


def test_empty_batch_and_empty_table():
    r = keys.route([], TABLE, keys=[])
    assert r == keys.Route([], [], [], [], [0] * 6, [0] * 5)
    r = keys.route(IDS, [], statuses=STATUS)
    assert r.offsets == [0, 9, 10] and r.counts == [9, 1] and r.buckets == [NONE] * 10
    assert [row[0] for row in r.rows] == [0] * 9 + [1] and r.rows[-1] == (1, 6, 6, H)
    assert keys.route([], []).offsets == [0, 0, 0]


def test_ids_compare_as_bytes():
    """bytes.Compare: byte 0 is the most significant, byte 15 the least."""
    lo, hi = bytes(15) + b"\x01", b"\x01" + bytes(15)
    table = [bytes(16), lo, hi, bytes([0xFF]) * 16]
    assert table == sorted(table)
    r = keys.route([hi, lo, bytes([0xFF]) * 16, bytes(16), bytes(15) + b"\x02"], table)
    assert r.buckets == [2, 1, 3, 0, NONE]


def test_docstring_cites_the_store():
    for cite in ("store.go:236-240", "tx.go:112-120", "tx.go:141-158", "collection.go:86", "honu_key_route"):
        assert cite in keys.route.__doc__, cite


def test_library_exports_the_entry_points():
    assert {"honu_key_route", "honu_key_route_workspace"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "honu_key_route") and hasattr(lib, "honu_key_route_workspace")


def test_workspace_function():
    lib = _lib.load()
    assert lib.honu_key_route_workspace(0) == 0
    last = 0
    for m in range(1, 5001):
        w = int(lib.honu_key_route_workspace(m))
        # the sort's own workspace, two 29-byte columns and an order at the least
        assert w % 256 == 0 and last <= w and w >= int(lib.honu_sort_keys_workspace(m)) + 62 * m, m
        last = w
    big = [int(lib.honu_key_route_workspace(m)) for m in (1 << 20, (1 << 32) - 1)]
    assert last <= big[0] <= big[1] and all(w % 256 == 0 for w in big)


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_route(None, *([0] * 16), None) == E_ARG
