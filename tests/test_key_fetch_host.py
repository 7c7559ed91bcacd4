"""keys.fetch, the host statement of honu_key_fetch (Cursor.Object(),
iterator/cursor.go:31-38, at every row that List, Versions or Retrieve visits,
collection.go:32-35, 97-110), against expectations written out by hand over
the cursor fixture of tests/test_key_list_host.py (ten one-byte keys); and the
entry point's presence, flag value and first refusal, which need no device."""
from honu_amd import _lib, keys, metadata

E_ARG = -1

# the fixture of test_empty_repeated_and_overlapping_ranges: position p holds the key bytes([p])
A = sorted(bytes([i]) for i in range(10))
# the record of position p is ORDER[p]; record r holds VALUES[r]
ORDER = [3, 7, 0, 9, 1, 8, 2, 6, 4, 5]
VALUES = [b"zero", b"", b"two", b"three" * 40, b"\x00four", b"5", b"six", b"seven", b"eight", b"nine"]


def test_forward_is_the_records_in_key_order():
    visits = keys.scan(A, [(2, 6)])
    assert visits == [(0, 2), (0, 3), (0, 4), (0, 5)]
    assert keys.fetch(VALUES, visits, ORDER) == [b"zero", b"nine", b"", b"eight"]


def test_reverse_is_most_recent_first():
    visits = keys.scan(A, [(2, 6), (8, 10)], reverse=True)
    assert keys.fetch(VALUES, visits, ORDER) == [b"eight", b"", b"nine", b"zero", b"5", b"\x00four"]


def test_reverse_limit_one_is_retrieve():
    """Retrieve's "latest version" (collection.go:97-104): the value at end - 1 of each range."""
    visits = keys.scan(A, [(0, 4), (4, 4), (5, 10)], reverse=True, limit=1)
    assert visits == [(0, 3), (2, 9)]
    assert keys.fetch(VALUES, visits, ORDER) == [b"nine", b"5"]


def test_a_repeated_range_returns_its_records_once_per_row():
    visits = keys.scan(A, [(0, 2), (0, 2), (1, 3)])
    got = keys.fetch(VALUES, visits, ORDER)
    assert got == [b"three" * 40, b"seven", b"three" * 40, b"seven", b"seven", b"zero"]
    mutable = [bytearray(v) for v in VALUES]
    got = keys.fetch(mutable, visits, ORDER)
    mutable[3][0] = 0
    assert got[0] == b"three" * 40 and type(got[0]) is bytes  # Object()'s make + copy


def test_an_index_out_of_range_gives_none():
    order = list(ORDER)
    order[4] = len(VALUES)      # one past the records
    order[5] = 0xFFFFFFFF       # HONU_SEEK_NONE
    visits = keys.scan(A, [(3, 7)]) + [(1, 10), (1, 99), (1, -1)]  # and positions past the order
    assert keys.fetch(VALUES, visits, order) == [b"nine", None, None, b"two", None, None, None]
    assert keys.fetch(VALUES[:3], [(0, 0), (0, 2)], ORDER) == [None, b"zero"]
    assert keys.fetch(VALUES, [], ORDER) == []


def test_live_leaves_tombstones_in_place_as_none():
    tomb = {0, 9, 6}
    visits = keys.scan(A, [(0, 10)])
    got = keys.fetch(VALUES, visits, ORDER, live=lambda r: r not in tomb)
    assert got == [b"three" * 40, b"seven", None, None, b"", b"eight", b"two", None, b"\x00four", b"5"]
    assert len(got) == len(visits)
    # without the predicate nothing is left out
    assert keys.fetch(VALUES, visits, ORDER) == [VALUES[r] for r in ORDER]
    # a row whose index is out of range is None with or without it
    assert keys.fetch(VALUES, [(0, 0)], [77], live=lambda r: True) == [None]


def test_docstrings_cite_the_cursor():
    assert "cursor.go:31-38" in keys.fetch.__doc__ and "fetch()" in keys.__doc__


def test_library_exports_the_entry_point():
    assert "honu_key_fetch" in _lib.EXPORTS
    assert hasattr(_lib.load(), "honu_key_fetch")


def test_flag_value():
    assert metadata.FETCH_LIVE == 1


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_fetch(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E_ARG
