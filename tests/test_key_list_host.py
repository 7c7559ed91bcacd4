"""keys.scan, the host statement of honu_key_list (the walk with Cursor.Next()
or Cursor.Prev(), iterator/cursor.go:57-89, that follows the Seek in List,
Versions and Retrieve, collection.go:32-35, 97-110, and in the loop of
store.go:379), against a brute-force list comprehension, on the short-key
random cases of tests/test_key_delete_host.py; and the entry point's presence,
row size and first refusal, which need no device.

The brute force never slices a range: it asks of every position of the list
whether the walk visits it."""
import numpy as np

from honu_amd import _lib, keys

E_ARG = -1
ALPHABET = (b"\x00", b"\x01", b"\x7f", b"\x80", b"\xff")
P = keys.PREFIX_SIZE


def random_cases(cases=200, max_len=40, seed=232):
    """(a, b): sorted lists of short keys over a small alphabet, so prefixes and ties are common."""
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        sides = []
        for n in rng.integers(0, max_len + 1, 2):
            ks = [b"".join(ALPHABET[c] for c in rng.integers(0, len(ALPHABET), int(rng.integers(1, 3))))
                  for _ in range(int(n))]
            sides.append(sorted(ks))
        yield tuple(sides)


def ranges_of(a, b):
    """Seek ranges of b's keys and their one-byte prefixes over a, an empty
    range, the whole list, a repeat, and bounds past the end."""
    rs = [keys.seek(a, k) for k in b[:6]] + [keys.seek(a, k[:1]) for k in b[:6]]
    rs += [(3, 3), (0, len(a)), (0, len(a)), (len(a) + 5, len(a) + 9), (2, len(a) + 7), (5, 2)]
    return rs


def brute(a, ranges, reverse=False, limit=0, latest=False):
    n = len(a)
    out = []
    for q, (pos, end) in enumerate(ranges):
        visited = [p for p in range(n) if pos <= p < end and
                   (not latest or not any(a[x][:P] == a[p][:P] for x in range(p + 1, n)))]
        if reverse:
            visited = visited[::-1]
        out += [(q, p) for i, p in enumerate(visited) if not limit or i < limit]
    return out


def test_scan_is_the_brute_force_walk():
    rows = 0
    for a, b in random_cases():
        rs = ranges_of(a, b)
        above = len(a) + 1  # above every range
        for reverse in (False, True):
            for limit in (0, 1, 2, above):
                got = keys.scan(a, rs, reverse=reverse, limit=limit)
                assert got == brute(a, rs, reverse, limit), (a, rs, reverse, limit)
                rows += len(got)
        assert keys.scan(a, rs, limit=above) == keys.scan(a, rs)
    assert rows >= 10000


def long_cases(cases=60, seed=17):
    """Sorted 29-byte keys of a few objects with 1 to 5 versions each."""
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        ids = rng.integers(0, 256, (int(rng.integers(1, 8)), 16), dtype=np.uint8)
        ks = []
        for oid in ids:
            for v in range(int(rng.integers(1, 6))):
                ks.append(b"\x01" + oid.tobytes() + int(v + 1).to_bytes(8, "big") + int(rng.integers(0, 3)).to_bytes(4, "big"))
        yield sorted(ks)


def test_latest_is_one_row_per_object():
    rows = 0
    for a in long_cases():
        n = len(a)
        rs = [keys.seek(a, k[:P]) for k in a[::2]] + [(0, n), (1, n - 1), (n // 2, n + 3), (2, 2)]
        rs += [keys.seek(a, k) for k in a[:5]]  # a whole key: its row alone, emitted only when it is its object's last
        for reverse in (False, True):
            for limit in (0, 1, 2):
                got = keys.scan(a, rs, reverse=reverse, limit=limit, latest=True)
                assert got == brute(a, rs, reverse, limit, latest=True), (a, rs, reverse, limit)
                rows += len(got)
        whole = keys.scan(a, [(0, n)], latest=True)
        assert [a[p][:P] for _, p in whole] == sorted({k[:P] for k in a})  # every object once
        for _, p in whole:
            assert a[p] == max(k for k in a if k[:P] == a[p][:P])  # at its greatest version
        # a range that ends inside an object omits that object
        for q, p in whole:
            pos, end = keys.seek(a, a[p][:P])
            if end - pos > 1:
                assert keys.scan(a, [(pos, end - 1)], latest=True) == []
    assert rows >= 500
    # short keys too: the group is the key itself when it is shorter than the prefix
    for a, b in random_cases(cases=50, seed=5):
        rs = ranges_of(a, b)
        assert keys.scan(a, rs, latest=True) == brute(a, rs, latest=True)


def test_reverse_limit_one_is_the_seeks_last_row():
    """Retrieve's "latest version" (collection.go:97-104): the row at end - 1."""
    hits = 0
    for a, b in random_cases(seed=97):
        for probe in [k for k in b[:8]] + [k[:1] for k in b[:8]]:
            pos, end = keys.seek(a, probe)
            got = keys.scan(a, [keys.seek(a, probe)], reverse=True, limit=1)
            assert got == ([(0, end - 1)] if end > pos else [])
            hits += len(got)
    assert hits >= 100


def test_empty_repeated_and_overlapping_ranges():
    a = sorted(bytes([i]) for i in range(10))
    assert keys.scan(a, []) == []
    assert keys.scan([], [(0, 5), (0, 0)]) == []
    assert keys.scan(a, [(4, 4), (7, 3), (10, 12)]) == []
    assert keys.scan(a, [(2, 4), (2, 4)]) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    got = keys.scan(a, [(5, 8), (0, 10), (6, 7), (4, 4), (7, 20)], reverse=True, limit=2)
    assert got == [(0, 7), (0, 6), (1, 9), (1, 8), (2, 6), (4, 9), (4, 8)]
    assert len(keys.scan(a, [(0, 10)] * 3)) == 30  # more rows than the list has


def test_library_exports_the_entry_point():
    assert "honu_key_list" in _lib.EXPORTS and "honu_sizeof_list_row" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "honu_key_list")
    assert int(lib.honu_sizeof_list_row()) == 16


def test_row_dtype_matches_the_struct():
    from honu_amd.metadata import LIST_ROW_DTYPE
    assert LIST_ROW_DTYPE.itemsize == int(_lib.load().honu_sizeof_list_row())
    assert LIST_ROW_DTYPE.names == ("range", "pos", "record", "flags")


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_list(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E_ARG
