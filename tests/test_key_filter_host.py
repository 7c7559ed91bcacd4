"""keys.filter, the host statement of honu_key_filter (an object deleted with a
tombstone version "will not be returned in list queries or retrieval",
collection.go:132-134; Retrieve of it "not found", collection.go:97-101), against
a brute force that asks of every visit whether it stays, on the random cases
and ranges of tests/test_key_list_host.py; and the entry points' presence, the
workspace size and the first refusal, which need no device."""
import numpy as np

from honu_amd import _lib, keys
from test_key_list_host import long_cases, random_cases, ranges_of

E_ARG = -1
P = keys.PREFIX_SIZE


def brute_stays(a, visits, dead, order=None, deleted=False):
    """The visits that stay. dead: the set of tombstone record indices. With
    `deleted` a visit is judged by the greatest position of the same object."""
    n = len(a)
    out = []
    for q, p in visits:
        last = max(x for x in range(n) if a[x][:P] == a[p][:P]) if deleted and 0 <= p < n else p
        r = last if order is None else (order[last] if 0 <= last < n else None)
        if not (0 <= p < n and r in dead):
            out.append((q, p))
    return out


def cases_with_tombstones(seed=71):
    """(keys, ranges, order, tombstone set) over the short-key and the 29-byte cases."""
    rng = np.random.default_rng(seed)
    lists = [(a, ranges_of(a, b)) for a, b in random_cases(cases=120, seed=seed)]
    for a in long_cases(cases=60, seed=seed + 1):
        n = len(a)
        lists.append((a, [keys.seek(a, k[:P]) for k in a[::2]] + [(0, n), (1, n - 1), (n // 2, n + 3), (2, 2)]))
    for a, rs in lists:
        n = len(a)
        order = rng.permutation(n).tolist()
        for share in (0.0, 0.3, 1.0):
            dead = {r for r in range(n) if rng.random() < share}
            yield a, rs, order, dead


def test_filter_is_the_brute_force():
    seen = kept = 0
    for a, rs, order, dead in cases_with_tombstones():
        tomb = dead.__contains__
        for visits in (keys.scan(a, rs), keys.scan(a, rs, reverse=True, limit=2), keys.scan(a, rs, latest=True)):
            for od in (order, None):
                rows = keys.filter(a, visits, tomb, od)
                objs = keys.filter(a, visits, tomb, od, deleted=True)
                assert rows == brute_stays(a, visits, dead, od), (a, rs, od, dead)
                assert objs == brute_stays(a, visits, dead, od, deleted=True), (a, rs, od, dead)
                # both rules: one after the other, in either order
                both = [v for v in visits if v in set(rows) and v in set(objs)]
                assert keys.filter(a, rows, tomb, od, deleted=True) == both
                assert keys.filter(a, objs, tomb, od) == both
                seen += len(visits)
                kept += len(rows)
    assert seen >= 20000 and 0 < kept < seen


def test_no_tombstone_keeps_and_all_tombstones_empty_the_list():
    for a, b in random_cases(cases=30, seed=9):
        visits = keys.scan(a, ranges_of(a, b))
        for deleted in (False, True):
            assert keys.filter(a, visits, lambda r: False, deleted=deleted) == visits
            assert keys.filter(a, visits, lambda r: True, deleted=deleted) == []


def versions(oid, count):
    return [keys.new(bytes([oid]) * 16, keys.Scalar(PID=1, VID=v + 1)) for v in range(count)]


def test_a_tombstone_in_the_middle_of_a_history_stays_whole_under_deleted():
    a = keys.sort(versions(1, 3) + versions(2, 5) + versions(3, 2))
    order = list(range(len(a)))[::-1]  # position p holds record n - 1 - p
    n = len(a)
    mid = 3 + 2  # object 2's third version
    dead = {order[mid]}
    visits = keys.scan(a, [keys.seek(a, a[mid][:P]), (0, n)], reverse=True)
    assert keys.filter(a, visits, dead.__contains__, order, deleted=True) == visits  # Versions() includes it
    assert keys.filter(a, visits, dead.__contains__, order) == [v for v in visits if v[1] != mid]


def test_an_object_whose_latest_is_a_tombstone_goes_whole():
    a = keys.sort(versions(1, 3) + versions(2, 5) + versions(3, 2))
    n = len(a)
    order = list(range(n))
    dead = {7}  # object 2's latest version, position 3 + 5 - 1
    whole = keys.scan(a, [(0, n)])
    assert keys.filter(a, whole, dead.__contains__, order, deleted=True) == [(0, p) for p in (0, 1, 2, 8, 9)]
    assert keys.filter(a, whole, dead.__contains__, order) == [(0, p) for p in range(n) if p != 7]
    # a range that sees only the older half of the object: still judged by the column's latest row
    older = keys.scan(a, [(3, 5)])
    assert keys.filter(a, older, dead.__contains__, order, deleted=True) == []
    assert keys.filter(a, older, dead.__contains__, order) == older
    # Retrieve: the range of the deleted object comes out empty
    retrieve = keys.scan(a, [keys.seek(a, k[:P]) for k in (a[0], a[3], a[8])], reverse=True, limit=1)
    assert retrieve == [(0, 2), (1, 7), (2, 9)]
    assert keys.filter(a, retrieve, dead.__contains__, order) == [(0, 2), (2, 9)]


def test_a_position_outside_the_list_stays():
    a = keys.sort(versions(1, 2))
    assert keys.filter(a, [(0, 2), (0, 7), (1, -1)], lambda r: True) == [(0, 2), (0, 7), (1, -1)]
    assert keys.filter(a, [(0, 1), (0, 2)], lambda r: True, order=[0], deleted=False) == [(0, 1), (0, 2)]
    assert keys.filter([], [(0, 0)], lambda r: True, deleted=True) == [(0, 0)]


def test_library_exports_the_entry_points():
    assert "honu_key_filter" in _lib.EXPORTS and "honu_key_filter_workspace" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "honu_key_filter") and hasattr(lib, "honu_key_filter_workspace")


def test_flags_match_the_header():
    from honu_amd.metadata import FILTER_DELETED, FILTER_TOMBSTONE
    assert (FILTER_TOMBSTONE, FILTER_DELETED) == (1, 2)


def test_workspace_is_whole_256_byte_units_and_monotone():
    lib = _lib.load()
    assert int(lib.honu_key_filter_workspace(0)) % 256 == 0
    sizes = [int(lib.honu_key_filter_workspace(c)) for c in
             (0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 1 << 20, (1 << 20) + 1, (1 << 32) - 1)]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[1] > 0
    # of the order of 136 bytes per 1024 rows
    assert sizes[10] <= 2 * 136 * (1 << 10)


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_filter(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E_ARG
