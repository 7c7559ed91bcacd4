"""keys.merge, the host statement of honu_key_merge (a batch of Puts into the
sorted key list: store.go:232, 395, 530; cursor_test.go:235), against a stable
sort of the tagged concatenation; what keys.seek sees afterwards; and the
entry point's presence and first refusal, which need no device.

keys.merge returns the objects it was given, so a row is a bytes subclass that
remembers its side and its index there: where a row of the result came from is
read off the row, not inferred."""
import numpy as np

from honu_amd import _lib, keys

E_ARG = -1
ALPHABET = (b"\x00", b"\x01", b"\x7f", b"\x80", b"\xff")
A, B = 0, 1


class Row(bytes):
    side = index = None


def tag(keys_, side):
    out = []
    for i, k in enumerate(keys_):
        r = Row(k)
        r.side, r.index = side, i
        out.append(r)
    return out


def random_cases(cases=200, max_len=40, seed=232):
    """(a, b): sorted lists of tagged short keys over a small alphabet, so ties are common."""
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        sides = []
        for side, n in enumerate(rng.integers(0, max_len + 1, 2)):
            ks = [b"".join(ALPHABET[c] for c in rng.integers(0, len(ALPHABET), int(rng.integers(1, 3))))
                  for _ in range(int(n))]
            sides.append(tag(sorted(ks), side))
        yield tuple(sides)


def where(rows):
    return [(bytes(r), r.side, r.index) for r in rows]


def test_merge_is_the_stable_sort_of_the_tagged_concatenation():
    ties = 0
    for a, b in random_cases():
        # key, then side (A first), then the side's own order
        assert where(keys.merge(a, b)) == sorted(where(a) + where(b)), (a, b)
        ties += len(set(a) & set(b))
    assert ties > 100  # the alphabet is small enough that the tie rule is exercised


def test_a_rows_precede_b_rows_in_every_run():
    for a, b in random_cases(seed=395):
        merged = keys.merge(a, b)
        for key in set(merged):
            pos, end = keys.seek(merged, key)
            run = [r for r in merged[pos:end] if r == key]
            na = sum(r.side == A for r in run)
            assert all(r.side == A for r in run[:na]) and all(r.side == B for r in run[na:]), (key, where(run))
            for part in (run[:na], run[na:]):  # each side's own order is kept
                assert [r.index for r in part] == sorted(r.index for r in part)
            assert na == a.count(key) and len(run) - na == b.count(key)


def test_an_empty_side_is_the_identity():
    for a, b in random_cases(cases=20, seed=530):
        assert where(keys.merge(a, [])) == where(a)
        assert where(keys.merge([], b)) == where(b)
    assert keys.merge([], []) == []


def test_seek_finds_every_key_of_both_sides():
    for a, b in random_cases(cases=50, seed=235):
        merged = keys.merge(a, b)
        for k in a + b:
            pos, end = keys.seek(merged, k)
            assert pos < end and merged[pos].startswith(k) and keys.has(merged, k)
            assert merged[pos:end].count(k) == a.count(k) + b.count(k)


def test_the_last_row_of_a_shared_keys_run_is_the_batchs():
    """bbolt's Put of a stored key replaces its value: the run's last row is
    the batch's (B's), which is what honu_seek.latest returns."""
    rng = np.random.default_rng(7)
    rows = [bytes(r) for r in rng.integers(0, 256, (60, 29), dtype=np.uint8)]
    a, b = tag(sorted(rows[:40]), A), tag(sorted(rows[30:] + rows[35:40]), B)  # rows 30..39 in both, 35..39 twice in B
    merged = keys.merge(a, b)
    shared = set(a) & set(b)
    assert len(shared) == 10
    for k in shared:
        pos, end = keys.seek(merged, k)
        assert end - pos == 2 + (k in rows[35:40])
        assert merged[pos].side == A and merged[end - 1].side == B
        assert merged[end - 1].index == max(r.index for r in b if r == k)  # and B's latest at that
    for k in set(a) - shared:
        pos, end = keys.seek(merged, k)
        assert end - pos == 1 and merged[pos].side == A


def test_library_exports_the_entry_point():
    assert "honu_key_merge" in _lib.EXPORTS
    assert hasattr(_lib.load(), "honu_key_merge")


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_merge(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E_ARG
