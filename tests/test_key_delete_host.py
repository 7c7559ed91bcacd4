"""keys.delete and keys.compact, the host statement of honu_key_delete (the
loop "Delete all collection versions" of Store.Drop, store.go:378-383, its
DeleteBucket, store.go:399-404, and the row a Put of a stored key replaces),
against a brute-force list comprehension; what keys.seek sees afterwards; and
the entry point's presence, first refusal and workspace size, which need no
device.

Both functions return the objects they were given, so a row is a bytes
subclass that remembers its side and its index there (as in
tests/test_key_merge_host.py): where a row of the result came from is read off
the row, not inferred."""
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
    """(a, b): sorted lists of tagged short keys over a small alphabet, so prefixes and ties are common."""
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        sides = []
        for side, n in enumerate(rng.integers(0, max_len + 1, 2)):
            ks = [b"".join(ALPHABET[c] for c in rng.integers(0, len(ALPHABET), int(rng.integers(1, 3))))
                  for _ in range(int(n))]
            sides.append(tag(sorted(ks), side))
        yield tuple(sides)


def ids(rows):
    return [id(r) for r in rows]


def test_delete_is_the_brute_force_prefix_filter():
    kept_n = removed_n = 0
    for a, b in random_cases():
        probes = [bytes(k) for k in b[::3]]  # one or two bytes: whole keys and proper prefixes of a's
        kept, removed = keys.delete(a, probes)
        gone = [any(k.startswith(p) for p in probes) for k in a]
        assert ids(kept) == ids([k for k, g in zip(a, gone) if not g]), (a, probes)
        assert ids(removed) == ids([k for k, g in zip(a, gone) if g]), (a, probes)
        assert sorted(ids(kept + removed)) == sorted(ids(a))  # a permutation of the objects given
        for p in probes:  # nothing with the prefix is left
            pos, end = keys.seek(kept, p)
            assert pos == end and not keys.has(kept, p)
        kept_n += len(kept)
        removed_n += len(removed)
    assert kept_n >= 100 and removed_n >= 100  # the rule is exercised both ways


def test_compact_keeps_the_last_row_of_every_run():
    kept_n = removed_n = 0
    for a, _ in random_cases(seed=395):
        kept, removed = keys.compact(a)
        gone = [any(bytes(x) == bytes(k) for x in a[p + 1:]) for p, k in enumerate(a)]
        assert ids(kept) == ids([k for k, g in zip(a, gone) if not g])
        assert ids(removed) == ids([k for k, g in zip(a, gone) if g])
        assert sorted(ids(kept + removed)) == sorted(ids(a))
        assert [bytes(k) for k in kept] == sorted(set(bytes(k) for k in a))
        for k in kept:  # every stored key once: end - pos counts the stored keys again
            pos, end = keys.seek(kept, k)
            assert sum(bytes(x) == bytes(k) for x in kept[pos:end]) == 1
        kept_n += len(kept)
        removed_n += len(removed)
    assert kept_n >= 100 and removed_n >= 100


def test_an_absent_probe_removes_nothing():
    for a, _ in random_cases(cases=20, seed=530):
        for probes in ([b"\x02"], [b"\x00\x02", b"\xff\xff\xff"], []):
            kept, removed = keys.delete(a, probes)
            assert ids(kept) == ids(a) and removed == []
    assert keys.delete([], [b"\x00"]) == ([], [])


def test_the_empty_probe_removes_all():
    """tx.DeleteBucket (store.go:399-404)."""
    for a, _ in random_cases(cases=20, seed=402):
        kept, removed = keys.delete(a, [b""])
        assert kept == [] and ids(removed) == ids(a)
    assert keys.compact([]) == ([], [])


def test_duplicate_and_nested_probes():
    a = tag(sorted([b"\x00", b"\x00\x01", b"\x00\x01", b"\x01", b"\x01\x7f", b"\x7f"]), A)
    kept, removed = keys.delete(a, [b"\x00\x01", b"\x00", b"\x00\x01", b"\x01\x7f"])
    assert [bytes(k) for k in kept] == [b"\x01", b"\x7f"]
    assert [r.index for r in removed] == [0, 1, 2, 4]


def test_compact_after_merge_keeps_the_batchs_row():
    """bbolt's Put of a stored key replaces its value: of a key in both sides
    the batch's (B's) last row stays."""
    rng = np.random.default_rng(7)
    rows = [bytes(r) for r in rng.integers(0, 256, (60, 29), dtype=np.uint8)]
    a, b = tag(sorted(rows[:40]), A), tag(sorted(rows[30:] + rows[35:40]), B)  # rows 30..39 in both, 35..39 twice in B
    merged = keys.merge(a, b)
    kept, removed = keys.compact(merged)
    assert len(kept) == 60 and len(removed) == 15
    shared = set(a) & set(b)
    assert len(shared) == 10
    for k in kept:
        pos, end = keys.seek(kept, k)
        assert end - pos == 1
        if k in shared:
            assert k.side == B and k.index == max(r.index for r in b if r == k)
        else:
            assert k.side == (A if k in set(a) else B)
    assert sum(r.side == A for r in removed) == 10 and sum(r.side == B for r in removed) == 5


def test_the_drop_loop_selects_what_delete_removes():
    """store.go:378-383 as it is stated: Seek(id), then walk while HasPrefix."""
    n = 0
    for a, b in random_cases(cases=100, seed=378):
        for probe in [bytes(k)[:1] for k in b[:4]] + [bytes(k) for k in b[:4]]:
            pos, _ = keys.seek(a, probe)
            walked = []
            while pos < len(a) and a[pos].startswith(probe):
                walked.append(a[pos])
                pos += 1
            kept, removed = keys.delete(a, [probe])
            assert ids(walked) == ids(removed)
            n += len(walked)
    assert n >= 100


def test_library_exports_the_entry_point():
    assert "honu_key_delete" in _lib.EXPORTS and "honu_key_delete_workspace" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "honu_key_delete") and hasattr(lib, "honu_key_delete_workspace")


def test_null_ctx_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.honu_key_delete(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E_ARG


def test_workspace_is_a_multiple_of_256_and_monotonic():
    lib = _lib.load()
    sizes = [int(lib.honu_key_delete_workspace(n)) for n in
             (0, 1, 2, 1023, 1024, 1025, 4105, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 32) - 1)]
    assert all(s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[1] > 0 and sizes[-1] > sizes[1]
    # no per-row column: a keep bit per row and a count per tile are under one byte per key at 1M keys
    assert sizes[7] < 1 << 20
