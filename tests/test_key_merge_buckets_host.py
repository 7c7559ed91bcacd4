"""keys.merge_buckets, the host statement of honu_key_merge_buckets (a routed
batch of Puts into every collection's bucket at once): by hand, and against
keys.merge bucket by bucket over random buckets with empty A buckets, empty B
buckets, buckets empty on both sides and valid counts below a bucket's rows.
"""
import numpy as np
import pytest

from honu_amd import _lib, keys


def key(oid, vid=1, pid=1):
    return keys.new(bytes([oid]) * 16, keys.Scalar(PID=pid, VID=vid))


def test_by_hand():
    k1, k2, k3, k4 = key(1), key(2), key(3), key(4)
    a = [[k1, k3], [], [k2, k2, k4], []]
    b = [[k2, k3], [k1], [], []]
    got = keys.merge_buckets(a, b)
    assert got == [
        [(k1, 0, 0), (k2, 1, 0), (k3, 0, 1), (k3, 1, 1)],  # on equal keys a's row first
        [(k1, 1, 0)],                                      # a's bucket empty
        [(k2, 0, 0), (k2, 0, 1), (k4, 0, 2)],              # b's bucket empty
        [],                                                # both
    ]
    assert all(isinstance(r, keys.BucketRow) and r.key == r[0] for rows in got for r in rows)
    # counts: the first min(count, rows) rows of a's bucket are valid, the rest are dropped
    got = keys.merge_buckets(a, b, counts=[1, 5, 2, 0])
    assert got == [[(k1, 0, 0), (k2, 1, 0), (k3, 1, 1)], [(k1, 1, 0)], [(k2, 0, 0), (k2, 0, 1)], []]
    assert keys.merge_buckets([], []) == []
    with pytest.raises(ValueError):
        keys.merge_buckets([[k1]], [])
    with pytest.raises(ValueError):
        keys.merge_buckets([[k1]], [[k2]], counts=[])


def random_bucket(rng, pool, n):
    return sorted(pool[int(j)] for j in rng.integers(0, len(pool), n))


@pytest.mark.parametrize("seed", range(4))
def test_against_merge_bucket_by_bucket(seed):
    rng = np.random.default_rng(8800 + seed)
    pool = [bytes(rng.integers(0, 256, 29, dtype=np.uint8)) for _ in range(40)]  # few keys: ties within and across
    k = 23
    kind = rng.integers(0, 4, k)  # 0: both sides, 1: A empty, 2: B empty, 3: both empty
    kind[:4] = (0, 1, 2, 3)
    a = [random_bucket(rng, pool, 0 if kind[c] in (1, 3) else int(rng.integers(1, 30))) for c in range(k)]
    b = [random_bucket(rng, pool, 0 if kind[c] in (2, 3) else int(rng.integers(1, 30))) for c in range(k)]
    for counts in (None, [len(x) for x in a], [len(x) + 3 for x in a], [len(x) * 4 // 5 for x in a], [0] * k):
        got = keys.merge_buckets(a, b, counts)
        assert len(got) == k
        for c in range(k):
            va = len(a[c]) if counts is None else min(counts[c], len(a[c]))
            assert [r.key for r in got[c]] == keys.merge(a[c][:va], b[c])
            assert len(got[c]) == va + len(b[c])
            # every row is the row it names; each side keeps its order; a's rows before b's on equal keys
            for r in got[c]:
                assert r.key == (a[c] if r.side == 0 else b[c])[r.index]
            assert [r.index for r in got[c] if r.side == 0] == list(range(va))
            assert [r.index for r in got[c] if r.side == 1] == list(range(len(b[c])))
            for x, y in zip(got[c], got[c][1:]):
                assert x.key < y.key or (x.key == y.key and x.side <= y.side)
    assert any(counts_cut for counts_cut in [len(x) * 4 // 5 < len(x) for x in a])


def test_the_export_and_its_refusal_without_a_context():
    assert "honu_key_merge_buckets" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "honu_key_merge_buckets")
    assert lib.honu_key_merge_buckets(None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == -1
