"""keys.next, the host statement of honu_key_next, and the parts of the ABI
that need no device.

pid_next against the literals of lamport/pid_test.go. keys.next against an
independent sequential simulation: a bucket that is a sorted list of (key,
tombstone) pairs of its own; for each request in turn it seeks the object, acts
as the Go call would (Create, Update, Merge, Delete as collection.go:75-137
document them, Tombstone() as metadata/collection.go:56-63 has it), and puts
the new key into the bucket with bisect, so that the next request meets it
there. It shares no code with keys.next but keys.new.
"""
import bisect
import os
import subprocess

import numpy as np
import pytest

from honu_amd import _lib
from honu_amd import keys as hkeys
from honu_amd.metadata import (NEXT_ASSIGNED, NEXT_BAD_KEY, NEXT_CREATE, NEXT_DELETE, NEXT_DTYPE, NEXT_EXISTS,
                               NEXT_FOUND, NEXT_HAS_PARENT, NEXT_LIVE, NEXT_MERGE, NEXT_NOT_FOUND, NEXT_SKIPPED,
                               NEXT_TOMBSTONE, NEXT_UPDATE, NEXT_WRAPPED, Scalar, pid_next)

OPS = (NEXT_CREATE, NEXT_UPDATE, NEXT_MERGE, NEXT_DELETE)
M64 = (1 << 64) - 1


# --------------------------------------------------------------------------
# lamport.PID.Next / lamport.Next
# --------------------------------------------------------------------------
def test_pid_next_literals():
    """lamport/pid_test.go:12-14 and 30-31."""
    assert pid_next(42, None) == Scalar(42, 1)
    assert pid_next(42, Scalar()) == Scalar(42, 1)
    assert pid_next(42, Scalar(42, 18)) == Scalar(42, 19)
    assert pid_next(7, None) == Scalar(7, 1)
    assert pid_next(7, Scalar(7, 18)) == Scalar(7, 19)


def test_pid_next_wraps_as_uint64():
    assert pid_next(3, Scalar(9, M64)) == Scalar(3, 0)
    assert pid_next(3, Scalar(9, M64 - 1)) == Scalar(3, M64)


# --------------------------------------------------------------------------
# the sequential simulation
# --------------------------------------------------------------------------
def simulate(sorted_keys, tombs, requests, op, pid, skip=None):
    """(flags of the write, scalar or None, parent or None, key) per request,
    the bucket changing under the requests. The flags are those a single Go
    call could report: ASSIGNED, HAS_PARENT, TOMBSTONE, NOT_FOUND, EXISTS,
    BAD_KEY, SKIPPED."""
    bucket = list(zip(sorted_keys, tombs))
    out = []
    for i, req in enumerate(requests):
        prefix = bytes(req[:17])
        blank = prefix + bytes(12)
        if skip is not None and skip[i]:
            out.append((NEXT_SKIPPED, None, None, blank))
            continue
        if prefix[0] != 1:
            out.append((NEXT_BAD_KEY, None, None, blank))
            continue
        lo = bisect.bisect_left(bucket, (prefix,))
        hi = lo
        while hi < len(bucket) and bucket[hi][0][:17] == prefix:
            hi += 1
        exists = hi > lo
        latest = tomb = None
        if exists:
            k, tomb = bucket[hi - 1]
            latest = Scalar(PID=int.from_bytes(k[25:29], "big"), VID=int.from_bytes(k[17:25], "big"))
        if op == NEXT_CREATE:
            if exists:
                out.append((NEXT_EXISTS, None, None, blank))
                continue
            new, parent = Scalar(0, 1), None
        elif op == NEXT_MERGE or (exists and not tomb):
            new, parent = Scalar(pid, latest.VID + 1 if exists else 1), latest
        else:
            out.append((NEXT_NOT_FOUND, None, None, blank))
            continue
        key = hkeys.new(prefix[1:], new)
        bisect.insort(bucket, (key, op == NEXT_DELETE))
        flags = NEXT_ASSIGNED | (NEXT_HAS_PARENT if parent else 0) | (NEXT_TOMBSTONE if op == NEXT_DELETE else 0)
        out.append((flags, new, parent, key))
    return out


WRITE_FLAGS = (NEXT_ASSIGNED | NEXT_HAS_PARENT | NEXT_TOMBSTONE | NEXT_NOT_FOUND | NEXT_EXISTS | NEXT_BAD_KEY |
               NEXT_SKIPPED)


def agree(got, sim, sorted_keys, tombs):
    assert len(got) == len(sim)
    for i, (g, (flags, scalar, parent, key)) in enumerate(zip(got, sim)):
        assert g.flags & WRITE_FLAGS == flags, (i, g, flags)
        assert g.scalar == scalar and g.parent == parent and g.key == key, (i, g, scalar, parent)
        assert not g.flags & NEXT_WRAPPED
        if g.parent_pos is not None:  # the stored row that is the parent
            assert hkeys.version(sorted_keys[g.parent_pos]) == parent
            assert sorted_keys[g.parent_pos][:17] == key[:17]
        if flags & (NEXT_BAD_KEY | NEXT_SKIPPED):
            assert g.flags == flags
            continue
        pos, end = hkeys.seek(sorted_keys, key[:17])
        assert bool(g.flags & NEXT_FOUND) == (pos < end)
        assert bool(g.flags & NEXT_LIVE) == (pos < end and not tombs[end - 1])


def random_column(rng, objects, max_versions, with_ff=True):
    """A sorted column of `objects` objects with 1..max_versions versions each,
    a tombstone bit per key (some objects' latest version is one), and the
    object IDs (stored and a few that are not)."""
    oids = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(objects + 4)]
    if with_ff:
        oids[0] = oids[0][:15] + b"\xff"
        oids[-1] = b"\xff" * 16
    col = []
    for oid in oids[:objects]:
        vids = rng.choice(1000, size=int(rng.integers(1, max_versions + 1)), replace=False) + 1
        col += [(hkeys.new(oid, Scalar(int(rng.integers(0, 5)), int(v))), bool(rng.integers(0, 3) == 0)) for v in vids]
    col.sort()
    sorted_keys, tombs = [k for k, _ in col], [t for _, t in col]
    tombs[hkeys.seek(sorted_keys, b"\x01" + oids[1])[1] - 1] = True   # object 1 is deleted,
    tombs[hkeys.seek(sorted_keys, b"\x01" + oids[2])[1] - 1] = False  # object 2 is not
    return sorted_keys, tombs, oids


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("seed", range(4))
def test_next_equals_the_sequential_simulation(op, seed):
    rng = np.random.default_rng(seed)
    sorted_keys, tombs, oids = random_column(rng, 12, 5)
    pick = rng.integers(0, len(oids), 90)  # few objects, many requests: long runs, interleaved
    requests = [b"\x01" + oids[j] + bytes(rng.integers(0, 256, 12, dtype=np.uint8)) for j in pick]
    for i in (5, 30, 31):
        requests[i] = bytes([int(rng.integers(2, 256))]) + requests[i][1:]  # Key.Check fails
    requests[40] = b"\x00" + requests[40][1:]
    skip = [bool(x) for x in rng.integers(0, 8, len(requests)) == 0]
    got = hkeys.next(sorted_keys, requests, op, 9, live=lambda p: not tombs[p], skip=skip)
    agree(got, simulate(sorted_keys, tombs, requests, op, 9, skip), sorted_keys, tombs)
    flags = [g.flags for g in got]
    assert any(f & NEXT_ASSIGNED for f in flags) and any(f & NEXT_SKIPPED for f in flags)
    assert sum(f == NEXT_BAD_KEY for f in flags) >= 1
    if op in (NEXT_UPDATE, NEXT_DELETE):
        assert any(f & NEXT_NOT_FOUND and f & NEXT_FOUND for f in flags)  # a deleted object
        assert any(f & NEXT_NOT_FOUND and not f & NEXT_FOUND for f in flags)  # an absent one
    if op == NEXT_CREATE:
        assert any(f & NEXT_EXISTS and not f & NEXT_FOUND for f in flags)  # made by an earlier request


@pytest.mark.parametrize("op", OPS)
def test_without_live_every_stored_object_is_live(op):
    rng = np.random.default_rng(10)
    sorted_keys, tombs, oids = random_column(rng, 6, 3)
    requests = [b"\x01" + oids[j] for j in rng.integers(0, len(oids), 40)]
    got = hkeys.next(sorted_keys, requests, op, 2)
    agree(got, simulate(sorted_keys, [False] * len(tombs), requests, op, 2), sorted_keys, [False] * len(tombs))


def test_empty_column_and_no_requests():
    assert hkeys.next([], [], NEXT_MERGE, 1) == []
    oid = bytes(range(16))
    got = hkeys.next([], [b"\x01" + oid] * 3, NEXT_MERGE, 4)
    assert [g.scalar for g in got] == [Scalar(4, 1), Scalar(4, 2), Scalar(4, 3)]
    assert [g.parent for g in got] == [None, Scalar(4, 1), Scalar(4, 2)]
    assert [g.parent_pos for g in got] == [None] * 3
    got = hkeys.next([], [b"\x01" + oid] * 2, NEXT_CREATE, 4)
    assert got[0].scalar == Scalar(0, 1) and got[0].flags == NEXT_ASSIGNED and got[1].flags == NEXT_EXISTS
    with pytest.raises(ValueError):
        hkeys.next([], [], 4, 1)


def test_the_table_on_one_object():
    """The closed form of the issue's table: rank r of an object with stored latest (P, V)."""
    oid = bytes(range(1, 17))
    col = [hkeys.new(oid, Scalar(3, 5)), hkeys.new(oid, Scalar(8, 20))]
    other = b"\x01" + bytes(16)
    reqs = [b"\x01" + oid, other, b"\x01" + oid, b"\x02" + oid, b"\x01" + oid]
    up = hkeys.next(col, reqs, NEXT_UPDATE, 6, skip=[False, False, False, False, False])
    assert [g.scalar for g in up] == [Scalar(6, 21), None, Scalar(6, 22), None, Scalar(6, 23)]
    assert [g.parent for g in up] == [Scalar(8, 20), None, Scalar(6, 21), None, Scalar(6, 22)]
    assert [g.parent_pos for g in up] == [1, None, None, None, None]
    assert up[1].flags == NEXT_NOT_FOUND and up[3].flags == NEXT_BAD_KEY
    assert up[0].key == hkeys.new(oid, Scalar(6, 21)) and up[3].key == b"\x02" + oid + bytes(12)
    de = hkeys.next(col, reqs, NEXT_DELETE, 6)
    both = NEXT_FOUND | NEXT_LIVE
    assert [g.flags for g in de] == [NEXT_ASSIGNED | NEXT_HAS_PARENT | NEXT_TOMBSTONE | both, NEXT_NOT_FOUND,
                                     NEXT_NOT_FOUND | both, NEXT_BAD_KEY, NEXT_NOT_FOUND | both]
    assert de[0].scalar == Scalar(6, 21) and de[0].parent == Scalar(8, 20)
    dead = hkeys.next(col, reqs[:1], NEXT_UPDATE, 6, live=lambda p: p != 1)
    assert dead[0].flags == NEXT_NOT_FOUND | NEXT_FOUND
    me = hkeys.next(col, reqs[:3], NEXT_MERGE, 6, live=lambda p: False)
    assert [g.scalar for g in me] == [Scalar(6, 21), Scalar(6, 1), Scalar(6, 22)]
    assert me[0].flags == NEXT_ASSIGNED | NEXT_HAS_PARENT | NEXT_FOUND and me[1].flags == NEXT_ASSIGNED


@pytest.mark.parametrize("op", (NEXT_UPDATE, NEXT_MERGE))
def test_vid_wraps(op):
    oid = b"\xee" * 16
    req = [b"\x01" + oid] * 3
    got = hkeys.next([hkeys.new(oid, Scalar(2, M64))], req, op, 5)
    assert [g.scalar for g in got] == [Scalar(5, 0), Scalar(5, 1), Scalar(5, 2)]
    assert [g.parent for g in got] == [Scalar(2, M64), Scalar(5, 0), Scalar(5, 1)]
    assert all(g.flags & NEXT_WRAPPED for g in got)
    got = hkeys.next([hkeys.new(oid, Scalar(2, M64 - 1))], req, op, 5)
    assert [g.scalar for g in got] == [Scalar(5, M64), Scalar(5, 0), Scalar(5, 1)]
    assert [g.parent for g in got] == [Scalar(2, M64 - 1), Scalar(5, M64), Scalar(5, 0)]
    assert [bool(g.flags & NEXT_WRAPPED) for g in got] == [False, True, True]
    assert got[1].key == hkeys.new(oid, Scalar(5, 0))
    de = hkeys.next([hkeys.new(oid, Scalar(2, M64))], req, NEXT_DELETE, 5)
    assert de[0].scalar == Scalar(5, 0) and de[0].flags & NEXT_WRAPPED and de[1].flags & NEXT_NOT_FOUND


def test_object_id_ending_in_ff():
    """No ObjectLimit wrap (keys.go:88-91): the rows of ...ff end where the next object starts."""
    a, b = bytes(15) + b"\xff", bytes(14) + b"\x01\x00"
    col = sorted([hkeys.new(a, Scalar(1, 7)), hkeys.new(a, Scalar(1, 9)), hkeys.new(b, Scalar(1, 3)),
                  hkeys.new(b"\xff" * 16, Scalar(4, 11))])
    got = hkeys.next(col, [b"\x01" + a, b"\x01" + b"\xff" * 16, b"\x01" + b], NEXT_UPDATE, 2)
    assert [g.scalar for g in got] == [Scalar(2, 10), Scalar(2, 12), Scalar(2, 4)]
    assert [g.parent_pos for g in got] == [1, 3, 2]


# --------------------------------------------------------------------------
# the ABI without a device
# --------------------------------------------------------------------------
def test_sizeof_next():
    lib = _lib.load()
    assert lib.honu_sizeof_next() == NEXT_DTYPE.itemsize == 32


def test_next_offsets_match_numpy(tmp_path):
    """offsetof() of every honu_next field by the system C compiler, as tests/test_abi.py does for the other rows."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "honu_codec.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(){"]
    lines += [f'printf("{name} %zu\\n", offsetof(honu_next, {name}));' for name in NEXT_DTYPE.names]
    lines.append('printf("flags %u %u\\n", (unsigned)HONU_NEXT_WRAPPED, (unsigned)HONU_NEXT_DELETE);')
    lines.append("return 0;}")
    src = tmp_path / "off.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for name, line in zip(NEXT_DTYPE.names, out):
        assert line == f"{name} {NEXT_DTYPE.fields[name][1]}"
    assert out[-1] == f"flags {NEXT_WRAPPED} {NEXT_DELETE}"


def test_workspace_size():
    lib = _lib.load()
    assert lib.honu_key_next_workspace(0) == 0
    sizes = [int(lib.honu_key_next_workspace(m)) for m in range(5001)]
    assert all(s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # the sort's own workspace, the packed and the sorted column, the order, the status column, the count
    for m in (1, 77, 5000):
        assert sizes[m] >= int(lib.honu_sort_keys_workspace(m)) + 2 * 29 * m + 2 * 4 * m + 8


def test_exported():
    assert {"honu_key_next", "honu_key_next_workspace", "honu_sizeof_next"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "honu_key_next")
