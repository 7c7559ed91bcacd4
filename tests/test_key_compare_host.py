"""keys.compare, the host statement of honu_key_compare, metadata.scalar_compare
and the parts of the ABI that need no device.

scalar_compare against the 14 literals of lamport/scalar_test.go:94-141.
keys.compare against an independent simulation that shares no code with it but
keys.new: it parses every key into (object ID, (VID, PID)) itself, keeps a dict
of version lists per object ID and side, compares the tuples in Python, and
derives "what to send" as the versions greater than the peer's maximum.
"""
import random

from honu_amd import _lib
from honu_amd import keys as hkeys
from honu_amd.metadata import (CMP_ANCESTOR, CMP_COUNTS_DTYPE, CMP_EARLIER, CMP_EQUAL, CMP_LATER, CMP_PEER_HAS,
                               SEEK_DTYPE, SEEK_FOUND, SEEK_SKIPPED, Scalar, scalar_compare)

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
CLASSES = CMP_LATER | CMP_EARLIER | CMP_EQUAL


def oid(tail: int, head: int = 0x42) -> bytes:
    return bytes([head]) + bytes(14) + bytes([tail])


def K(tail: int, vid: int, pid: int = 0, head: int = 0x42) -> bytes:
    return hkeys.new(oid(tail, head), Scalar(PID=pid, VID=vid))


# --------------------------------------------------------------------------
# lamport.Compare
# --------------------------------------------------------------------------
def test_scalar_compare_literals():
    """lamport/scalar_test.go:94-141; Scalar{PID, VID} positionally."""
    S = Scalar
    cases = [
        (None, None, 0), (S(), S(), 0), (None, S(), 0), (S(), None, 0),
        (S(1, 1), S(), 1), (S(), S(1, 1), -1),
        (S(1, 2), S(1, 1), 1), (S(1, 1), S(1, 2), -1), (S(1, 1), S(1, 1), 0),
        (S(2, 1), S(1, 1), 1), (S(1, 1), S(2, 1), -1), (S(2, 2), S(2, 2), 0),
        (S(4, 4), S(4, 9), -1), (S(1, 10), S(10, 10), -1),
    ]
    assert len(cases) == 14
    for i, (a, b, want) in enumerate(cases):
        assert scalar_compare(a, b) == want, i
        assert scalar_compare(b, a) == -want, i


def test_key_order_is_scalar_compare():
    """keys.go:35-36: the order of two keys of one object is lamport.Compare of their versions."""
    vs = [Scalar(p, v) for v in (0, 1, 2, 255, 256, M64 - 1, M64) for p in (0, 1, 10, 256, M32)]
    for x in vs:
        for y in vs:
            kx, ky = hkeys.new(oid(7), x), hkeys.new(oid(7), y)
            assert (kx > ky) - (kx < ky) == scalar_compare(x, y)


# --------------------------------------------------------------------------
# the simulation
# --------------------------------------------------------------------------
def parse(key):
    key = bytes(key)
    assert len(key) == 29 and key[0] == 1
    return key[1:17], (int.from_bytes(key[17:25], "big"), int.from_bytes(key[25:29], "big"))


def by_object(column):
    d = {}
    for key in column:
        i, v = parse(key)
        d.setdefault(i, []).append(v)
    return d


def simulate(a, b):
    """Per object ID of a, ascending: (id, class, peer has, ancestor, versions to send, mine, peer's or None)."""
    A, B = by_object(a), by_object(b)
    out = []
    for i in sorted(A):
        mine = max(A[i])
        if i not in B:
            out.append((i, "later", False, False, sorted(A[i]), mine, None))
            continue
        theirs = max(B[i])
        send = sorted(v for v in A[i] if v > theirs)
        if mine > theirs:
            out.append((i, "later", True, theirs in A[i], send, mine, theirs))
        elif mine < theirs:
            out.append((i, "earlier", True, mine in B[i], send, mine, theirs))
        else:
            out.append((i, "equal", True, True, send, mine, theirs))
    return out


def check(a, b):
    a, b = sorted(a), sorted(b)
    got = hkeys.compare(a, b)
    want = simulate(a, b)
    assert len(got) == len(want)
    prev_end = 0
    for g, (i, cls, has, anc, send, mine, theirs) in zip(got, want):
        assert g.flags & SEEK_SKIPPED == 0
        assert bin(g.flags & CLASSES).count("1") == 1
        assert g.flags & CLASSES == {"later": CMP_LATER, "earlier": CMP_EARLIER, "equal": CMP_EQUAL}[cls]
        assert bool(g.flags & CMP_PEER_HAS) == has
        assert bool(g.flags & CMP_ANCESTOR) == anc
        assert bool(g.flags & SEEK_FOUND) == (g.pos < g.end) == bool(send)
        assert g.flags & ~(SEEK_FOUND | CMP_PEER_HAS | CLASSES | CMP_ANCESTOR) == 0
        # end: one past the object's latest row; the objects tile a
        assert prev_end <= g.pos <= g.end <= len(a)
        assert all(parse(k)[0] == i for k in a[prev_end:g.end])
        assert g.end == len(a) or parse(a[g.end])[0] != i
        assert parse(a[g.end - 1]) == (i, mine)
        prev_end = g.end
        # [pos, end): the versions greater than the peer's maximum, duplicates included
        assert [parse(k)[1] for k in a[g.pos:g.end]] == send
        if has:
            assert parse(b[g.peer]) == (i, theirs)
            assert g.peer + 1 == len(b) or b[g.peer + 1] != b[g.peer]  # the last row of the peer's latest run
        else:
            assert g.peer is None
    assert prev_end == len(a)
    return got


IDS = [oid(t, h) for h in (0x00, 0x42, 0xFF) for t in (0x00, 0x01, 0xFE, 0xFF)] + [bytes(16), bytes([0xFF] * 16)]
VIDS = (0, 1, 2, 3, M64 - 1, M64)
PIDS = (0, 1, 10, M32)


def random_column(rng, digest=False):
    col = []
    for i in rng.sample(IDS, rng.randrange(len(IDS) + 1)):
        vs = [Scalar(rng.choice(PIDS), rng.choice(VIDS)) for _ in range(rng.randrange(1, 6))]
        if digest:
            vs = [max(vs, key=lambda s: (s.VID, s.PID))]
        for s in vs:
            col.extend([hkeys.new(i, s)] * rng.choice((1, 1, 1, 2, 3)))
    return col


def test_compare_random_against_simulation():
    rng = random.Random(20261021)
    seen = set()
    for r in range(3000):
        a = random_column(rng)
        if r % 3 == 0 and a:  # a peer derived from a: shared history
            b = [k for k in a if rng.random() < 0.6] + random_column(rng)[:rng.randrange(4)]
        else:
            b = random_column(rng, digest=r % 5 == 1)
        for g in check(a, b):
            seen.add(g.flags)
    for cls in (CMP_LATER, CMP_EARLIER):
        assert cls | CMP_PEER_HAS in {f & ~SEEK_FOUND for f in seen}
        assert cls | CMP_PEER_HAS | CMP_ANCESTOR in {f & ~SEEK_FOUND for f in seen}
    assert CMP_LATER in {f & ~SEEK_FOUND for f in seen}
    assert CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR in seen


# --------------------------------------------------------------------------
# hand-written cases
# --------------------------------------------------------------------------
def flags_of(a, b):
    return [(g.pos, g.end, g.flags, g.peer) for g in check(a, b)]


def test_pid_tie_break():
    """scalar_test.go: {1, 10} before {10, 10}: the same VID, the PID decides."""
    a, b = [K(1, 10, 10)], [K(1, 10, 1)]
    assert flags_of(a, b) == [(0, 1, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER, 0)]
    assert flags_of(b, a) == [(1, 1, CMP_PEER_HAS | CMP_EARLIER, 0)]


def test_vid_max():
    a = [K(1, 1), K(1, M64, M32)]
    b = [K(1, 1), K(1, M64, M32 - 1)]
    assert flags_of(a, b) == [(1, 2, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER, 1)]  # {M32 - 1, M64} is not mine: a fork
    assert flags_of(a, a) == [(2, 2, CMP_PEER_HAS | CMP_EQUAL | CMP_ANCESTOR, 1)]
    assert flags_of(a, [K(1, 1)]) == [(1, 2, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER | CMP_ANCESTOR, 0)]


def test_id_ending_ff_beside_its_successor():
    """ObjectLimit's limit[16]++ wraps for the first ID (keys.go:88-91); the ranges here are by prefix equality."""
    lo, hi = oid(0xFF, 0x42), bytes([0x43]) + bytes(15)
    a = [hkeys.new(lo, Scalar(1, 1)), hkeys.new(lo, Scalar(1, 2)), hkeys.new(hi, Scalar(1, 1))]
    b = [hkeys.new(lo, Scalar(1, 1)), hkeys.new(hi, Scalar(1, 5))]
    assert flags_of(a, b) == [(1, 2, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER | CMP_ANCESTOR, 0),
                              (3, 3, CMP_PEER_HAS | CMP_EARLIER, 1)]


def test_equal_key_runs_on_each_side():
    a = [K(1, 1), K(1, 2), K(1, 2), K(1, 3), K(1, 3)]
    b = [K(1, 1), K(1, 2), K(1, 2), K(1, 2)]
    # the upper bound of the peer's latest in a passes its whole run; the peer's row is the run's last
    assert flags_of(a, b) == [(3, 5, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER | CMP_ANCESTOR, 3)]
    assert flags_of(b, a) == [(4, 4, CMP_PEER_HAS | CMP_EARLIER | CMP_ANCESTOR, 4)]
    assert flags_of(a, a) == [(5, 5, CMP_PEER_HAS | CMP_EQUAL | CMP_ANCESTOR, 4)]


def test_fork_both_ways():
    a = [K(1, 1), K(1, 2, 7)]
    b = [K(1, 1), K(1, 2, 9), K(1, 3, 9)]
    assert flags_of(a, b) == [(2, 2, CMP_PEER_HAS | CMP_EARLIER, 2)]
    assert flags_of(b, a) == [(1, 3, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER, 1)]


def test_digest_peer():
    a = [K(1, 1), K(1, 2), K(1, 3), K(2, 1), K(3, 4), K(4, 1)]
    whole = [K(1, 1), K(1, 2), K(2, 1), K(2, 2), K(3, 4)]
    digest = [K(1, 2), K(2, 2), K(3, 4)]
    w, d = flags_of(a, whole), flags_of(a, digest)
    assert w == [(2, 3, SEEK_FOUND | CMP_PEER_HAS | CMP_LATER | CMP_ANCESTOR, 1),
                 (4, 4, CMP_PEER_HAS | CMP_EARLIER | CMP_ANCESTOR, 3),
                 (5, 5, CMP_PEER_HAS | CMP_EQUAL | CMP_ANCESTOR, 4),
                 (5, 6, SEEK_FOUND | CMP_LATER, None)]
    # only the peer's latest row decides pos, end and the class; EARLIER's ANCESTOR needs the whole column
    assert [(p, e, f & ~CMP_ANCESTOR) for p, e, f, _ in d] == [(p, e, f & ~CMP_ANCESTOR) for p, e, f, _ in w]
    assert [f & CMP_ANCESTOR for _, _, f, _ in d] == [CMP_ANCESTOR, 0, CMP_ANCESTOR, 0]
    assert [q for _, _, _, q in d] == [0, 1, 2, None]


def test_empty_sides():
    a = [K(1, 1), K(1, 2), K(2, 1)]
    assert hkeys.compare([], a) == []
    assert hkeys.compare([], []) == []
    assert flags_of(a, []) == [(0, 2, SEEK_FOUND | CMP_LATER, None), (2, 3, SEEK_FOUND | CMP_LATER, None)]


def test_only_the_peer_has_is_the_exchanged_call():
    a, b = [K(1, 1)], [K(1, 1), K(2, 1), K(3, 9)]
    assert [g.flags & CMP_PEER_HAS for g in hkeys.compare(b, a)] == [CMP_PEER_HAS, 0, 0]


# --------------------------------------------------------------------------
# the ABI without a device
# --------------------------------------------------------------------------
def test_flag_bits_lie_above_the_seek_bits():
    bits = (CMP_PEER_HAS, CMP_LATER, CMP_EARLIER, CMP_EQUAL, CMP_ANCESTOR)
    assert bits == tuple(1 << b for b in range(8, 13))
    assert CMP_COUNTS_DTYPE.itemsize == 64 and SEEK_DTYPE.itemsize == 20


def test_exported():
    assert {"honu_key_compare", "honu_key_compare_workspace"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "honu_key_compare")


def test_workspace_size():
    lib = _lib.load()
    assert lib.honu_key_compare_workspace(0) == 0
    sizes = [int(lib.honu_key_compare_workspace(n)) for n in range(5001)]
    assert all(s % 256 == 0 for s in sizes)
    assert all(x <= y for x, y in zip(sizes, sizes[1:]))
    assert sizes[1] > 0
    big = [int(lib.honu_key_compare_workspace(n)) for n in (1 << 20, 1 << 31, M32)]
    assert big == sorted(big) and big[0] >= sizes[-1]


def test_refusals_with_a_null_context():
    """A NULL ctx is refused before anything is looked at: every pointer here is one no call may touch."""
    lib = _lib.load()
    bad = 0x1000
    for na, nb in ((0, 0), (5, 7), (M32 + 1, 0)):
        st = lib.honu_key_compare(None, bad, bad, bad, na, bad, bad, bad, bad, nb, bad, bad, bad, bad, 1 << 40, None)
        assert st == -1  # HONU_E_ARG
        assert b"ctx" in lib.honu_last_error()
