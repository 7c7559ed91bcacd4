"""The host mirror of pkg/store/keys (honu_amd/keys.py) against the reference's
own tests (keys/keys_test.go), and the size contract of the sort workspace
(include/honu_codec.h: honu_sort_keys_workspace), which needs no GPU."""
import json
import os

import pytest

from honu_amd import _lib, keys
from honu_amd.metadata import Scalar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_versions.json")
OID = bytes(range(0x30, 0x40))  # a fixed ObjectID; its last byte is not 0xff


def test_new_key_layout():
    """keys_test.go:18-27 and keys.go:42-51: 01 | oid | BE64(VID) | BE32(PID)."""
    k = keys.new(OID, Scalar(PID=2, VID=1))
    assert len(k) == 29 and k[0] == 0x01 and k[1:17] == OID
    assert k[17:25] == bytes([0, 0, 0, 0, 0, 0, 0, 1]) and k[25:29] == bytes([0, 0, 0, 2])
    assert keys.object_id(k) == OID
    assert keys.version(k) == Scalar(PID=2, VID=1)
    big = keys.new(OID, Scalar(PID=0xA1B2C3D4, VID=0x0102030405060708))
    assert big[17:29] == bytes([1, 2, 3, 4, 5, 6, 7, 8, 0xA1, 0xB2, 0xC3, 0xD4])
    assert keys.version(big) == Scalar(PID=0xA1B2C3D4, VID=0x0102030405060708)


def test_new_key_without_version():
    """A nil version leaves the prefix and twelve zero bytes (keys.go:46-49)."""
    k = keys.new(OID, None)
    assert len(k) == 29 and k[:17] == b"\x01" + OID and k[17:] == bytes(12)
    assert keys.version(k) == Scalar()
    assert not keys.has_version(k)
    assert not keys.has_version(keys.new(OID, Scalar()))  # keys_test.go:231-232


def test_check_errors():
    """keys_test.go:107-126,262-267: size first, then the version byte; the
    accessors fail with Check's error where Go panics with it."""
    keys.check(keys.new(OID, Scalar(PID=2, VID=1)))
    with pytest.raises(keys.ErrBadSize):
        keys.check(bytes(26))
    with pytest.raises(keys.ErrBadSize):
        keys.check(bytes(42))
    bad = bytearray(keys.new(OID, Scalar(PID=2, VID=1)))
    bad[0] = 0x28
    with pytest.raises(keys.ErrBadVersion):
        keys.check(bytes(bad))
    for fn in (keys.object_id, keys.version, keys.object_prefix, keys.object_limit, keys.has_version):
        with pytest.raises(keys.ErrBadSize):
            fn(bytes(26))
        with pytest.raises(keys.ErrBadVersion):
            fn(bytes(bad))
    assert issubclass(keys.ErrMalformed, keys.KeyError_)
    assert str(keys.ErrMalformed()) == "key is malformed: cannot parse version components"


@pytest.mark.parametrize("pos", range(12))
def test_has_version_one_ff_byte(pos):
    """keys_test.go:236-259: one 0xff byte anywhere in the 12 version bytes."""
    vers = bytearray(12)
    vers[pos] = 0xFF
    for oid in (OID, bytes(16)):  # ulid.Null too
        k = bytearray(keys.new(oid, None))
        k[17:29] = vers
        assert keys.has_version(bytes(k))


def test_object_prefix_and_limit():
    """keys_test.go:162-201."""
    k = keys.new(OID, Scalar(PID=2, VID=1))
    prefix, limit = keys.object_prefix(k), keys.object_limit(k)
    assert len(prefix) == 17 and prefix == b"\x01" + OID
    assert len(limit) == 17 and limit[:16] == b"\x01" + OID[:15] and limit[16] == OID[15] + 1
    wrap = keys.new(OID[:15] + b"\xff", None)
    assert keys.object_limit(wrap)[16] == 0  # limit[16]++ wraps (keys.go:88-91)


def test_object_range_orderings():
    """TestObjectRange (keys_test.go:203-222): prefix < key; limit > the
    largest version; limit < the next object's zero version."""
    k = keys.new(OID, None)
    prefix, limit = keys.object_prefix(k), keys.object_limit(k)
    assert prefix < k
    maxver = keys.new(OID, Scalar(PID=0xFFFFFFFF, VID=0xFFFFFFFFFFFFFFFF))
    assert limit > maxver
    nxt = keys.new(OID[:15] + bytes([OID[15] + 1]), None)
    assert limit < nxt


def test_static_versions_are_in_byte_order():
    """keys_test.go:36-63: the 13 versions, in lamport.Compare order, give keys
    that are non-decreasing in byte order; sort() leaves them as they are."""
    vs = [Scalar(PID=v["PID"], VID=v["VID"]) for v in json.load(open(GOLDEN))["versions"]]
    assert len(vs) == 13
    ks = [keys.new(OID, v) for v in vs]
    for a, b in zip(vs, vs[1:]):
        assert (a.VID, a.PID) <= (b.VID, b.PID)  # lamport.Compare (scalar.go:50-78)
    for a, b in zip(ks, ks[1:]):
        assert a <= b
    assert keys.sort(reversed(ks)) == ks
    assert [keys.version(k) for k in ks] == vs


def test_sort_is_bytes_compare():
    """TestSort (keys_test.go:270-287): random 29-byte keys, byte 0 included."""
    import random
    rng = random.Random(5)
    ks = [bytes(rng.randrange(256) for _ in range(29)) for _ in range(128)]
    out = keys.sort(ks)
    assert sorted(out) == out and sorted(ks) == out
    assert all(a <= b for a, b in zip(out, out[1:]))


def test_sort_workspace_contract():
    """At most 96 n + 2^20 bytes, monotonic in n, a multiple of 256; computed
    on the host."""
    lib = _lib.load()
    ns = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 100003, 1 << 20, (1 << 20) + 1, 1 << 24, (1 << 32) - 1]
    sizes = [int(lib.honu_sort_keys_workspace(n)) for n in ns]
    for n, s in zip(ns, sizes):
        assert 0 < s <= 96 * n + 2 ** 20, (n, s)
        assert s % 256 == 0, (n, s)
    assert sizes == sorted(sizes)
    assert sizes[-1] >= 72 * ns[-1]  # two sides of 32-byte keys and 4-byte indices at the least
