"""keys.seek / keys.has, the host statement of honu_key_seek, against two
independent routes (a linear scan with startswith; bisect_right over truncated
keys), the three cases of the reference's cursor test (cursor_test.go:95-121)
restated, and the honu_seek row's layout."""
import bisect
import os
import subprocess

import numpy as np

from honu_amd import _lib, keys
from honu_amd.metadata import SEEK_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "honu_codec.h")


def seek_linear(srt, probe):
    """First key >= probe by a scan; then while the keys start with the probe."""
    pos = next((i for i, k in enumerate(srt) if k >= probe), len(srt))
    end = pos
    while end < len(srt) and srt[end].startswith(probe):
        end += 1
    return pos, end


def seek_truncated(srt, probe):
    """Lower and upper bound of the probe among the keys cut to its length
    (every key here is at least as long as every probe)."""
    cut = [k[:len(probe)] for k in srt]
    return bisect.bisect_left(cut, probe), bisect.bisect_right(cut, probe)


def key_sets():
    rng = np.random.default_rng(5)
    rand = [bytes(r) for r in rng.integers(0, 256, (300, 29), dtype=np.uint8)]
    two = [bytes(r) for r in rng.choice(np.array([0x7F, 0x80], np.uint8), (200, 29))]
    oids = rng.integers(0, 256, (12, 16), dtype=np.uint8)
    oids[3, 15] = oids[4, 15] = 0xFF
    oids[5] = 0xFF
    vers = []
    for i in range(240):
        o = oids[i % 12]
        vers.append(bytes([1]) + bytes(o) + int(rng.integers(1, 5)).to_bytes(8, "big") +
                    int(rng.integers(0, 3)).to_bytes(4, "big"))
    return {"random": keys.sort(rand), "two_values": keys.sort(two), "versions": keys.sort(vers),
            "equal": [rand[0]] * 17, "empty": [], "one": [rand[1]]}


def probes_for(srt, plen):
    out = {b"\x00" * plen, b"\xff" * plen}
    for k in srt[::3] + srt[-1:]:
        p = bytearray(k[:plen])
        out.add(bytes(p))
        if plen:
            for d in (1, 255):
                q = bytearray(p)
                q[-1] = (q[-1] + d) & 0xFF
                out.add(bytes(q))
    return sorted(out)


def test_seek_matches_both_routes():
    for name, srt in key_sets().items():
        for plen in (0, 1, 15, 16, 17, 28, 29):
            for probe in probes_for(srt, plen):
                got = keys.seek(srt, probe)
                assert got == seek_linear(srt, probe) == seek_truncated(srt, probe), (name, plen, probe.hex())
                pos, end = got
                assert keys.has(srt, probe) == (pos < end) == any(k.startswith(probe) for k in srt)


def cursor_keys(n=128):
    """Distinct sorted keys whose last byte leaves room above it (the
    reference's test seeks to key 63 with its last byte incremented and expects
    key 64, cursor_test.go:106-113)."""
    rng = np.random.default_rng(95)
    rows = rng.integers(0, 256, (n, 29), dtype=np.uint8)
    rows[:, 28] = rng.integers(0, 255, n)
    rows[:, 0] = np.arange(n)  # distinct, and already in order
    return [bytes(r) for r in rows]


def test_cursor_seek_cases():
    srt = cursor_keys()
    assert srt == keys.sort(srt)
    # an existing key returns itself (cursor_test.go:98-104)
    assert keys.seek(srt, srt[16]) == (16, 17) and keys.has(srt, srt[16])
    # a key between two keys lands on the next one (cursor_test.go:106-113)
    between = srt[63][:28] + bytes([srt[63][28] + 1])
    assert srt[63] < between < srt[64]
    assert keys.seek(srt, between) == (64, 64) and not keys.has(srt, between)
    # beyond the last key Seek returns nil (cursor_test.go:116-121)
    beyond = srt[-1][:28] + bytes([srt[-1][28] + 1])
    assert keys.seek(srt, beyond) == (len(srt), len(srt)) and not keys.has(srt, beyond)


def test_object_id_ending_in_ff_has_its_range():
    """ObjectLimit()'s limit[16]++ wraps there (keys.go:88-91) and leaves the
    reference's own range empty; seek's end carries instead."""
    from honu_amd.metadata import Scalar
    oid = bytes(range(15)) + b"\xff"
    other = bytes(range(15)) + b"\xfe"
    srt = keys.sort([keys.new(oid, Scalar(PID=1, VID=v)) for v in (1, 2, 3)] +
                    [keys.new(other, Scalar(PID=1, VID=9)), keys.new(b"\xff" * 16, Scalar(PID=2, VID=1))])
    prefix = keys.object_prefix(srt[1])
    assert keys.object_limit(srt[1]) < prefix  # the wrap
    assert keys.seek(srt, prefix) == (1, 4)
    assert keys.has(srt, prefix) and keys.has(srt, prefix[:16]) and not keys.has(srt, prefix[:16] + b"\xfd")
    assert keys.seek(srt, b"\x01" + b"\xff" * 16) == (4, 5)  # nothing above an all-0xff id but the end


def test_probe_len_zero_matches_everything():
    srt = key_sets()["random"]
    assert keys.seek(srt, b"") == (0, len(srt)) and keys.has(srt, b"")
    assert keys.seek([], b"") == (0, 0) and not keys.has([], b"")


def test_seek_row_layout(tmp_path):
    lib = _lib.load()
    assert lib.honu_sizeof_seek() == 20 == SEEK_DTYPE.itemsize
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(){"]
    for name in SEEK_DTYPE.names:
        lines.append(f'printf("{name} %zu\\n", offsetof(honu_seek, {name}));')
    lines.append('printf("flags %u %u %u %u %u %u %u\\n", HONU_SEEK_FOUND, HONU_SEEK_END, HONU_SEEK_EXACT,'
                 ' HONU_SEEK_FIRST_LIVE, HONU_SEEK_LATEST_LIVE, HONU_SEEK_SKIPPED, HONU_SEEK_NONE);')
    lines.append("return 0;}")
    c = tmp_path / "off.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got = dict(line.split(" ", 1) for line in out)
    for name in SEEK_DTYPE.names:
        if name != "flags":
            assert int(got[name]) == SEEK_DTYPE.fields[name][1], name
    from honu_amd import metadata as md
    assert out[-2] == "flags 16"
    assert [int(x) for x in out[-1].split()[1:]] == [
        md.SEEK_FOUND, md.SEEK_END, md.SEEK_EXACT, md.SEEK_FIRST_LIVE, md.SEEK_LATEST_LIVE, md.SEEK_SKIPPED,
        md.SEEK_NONE]
