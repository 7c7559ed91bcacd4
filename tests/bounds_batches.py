"""Batches of the write-set and placement tests (test_gpu_bounds.py,
test_gpu_placement.py, test_oracle_capacity.py), built once per process on
the CPU. Small on purpose: one call lasts milliseconds, and every edge the
kernels have (ends of ranges, partial chunks, both copy classes, range
tails) is still inside."""
import functools

import numpy as np

from corpora import odd_metas, random_metas
from honu_amd.metadata import HostBatch, pack_batch
from honu_amd.workload import gen_host_batch

ENCODE_BATCHES = ("tiny", "units", "edges", "steal", "two_class")
SMALL_BATCHES = ("tiny", "units", "edges")


@functools.lru_cache(maxsize=None)
def encode_batch(name) -> HostBatch:
    """tiny / units / edges: 192 random_metas rows (nil sub-structs, nil ACL
    entries, every frame size; two rows are nil metas, Marshal(nil, ...)) with
    payloads of 0-40 bytes (head and tail bytes only), 0-200 bytes (inside,
    touching and straddling one or two 64-byte units) and 16 k + {-2..2}
    bytes; steal: 48 generator rows with 16-40 KB payloads (the copy's range
    tails need an average of 16 KB); two_class: 64 generator rows, 70 % at
    512-4608 B and 30 % at 200-400 KB (an average above 64 KB: both copy
    classes run)."""
    rng = np.random.default_rng(sum(name.encode()))
    if name in SMALL_BATCHES:
        n = 192
        metas, _ = random_metas(n, 7)
        metas[5] = metas[130] = None
        base = pack_batch(metas, [None] * n)
        if name == "tiny":
            ln = rng.integers(0, 41, n)
        elif name == "units":
            ln = rng.integers(0, 201, n)
        else:
            ln = rng.integers(1, 201, n) * 16 + rng.integers(-2, 3, n)
    elif name == "steal":
        n = 48
        base = gen_host_batch(9, "small", 0, n)
        ln = rng.integers(16 << 10, 40 << 10, n)
    elif name == "two_class":
        n = 64
        base = gen_host_batch(10, "small", 0, n)
        ln = rng.integers(512, 4608, n)
        big = np.arange(n) % 10 >= 7  # 30 %, spread through the batch
        ln[big] = rng.integers(200 << 10, 400 << 10, int(big.sum()))
    else:
        raise KeyError(name)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(ln)
    pay = rng.integers(0, 256, int(off[-1]) + 1, dtype=np.uint8)
    return HostBatch(base.meta, base.var, base.acl, base.regions, pay, off)


def slice_batch(hb: HostBatch, k: int) -> HostBatch:
    """Rows [k, n) of a batch as a caller passes them: d_meta + k and
    d_payload_off + k over the same arenas and tables."""
    return HostBatch(hb.meta[k:], hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off[k:])


@functools.lru_cache(maxsize=None)
def decode_batch():
    """(rec, off) of 64 * 3 + 5 encoded records: generator Small records with
    the odd_metas records (long tails, nil ACL entries, lists of more than 8
    regions, nil payloads) spread among them."""
    from oracle import oracle
    n, odd = 64 * 3 + 5, 48
    r1, o1, s1 = oracle.marshal_batch(gen_host_batch(12, "small", 0, n - odd))
    r2, o2, s2 = oracle.marshal_batch(pack_batch(*odd_metas()))
    assert (s1 == 0).all() and (s2 == 0).all()
    small = [r1[int(o1[i]):int(o1[i + 1])] for i in range(n - odd)]
    odds = [r2[int(o2[i]):int(o2[i + 1])] for i in range(odd)]
    recs = []
    for i in range(n):  # every fourth record an odd one, while they last
        recs.append(odds.pop(0) if (i % 4 == 1 and odds) else small.pop(0))
    assert not odds and not small
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    rec = np.concatenate(recs)
    rec.setflags(write=False)
    off.setflags(write=False)
    return rec, off


def ok_ranges(off, status):
    """The byte ranges of the records a call completes."""
    return [(int(off[i]), int(off[i + 1])) for i in range(len(status)) if status[i] == 0]
