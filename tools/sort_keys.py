#!/usr/bin/env python3
"""Time honu_sort_keys and honu_key_objects on 1M keys of three distributions,
next to two yardsticks measured in the same process: (i) the same order from
stock torch on the GPU (the keys as four big-endian u64 words, four stable
torch.sort passes from the least significant word, gathers in between), which
is what a caller would write without these entry points, and (ii) np.lexsort
on the host, a stand-in for sort.Sort(keys.Keys) (there is no Go toolchain to
time the reference itself).

Device times are HIP events around windows of --inner calls after a warm-up;
the figure is the median window over --reps, per call. The fixed cost of a
call (pack, plan, the launches of 30 passes that all return at once, emit) is
measured on a column of equal keys, which has no pass to run; a pass's time
is (sort - fixed) / passes. Bytes per pass come from the packed layout: the
count kernel reads one word of every 32-byte key (every sector of the side),
the scatter reads and writes 32 + 4 bytes per key: 104 n, of 8 TB/s.

Prints one JSON line per distribution; --out also writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from honu_amd import _lib  # noqa: E402
from honu_amd.object import Codec  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12


def keys_random(n, rng):
    """29 random bytes, as randKey() (keys_test.go:283-287)."""
    return rng.integers(0, 256, (n, 29), dtype=np.uint8)


def keys_columns(oid, vid, pid):
    n = len(vid)
    k = np.zeros((n, 29), np.uint8)
    k[:, 0] = 1
    k[:, 1:17] = oid
    k[:, 17:25] = vid.astype(">u8").view(np.uint8).reshape(n, 8)
    k[:, 25:29] = pid.astype(">u4").view(np.uint8).reshape(n, 4)
    return k


def keys_generator(n, rng):
    """The bench generator's keys (gen.cpp): ObjectID zero, uniform VID and PID."""
    return keys_columns(np.zeros((n, 16), np.uint8), rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 +
                        rng.integers(0, 2, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint32))


def keys_objects(n, rng, versions=16):
    """n / 16 objects x 16 versions in random row order. ULID-like object IDs:
    a 48-bit millisecond timestamp within one hour (its leading bytes shared)
    and 80 random bits; VID 1..16, PID 0..3."""
    nobj = n // versions
    ms = np.uint64(1_760_000_000_000) + rng.integers(0, 3_600_000, nobj, dtype=np.uint64)
    oid = np.zeros((nobj, 16), np.uint8)
    oid[:, :6] = ms.astype(">u8").view(np.uint8).reshape(nobj, 8)[:, 2:]
    oid[:, 6:] = rng.integers(0, 256, (nobj, 10), dtype=np.uint8)
    which = np.repeat(np.arange(nobj), versions)
    vid = np.tile(np.arange(1, versions + 1, dtype=np.uint64), nobj)
    perm = rng.permutation(nobj * versions)
    return keys_columns(oid[which][perm], vid[perm], rng.integers(0, 4, nobj * versions, dtype=np.uint32))


def device_time_us(fn, reps, inner):
    """Median over `reps` windows of `inner` calls, per call, by device events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def torch_order(dk, n, sign):
    """Yardstick (i): the stable order of the column with stock torch."""
    pad = torch.zeros((n, 32), dtype=torch.uint8, device=dk.device)
    pad[:, :29] = dk.view(n, 29)
    words = pad.view(n, 4, 8).flip(2).contiguous().view(torch.int64).view(n, 4) ^ sign  # unsigned order
    order = torch.arange(n, device=dk.device)
    for w in (3, 2, 1, 0):
        _, idx = torch.sort(words[order, w], stable=True)
        order = order[idx]
    return order, dk.view(n, 29)[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the np.lexsort stand-in")
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/sort_keys.py measures on the GPU: no device found")
    n = a.n
    dev = torch.device("cuda", 0)
    codec = Codec(0, n)
    L, c = codec.lib, codec.ctx
    s = torch.cuda.current_stream().cuda_stream
    tile = _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"sort_tile", _lib.C.byref(tile)), "sort_tile")
    wb = int(L.honu_sort_keys_workspace(n))
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    work, order, srt, valid = u8(wb), u8(4 * n), u8(29 * n), u8(8)
    obj_off, latest, objects = u8(8 * (n + 1)), u8(4 * n), u8(8)
    dk = u8(29 * n)
    sign = torch.tensor(-(1 << 63), dtype=torch.int64, device=dev)

    def sort():
        _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(order), P(srt), P(valid), P(work), wb, s), "sort")

    def sort_objects():
        sort()
        _lib.check(L.honu_key_objects(c, P(dk), P(order), P(valid), n, P(obj_off), P(latest), P(objects),
                                      P(work), wb, s), "objects")

    def load(k):
        dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))

    rng = np.random.default_rng(a.seed)
    load(np.tile(keys_random(1, rng), (n, 1)))  # equal keys: no pass runs
    fixed_us = device_time_us(sort, a.reps, a.inner)[0]
    lines = []
    for name, make in (("random", keys_random), ("generator", keys_generator), ("objects_x16", keys_objects)):
        k = make(n, rng)
        load(k)
        passes = int((k != k[0]).any(axis=0).sum())
        sort_us, sort_min, sort_max = device_time_us(sort, a.reps, a.inner)
        both_us = device_time_us(sort_objects, a.reps, a.inner)[0]
        torch_us, torch_min, torch_max = device_time_us(lambda: torch_order(dk[:29 * n], n, sign), a.reps, 2)
        sort_objects()
        t_order, t_sorted = torch_order(dk[:29 * n], n, sign)
        torch.cuda.synchronize()
        got = order[:4 * n].view(torch.int32).to(torch.int64)
        match = bool((got == t_order).all()) and bool((srt[:29 * n].view(n, 29) == t_sorted).all())
        per_pass_us = (sort_us - fixed_us) / passes if passes else 0.0
        pass_bytes = 104 * n
        rec = {"tool": "sort_keys", "keys": n, "distribution": name, "sort_tile": int(tile.value),
               "passes": passes, "sort_us": round(sort_us, 1), "sort_us_min_max": [round(sort_min, 1), round(sort_max, 1)],
               "sort_objects_us": round(both_us, 1), "fixed_us": round(fixed_us, 1),
               "per_pass_us": round(per_pass_us, 1), "bytes_per_pass": pass_bytes,
               "hbm_fraction_per_pass": round(pass_bytes / (per_pass_us * 1e-6) / HBM_BYTES_PER_S, 3) if passes else None,
               "torch_sort_us": round(torch_us, 1), "torch_sort_us_min_max": [round(torch_min, 1), round(torch_max, 1)],
               "speedup_vs_torch": round(torch_us / sort_us, 2), "matches_torch": match,
               "valid": int(valid[:8].view(torch.int64).item()), "objects": int(objects[:8].view(torch.int64).item()),
               "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0), "commit": a.commit}
        if not a.no_host:
            t0 = time.perf_counter()
            h_order = np.lexsort(k.T[::-1])
            rec["host_lexsort_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            rec["host_lexsort_note"] = "np.lexsort on one host core: a stand-in for sort.Sort(keys.Keys)"
            rec["matches_host"] = bool(np.array_equal(h_order, got.cpu().numpy()))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
