#!/usr/bin/env python3
"""Time honu_key_route: a sorted batch of --n keys (1M; tools/sort_keys.py's
objects_x16 column) taken apart by collection, for tables of k = 1, 16, 256 and
4096 collections drawn uniformly, and for k = 16 drawn heavily skewed (half of
the records in one collection, a quarter in the next, ...). One record in a
hundred is of a collection the table does not hold. The call is given the
packed ID column (stride 16), the order honu_sort_keys wrote as d_seq and the
key column, and writes every output it has.
Next to it, timed in the same run:
    sort    honu_sort_keys over the whole batch alone: what a caller pays
            before the route, and what the route's own sort of the classes is
            to be held against.
    sorts   what a caller needs today for the same result: one honu_sort_keys
            per collection, over the batch ALREADY SPLIT. This yardstick gets
            the split for free (the host groups the keys by collection before
            the upload); a caller today would have to read the decoded rows
            back to make it. Above 16 collections 16 of the k calls are timed
            (uniform draws: every collection has n / k keys within a few
            percent) and the figure is scaled by k / 16; the output says which.
Every point is verified before it is timed: d_bucket_off, d_bucket_count,
d_rows, d_local, d_keys_out and d_bucket against numpy (a stable argsort of
the classes along the sort's order), and every collection's segment of
d_keys_out against the sorted column of that collection's keys alone.

Timed as tools/key_reclaim.py times its call: HIP events around windows, a
window one replay of a graph of `inner` calls, the windows alternating between
the three, the figure the median window per call with min and max.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's outputs are not numpy's."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from honu_amd import _lib  # noqa: E402
from honu_amd.metadata import LIST_ROW_HEAD, SEEK_NONE  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
SAMPLE = 16  # the per-collection sorts timed at most
POINTS = ((1, "uniform"), (16, "uniform"), (256, "uniform"), (4096, "uniform"), (16, "skewed"))


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| k | draw | keys | largest collection | honu_key_route us | honu_sort_keys (whole batch) us | sort + route us | "
          "k sorts of the split batch us | sorts timed | k sorts / (sort + route) | route / sort | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['k']} | {r['draw']} | {r['keys']} | {r['largest']} | {cell('route')} | {cell('sort')} | "
              f"{r['sort_plus_route_us']} | {cell('sorts')} | {r['sorts_timed']} of {r['k']}"
              f"{' (scaled)' if r['sorts_scaled_by'] != 1 else ''} | {r['sorts_over_sort_plus_route']}x | "
              f"{r['route_over_sort']}x | {'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] for r in rows),
                      "note": "the k sorts are given the batch already split: the split itself is not in their time"}))


def run(a, lines):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    keys = keys_objects(a.n, rng)
    n = len(keys)
    codec = Codec(0, n + 2)
    L, c, s = codec.lib, codec.ctx, codec.stream
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    host = lambda t, nbytes, dt=np.uint8: t[:nbytes].cpu().numpy().view(dt)  # noqa: E731
    d_keys = up(keys)
    wb, rwb = int(L.honu_sort_keys_workspace(n)), int(L.honu_key_route_workspace(n))
    work, rwork = u8(wb), u8(rwb)
    order, sorted_, valid = u8(4 * n), u8(29 * n), u8(8)

    def sort():
        _lib.check(L.honu_sort_keys(c, P(d_keys), 0, n, P(order), P(sorted_), P(valid), P(work), wb, codec.stream),
                   "honu_sort_keys")

    sort()
    torch.cuda.synchronize()
    seq = host(order, 4 * n, np.uint32).astype(np.int64)
    assert np.array_equal(keys[seq], host(sorted_, 29 * n).reshape(n, 29))
    bucket, rows, local, keys_out = u8(4 * n), u8(16 * n), u8(4 * n), u8(29 * n)
    split, s_order, s_sorted, s_valid = u8(29 * n), u8(4 * n), u8(29 * n), u8(8)
    for k, draw in [p for p in POINTS if f"{p[0]}:{p[1]}" in a.points.split(",")]:
        table = rng.integers(0, 256, (k, 16), dtype=np.uint8)
        table = table[np.lexsort(table.T[::-1])]
        assert len(np.unique(table, axis=0)) == k
        if draw == "uniform":
            member = rng.integers(0, k, n)
        else:  # collection j holds about n / 2^(j + 1) records
            member = np.minimum(rng.geometric(0.5, n) - 1, k - 1)
        ids = table[member]
        unknown = rng.random(n) < 0.01
        ids[unknown] = rng.integers(0, 256, (int(unknown.sum()), 16), dtype=np.uint8)
        cls = np.where(unknown, k, member)
        d_ids, d_table = up(ids), up(table)
        off, count = u8(8 * (k + 3)), u8(8 * (k + 2))

        def route():
            _lib.check(L.honu_key_route(c, P(d_ids), 16, 0, n, P(order), P(d_table), k, P(d_keys), P(bucket), P(rows),
                                        P(local), P(keys_out), P(off), P(count), P(rwork), rwb, codec.stream),
                       "honu_key_route")

        # numpy's route: a stable argsort of the classes along the sort's order
        along = cls[seq]
        g = np.argsort(along, kind="stable")
        want_off = np.searchsorted(along[g], np.arange(k + 3))
        cg = along[g]
        head = np.ones(n, bool)
        head[1:] = cg[1:] != cg[:-1]
        want_rows = np.stack([cg, g, seq[g], np.where(head, LIST_ROW_HEAD, 0)], 1).astype(np.uint32)
        for t in (bucket, rows, local, keys_out, off, count):
            t.zero_()
        route()
        torch.cuda.synchronize()
        got_off = host(off, 8 * (k + 3), np.int64)
        equal = bool(
            np.array_equal(got_off, want_off) and
            np.array_equal(host(count, 8 * (k + 2), np.int64), np.diff(want_off)) and
            np.array_equal(host(rows, 16 * n, np.uint32).reshape(n, 4), want_rows) and
            np.array_equal(host(local, 4 * n, np.uint32), np.arange(n) - want_off[cg]) and
            np.array_equal(host(keys_out, 29 * n).reshape(n, 29), keys[seq[g]]) and
            np.array_equal(host(bucket, 4 * n, np.uint32), np.where(unknown, SEEK_NONE, member).astype(np.uint32)))
        # the batch already split, for the yardstick: the keys grouped by collection, in arrival order
        by = np.argsort(cls, kind="stable")
        starts = np.searchsorted(cls[by], np.arange(k + 2))
        split[:29 * n].copy_(up(keys[by]))
        timed = list(range(k)) if k <= SAMPLE else sorted(rng.choice(k, SAMPLE, replace=False).tolist())
        routed = host(keys_out, 29 * n).reshape(n, 29)
        for j in timed:  # each per-collection sort gives the route's segment
            a0, cnt = int(starts[j]), int(starts[j + 1] - starts[j])
            _lib.check(L.honu_sort_keys(c, P(split) + 29 * a0, 0, cnt, P(s_order), P(s_sorted), P(s_valid), P(work), wb, s),
                       "honu_sort_keys")
            torch.cuda.synchronize()
            equal = equal and bool(np.array_equal(host(s_sorted, 29 * cnt).reshape(cnt, 29),
                                                  routed[want_off[j]:want_off[j + 1]]))

        def sorts():
            for j in timed:
                a0, cnt = int(starts[j]), int(starts[j + 1] - starts[j])
                _lib.check(L.honu_sort_keys(c, P(split) + 29 * a0, 0, cnt, P(s_order) + 4 * a0, P(s_sorted) + 29 * a0,
                                            P(s_valid), P(work), wb, codec.stream), "honu_sort_keys")

        inners = {"route": a.inner, "sort": a.inner, "sorts": 1 if len(timed) > 1 else a.inner}
        times = windows_us({"route": route, "sort": sort, "sorts": sorts}, inners, a.reps)
        scale = k / len(timed)
        times["sorts"] = tuple(x * scale for x in times["sorts"])
        rec = {"tool": "key_route", "k": k, "draw": draw, "keys": n, "unknown": int(unknown.sum()),
               "largest": int(np.diff(want_off)[:k].max()), "reps": a.reps, "inner": a.inner, "sorts_inner": inners["sorts"],
               "sorts_timed": len(timed), "sorts_scaled_by": scale, "sorts_get_the_split_for_free": True,
               "equals_numpy": equal}
        for name in ("route", "sort", "sorts"):
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        both = times["sort"][0] + times["route"][0]
        rec["sort_plus_route_us"] = round(both, 1)
        rec["sorts_over_sort_plus_route"] = round(times["sorts"][0] / both, 2)
        rec["route_over_sort"] = round(times["route"][0] / times["sort"][0], 2)
        rec["route_ns_per_key"] = round(times["route"][0] * 1e3 / n, 2)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["commit"] = a.commit
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the batch")
    ap.add_argument("--points", default=",".join(f"{k}:{d}" for k, d in POINTS), help="k:draw, comma separated")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_route.py measures on the GPU: no device found")
    lines = []
    run(a, lines)
    print_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    wrong = [f"k {r['k']} {r['draw']}" for r in map(json.loads, lines) if not r["equals_numpy"]]
    if wrong:  # a run whose outputs are wrong is no profile
        sys.exit("honu_key_route's outputs differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
