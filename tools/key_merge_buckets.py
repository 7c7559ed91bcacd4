#!/usr/bin/env python3
"""Time honu_key_merge_buckets: a routed batch of --batch keys (64 K and 1 M)
merged into a resident bucketed column of --n keys (1M; tools/sort_keys.py's
objects_x16 column) for k = 1, 16, 256 and 4096 collections drawn uniformly,
and for k = 16 drawn heavily skewed (half of the rows in one collection, a
quarter in the next, ...). Both sides are bucket-major arenas as the call takes
them: the resident column with its order and offsets, the batch with the
offsets a route would have written. The call writes every output it has.
Next to it, timed in the same run, what a caller runs today for the same
result:
    merges  one honu_key_merge per collection over the views of the same two
            arenas. Above 16 collections 16 of the k calls are timed (uniform
            draws: every collection has n / k rows within a few percent) and
            the figure is scaled by k / 16; the output says which. At k = 1
            this is honu_key_merge itself.
    read    the one host read of the batch's k + 1 offsets that those calls
            need for their nb and pointers (a device-to-host copy and the wait
            for it, by the host's clock, after the stream has drained).
The new call is never measured against itself: the yardstick is merges + read
(merges alone at k = 1).
Every point is verified before it is timed: the call's column, order, offsets
and counts against numpy (the sort of the two sides' keys together, stable, cut
by collection: per bucket A's rows before B's on equal keys), and the timed
per-collection merges against the same rows.

Timed as tools/key_route.py times its call: HIP events around windows, a
window one replay of a graph of `inner` calls, the windows alternating between
the two, the figure the median window per call with min and max.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's outputs are not numpy's."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from honu_amd import _lib  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
SAMPLE = 16  # the per-collection merges timed at most
POINTS = ((1, "uniform"), (16, "uniform"), (256, "uniform"), (4096, "uniform"), (16, "skewed"))


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| k | draw | resident | batch | largest bucket (A + B) | honu_key_merge_buckets us | k honu_key_merge us | "
          "merges timed | offsets read us | yardstick us | yardstick / merge_buckets | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['k']} | {r['draw']} | {r['resident']} | {r['batch']} | {r['largest']} | {cell('buckets')} | "
              f"{cell('merges')} | {r['merges_timed']} of {r['k']}{' (scaled)' if r['merges_scaled_by'] != 1 else ''} | "
              f"{cell('read') if r['k'] > 1 else '-'} | {r['yardstick_us']} | {r['yardstick_over_buckets']}x | "
              f"{'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] for r in rows)}))


def draw_members(rng, k, n, draw):
    if draw == "uniform":
        return rng.integers(0, k, n)
    return np.minimum(rng.geometric(0.5, n) - 1, k - 1)  # collection j holds about n / 2^(j + 1) rows


def run(a, lines):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    na = a.n
    batches = [int(x) for x in a.batch.split(",")]
    nmax = na + max(batches)
    codec = Codec(0, nmax + 2)
    L, c, s = codec.lib, codec.ctx, codec.stream
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    host = lambda t, nbytes, dt=np.uint8: t[:nbytes].cpu().numpy().view(dt)  # noqa: E731
    wb = int(L.honu_sort_keys_workspace(nmax))
    work, order, sorted_, valid = u8(wb), u8(4 * nmax), u8(29 * nmax), u8(8)

    def sort_order(keys):
        """honu_sort_keys' order of a key column (stable)."""
        d = up(keys)
        _lib.check(L.honu_sort_keys(c, P(d), 0, len(keys), P(order), P(sorted_), P(valid), P(work), wb, s), "honu_sort_keys")
        torch.cuda.synchronize()
        seq = host(order, 4 * len(keys), np.uint32).astype(np.int64)
        got = host(sorted_, 29 * len(keys)).reshape(-1, 29)
        assert np.array_equal(keys[seq], got)
        return seq

    def arena(keys, cls, k):
        """The keys bucket-major, each bucket in key order: (rows, offsets k + 1, each key's arena row)."""
        seq = sort_order(keys)
        g = np.argsort(cls[seq], kind="stable")
        src = seq[g]
        pos = np.empty(len(keys), np.int64)
        pos[src] = np.arange(len(keys))
        return keys[src], np.searchsorted(cls[src], np.arange(k + 1)).astype(np.uint64), pos

    keys_a = keys_objects(na, rng)
    na = len(keys_a)
    for nb in batches:
        keys_b = keys_objects(nb, rng)
        keys_b[: nb // 8] = keys_a[rng.integers(0, na, nb // 8)]  # an eighth of the batch puts stored keys again
        nb = len(keys_b)
        n = na + nb
        for k, draw in [p for p in POINTS if f"{p[0]}:{p[1]}" in a.points.split(",")]:
            cls_a, cls_b = draw_members(rng, k, na, draw), draw_members(rng, k, nb, draw)
            rows_a, off_a, pos_a = arena(keys_a, cls_a, k)
            rows_b, off_b, pos_b = arena(keys_b, cls_b, k)
            # numpy's merge: the sort of both sides' keys together (stable: A's first on equal keys), cut by collection
            seq = sort_order(np.concatenate([keys_a, keys_b]))
            cls = np.concatenate([cls_a, cls_b])
            src = seq[np.argsort(cls[seq], kind="stable")]
            want_rows = np.concatenate([keys_a, keys_b])[src]
            want_order = np.where(src < na, pos_a[np.minimum(src, na - 1)], pos_b[np.maximum(src - na, 0)] + na).astype(np.uint32)
            want_off = (off_a + off_b).astype(np.uint64)
            sa, sb = up(rows_a), up(rows_b)
            oa, ob = up(np.arange(na, dtype=np.uint32)), up(np.arange(nb, dtype=np.uint32))
            d_off_a, d_off_b = up(off_a), up(off_b)
            va, vb = up(np.diff(off_a)), up(np.diff(off_b))
            out, oout, off_out, cnt_out = u8(29 * n), u8(4 * n), u8(8 * (k + 1)), u8(8 * k)
            m_out, m_oout, m_valid = u8(29 * n), u8(4 * n), u8(8 * k)

            def buckets():
                _lib.check(L.honu_key_merge_buckets(c, k, P(sa), P(oa), P(d_off_a), 0, na, P(sb), P(ob), P(d_off_b), nb, 0,
                                                    na, P(out), P(oout), P(off_out), P(cnt_out), codec.stream),
                           "honu_key_merge_buckets")

            for t in (out, oout, off_out, cnt_out, m_out, m_oout):
                t.zero_()
            buckets()
            torch.cuda.synchronize()
            equal = bool(np.array_equal(host(off_out, 8 * (k + 1), np.uint64), want_off) and
                         np.array_equal(host(cnt_out, 8 * k, np.uint64), np.diff(want_off)) and
                         np.array_equal(host(out, 29 * n).reshape(n, 29), want_rows) and
                         np.array_equal(host(oout, 4 * n, np.uint32), want_order))
            timed = list(range(k)) if k <= SAMPLE else sorted(rng.choice(k, SAMPLE, replace=False).tolist())
            oa_h, ob_h, oo_h = off_a.astype(np.int64), off_b.astype(np.int64), want_off.astype(np.int64)

            def merges():
                for j in timed:
                    fa, fb, fo = int(oa_h[j]), int(ob_h[j]), int(oo_h[j])
                    _lib.check(L.honu_key_merge(c, P(sa) + 29 * fa, P(oa) + 4 * fa, P(va) + 8 * j, int(oa_h[j + 1]) - fa,
                                                P(sb) + 29 * fb, P(ob) + 4 * fb, P(vb) + 8 * j, int(ob_h[j + 1]) - fb, na,
                                                P(m_out) + 29 * fo, P(m_oout) + 4 * fo, P(m_valid) + 8 * j, codec.stream),
                               "honu_key_merge")

            merges()
            torch.cuda.synchronize()
            got_rows, got_order = host(m_out, 29 * n).reshape(n, 29), host(m_oout, 4 * n, np.uint32)
            for j in timed:
                lo, hi = int(oo_h[j]), int(oo_h[j + 1])
                equal = equal and bool(np.array_equal(got_rows[lo:hi], want_rows[lo:hi]) and
                                       np.array_equal(got_order[lo:hi], want_order[lo:hi]))
            inners = {"buckets": a.inner, "merges": 1 if len(timed) > 1 else a.inner}
            times = windows_us({"buckets": buckets, "merges": merges}, inners, a.reps)
            scale = k / len(timed)
            times["merges"] = tuple(x * scale for x in times["merges"])
            reads = []
            for _ in range(a.reps):  # the host read of the batch's offsets, the stream drained before it
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d_off_b[:8 * (k + 1)].cpu()
                reads.append((time.perf_counter() - t0) * 1e6)
            times["read"] = (statistics.median(reads), min(reads), max(reads))
            rec = {"tool": "key_merge_buckets", "k": k, "draw": draw, "resident": na, "batch": nb,
                   "largest": int(np.diff(oo_h).max()), "reps": a.reps, "inner": a.inner, "merges_inner": inners["merges"],
                   "merges_timed": len(timed), "merges_scaled_by": scale, "equals_numpy": equal}
            for name in ("buckets", "merges", "read"):
                med, lo, hi = times[name]
                rec[name + "_us"] = round(med, 1)
                rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
            yard = times["merges"][0] + (times["read"][0] if k > 1 else 0.0)
            rec["yardstick_us"] = round(yard, 1)
            rec["yardstick_over_buckets"] = round(yard / times["buckets"][0], 2)
            rec["buckets_ns_per_row"] = round(times["buckets"][0] * 1e3 / n, 3)
            rec["device"] = torch.cuda.get_device_name(0)
            rec["commit"] = a.commit
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="rows of the resident column")
    ap.add_argument("--batch", default=f"{1 << 16},{1 << 20}", help="rows of the batch, comma separated")
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
        sys.exit("tools/key_merge_buckets.py measures on the GPU: no device found")
    lines = []
    run(a, lines)
    print_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    wrong = [f"k {r['k']} {r['draw']} batch {r['batch']}" for r in map(json.loads, lines) if not r["equals_numpy"]]
    if wrong:  # a run whose outputs are wrong is no profile
        sys.exit("honu_key_merge_buckets' outputs differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
