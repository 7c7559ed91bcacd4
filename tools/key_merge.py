#!/usr/bin/env python3
"""Time honu_key_merge: a batch of Puts merged into a resident sorted column
of --n keys (1M), at every point of
    key set   random, generator, objects_x16 (tools/sort_keys.py's three)
    batch     1 K, 64 K, 1 M keys (--batches)
next to the two other ways to the same three outputs, timed in the same run:
    resort    honu_sort_keys over the concatenated key column, which is all a
              caller could do before this entry point;
    torch     the same order from stock torch (tools/sort_keys.py's
              torch_order: four stable torch.sort passes over u64 words).
The resident column and the batch are sorted by honu_sort_keys first (not
timed: the column is resident, and a batch has to be sorted on either route
only where it is merged), so the run is the pipeline's own sort -> merge. In
every point the merge's column, order and valid count must equal the
re-sort's bit for bit, and its order torch's.

Device times are HIP events around windows after a warm-up. A window of the
merge or the re-sort is one replay of a graph that holds `inner` calls, so a
call of tens of microseconds is not timed at the rate the host issues it and
a window lasts milliseconds; torch's window is two eager calls (milliseconds
each). The windows alternate between the three, so a drift of the machine
falls on all alike; the figure is the median window over --reps, per call,
with the windows' min and max as the spread. The merge's bytes are its
layout's: every row and index read once and written once, 66 bytes per key,
against the 8 TB/s of the specification.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from honu_amd import _lib  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from sort_keys import keys_generator, keys_objects, keys_random, torch_order  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
BYTES_PER_KEY = 66  # 29 + 4 read, 29 + 4 written
NAMES = ("merge", "resort", "torch")


def windows_us(fns, inners, graphed, reps):
    """Per name: median, min and max over `reps` windows, per call, by device
    events; a graphed name's window is one replay of a graph of its `inner`
    calls, another's `inner` eager calls. The windows alternate between the names."""
    run = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if graphed[name]:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(inners[name]):
                    fn()
            g.replay()
            run[name] = g.replay
        else:
            run[name] = lambda fn=fn, k=inners[name]: [fn() for _ in range(k)]
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run[name]()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / inners[name])
    return {name: (statistics.median(t), min(t), max(t)) for name, t in out.items()}


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| resident | batch | set | merge us | re-sort us | torch us | re-sort / merge | GB/s (66 B/key) | of 8 TB/s | "
          "merge max < re-sort min |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['resident']} | {r['batch']} | {r['set']} | {cell('merge')} | {cell('resort')} | {cell('torch')} | "
              f"{r['resort_over_merge']}x | {r['merge_gb_per_s']} | {r['merge_hbm_fraction']} | "
              f"{'yes' if r['merge_max_below_resort_min'] else 'NO'} |")
    print(json.dumps({"points": len(rows),
                      "merge_beats_resort_everywhere": all(r["merge_max_below_resort_min"] for r in rows),
                      "all_equal": all(r["equals_resort"] and r["order_equals_torch"] for r in rows)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--batches", default="1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner-merge", type=int, default=0, help="merges per window (0: 100, or 25 from 256 K keys in the batch)")
    ap.add_argument("--inner-resort", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_merge.py measures on the GPU: no device found")
    na = a.n
    batches = [int(x) for x in a.batches.split(",")]
    top = na + max(batches)
    dev = torch.device("cuda", 0)
    codec = Codec(0, top)
    L, c = codec.lib, codec.ctx
    tile = _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"merge_tile", _lib.C.byref(tile)), "merge_tile")
    wb = int(L.honu_sort_keys_workspace(top))
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    work = u8(wb)
    dk = u8(29 * top)                                         # A's keys, then B's: the concatenated column
    sa, oa, va = u8(29 * na), u8(4 * na), u8(8)               # the resident sorted column
    sb, ob, vb = u8(29 * max(batches)), u8(4 * max(batches)), u8(8)
    m_s, m_o, m_v = u8(29 * top), u8(4 * top), u8(8)          # the merge's outputs
    r_s, r_o, r_v = u8(29 * top), u8(4 * top), u8(8)          # the re-sort's
    sign = torch.tensor(-(1 << 63), dtype=torch.int64, device=dev)
    rng = np.random.default_rng(a.seed)
    lines = []
    for set_name, make in (("random", keys_random), ("generator", keys_generator), ("objects_x16", keys_objects)):
        for nb in batches:
            n = na + nb
            s = codec.stream
            k = make(n, rng)
            dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))
            _lib.check(L.honu_sort_keys(c, P(dk), 0, na, P(oa), P(sa), P(va), P(work), wb, s), "sort A")
            _lib.check(L.honu_sort_keys(c, P(dk) + 29 * na, 0, nb, P(ob), P(sb), P(vb), P(work), wb, s), "sort B")
            torch.cuda.synchronize()

            def merge():
                _lib.check(L.honu_key_merge(c, P(sa), P(oa), P(va), na, P(sb), P(ob), P(vb), nb, na, P(m_s), P(m_o),
                                            P(m_v), codec.stream), "honu_key_merge")

            def resort():
                _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(r_o), P(r_s), P(r_v), P(work), wb, codec.stream),
                           "honu_sort_keys")

            def by_torch():
                return torch_order(dk[:29 * n], n, sign)

            inner_merge = a.inner_merge or (25 if nb >= 1 << 18 else 100)
            times = windows_us({"merge": merge, "resort": resort, "torch": by_torch},
                               {"merge": inner_merge, "resort": a.inner_resort, "torch": 2},
                               {"merge": True, "resort": True, "torch": False}, a.reps)
            for t in (m_s, m_o, m_v, r_s, r_o, r_v):
                t.zero_()
            merge()
            resort()
            t_order, _ = by_torch()
            torch.cuda.synchronize()
            rec = {"tool": "key_merge", "resident": na, "batch": nb, "set": set_name, "merge_tile": int(tile.value),
                   "reps": a.reps, "inner": {"merge": inner_merge, "resort": a.inner_resort, "torch": 2}}
            for name in NAMES:
                med, lo, hi = times[name]
                rec[name + "_us"] = round(med, 1)
                rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
            rec["equals_resort"] = bool(torch.equal(m_s[:29 * n], r_s[:29 * n]) and torch.equal(m_o[:4 * n], r_o[:4 * n])
                                        and torch.equal(m_v[:8], r_v[:8]))
            rec["order_equals_torch"] = bool((m_o[:4 * n].view(torch.int32).to(torch.int64) == t_order).all())
            rec["valid"] = int(m_v[:8].view(torch.int64).item())
            rec["resort_over_merge"] = round(times["resort"][0] / times["merge"][0], 1)
            rec["torch_over_merge"] = round(times["torch"][0] / times["merge"][0], 1)
            rec["merge_max_below_resort_min"] = bool(times["merge"][2] < times["resort"][1])
            rec["merge_bytes"] = BYTES_PER_KEY * n
            rec["merge_gb_per_s"] = round(BYTES_PER_KEY * n / (times["merge"][0] * 1e-6) / 1e9, 1)
            rec["merge_hbm_fraction"] = round(BYTES_PER_KEY * n / (times["merge"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
            rec["device"] = torch.cuda.get_device_name(0)
            rec["commit"] = a.commit
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    print_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
