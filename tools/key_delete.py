#!/usr/bin/env python3
"""Time honu_key_delete: a batch of Deletes from a resident sorted column of
--n keys (1M), at the points
    exact       1 K, 64 K, 1 M delete rows at probe_len 29 over each key set
                (random, generator, objects_x16: tools/sort_keys.py's three);
                half of the rows are keys of the column, half are not stored
    objects     1 K, 16 K ObjectPrefix rows at probe_len 17 over objects_x16
                (every version of those objects goes: the loop of Store.Drop)
    superseded  HONU_DELETE_SUPERSEDED alone over each key set with one key in
                16 stored twice
next to two yardsticks timed in the same run:
    resort      honu_sort_keys over the column's keys with the removed records'
                statuses set, which is all a caller could do before this entry
                point; the status column is prepared before the clock starts,
                which favours this route;
    merge       honu_key_merge of the column and 1 K keys: the sibling that
                moves the same rows once, reported beside the delete, not a bar.
The column and the delete list are sorted by honu_sort_keys first (not timed).
In every point the delete's rows [0, kept), their indices and the count must
equal the re-sort's bit for bit, and all n rows, indices and both counts
numpy's (kept rows, removed rows in column order, computed on the host from
the sorted column).

Device times are HIP events around windows after a warm-up. A window is one
replay of a graph that holds `inner` calls, so a call of tens of microseconds
is not timed at the rate the host issues it and a window lasts milliseconds.
The windows alternate between the three, so a drift of the machine falls on
all alike; the figure is the median window over --reps, per call, with the
windows' min and max as the spread. The delete's bytes are its layout's: the
mark pass reads every row (29), the place pass reads and writes every row and
index (66), 95 bytes per key, against the 8 TB/s of the specification; the
delete list and the 136 bytes of mask and count per tile are not counted.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's outputs are not the re-sort's and numpy's; a
point at which the delete is not ahead of the re-sort is reported as it is."""
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
from honu_amd.metadata import DELETE_SUPERSEDED  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from sort_keys import keys_generator, keys_objects, keys_random  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
BYTES_PER_KEY = 95  # mark: 29 read; place: 29 + 4 read, 29 + 4 written
NAMES = ("delete", "resort", "merge")
MAKE = {"random": keys_random, "generator": keys_generator, "objects_x16": keys_objects}


def windows_us(fns, inners, reps):
    """Per name: median, min and max over `reps` windows, per call, by device
    events; a window is one replay of a graph of the name's `inner` calls. The
    windows alternate between the names."""
    run = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(inners[name]):
                fn()
        g.replay()
        run[name] = g.replay
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
    print("| point | set | delete rows | probe_len | removed | delete us | re-sort us | merge 1M + 1 K us | re-sort / delete | "
          "GB/s (95 B/key) | of 8 TB/s | delete max < re-sort min |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['point']} | {r['set']} | {r['delete_rows']} | {r['probe_len']} | {r['removed']} | {cell('delete')} | "
              f"{cell('resort')} | {cell('merge')} | {r['resort_over_delete']}x | {r['delete_gb_per_s']} | "
              f"{r['delete_hbm_fraction']} | {'yes' if r['delete_max_below_resort_min'] else 'NO'} |")
    print(json.dumps({"points": len(rows),
                      "delete_beats_resort_everywhere": all(r["delete_max_below_resort_min"] for r in rows),
                      "all_equal": all(r["equals_resort"] and r["equals_numpy"] for r in rows)}))


def prefixes(k, probe_len):
    """The rows' first probe_len bytes as one fixed-length bytes value each (equal values: equal bytes)."""
    return np.ascontiguousarray(k[:, :probe_len]).view(f"S{probe_len}").reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--exact", default="1024,65536,1048576", help="delete rows at probe_len 29")
    ap.add_argument("--objects", default="1024,16384", help="ObjectPrefix rows at probe_len 17")
    ap.add_argument("--sets", default="random,generator,objects_x16", help="key sets of the exact and superseded points")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner-delete", type=int, default=50)
    ap.add_argument("--inner-resort", type=int, default=4)
    ap.add_argument("--inner-merge", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_delete.py measures on the GPU: no device found")
    n = a.n
    exact = [int(x) for x in a.exact.split(",") if x]
    objects = [int(x) for x in a.objects.split(",") if x]
    sets = [s for s in a.sets.split(",") if s]
    points = [("exact", s, m, 29, 0) for s in sets for m in exact]
    points += [("objects", "objects_x16", m, 17, 0) for m in objects]
    points += [("superseded", s, 0, 29, DELETE_SUPERSEDED) for s in sets]
    mmax = max([1] + [p[2] for p in points])
    nb = 1024  # the merge yardstick's batch
    dev = torch.device("cuda", 0)
    codec = Codec(0, max(n, mmax))
    L, c = codec.lib, codec.ctx
    tile = _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"delete_tile", _lib.C.byref(tile)), "delete_tile")
    wb = int(L.honu_sort_keys_workspace(max(n, mmax)))
    dwb = int(L.honu_key_delete_workspace(n))
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    work, dwork = u8(wb), u8(dwb)
    dk, st2 = u8(29 * n), u8(4 * n)                          # the column's keys in record order; the re-sort's statuses
    sa, oa, va = u8(29 * n), u8(4 * n), u8(8)                # the resident sorted column
    kd, sd, od, vd = u8(29 * mmax), u8(29 * mmax), u8(4 * mmax), u8(8)  # the delete list
    kb, sb, ob, vb = u8(29 * nb), u8(29 * nb), u8(4 * nb), u8(8)        # the merge yardstick's batch
    d_s, d_o, d_v, d_r = u8(29 * n), u8(4 * n), u8(8), u8(8)            # the delete's outputs
    r_s, r_o, r_v = u8(29 * n), u8(4 * n), u8(8)                        # the re-sort's
    m_s, m_o, m_v = u8(29 * (n + nb)), u8(4 * (n + nb)), u8(8)          # the merge's
    rng = np.random.default_rng(a.seed)
    lines = []
    for point, set_name, m, probe_len, flags in points:
        s = codec.stream
        make = MAKE[set_name]
        k = make(n, rng)
        if flags:  # one key in 16 stored twice: rows 0, 16, ... repeat rows 1, 17, ...
            k[0::16] = k[1::16]
        if point == "objects":  # m of the column's objects by their ObjectPrefix, the version bytes zero
            pre = np.unique(prefixes(k, 17))
            del_k = np.zeros((m, 29), np.uint8)
            del_k[:, :17] = np.frombuffer(rng.choice(pre, m, replace=False).tobytes(), np.uint8).reshape(m, 17)
        else:  # half of the rows are keys of the column, half fresh ones
            del_k = np.concatenate([k[rng.choice(n, (m + 1) // 2, replace=False)], make(max(m // 2, 16), rng)[:m // 2]])
        dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))
        _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(oa), P(sa), P(va), P(work), wb, s), "sort the column")
        if m:
            kd[:29 * m].copy_(torch.from_numpy(del_k.reshape(-1)))
            _lib.check(L.honu_sort_keys(c, P(kd), 0, m, P(od), P(sd), P(vd), P(work), wb, s), "sort the delete list")
        kb[:29 * nb].copy_(torch.from_numpy(make(max(nb, 16), rng)[:nb].reshape(-1)))
        _lib.check(L.honu_sort_keys(c, P(kb), 0, nb, P(ob), P(sb), P(vb), P(work), wb, s), "sort the merge's batch")
        torch.cuda.synchronize()
        # which rows go, by numpy over the sorted column
        order_h = oa[:4 * n].cpu().numpy().view(np.uint32)
        S_h = k[order_h]
        assert np.array_equal(S_h, sa[:29 * n].cpu().numpy().reshape(n, 29))
        drop = np.isin(prefixes(S_h, probe_len), prefixes(del_k, probe_len)) if m else np.zeros(n, bool)
        if flags:
            drop[:-1] |= (S_h[:-1] == S_h[1:]).all(axis=1)
        kept, removed = int((~drop).sum()), int(drop.sum())
        want_order = np.concatenate([order_h[~drop], order_h[drop]])
        status = np.zeros(n, np.int32)
        status[order_h[drop]] = 8  # the removed records, for the re-sort: prepared here, not timed
        st2[:4 * n].copy_(torch.from_numpy(status).view(torch.uint8))
        torch.cuda.synchronize()

        def delete():
            _lib.check(L.honu_key_delete(c, P(sa), P(oa), P(va), n, P(sd) if m else 0, P(vd) if m else 0, m, probe_len,
                                         flags, P(d_s), P(d_o), P(d_v), P(d_r), P(dwork), dwb, codec.stream),
                       "honu_key_delete")

        def resort():
            _lib.check(L.honu_sort_keys(c, P(dk), P(st2), n, P(r_o), P(r_s), P(r_v), P(work), wb, codec.stream),
                       "honu_sort_keys")

        def merge():
            _lib.check(L.honu_key_merge(c, P(sa), P(oa), P(va), n, P(sb), P(ob), P(vb), nb, n, P(m_s), P(m_o), P(m_v),
                                        codec.stream), "honu_key_merge")

        inners = {"delete": a.inner_delete, "resort": a.inner_resort, "merge": a.inner_merge}
        times = windows_us({"delete": delete, "resort": resort, "merge": merge}, inners, a.reps)
        for t in (d_s, d_o, d_v, d_r, r_s, r_o, r_v):
            t.zero_()
        delete()
        resort()
        torch.cuda.synchronize()
        rec = {"tool": "key_delete", "point": point, "resident": n, "delete_rows": m, "probe_len": probe_len,
               "flags": flags, "set": set_name, "delete_tile": int(tile.value), "reps": a.reps, "inner": inners,
               "kept": kept, "removed": removed}
        for name in NAMES:
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        got_kept, got_removed = int(d_v[:8].view(torch.int64).item()), int(d_r[:8].view(torch.int64).item())
        rec["equals_resort"] = bool(got_kept == kept and torch.equal(d_v[:8], r_v[:8]) and
                                    torch.equal(d_s[:29 * kept], r_s[:29 * kept]) and
                                    torch.equal(d_o[:4 * kept], r_o[:4 * kept]))
        got_order = d_o[:4 * n].cpu().numpy().view(np.uint32)
        rec["equals_numpy"] = bool(got_kept == kept and got_removed == removed and np.array_equal(got_order, want_order)
                                   and np.array_equal(d_s[:29 * n].cpu().numpy().reshape(n, 29), k[want_order]))
        rec["resort_over_delete"] = round(times["resort"][0] / times["delete"][0], 1)
        rec["delete_over_merge"] = round(times["delete"][0] / times["merge"][0], 2)
        rec["delete_max_below_resort_min"] = bool(times["delete"][2] < times["resort"][1])
        rec["delete_bytes"] = BYTES_PER_KEY * n
        rec["delete_gb_per_s"] = round(BYTES_PER_KEY * n / (times["delete"][0] * 1e-6) / 1e9, 1)
        rec["delete_hbm_fraction"] = round(BYTES_PER_KEY * n / (times["delete"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
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
    wrong = [f"{r['point']}/{r['set']}/{r['delete_rows']}" for r in map(json.loads, lines)
             if not (r["equals_resort"] and r["equals_numpy"])]
    if wrong:  # a run whose outputs are wrong is no profile
        sys.exit("honu_key_delete's outputs differ from the re-sort's or numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
