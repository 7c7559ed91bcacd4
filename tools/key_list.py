#!/usr/bin/env python3
"""Time honu_key_list: a batch of cursor walks over a resident sorted column of
--n keys (1M, tools/sort_keys.py's objects_x16: n / 16 objects of 16 versions),
at the points
    versions   the probe_len 17 range of every object, reversed (Versions())
    list       one range over everything (List() as written)
    singles    n single-key ranges (the probe_len 29 range of every key)
    skewed     the whole-column range and then every object's range
    latest     HONU_LIST_LATEST over the whole column
    retrieve   every object's range, reversed, limit 1 (Retrieve())
next to one yardstick timed in the same run, the torch stand-in a caller has
today once the seek rows are on the device: repeat_interleave of the counts,
cumsum, index arithmetic, index_select of the rows and of the order (for
`latest` a gather at d_obj_off[1:] - 1). Its total is handed over before the
clock starts, which favours the stand-in: reading it is the host round trip
the call avoids.
The column is sorted by honu_sort_keys and the ranges are honu_key_seek's (not
timed). Every point is verified against numpy before it is timed: range, pos,
record and flags of every row, d_range_off, d_total and the 29 key bytes.

Device times are HIP events around windows after a warm-up. A window is one
replay of a graph that holds `inner` calls; the windows alternate between the
two, the figure is the median window over --reps, per call, with the windows'
min and max as the spread (tools/key_delete.py's windows). The bytes per
emitted row are the layout's: 29 + 4 read (the row, its order entry), 16 + 29
written, 78, against the 8 TB/s of the specification; the seek rows and offsets
are not counted. ns per emitted row of the skewed point beside the uniform
points' is the evidence that the expansion is load-balanced.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's rows are not numpy's; a point at which the
call is not ahead of the stand-in is reported as it is."""
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
from honu_amd.metadata import LIST_LATEST, LIST_REVERSE, LIST_ROW_DTYPE, LIST_ROW_HEAD, SEEK_DTYPE  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
BYTES_PER_ROW = 78  # 29 + 4 read, 16 + 29 written
NAMES = ("list", "torch")
POINTS = ("versions", "list", "singles", "skewed", "latest", "retrieve")


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| point | ranges | rows emitted | honu_key_list us | torch stand-in us | stand-in / list | ns per row | "
          "GB/s (78 B/row) | of 8 TB/s | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['point']} | {r['ranges']} | {r['rows']} | {cell('list')} | {cell('torch')} | "
              f"{r['torch_over_list']}x | {r['list_ns_per_row']} | {r['list_gb_per_s']} | {r['list_hbm_fraction']} | "
              f"{'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "list_ahead_everywhere": all(r["torch_over_list"] > 1 for r in rows),
                      "all_equal": all(r["equals_numpy"] for r in rows)}))


def expected(pos, end, limit, reverse):
    """numpy's rows of a plain call: (range, pos, range_off)."""
    counts = end - pos
    if limit:
        counts = np.minimum(counts, limit)
    off = np.concatenate([[0], np.cumsum(counts)])
    rng = np.repeat(np.arange(len(pos)), counts)
    k = np.arange(off[-1]) - off[rng]
    return rng, (end[rng] - 1 - k if reverse else pos[rng] + k), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner-list", type=int, default=40)
    ap.add_argument("--inner-torch", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_list.py measures on the GPU: no device found")
    n = a.n
    dev = torch.device("cuda", 0)
    codec = Codec(0, n + 2)
    L, c = codec.lib, codec.ctx
    tile, stage = _lib.C.c_int64(0), _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"list_tile", _lib.C.byref(tile)), "list_tile")
    _lib.check(L.honu_ctx_get_param(c, b"list_stage", _lib.C.byref(stage)), "list_stage")
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    rng = np.random.default_rng(a.seed)
    k = keys_objects(n, rng)
    n = len(k)
    s = codec.stream
    wb = int(L.honu_sort_keys_workspace(n))
    work, dk = u8(wb), u8(29 * n)
    sa, oa, va = u8(29 * n), u8(4 * n), u8(8)
    obj_off, obj_latest, objects = u8(8 * (n + 1)), u8(4 * n), u8(8)
    dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))
    _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(oa), P(sa), P(va), P(work), wb, s), "sort the column")
    _lib.check(L.honu_key_objects(c, P(dk), P(oa), P(va), n, P(obj_off), P(obj_latest), P(objects), P(work), wb, s),
               "honu_key_objects")
    torch.cuda.synchronize()
    order_h = oa[:4 * n].cpu().numpy().view(np.uint32)
    S_h = k[order_h]
    assert np.array_equal(S_h, sa[:29 * n].cpu().numpy().reshape(n, 29))
    starts = np.concatenate([[0], np.flatnonzero((S_h[1:, :17] != S_h[:-1, :17]).any(axis=1)) + 1])
    nobj = len(starts)
    ends = np.concatenate([starts[1:], [n]])
    assert int(objects[:8].view(torch.int64).item()) == nobj
    # the seek rows: every object's range (probe_len 17), every key's (probe_len 29), the whole column (probe_len 0)
    po, pk = u8(29 * nobj), sa
    po[:29 * nobj].copy_(torch.from_numpy(S_h[starts].reshape(-1)))
    r_obj, r_key, r_all = u8(20 * nobj), u8(20 * n), u8(20)
    for probes, plen, m, out in ((po, 17, nobj, r_obj), (pk, 29, n, r_key), (po, 0, 1, r_all)):
        _lib.check(L.honu_key_seek(c, P(sa), P(va), n, P(probes), 0, plen, m, P(oa), 0, P(out), s), "honu_key_seek")
    r_skew = torch.cat([r_all[:20], r_obj[:20 * nobj]])
    torch.cuda.synchronize()
    host = lambda t, m: t[:20 * m].cpu().numpy().view(SEEK_DTYPE)  # noqa: E731
    assert np.array_equal(host(r_obj, nobj)["pos"], starts) and np.array_equal(host(r_obj, nobj)["end"], ends)
    assert np.array_equal(host(r_key, n)["pos"], np.arange(n)) and np.array_equal(host(r_key, n)["end"], np.arange(n) + 1)
    assert (host(r_all, 1)["pos"][0], host(r_all, 1)["end"][0]) == (0, n)
    table = {  # point -> (seek rows, m, limit, flags)
        "versions": (r_obj, nobj, 0, LIST_REVERSE), "list": (r_all, 1, 0, 0), "singles": (r_key, n, 0, 0),
        "skewed": (r_skew, nobj + 1, 0, 0), "latest": (r_all, 1, 0, LIST_LATEST),
        "retrieve": (r_obj, nobj, 1, LIST_REVERSE)}
    cap = 2 * n
    d_rows, d_keys, d_off, d_total = u8(16 * cap), u8(29 * cap), u8(8 * (n + 2)), u8(8)
    S_t, order_t = sa[:29 * n].view(n, 29), oa[:4 * n].view(torch.int32)
    off_t = obj_off[:8 * (n + 1)].view(torch.int64)
    lines = []
    for point in [p for p in a.points.split(",") if p]:
        ranges, m, limit, flags = table[point]
        rh = host(ranges, m)
        pos_h, end_h = rh["pos"].astype(np.int64), rh["end"].astype(np.int64)
        if flags & LIST_LATEST:
            want_range, want_pos, want_off = np.zeros(nobj, np.int64), ends - 1, np.array([0, nobj])
        else:
            want_range, want_pos, want_off = expected(pos_h, end_h, limit, flags & LIST_REVERSE)
        total = int(want_off[-1])
        assert total <= cap

        def call():
            _lib.check(L.honu_key_list(c, P(sa), P(oa), P(va), n, P(ranges), m, limit, flags, P(obj_off), P(objects), 0,
                                       P(d_off), P(d_rows), P(d_keys), cap, P(d_total), codec.stream), "honu_key_list")

        # verified before it is timed
        for t in (d_rows, d_keys, d_off, d_total):
            t.zero_()
        call()
        torch.cuda.synchronize()
        got = d_rows[:16 * total].cpu().numpy().view(LIST_ROW_DTYPE)
        head = np.zeros(total, np.uint32)
        head[want_off[:-1][np.diff(want_off) > 0]] = LIST_ROW_HEAD
        equal = bool(int(d_total[:8].view(torch.int64).item()) == total and
                     np.array_equal(d_off[:8 * (m + 1)].cpu().numpy().view(np.uint64), want_off.astype(np.uint64)) and
                     np.array_equal(got["range"], want_range) and np.array_equal(got["pos"], want_pos) and
                     np.array_equal(got["record"], order_h[want_pos]) and np.array_equal(got["flags"], head) and
                     np.array_equal(d_keys[:29 * total].cpu().numpy().reshape(total, 29), S_h[want_pos]))
        # the stand-in: pos and end of the seek rows as int64 columns (prepared, not timed), the total from the host
        seek_t = ranges[:20 * m].view(torch.int32).view(m, 5)
        pos_t, end_t = seek_t[:, 0].to(torch.int64), seek_t[:, 1].to(torch.int64)
        ids, idx = torch.arange(m, device=dev), torch.arange(total, device=dev)
        kept = {}

        def stand_in():
            if flags & LIST_LATEST:
                p = off_t[1:nobj + 1] - 1
            else:
                counts = end_t - pos_t
                if limit:
                    counts = counts.clamp(max=limit)
                q = torch.repeat_interleave(ids, counts, output_size=total)
                kk = idx - (torch.cumsum(counts, 0) - counts)[q]
                p = end_t[q] - 1 - kk if flags & LIST_REVERSE else pos_t[q] + kk
            kept["pos"], kept["keys"], kept["rec"] = p, S_t.index_select(0, p), order_t.index_select(0, p)

        stand_in()
        torch.cuda.synchronize()
        equal = equal and bool(np.array_equal(kept["pos"].cpu().numpy(), want_pos) and
                               np.array_equal(kept["keys"].cpu().numpy(), S_h[want_pos]))
        inners = {"list": a.inner_list, "torch": a.inner_torch}
        times = windows_us({"list": call, "torch": stand_in}, inners, a.reps)
        rec = {"tool": "key_list", "point": point, "resident": n, "objects": nobj, "ranges": m, "limit": limit,
               "flags": flags, "rows": total, "list_tile": int(tile.value), "list_stage": int(stage.value),
               "reps": a.reps, "inner": inners, "equals_numpy": equal}
        for name in NAMES:
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        rec["torch_over_list"] = round(times["torch"][0] / times["list"][0], 1)
        rec["list_max_below_torch_min"] = bool(times["list"][2] < times["torch"][1])
        rec["list_ns_per_row"] = round(times["list"][0] * 1e3 / max(total, 1), 4)
        rec["bytes_per_row"] = BYTES_PER_ROW
        rec["list_gb_per_s"] = round(BYTES_PER_ROW * total / (times["list"][0] * 1e-6) / 1e9, 1)
        rec["list_hbm_fraction"] = round(BYTES_PER_ROW * total / (times["list"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
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
    wrong = [r["point"] for r in map(json.loads, lines) if not r["equals_numpy"]]
    if wrong:  # a run whose outputs are wrong is no profile
        sys.exit("honu_key_list's rows differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
