#!/usr/bin/env python3
"""Time honu_key_filter: the live-object filter over the rows honu_key_list
wrote for a resident sorted column of --n keys (1M, tools/sort_keys.py's
objects_x16: n / 16 objects of 16 versions). The latest version of every
fourth object is a tombstone (a quarter of the objects are deleted) and one
older version of every eighth object is one too (every eighth object is also
a fourth one, so these lie in deleted objects; no point's kept rows depend on
them). The points:
    list_deleted        one range over everything (List() as written), HONU_FILTER_DELETED
    latest_tombstone    HONU_LIST_LATEST over the whole column, HONU_FILTER_TOMBSTONE
    retrieve_tombstone  every object's range, reversed, limit 1 (Retrieve()), HONU_FILTER_TOMBSTONE
    nothing             the whole-column list made without d_info: no row is flagged, none goes
    everything          the whole-column list over an info of tombstones only: every row goes
next to one yardstick timed in the same run, the torch stand-in a caller has
once the rows are on the device: a boolean mask over the rows' flags (for
DELETED a searchsorted of pos over d_obj_off[1:], a gather of d_latest and one
of the info's tombstone bytes), rows[mask] and keys[mask], and a cumsum of the
mask looked up at the range offsets. rows[mask] needs the kept count on the
host, so the stand-in is given it before the clock starts, as nonzero_static's
size, which favours the stand-in: reading it is the host round trip the call
avoids. The stand-in does not recompute HEAD.

The lists are honu_key_list's (not timed). Every point is verified against
numpy before it is timed: every kept row with its recomputed HEAD, the key
bytes, d_range_off_out and d_total_out.

Device times are HIP events around windows after a warm-up. A window is one
replay of a graph that holds `inner` calls; the windows alternate between the
two, the figure is the median window over --reps, per call, with the windows'
min and max as the spread (tools/key_delete.py's windows). The bytes per
listed row are the layout's: 16 read twice (mark, place) and, for a kept row,
29 read and 16 + 29 written; the masks, counts and offsets are not counted.

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
from honu_amd.metadata import (FILTER_DELETED, FILTER_TOMBSTONE, INFO_DTYPE, LIST_LATEST, LIST_REVERSE,  # noqa: E402
                               LIST_ROW_DTYPE, LIST_ROW_HEAD, LIST_ROW_TOMBSTONE)
from honu_amd.object import Codec  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
NAMES = ("filter", "torch")
POINTS = ("list_deleted", "latest_tombstone", "retrieve_tombstone", "nothing", "everything")


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| point | ranges | rows listed | rows kept | honu_key_filter us | torch stand-in us | stand-in / filter | "
          "ns per listed row | GB/s | of 8 TB/s | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['point']} | {r['ranges']} | {r['rows']} | {r['kept']} | {cell('filter')} | {cell('torch')} | "
              f"{r['torch_over_filter']}x | {r['filter_ns_per_row']} | {r['filter_gb_per_s']} | "
              f"{r['filter_hbm_fraction']} | {'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "filter_ahead_everywhere": all(r["torch_over_filter"] > 1 for r in rows),
                      "all_equal": all(r["equals_numpy"] for r in rows)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner-filter", type=int, default=40)
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
        sys.exit("tools/key_filter.py measures on the GPU: no device found")
    n = a.n
    dev = torch.device("cuda", 0)
    codec = Codec(0, n + 2)
    L, c = codec.lib, codec.ctx
    tile = _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"filter_tile", _lib.C.byref(tile)), "filter_tile")
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
    starts = np.concatenate([[0], np.flatnonzero((S_h[1:, :17] != S_h[:-1, :17]).any(axis=1)) + 1])
    nobj = len(starts)
    ends = np.concatenate([starts[1:], [n]])
    assert int(objects[:8].view(torch.int64).item()) == nobj
    latest_h = obj_latest[:4 * nobj].cpu().numpy().view(np.uint32)
    assert np.array_equal(latest_h, order_h[ends - 1])
    # the tombstones: the latest record of every fourth object, an older one of every eighth
    tomb_h = np.zeros(n, np.uint8)
    tomb_h[order_h[ends[0::4] - 1]] = 1
    older = np.arange(0, nobj, 8)
    older = older[ends[older] - starts[older] > 1]
    tomb_h[order_h[starts[older] + (ends[older] - starts[older] - 1) // 2]] = 1
    deleted_h = tomb_h[order_h[ends - 1]] != 0  # per object
    deleted_share = float(deleted_h.mean())

    def info_of(tomb):
        info = np.zeros(n, INFO_DTYPE)
        info["tombstone"] = tomb
        t = u8(32 * n)
        t[:32 * n].copy_(torch.from_numpy(info.view(np.uint8).reshape(-1)))
        return t

    info_d, info_all = info_of(tomb_h), info_of(np.ones(n, np.uint8))
    # the seek rows: every object's range (probe_len 17) and the whole column (probe_len 0)
    po = u8(29 * nobj)
    po[:29 * nobj].copy_(torch.from_numpy(S_h[starts].reshape(-1)))
    r_obj, r_all = u8(20 * nobj), u8(20)
    for probes, plen, m, out in ((po, 17, nobj, r_obj), (po, 0, 1, r_all)):
        _lib.check(L.honu_key_seek(c, P(sa), P(va), n, P(probes), 0, plen, m, P(oa), 0, P(out), s), "honu_key_seek")
    table = {  # point -> (seek rows, m, limit, list flags, the list's info, the info's tombstones, filter flags)
        "list_deleted": (r_all, 1, 0, 0, info_d, tomb_h, FILTER_DELETED),
        "latest_tombstone": (r_all, 1, 0, LIST_LATEST, info_d, tomb_h, FILTER_TOMBSTONE),
        "retrieve_tombstone": (r_obj, nobj, 1, LIST_REVERSE, info_d, tomb_h, FILTER_TOMBSTONE),
        "nothing": (r_all, 1, 0, 0, None, tomb_h, FILTER_TOMBSTONE),
        "everything": (r_all, 1, 0, 0, info_all, np.ones(n, np.uint8), FILTER_TOMBSTONE)}
    cap = n
    d_rows, d_keys, d_off, d_total = u8(16 * cap), u8(29 * cap), u8(8 * (nobj + 2)), u8(8)
    o_rows, o_keys, o_off, o_total = u8(16 * cap), u8(29 * cap), u8(8 * (nobj + 2)), u8(8)
    fwb = int(L.honu_key_filter_workspace(cap))
    fwork = u8(fwb)
    off_t = obj_off[:8 * (n + 1)].view(torch.int64)
    latest_t = obj_latest[:4 * n].view(torch.int32)
    lines = []
    for point in [p for p in a.points.split(",") if p]:
        ranges, m, limit, lflags, linfo, tomb, fflags = table[point]
        _lib.check(L.honu_key_list(c, P(sa), P(oa), P(va), n, P(ranges), m, limit, lflags, P(obj_off), P(objects),
                                   P(linfo), P(d_off), P(d_rows), P(d_keys), cap, P(d_total), s), "honu_key_list")
        torch.cuda.synchronize()
        total = int(d_total[:8].view(torch.int64).item())
        assert 0 < total <= cap
        rows_h = d_rows[:16 * total].cpu().numpy().view(LIST_ROW_DTYPE)
        keys_h = d_keys[:29 * total].cpu().numpy().reshape(total, 29)
        off_h = d_off[:8 * (m + 1)].cpu().numpy().view(np.uint64).astype(np.int64)
        finfo = linfo if linfo is not None else info_d

        def call():
            _lib.check(L.honu_key_filter(c, P(d_rows), P(d_keys), P(d_off), m, P(d_total), cap, fflags, P(va), n,
                                         P(obj_off), P(obj_latest), P(objects), P(finfo), P(o_rows), P(o_keys),
                                         P(o_off), P(o_total), P(fwork), fwb, codec.stream), "honu_key_filter")

        # numpy's answer
        if fflags & FILTER_DELETED:
            obj = np.searchsorted(ends, rows_h["pos"].astype(np.int64), side="right")
            keep = tomb[order_h[ends[obj] - 1]] == 0
        else:
            keep = (rows_h["flags"] & LIST_ROW_TOMBSTONE) == 0
        kept = int(keep.sum())
        rank = np.concatenate([[0], np.cumsum(keep)])
        want_off = rank[np.minimum(off_h, total)]
        want = rows_h[keep].copy()
        want["flags"] = (want["flags"] & ~np.uint32(LIST_ROW_HEAD)) | np.where(
            want_off[want["range"].astype(np.int64)] == np.arange(kept), np.uint32(LIST_ROW_HEAD), np.uint32(0))
        # verified before it is timed
        for t in (o_rows, o_keys, o_off, o_total):
            t.zero_()
        call()
        torch.cuda.synchronize()
        equal = bool(int(o_total[:8].view(torch.int64).item()) == kept and
                     np.array_equal(o_off[:8 * (m + 1)].cpu().numpy().view(np.uint64), want_off.astype(np.uint64)) and
                     o_rows[:16 * kept].cpu().numpy().tobytes() == want.tobytes() and
                     np.array_equal(o_keys[:29 * kept].cpu().numpy().reshape(kept, 29), keys_h[keep]))
        # the stand-in: the rows as int32 columns and the keys as rows (views, not timed), the kept count from the host
        rows_t = d_rows[:16 * total].view(torch.int32).view(total, 4)
        keys_t = d_keys[:29 * total].view(total, 29)
        loff_t = d_off[:8 * (m + 1)].view(torch.int64)
        tomb_t = finfo[:32 * n].view(n, 32)[:, 25]
        ends_t = off_t[1:nobj + 1]
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        out = {}

        def stand_in():
            if fflags & FILTER_DELETED:
                j = torch.searchsorted(ends_t, rows_t[:, 1].to(torch.int64), right=True)
                mask = tomb_t[latest_t[j].to(torch.int64)] == 0
            else:
                mask = (rows_t[:, 3] & LIST_ROW_TOMBSTONE) == 0
            idx = torch.nonzero_static(mask, size=kept).squeeze(1)  # rows[mask] with the count given
            out["rows"], out["keys"] = rows_t.index_select(0, idx), keys_t.index_select(0, idx)
            rank_t = torch.cat([zero, torch.cumsum(mask, 0)])
            out["off"] = rank_t[loff_t.clamp(max=total)]

        stand_in()
        torch.cuda.synchronize()
        equal = equal and bool(np.array_equal(out["rows"].cpu().numpy()[:, :3], want.view(np.uint32).reshape(kept, 4)[:, :3])
                               and np.array_equal(out["keys"].cpu().numpy(), keys_h[keep]) and
                               np.array_equal(out["off"].cpu().numpy(), want_off))
        inners = {"filter": a.inner_filter, "torch": a.inner_torch}
        times = windows_us({"filter": call, "torch": stand_in}, inners, a.reps)
        nbytes = 2 * 16 * total + (29 + 16 + 29) * kept
        rec = {"tool": "key_filter", "point": point, "resident": n, "objects": nobj, "deleted_share": round(deleted_share, 4),
               "ranges": m, "limit": limit, "list_flags": lflags, "filter_flags": fflags, "rows": total, "kept": kept,
               "filter_tile": int(tile.value), "reps": a.reps, "inner": inners, "equals_numpy": equal}
        for name in NAMES:
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        rec["torch_over_filter"] = round(times["torch"][0] / times["filter"][0], 1)
        rec["filter_max_below_torch_min"] = bool(times["filter"][2] < times["torch"][1])
        rec["filter_ns_per_row"] = round(times["filter"][0] * 1e3 / total, 4)
        rec["bytes"] = nbytes
        rec["filter_gb_per_s"] = round(nbytes / (times["filter"][0] * 1e-6) / 1e9, 1)
        rec["filter_hbm_fraction"] = round(nbytes / (times["filter"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
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
        sys.exit("honu_key_filter's rows differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
