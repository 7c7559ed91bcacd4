#!/usr/bin/env python3
"""Time honu_key_fetch: Cursor.Object() over the rows of a list, on a resident
sorted column of --n keys (1M, tools/sort_keys.py's objects_x16: n / 16 objects
of 16 versions) whose records are an encoded arena (the generator's --shape
records carrying those keys, marshalled on the device), at the points
    retrieve   every object's range, reversed, limit 1 (Retrieve(): n / 16 rows)
    versions   every object's range, reversed (Versions(): n rows)
    list       one range over everything (List(): n rows)
next to two yardsticks timed in the same run:
    torch      the stand-in a caller has today once the rows are on the device:
               the lengths from rec_off, cumsum, and a byte gather by
               repeat_interleave indices. Its byte total is handed over before
               the clock starts, which favours the stand-in: reading it is the
               host round trip the call avoids. Timed eagerly (events around
               --reps-torch runs after a warm-up), not from a graph: its index
               tensors take 16 bytes per fetched byte, and a graph would hold
               them once per captured call. A stand-in that does not fit the
               device's memory is reported as null.
    probe      honu_hbm_probe, the library's plain copy (mode 2: per-wave
               ranges, default cache policy, 2 workgroups per CU) over the same
               number of bytes, arena to values: what moving the bytes alone
               costs, with no rows, offsets or scan.
The column is sorted by honu_sort_keys, the ranges are honu_key_seek's and the
rows honu_key_list's (none of them timed). Every point is verified before it
is timed: d_val_off, d_val_total, d_status and every byte of d_values against
numpy's concatenation of the records the rows name.

The fetch and the probe are timed as tools/key_list.py times its call: HIP
events around windows, a window one replay of a graph of `inner` calls, the
windows alternating, the figure the median window per call with min and max.
GB/s counts the bytes read and written, 2 x the fetched bytes; the rows (16 B),
offsets (2 x 8 B read, 8 B written) and statuses per row are not counted.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's bytes are not numpy's."""
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
from honu_amd.metadata import HAS_VERSION, LIST_REVERSE, LIST_ROW_DTYPE  # noqa: E402
from honu_amd.object import Codec, DeviceBatch, _dev_bytes  # noqa: E402
from honu_amd.workload import gen_meta  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
POINTS = ("retrieve", "versions", "list")


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| point | rows | bytes fetched | mean B/row | honu_key_fetch us | hbm probe us | fetch / probe | "
          "torch stand-in us | stand-in / fetch | fetch GB/s (read + write) | of 8 TB/s | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        torch_cell = cell("torch") if r["torch_us"] is not None else "did not fit"
        ratio = f"{r['torch_over_fetch']}x" if r["torch_us"] is not None else "-"
        print(f"| {r['point']} | {r['rows']} | {r['bytes']} | {r['mean_bytes_per_row']} | {cell('fetch')} | "
              f"{cell('probe')} | {r['fetch_over_probe']}x | {torch_cell} | {ratio} | {r['fetch_gb_per_s']} | "
              f"{r['fetch_hbm_fraction']} | {'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] for r in rows)}))


def eager_us(fn, reps):
    """median, min, max over `reps` runs, by device events; one warm-up run first."""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--shape", default="small", help="the generator shape of the records")
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--reps-torch", type=int, default=3)
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
        sys.exit("tools/key_fetch.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    k = keys_objects(a.n, rng)
    n = len(k)
    codec = Codec(0, n + 2)
    L, c = codec.lib, codec.ctx
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    s = codec.stream
    # the records: generator rows that carry the column's keys, payloads filled on the device, marshalled
    meta, var, acl, reg, pay_off = gen_meta(a.seed, a.shape, 0, n)
    meta["present"] |= HAS_VERSION
    meta["object_id"] = k[:, 1:17]
    meta["vid"] = np.ascontiguousarray(k[:, 17:25]).view(">u8").reshape(n)
    meta["pid"] = np.ascontiguousarray(k[:, 25:29]).view(">u4").reshape(n)
    d_pay_off = _dev_bytes(pay_off, dev)
    d_payload = u8(int(pay_off[n]))
    _lib.check(L.honu_gen_payload(c, a.seed, 0, n, P(d_pay_off), P(d_payload), s), "honu_gen_payload")
    batch = DeviceBatch(_dev_bytes(meta, dev), _dev_bytes(var, dev), len(var), _dev_bytes(acl, dev), len(acl),
                        _dev_bytes(reg, dev), len(reg), d_payload, d_pay_off, n)
    enc = codec.marshal(batch)
    torch.cuda.synchronize()
    del batch, d_payload, meta, var
    rec_off_h = enc.out_off[:8 * (n + 1)].cpu().numpy().view(np.uint64).astype(np.int64)
    rec_bytes = int(rec_off_h[n])
    assert (enc.status[:4 * n].view(torch.int32) == 0).all()
    arena_h = enc.out[:rec_bytes].cpu().numpy()
    # the column, its objects' ranges and the whole-column range
    wb = int(L.honu_sort_keys_workspace(n))
    work, dk = u8(wb), u8(29 * n)
    sa, oa, va = u8(29 * n), u8(4 * n), u8(8)
    dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))
    _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(oa), P(sa), P(va), P(work), wb, s), "sort the column")
    torch.cuda.synchronize()
    order_h = oa[:4 * n].cpu().numpy().view(np.uint32)
    S_h = k[order_h]
    starts = np.concatenate([[0], np.flatnonzero((S_h[1:, :17] != S_h[:-1, :17]).any(axis=1)) + 1])
    nobj = len(starts)
    po = u8(29 * nobj)
    po[:29 * nobj].copy_(torch.from_numpy(S_h[starts].reshape(-1)))
    r_obj, r_all = u8(20 * nobj), u8(20)
    for plen, m, out in ((17, nobj, r_obj), (0, 1, r_all)):
        _lib.check(L.honu_key_seek(c, P(sa), P(va), n, P(po), 0, plen, m, P(oa), 0, P(out), s), "honu_key_seek")
    del work, dk
    table = {  # point -> (seek rows, m, limit, flags)
        "retrieve": (r_obj, nobj, 1, LIST_REVERSE), "versions": (r_obj, nobj, 0, LIST_REVERSE),
        "list": (r_all, 1, 0, 0)}
    d_rows, d_range_off, d_total = u8(16 * n), u8(8 * (nobj + 2)), u8(8)
    d_val_off, d_status, d_val_total = u8(8 * (n + 1)), u8(4 * n), u8(8)
    d_values = u8(rec_bytes)
    rec_off_t = enc.out_off[:8 * (n + 1)].view(torch.int64)
    arena_t = enc.out[:rec_bytes]
    lines = []
    for point in [p for p in a.points.split(",") if p]:
        ranges, m, limit, flags = table[point]
        _lib.check(L.honu_key_list(c, P(sa), P(oa), P(va), n, P(ranges), m, limit, flags, 0, 0, 0, P(d_range_off),
                                   P(d_rows), 0, n, P(d_total), s), "honu_key_list")
        torch.cuda.synchronize()
        w = int(d_total[:8].view(torch.int64).item())
        assert 0 < w <= n
        cap = w  # the list's rows, all of them: the call's scan and the copy's classes see cap, not the count
        rec_h = d_rows[:16 * w].cpu().numpy().view(LIST_ROW_DTYPE)["record"].astype(np.int64)
        lens_h = rec_off_h[rec_h + 1] - rec_off_h[rec_h]
        want_off = np.concatenate([[0], np.cumsum(lens_h)])
        total = int(want_off[-1])
        assert total <= rec_bytes  # no record twice at these points

        def call():
            _lib.check(L.honu_key_fetch(c, P(d_rows), P(d_total), cap, P(enc.out), P(enc.out_off), n, rec_bytes, 0,
                                        P(d_val_off), P(d_status), P(d_values), rec_bytes, P(d_val_total),
                                        codec.stream), "honu_key_fetch")

        def probe():
            _lib.check(L.honu_hbm_probe(c, 2, P(enc.out), P(d_values), total & ~15, 2, codec.stream), "honu_hbm_probe")

        # verified before it is timed
        for t in (d_val_off, d_status, d_val_total, d_values):
            t.zero_()
        call()
        torch.cuda.synchronize()
        want = np.concatenate([arena_h[x:y] for x, y in zip(rec_off_h[rec_h], rec_off_h[rec_h + 1])])
        equal = bool(int(d_val_total[:8].view(torch.int64).item()) == total and
                     np.array_equal(d_val_off[:8 * (cap + 1)].cpu().numpy().view(np.int64), want_off) and
                     not d_status[:4 * w].view(torch.int32).any().item() and
                     np.array_equal(d_values[:total].cpu().numpy(), want))
        # the stand-in: the rows' record column as int64 (prepared, not timed), the byte total from the host
        rec_t = d_rows[:16 * w].view(torch.int32).view(w, 4)[:, 2].to(torch.int64)
        kept = {}

        def stand_in():
            a0 = rec_off_t[rec_t]
            lens = rec_off_t[rec_t + 1] - a0
            off = torch.cumsum(lens, 0)
            shift = torch.repeat_interleave(a0 - (off - lens), lens, output_size=total)
            shift += torch.arange(total, device=dev)
            kept["values"], kept["off"] = arena_t[shift], off

        try:
            times_torch = eager_us(stand_in, a.reps_torch)
            equal = equal and bool(np.array_equal(kept["values"].cpu().numpy(), want))
        except torch.cuda.OutOfMemoryError:
            times_torch = None
        kept.clear()
        del want
        torch.cuda.empty_cache()
        inners = {"fetch": a.inner, "probe": a.inner}
        times = windows_us({"fetch": call, "probe": probe}, inners, a.reps)
        rec = {"tool": "key_fetch", "point": point, "resident": n, "objects": nobj, "shape": a.shape, "ranges": m,
               "limit": limit, "flags": flags, "rows": w, "cap": cap, "bytes": total, "arena_bytes": rec_bytes,
               "mean_bytes_per_row": round(total / w, 1), "reps": a.reps, "reps_torch": a.reps_torch, "inner": a.inner,
               "equals_numpy": equal}
        for name in ("fetch", "probe"):
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        rec["torch_us"] = round(times_torch[0], 1) if times_torch else None
        rec["torch_us_min_max"] = [round(times_torch[1], 1), round(times_torch[2], 1)] if times_torch else None
        rec["torch_over_fetch"] = round(times_torch[0] / times["fetch"][0], 1) if times_torch else None
        rec["fetch_over_probe"] = round(times["fetch"][0] / times["probe"][0], 2)
        rec["fetch_gb_per_s"] = round(2 * total / (times["fetch"][0] * 1e-6) / 1e9, 1)
        rec["probe_gb_per_s"] = round(2 * (total & ~15) / (times["probe"][0] * 1e-6) / 1e9, 1)
        rec["fetch_hbm_fraction"] = round(2 * total / (times["fetch"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
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
        sys.exit("honu_key_fetch's bytes differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
