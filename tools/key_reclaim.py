#!/usr/bin/env python3
"""Time honu_key_reclaim: the records arena and the per-record arrays of a
resident store compacted to the records its column still names, at two shapes
    small   --n-small keys (1M), the generator's Small records
    large   --n-large keys (64 K), the generator's Large records
(tools/sort_keys.py's objects_x16: n / 16 objects of 16 versions; the records
carry those keys and are marshalled on the device), each after a
honu_key_delete of the 17-byte prefixes of so many objects that 15/16, 1/2 and
1/16 of the records stay. The call is given everything a store holds: the
delete's order and count, the unsorted keys, their statuses, the
honu_record_info rows, the arena and its offsets, and d_remap.
Next to it two yardsticks, timed in the same run, neither the code under test:
    route   what the calls before it offer: honu_key_seek of the empty probe,
            then honu_key_list (cap n, with keys) -> honu_key_fetch ->
            honu_decode_headers: an arena in key order with its info rows
            decoded again. The renumbering of the column, which that route
            leaves to the caller, is not in it.
    probe   honu_hbm_probe, the library's plain copy (mode 2, 2 workgroups per
            CU) over the same number of bytes: what moving the bytes alone costs.
Every point is verified before it is timed: d_kept, d_val_total, d_order_out,
d_remap, d_source, d_rec_off_out, d_status, the three gathered arrays and every
byte of d_values against numpy; and reclaim's records against the route's:
record new(order[p]) of d_values is the same byte string as the route's row p.

Timed as tools/key_fetch.py times its call: HIP events around windows, a
window one replay of a graph of `inner` calls, the windows alternating between
the three, the figure the median window per call with min and max. GB/s counts
the record bytes read and written, 2 x the kept bytes; the bytes per record
beside them are not counted.

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
from honu_amd.metadata import HAS_VERSION, INFO_DTYPE, SEEK_NONE  # noqa: E402
from honu_amd.object import Codec, DeviceBatch, _dev_bytes  # noqa: E402
from honu_amd.workload import gen_meta  # noqa: E402
from key_delete import windows_us  # noqa: E402
from sort_keys import keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
HBM_BYTES_PER_S = 8e12
STAY = {"15/16": 15 / 16, "1/2": 1 / 2, "1/16": 1 / 16}


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| shape | records | stay | kept | kept bytes | honu_key_reclaim us | route (a) us | hbm probe (b) us | "
          "reclaim / (a) | reclaim / (b) | reclaim GB/s (read + write) | of 8 TB/s | reclaim max < (a) min | "
          "equals numpy | equals (a) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['shape']} | {r['records']} | {r['stay']} | {r['kept']} | {r['bytes']} | {cell('reclaim')} | "
              f"{cell('route')} | {cell('probe')} | {r['reclaim_over_route']}x | {r['reclaim_over_probe']}x | "
              f"{r['reclaim_gb_per_s']} | {r['reclaim_hbm_fraction']} | "
              f"{'yes' if r['reclaim_max_below_route_min'] else 'NO'} | {'yes' if r['equals_numpy'] else 'NO'} | "
              f"{'yes' if r['equals_route'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] and r["equals_route"] for r in rows),
                      "reclaim_beats_route_everywhere": all(r["reclaim_max_below_route_min"] for r in rows)}))


def same_runs(values, arena, off, source):
    """values == the records `source` (ascending) of the CSR arena, back to back: compared run by run."""
    if not len(source):
        return True
    cut = np.flatnonzero(np.diff(source) != 1) + 1
    first = np.concatenate([[0], cut])
    last = np.concatenate([cut, [len(source)]]) - 1
    at = 0
    for a, b in zip(off[source[first]], off[source[last] + 1]):
        if not np.array_equal(values[at:at + b - a], arena[a:b]):
            return False
        at += b - a
    return at == len(values)


def run_shape(a, shape, n_keys, lines):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    k = keys_objects(n_keys, rng)
    n = len(k)
    codec = Codec(0, n + 2)
    L, c = codec.lib, codec.ctx
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    s = codec.stream
    # the records: generator rows that carry the column's keys, payloads filled on the device, marshalled
    meta, var, acl, reg, pay_off = gen_meta(a.seed, shape, 0, n)
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
    torch.cuda.empty_cache()
    off_h = enc.out_off[:8 * (n + 1)].cpu().numpy().view(np.uint64).astype(np.int64)
    rec_bytes = int(off_h[n])
    assert (enc.status[:4 * n].view(torch.int32) == 0).all()
    arena_h = enc.out[:rec_bytes].cpu().numpy()
    # the store's per-record state: the unsorted keys, their statuses, the info rows
    dk, dst, d_info = u8(29 * n), u8(4 * n).zero_(), u8(32 * n)
    dk[:29 * n].copy_(torch.from_numpy(k.reshape(-1)))
    _lib.check(L.honu_decode_headers(c, P(enc.out), P(enc.out_off), n, P(d_info), s), "honu_decode_headers")
    # the column and its objects
    wb = int(L.honu_sort_keys_workspace(n))
    work = u8(wb)
    sa, oa, va = u8(29 * n), u8(4 * n), u8(8)
    _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(oa), P(sa), P(va), P(work), wb, s), "sort the column")
    torch.cuda.synchronize()
    info_h = d_info[:32 * n].cpu().numpy().reshape(n, 32)
    S_h = k[oa[:4 * n].cpu().numpy().view(np.uint32)]
    starts = np.concatenate([[0], np.flatnonzero((S_h[1:, :17] != S_h[:-1, :17]).any(axis=1)) + 1])
    nobj = len(starts)
    whole, r_all = u8(29).zero_(), u8(20)
    # the delete's and the calls' outputs
    dwb, rwb = int(L.honu_key_delete_workspace(n)), int(L.honu_key_reclaim_workspace(n))
    dwork, rwork = u8(dwb), u8(rwb)
    s3, o3, v3, r3 = u8(29 * n), u8(4 * n), u8(8), u8(8)
    pd, sd, od, vd = u8(29 * nobj), u8(29 * nobj), u8(4 * nobj), u8(8)
    order_out, remap, source = u8(4 * n), u8(4 * n), u8(4 * n)
    keys_out, kst_out, info_out = u8(29 * n), u8(4 * n), u8(32 * n)
    off_out, status, kept_d, total_d = u8(8 * (n + 1)), u8(4 * n), u8(8), u8(8)
    values_r, values_a = u8(rec_bytes), u8(rec_bytes)
    rows_a, range_off_a, total_a, keys_a = u8(16 * n), u8(16), u8(8), u8(29 * n)
    val_off_a, status_a, val_total_a, info_a = u8(8 * (n + 1)), u8(4 * n), u8(8), u8(32 * n)
    for stay in [p for p in a.points.split(",") if p]:
        # delete the 17-byte prefixes of the objects that go: every record of an object goes with it
        gone = np.sort(rng.permutation(nobj)[:nobj - int(round(nobj * STAY[stay]))])
        m = len(gone)
        pd[:29 * m].copy_(torch.from_numpy(S_h[starts[gone]].reshape(-1)))
        _lib.check(L.honu_sort_keys(c, P(pd), 0, m, P(od), P(sd), P(vd), P(work), wb, s), "sort the delete list")
        _lib.check(L.honu_key_delete(c, P(sa), P(oa), P(va), n, P(sd), P(vd), m, 17, 0, P(s3), P(o3), P(v3), P(r3),
                                     P(dwork), dwb, s), "honu_key_delete")
        torch.cuda.synchronize()
        v = int(v3[:8].view(torch.int64).item())
        o3_h = o3[:4 * n].cpu().numpy().view(np.uint32).astype(np.int64)

        def call():
            _lib.check(L.honu_key_reclaim(
                c, P(o3), P(v3), n, P(dk), P(dst), P(d_info), P(enc.out), P(enc.out_off), n, rec_bytes, 0,
                P(order_out), P(remap), P(source), P(keys_out), P(kst_out), P(info_out), P(off_out), P(status),
                P(values_r), rec_bytes, P(kept_d), P(total_d), P(rwork), rwb, codec.stream), "honu_key_reclaim")

        def route():
            st = codec.stream
            _lib.check(L.honu_key_seek(c, P(s3), P(v3), n, P(whole), 0, 0, 1, P(o3), 0, P(r_all), st), "honu_key_seek")
            _lib.check(L.honu_key_list(c, P(s3), P(o3), P(v3), n, P(r_all), 1, 0, 0, 0, 0, 0, P(range_off_a), P(rows_a),
                                       P(keys_a), n, P(total_a), st), "honu_key_list")
            _lib.check(L.honu_key_fetch(c, P(rows_a), P(total_a), n, P(enc.out), P(enc.out_off), n, rec_bytes, 0,
                                        P(val_off_a), P(status_a), P(values_a), rec_bytes, P(val_total_a), st),
                       "honu_key_fetch")
            _lib.check(L.honu_decode_headers(c, P(values_a), P(val_off_a), n, P(info_a), st), "honu_decode_headers")

        # numpy's reclaim
        mark = np.zeros(n, bool)
        mark[o3_h[:v]] = True
        src = np.flatnonzero(mark)
        kept = len(src)
        want_remap = np.full(n, SEEK_NONE, np.uint32)
        want_remap[src] = np.arange(kept, dtype=np.uint32)
        want_order = np.full(n, SEEK_NONE, np.uint32)
        want_order[:v] = want_remap[o3_h[:v]]
        lens = off_h[src + 1] - off_h[src]
        want_off = np.zeros(n + 1, np.int64)
        want_off[1:kept + 1] = np.cumsum(lens)
        want_off[kept + 1:] = want_off[kept]
        total = int(want_off[kept])
        # verified before it is timed
        for t in (order_out, remap, source, keys_out, kst_out, info_out, off_out, status, kept_d, total_d, values_r):
            t.zero_()
        call()
        route()
        torch.cuda.synchronize()
        host = lambda t, nbytes, dt=np.uint8: t[:nbytes].cpu().numpy().view(dt)  # noqa: E731
        values_h = host(values_r, total)
        equal = bool(
            int(kept_d[:8].view(torch.int64).item()) == kept and int(total_d[:8].view(torch.int64).item()) == total and
            np.array_equal(host(order_out, 4 * n, np.uint32), want_order) and
            np.array_equal(host(remap, 4 * n, np.uint32), want_remap) and
            np.array_equal(host(source, 4 * kept, np.uint32), src) and
            np.array_equal(host(off_out, 8 * (n + 1), np.int64), want_off) and
            not host(status, 4 * kept, np.int32).any() and not host(kst_out, 4 * kept, np.int32).any() and
            np.array_equal(host(keys_out, 29 * kept).reshape(kept, 29), k[src]) and
            np.array_equal(host(info_out, 32 * kept).reshape(kept, 32), info_h[src]) and
            same_runs(values_h, arena_h, off_h, src))
        # the route's records: row p of its arena is record new(order[p]) of reclaim's
        off_a = host(val_off_a, 8 * (n + 1), np.int64)
        values_a_h = host(values_a, int(off_a[v]))
        j = want_order[:v].astype(np.int64)
        same = bool(int(total_a[:8].view(torch.int64).item()) == v == kept and int(off_a[v]) == total and
                    np.array_equal(np.diff(off_a[:v + 1]), want_off[j + 1] - want_off[j]))
        if same:
            for p in range(v):
                x, y = want_off[j[p]], off_a[p]
                ln = off_a[p + 1] - y
                if values_h[x:x + ln].tobytes() != values_a_h[y:y + ln].tobytes():
                    same = False
                    break
        # the route's second decode gives the info rows reclaim copied, but for data_off, which it rebases
        ia, ir = host(info_a, 32 * v).view(INFO_DTYPE), info_h[src][j].copy().reshape(-1).view(INFO_DTYPE)
        for f in INFO_DTYPE.names:
            if f != "data_off":
                same = same and bool(np.array_equal(ia[f], ir[f]))
        del values_h, values_a_h

        def probe():
            _lib.check(L.honu_hbm_probe(c, 2, P(enc.out), P(values_r), total & ~15, 2, codec.stream), "honu_hbm_probe")

        inners = {"reclaim": a.inner, "route": a.inner, "probe": a.inner}
        times = windows_us({"reclaim": call, "route": route, "probe": probe}, inners, a.reps)
        rec = {"tool": "key_reclaim", "shape": shape, "records": n, "objects": nobj, "stay": stay, "deleted_objects": m,
               "kept": kept, "bytes": total, "arena_bytes": rec_bytes, "mean_bytes_per_record": round(total / kept, 1),
               "reps": a.reps, "inner": a.inner, "equals_numpy": equal, "equals_route": same}
        for name in ("reclaim", "route", "probe"):
            med, lo, hi = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo, 1), round(hi, 1)]
        rec["reclaim_over_route"] = round(times["reclaim"][0] / times["route"][0], 2)
        rec["reclaim_over_probe"] = round(times["reclaim"][0] / times["probe"][0], 2)
        rec["reclaim_max_below_route_min"] = bool(times["reclaim"][2] < times["route"][1])
        rec["reclaim_gb_per_s"] = round(2 * total / (times["reclaim"][0] * 1e-6) / 1e9, 1)
        rec["probe_gb_per_s"] = round(2 * (total & ~15) / (times["probe"][0] * 1e-6) / 1e9, 1)
        rec["reclaim_hbm_fraction"] = round(2 * total / (times["reclaim"][0] * 1e-6) / HBM_BYTES_PER_S, 3)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["commit"] = a.commit
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-small", type=int, default=1 << 20, help="keys of the resident column of Small records")
    ap.add_argument("--n-large", type=int, default=1 << 16, help="keys of the resident column of Large records")
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--points", default=",".join(STAY), help="the share of the records that stays")
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
        sys.exit("tools/key_reclaim.py measures on the GPU: no device found")
    lines = []
    for shape in [x for x in a.shapes.split(",") if x]:
        run_shape(a, shape, {"small": a.n_small, "large": a.n_large}[shape], lines)
        torch.cuda.empty_cache()
    print_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    wrong = [f"{r['shape']} {r['stay']}" for r in map(json.loads, lines) if not (r["equals_numpy"] and r["equals_route"])]
    if wrong:  # a run whose outputs are wrong is no profile
        sys.exit("honu_key_reclaim's outputs differ from numpy's or the route's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
