#!/usr/bin/env python3
"""Time honu_key_next: the version each of a batch of Updates writes, over a
resident sorted column of --n keys (1M, tools/sort_keys.py's objects_x16: n /
16 objects of 16 versions; the latest version of every fourth object is a
tombstone). The call is given d_order, d_info and d_meta, so a point holds the
whole of it: pack, sort, rank, both bounds in the column, the stored scalar,
the row, the key and the stamped honu_meta row. The points:
    distinct_1K, distinct_64K, distinct_1M   m requests, no two for the same
                        object: the column's objects in random order and, past
                        its n / 16 objects, object IDs it does not hold
    runs_64K_over_4K    64 K requests over 4 K stored objects, 16 each, shuffled
next to two yardsticks timed in the same run by the same method:
    sort_seek   honu_sort_keys over the m request rows and honu_key_seek of
                the m 17-byte probes (with d_order and d_info): the two
                existing calls whose work the new call contains. Its rows are
                the requests with 12 zero bytes behind the 17, as the call
                packs them, so both sorts skip the same twelve digit passes.
                What the call takes beyond them is its pack, rank and stamp;
                the margin of that comparison is the two calls' own window
                spread;
    torch       the stand-in a caller has on the device: the object IDs as two
                big-endian u64 words (given, not timed), two stable torch.sort
                passes, the run starts by a compare and a cummax (unique
                without its host read), searchsorted of the first word over
                the column's, gathers of the stored VID, PID and tombstone,
                and a scatter back through the order. It compares only the
                first 8 bytes of an ID in the column and builds neither the
                keys nor the honu_meta rows, which favours the stand-in.

Every point is verified against numpy before it is timed: every honu_next
row, key and key status, the stamped fields of d_meta and every byte of the
rows that are not assigned. The stand-in's versions are compared too and
reported apart (torch_equals_numpy): two stored objects that share the first 8
bytes of their IDs would fool it, not the call.

Device times are HIP events around windows after a warm-up. A window of the
call or of sort + seek is one replay of a graph that holds `inner` calls; the
stand-in's window is `inner` eager calls (tools/key_merge.py's windows: its
torch.sort passes run eagerly there too, so below a few thousand requests its
figure is the rate the host issues its launches at). The windows alternate
between the three; the figure is the median window over --reps, per call, with
the windows' min and max as the spread.

Prints one JSON line per point, then the points as a table; --out also writes
the lines to a file, and --summarize prints the table of such files again.
Exits non-zero when any point's rows are not numpy's."""
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
from honu_amd.metadata import (HAS_META, HAS_PARENT, HAS_VERSION, INFO_DTYPE, META_DTYPE, NEXT_ASSIGNED,  # noqa: E402
                               NEXT_DTYPE, NEXT_FOUND, NEXT_HAS_PARENT, NEXT_LIVE, NEXT_NOT_FOUND, NEXT_UPDATE,
                               SEEK_NONE)
from honu_amd.object import Codec  # noqa: E402
from key_merge import windows_us  # noqa: E402
from sort_keys import keys_columns, keys_objects  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
NAMES = ("next", "sort_seek", "torch")
POINTS = ("distinct_1K", "distinct_64K", "distinct_1M", "runs_64K_over_4K")
PID, REGION, NOW = 7, 3, 1_760_000_000_000_000_000


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| point | requests | objects asked | stored | assigned | honu_key_next us | sort + seek us | torch stand-in us | "
          "next / (sort + seek) | stand-in / next | ns per request | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['point']} | {r['requests']} | {r['objects_asked']} | {r['found']} | {r['assigned']} | {cell('next')} | "
              f"{cell('sort_seek')} | {cell('torch')} | {r['next_over_sort_seek']}x | {r['torch_over_next']}x | "
              f"{r['next_ns_per_request']} | {'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] for r in rows)}))


def words(ids):
    """The 16-byte IDs as two u64 columns in byte order (hi, lo)."""
    w = np.ascontiguousarray(ids).view(">u8").astype(np.uint64)
    return w[:, 0], w[:, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="keys of the resident column")
    ap.add_argument("--points", default=",".join(POINTS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner-next", type=int, default=10)
    ap.add_argument("--inner-torch", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_next.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    k = keys_objects(a.n, rng)
    n = len(k)
    codec = Codec(0, n + 2)
    L, c = codec.lib, codec.ctx
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731

    def up(x):
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        t = u8(x.nbytes)
        t[:x.nbytes].copy_(torch.from_numpy(x))
        return t

    s = codec.stream
    wb = int(L.honu_sort_keys_workspace(n))
    work, dk = u8(wb), up(k)
    sa, oa, va = u8(29 * n), u8(4 * n), u8(8)
    _lib.check(L.honu_sort_keys(c, P(dk), 0, n, P(oa), P(sa), P(va), P(work), wb, s), "sort the column")
    torch.cuda.synchronize()
    order_h = oa[:4 * n].cpu().numpy().view(np.uint32)
    S_h = k[order_h]
    starts = np.concatenate([[0], np.flatnonzero((S_h[1:, :17] != S_h[:-1, :17]).any(axis=1)) + 1])
    nobj = len(starts)
    ends = np.concatenate([starts[1:], [n]])
    oid_h = S_h[starts, 1:17]  # the column's objects, in key order
    last = S_h[ends - 1]
    V_h = np.ascontiguousarray(last[:, 17:25]).view(">u8").astype(np.uint64).reshape(-1)
    P_h = np.ascontiguousarray(last[:, 25:29]).view(">u4").astype(np.uint32).reshape(-1)
    rec_h = order_h[ends - 1]
    tomb_h = np.zeros(n, np.uint8)
    tomb_h[rec_h[0::4]] = 1  # the latest record of every fourth object
    info = np.zeros(n, INFO_DTYPE)
    info["tombstone"] = tomb_h
    info_d = up(info)
    live_h = tomb_h[rec_h] == 0
    # the stand-in's view of the column: the first word of every row's ID, sign-flipped for signed order; per row
    # the VID, PID and tombstone of the row itself (the stand-in reads them at end - 1)
    sign = np.uint64(1 << 63)
    col_hi = torch.from_numpy((words(S_h[:, 1:17])[0] ^ sign).view(np.int64)).to(dev)
    col_vid = torch.from_numpy(np.ascontiguousarray(S_h[:, 17:25]).view(">u8").astype(np.int64).reshape(-1)).to(dev)
    col_pid = torch.from_numpy(np.ascontiguousarray(S_h[:, 25:29]).view(">u4").astype(np.int64).reshape(-1)).to(dev)
    col_dead = torch.from_numpy(tomb_h[order_h].astype(np.int64)).to(dev)

    lines = []
    for point in [p for p in a.points.split(",") if p]:
        if point.startswith("distinct_"):
            m = {"1K": 1 << 10, "64K": 1 << 16, "1M": 1 << 20}[point.split("_")[1]]
            stored = rng.permutation(nobj)[:min(m, nobj)]
            absent = rng.integers(0, 256, (m - len(stored), 16), dtype=np.uint8)
            absent[:, 0] = 0xFF  # no stored ID starts so
            ids = np.concatenate([oid_h[stored], absent])
            obj = np.concatenate([stored, np.full(len(absent), -1)])
        else:
            m = 1 << 16
            obj = np.repeat(rng.permutation(nobj)[:1 << 12], 16)
            ids = oid_h[obj]
        perm = rng.permutation(m)
        ids, obj = ids[perm], obj[perm].astype(np.int64)
        reqs = rng.integers(0, 256, (m, 29), dtype=np.uint8)
        reqs[:, 0], reqs[:, 1:17] = 1, ids
        # numpy's answer for an Update: the rank among the requests of the same ID, in request order
        hi, lo = words(ids)
        by = np.lexsort((np.arange(m), lo, hi))
        new = np.ones(m, bool)
        new[1:] = (hi[by][1:] != hi[by][:-1]) | (lo[by][1:] != lo[by][:-1])
        first = np.maximum.accumulate(np.where(new, np.arange(m), 0))
        rank = np.empty(m, np.uint64)
        rank[by] = (np.arange(m) - first).astype(np.uint64)
        found = obj >= 0
        o = np.where(found, obj, 0)
        live = found & live_h[o]
        want = np.zeros(m, NEXT_DTYPE)
        want["vid"][live] = (V_h[o] + np.uint64(1) + rank)[live]
        want["pid"][live] = PID
        want["parent_vid"][live] = np.where(rank == 0, V_h[o], V_h[o] + rank)[live]
        want["parent_pid"][live] = np.where(rank == 0, P_h[o], np.uint32(PID))[live]
        want["parent_record"] = np.where(live & (rank == 0), rec_h[o], np.uint32(SEEK_NONE))
        want["flags"] = (np.where(found, NEXT_FOUND, 0) | np.where(live, NEXT_LIVE | NEXT_ASSIGNED | NEXT_HAS_PARENT,
                                                                   NEXT_NOT_FOUND)).astype(np.uint32)
        want_keys = np.zeros((m, 29), np.uint8)
        want_keys[:, :17] = reqs[:, :17]
        want_keys[live] = keys_columns(ids[live], want["vid"][live], want["pid"][live])
        meta0 = rng.integers(0, 256, 352 * m, dtype=np.uint8)

        d_reqs, d_meta = up(reqs), up(meta0)
        d_packed = up(np.pad(reqs[:, :17], ((0, 0), (0, 12))))  # the 17 bytes, 12 zeros
        d_out, d_keys, d_kst = u8(32 * m), u8(29 * m), u8(4 * m)
        nwb = int(L.honu_key_next_workspace(m))
        nwork = u8(nwb)
        swb = int(L.honu_sort_keys_workspace(m))
        swork, s_order, s_sorted, s_valid, s_seek = u8(swb), u8(4 * m), u8(29 * m), u8(8), u8(20 * m)

        def call():
            _lib.check(L.honu_key_next(c, P(sa), P(va), n, P(oa), P(info_d), P(d_reqs), 0, m, NEXT_UPDATE, PID, REGION,
                                       NOW, P(d_out), P(d_keys), P(d_kst), P(d_meta), P(nwork), nwb, codec.stream),
                       "honu_key_next")

        def sort_seek():
            _lib.check(L.honu_sort_keys(c, P(d_packed), 0, m, P(s_order), P(s_sorted), P(s_valid), P(swork), swb,
                                        codec.stream), "honu_sort_keys")
            _lib.check(L.honu_key_seek(c, P(sa), P(va), n, P(d_packed), 0, 17, m, P(oa), P(info_d), P(s_seek),
                                       codec.stream), "honu_key_seek")

        # verified before it is timed
        for t in (d_out, d_keys, d_kst):
            t.zero_()
        call()
        torch.cuda.synchronize()
        meta = d_meta[:352 * m].cpu().numpy().view(META_DTYPE)
        before = meta0.view(META_DTYPE)
        equal = bool(d_out[:32 * m].cpu().numpy().tobytes() == want.tobytes() and
                     np.array_equal(d_keys[:29 * m].cpu().numpy().reshape(m, 29), want_keys) and
                     np.array_equal(d_kst[:4 * m].cpu().numpy().view(np.int32), np.where(live, 0, 10)) and
                     np.array_equal(meta["vid"][live], want["vid"][live]) and
                     np.array_equal(meta["parent_vid"][live], want["parent_vid"][live]) and
                     np.array_equal(meta["object_id"][live], ids[live]) and
                     (meta["version_created"][live] == NOW).all() and (meta["region"][live] == REGION).all() and
                     np.array_equal(meta["present"][live], before["present"][live] | np.uint32(HAS_META | HAS_VERSION |
                                                                                              HAS_PARENT)) and
                     np.array_equal(d_meta[:352 * m].cpu().numpy().reshape(m, 352)[~live],
                                    meta0.reshape(m, 352)[~live]))
        # the stand-in: the IDs as two sign-flipped u64 words (given, not timed)
        hi_t = torch.from_numpy((hi ^ sign).view(np.int64)).to(dev)
        lo_t = torch.from_numpy((lo ^ sign).view(np.int64)).to(dev)
        idx_t = torch.arange(m, device=dev)
        out = {}

        def stand_in():
            _, o1 = torch.sort(lo_t, stable=True)
            _, o2 = torch.sort(hi_t[o1], stable=True)
            order = o1[o2]
            shi, slo = hi_t[order], lo_t[order]
            head = torch.ones(m, dtype=torch.bool, device=dev)
            head[1:] = (shi[1:] != shi[:-1]) | (slo[1:] != slo[:-1])
            r = idx_t - torch.cummax(torch.where(head, idx_t, 0), 0).values
            pos = torch.searchsorted(col_hi, shi)
            end = torch.searchsorted(col_hi, shi, right=True)
            at = (end - 1).clamp(min=0)
            ok = (end > pos) & (col_dead[at] == 0)
            vid = torch.where(ok, col_vid[at] + 1 + r, 0)
            pvid = torch.where(ok, torch.where(r == 0, col_vid[at], col_vid[at] + r), 0)
            ppid = torch.where(ok, torch.where(r == 0, col_pid[at], PID), 0)
            out["vid"] = torch.empty_like(vid).scatter_(0, order, vid)
            out["pvid"] = torch.empty_like(pvid).scatter_(0, order, pvid)
            out["ppid"] = torch.empty_like(ppid).scatter_(0, order, ppid)

        stand_in()
        torch.cuda.synchronize()
        torch_equal = bool(np.array_equal(out["vid"].cpu().numpy().view(np.uint64), want["vid"]) and
                           np.array_equal(out["pvid"].cpu().numpy().view(np.uint64), want["parent_vid"]) and
                           np.array_equal(out["ppid"].cpu().numpy().astype(np.uint32), want["parent_pid"]))
        inners = {"next": a.inner_next, "sort_seek": a.inner_next, "torch": a.inner_torch}
        times = windows_us({"next": call, "sort_seek": sort_seek, "torch": stand_in}, inners,
                           {"next": True, "sort_seek": True, "torch": False}, a.reps)
        rec = {"tool": "key_next", "point": point, "resident": n, "objects": nobj, "op": "update", "requests": m,
               "objects_asked": int(new.sum()), "found": int(found.sum()), "assigned": int(live.sum()),
               "with": ["d_order", "d_info", "d_meta"], "reps": a.reps, "inner": inners, "equals_numpy": equal,
               "torch_equals_numpy": torch_equal}
        for name in NAMES:
            med, lo_, hi_ = times[name]
            rec[name + "_us"] = round(med, 1)
            rec[name + "_us_min_max"] = [round(lo_, 1), round(hi_, 1)]
        rec["next_over_sort_seek"] = round(times["next"][0] / times["sort_seek"][0], 2)
        rec["next_minus_sort_seek_us"] = round(times["next"][0] - times["sort_seek"][0], 1)
        rec["sort_seek_spread_us"] = round(times["sort_seek"][2] - times["sort_seek"][1], 1)
        rec["torch_over_next"] = round(times["torch"][0] / times["next"][0], 2)
        rec["next_ns_per_request"] = round(times["next"][0] * 1e3 / m, 3)
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
        sys.exit("honu_key_next's rows differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
