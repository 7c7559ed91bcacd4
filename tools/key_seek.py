#!/usr/bin/env python3
"""Time honu_key_seek over 1M resident sorted keys: both forms ("seek_variant"
1 direct, 2 fenced) and auto (0) at every point of
    key set    64 K objects x 16 versions (tools/sort_keys.py's set), random 29-byte keys
    probes m   64, 1 K, 4 K, 16 K, 64 K, 1 M
    probe_len  17 (an ObjectPrefix), 29 (a key)
    mix        all-hit (stored keys), half-miss (every other probe's last
               significant byte changed)
next to a host stand-in for bbolt's Cursor.Seek, which the reference's reads
start from key by key (collection.go:47-65): honu_amd.keys.seek, two bisects
over a list of bytes on one core, timed on a sample of up to 64 K of the probes
and scaled to m. A stand-in: there is no Go toolchain to time bbolt itself.
--n takes another column size (where auto's row threshold lies was measured at
4 K and 64 K rows).

The column is sorted by honu_sort_keys, so the run is the pipeline's own
sort -> seek. Device times are HIP events around windows of --inner calls
(one graph replay) after a warm-up, the windows alternating between the three
variants; the figure is the median window over --reps, per call, with the
windows' min and max as the run-to-run spread. Auto runs one of the two forms,
so auto against that form is the same kernel measured twice ("repeat_spread"). In every point the three
variants' rows must be equal, and a sample of them equal to keys.seek.

Prints one JSON line per point, then the points as a table and the spreads
over all of them; --out also writes the lines to a file, and --summarize
prints the table and the spreads of such files again."""
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
from honu_amd import _lib, keys as hkeys  # noqa: E402
from honu_amd.object import Codec  # noqa: E402
from sort_keys import keys_objects, keys_random  # noqa: E402

VARIANTS = (("direct", 1), ("fenced", 2), ("auto", 0))


def device_times_us(fn, select, names, reps, inner):
    """Per name: median, min and max over `reps` windows of `inner` calls, per
    call, by device events. A window is one replay of a graph that holds the
    `inner` calls, so a call of a few microseconds is not timed at the rate the
    host can issue it and a window lasts milliseconds; select(name) configures
    the context before that name's calls are recorded. The windows alternate
    between the names, so a drift of the machine falls on all of them alike."""
    graphs = {}
    for name in names:
        select(name)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(inner):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()
    out = {name: [] for name in names}
    for _ in range(reps):
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in out.items()}


def print_table(lines):
    """The points as a table: us per call, median [min, max] of
    the windows; then the spreads over all points."""
    rows = [json.loads(ln) for ln in lines]
    print("| keys | set | probes | len | mix | direct us | fenced us | auto us (runs) | direct/fenced | auto/faster | "
          "host stand-in us | auto vs stand-in |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    spreads = []
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['keys']} | {r['set']} | {r['probes']} | {r['probe_len']} | {r['mix']} | {cell('direct')} | "
              f"{cell('fenced')} | {cell('auto')} ({r['auto_is']}) | {r['fenced_vs_direct']} | {r['auto_over_faster']} | "
              f"{r['host_bisect_us']} | {r['speedup_vs_host']}x |")
        spreads += [(r[k + "_us_min_max"][1] - r[k + "_us_min_max"][0]) / r[k + "_us"] for k, _ in VARIANTS]
    spreads.sort()
    print(json.dumps({"points": len(rows), "window_spread_median": round(spreads[len(spreads) // 2], 4),
                      "window_spread_max": round(spreads[-1], 4),
                      "repeat_spread_max": max(r["repeat_spread"] for r in rows),
                      "auto_over_faster_max": max(r["auto_over_faster"] for r in rows),
                      "all_equal_and_match_host": all(r["variants_equal"] and r["matches_host"] for r in rows)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", default="64,1024,4096,16384,65536,1048576")
    ap.add_argument("--probe-lens", default="17,29")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=0, help="calls per window (0: 200, or 25 from 256 K probes)")
    ap.add_argument("--host-sample", type=int, default=1 << 16)
    ap.add_argument("--check-sample", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_seek.py measures on the GPU: no device found")
    n = a.n
    dev = torch.device("cuda", 0)
    codec = Codec(0, n)
    L, c = codec.lib, codec.ctx
    fence, auto_m, auto_n = _lib.C.c_int64(0), _lib.C.c_int64(0), _lib.C.c_int64(0)
    _lib.check(L.honu_ctx_get_param(c, b"seek_fence", _lib.C.byref(fence)), "seek_fence")
    _lib.check(L.honu_ctx_get_param(c, b"seek_auto_probes", _lib.C.byref(auto_m)), "seek_auto_probes")
    _lib.check(L.honu_ctx_get_param(c, b"seek_auto_keys", _lib.C.byref(auto_n)), "seek_auto_keys")
    rng = np.random.default_rng(a.seed)
    lines = []
    for set_name, make in (("objects_x16", keys_objects), ("random", keys_random)):
        k = make(n, rng)
        dk = torch.from_numpy(k.reshape(-1)).to(dev)
        order, srt, valid = codec.sort_keys(dk, n=n, want_sorted=True)
        torch.cuda.synchronize()
        S = srt[:29 * n].cpu().numpy().reshape(n, 29)
        srt_list = [bytes(r) for r in S]
        assert int(valid.item()) == n
        for m in (int(x) for x in a.m.split(",")):
            for plen in (int(x) for x in a.probe_lens.split(",")):
                for mix in ("all_hit", "half_miss"):
                    P = S[rng.integers(0, n, m)].copy()
                    if mix == "half_miss":
                        P[::2, plen - 1] += np.uint8(7)
                    dp = torch.from_numpy(P.reshape(-1)).to(dev)
                    inner = a.inner or (25 if m >= 1 << 18 else 200)
                    rec = {"tool": "key_seek", "keys": n, "set": set_name, "probes": m, "probe_len": plen,
                           "mix": mix, "seek_fence": int(fence.value), "reps": a.reps, "inner": inner}
                    rows = {}
                    out = torch.empty((m, 5), dtype=torch.int32, device=dev)

                    def fn():
                        _lib.check(L.honu_key_seek(c, srt.data_ptr(), valid.data_ptr(), n, dp.data_ptr(), 0, plen, m,
                                                   order.data_ptr(), 0, out.data_ptr(), codec.stream), "honu_key_seek")

                    def select(name):
                        _lib.check(L.honu_ctx_set_param(c, b"seek_variant", dict(VARIANTS)[name]), "seek_variant")

                    times = device_times_us(fn, select, [name for name, _ in VARIANTS], a.reps, inner)
                    for name, _ in VARIANTS:
                        med, lo, hi = times[name]
                        rec[name + "_us"] = round(med, 2)
                        rec[name + "_us_min_max"] = [round(lo, 2), round(hi, 2)]
                        select(name)
                        out.zero_()
                        fn()
                        rows[name] = out.clone()
                    torch.cuda.synchronize()
                    rec["variants_equal"] = bool(torch.equal(rows["direct"], rows["fenced"]) and
                                                 torch.equal(rows["direct"], rows["auto"]))
                    got = rows["auto"].cpu().numpy().view(np.uint32)
                    sample = rng.integers(0, m, min(a.check_sample, m))
                    rec["matches_host"] = all(
                        tuple(got[q, :2]) == hkeys.seek(srt_list, bytes(P[q, :plen])) for q in sample)
                    rec["found"] = int((got[:, 4] & 1).sum())
                    hs = min(a.host_sample, m)
                    probes = [bytes(r[:plen]) for r in P[:hs]]
                    t0 = time.perf_counter()
                    for p in probes:
                        hkeys.seek(srt_list, p)
                    rec["host_bisect_us"] = round((time.perf_counter() - t0) * 1e6 * m / hs, 1)
                    rec["host_bisect_note"] = ("keys.seek (bisect over bytes) on one host core, timed on "
                                               f"{hs} probes and scaled: a stand-in for bbolt's Cursor.Seek")
                    best = min(rec["direct_us"], rec["fenced_us"])
                    rec["faster"] = "direct" if rec["direct_us"] <= rec["fenced_us"] else "fenced"
                    rec["fenced_vs_direct"] = round(rec["direct_us"] / rec["fenced_us"], 2)
                    rec["auto_over_faster"] = round(rec["auto_us"] / best, 3)
                    # auto runs one of the two forms: the same kernel measured twice, in alternating windows
                    rec["auto_is"] = "fenced" if m >= auto_m.value or n <= auto_n.value else "direct"
                    rec["repeat_spread"] = round(abs(rec["auto_us"] / rec[rec["auto_is"] + "_us"] - 1), 3)
                    rec["speedup_vs_host"] = round(rec["host_bisect_us"] / rec["auto_us"], 1)
                    rec["device"] = torch.cuda.get_device_name(0)
                    rec["commit"] = a.commit
                    lines.append(json.dumps(rec))
                    print(lines[-1], flush=True)
        del srt_list
    _lib.check(L.honu_ctx_set_param(c, b"seek_variant", 0), "seek_variant")
    print_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
