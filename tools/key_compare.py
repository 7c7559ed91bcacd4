#!/usr/bin/env python3
"""Time honu_key_compare: the versions of two resident sorted columns compared
object by object. The local column A holds --objects objects (1M) of 1 and of
4 versions each (VID 1..V, ULID-like object IDs as tools/sort_keys.py's); the
peer's column B is one of
    identical     A itself: every object EQUAL
    disjoint      as many objects of other IDs: every object only mine
    half_behind   every second object lacks its latest version at the peer
                  (with one version: the peer lacks the object): LATER with
                  ANCESTOR, or only mine
    digest        the latest key of every object of A and nothing else
The call is given d_order_a, d_peer and d_counts, so a point holds the whole of
it: the bracket, the stage, both bounds, the compare, the bisection in A, the
ancestor test, the row, the peer's row and both launches of the counts.

The yardstick, timed in the same run by the same method, is what a caller had
before for the same question:
    list_seek   honu_key_list with HONU_LIST_LATEST and keys over one range
                that is all of A (the latest key of every object), then
                honu_key_seek of those keys at 17 bytes into B. It answers
                less: whether the peer has the object and where, but no class,
                no range to send and no ancestor; the caller would still have
                to compare the version bytes.
With a library built by `make ab` (HONU_LIB_PATH) a third column is timed,
    unstaged    the call with HONU_COMPARE_STAGE=0: every tile searches its
                bracket of B in global memory, none stages it in LDS
which is the split that says what the stage is worth.

Every point is verified against numpy before it is timed: every honu_seek row,
peer row and count. Device times are HIP events around windows after a
warm-up; a window is one replay of a graph that holds `inner` calls; the
windows alternate between the routes; the figure is the median window over
--reps, per call, with the windows' min and max as the spread
(tools/key_merge.py's windows).

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
from honu_amd.metadata import (CMP_ANCESTOR, CMP_EQUAL, CMP_LATER, CMP_PEER_HAS, LIST_LATEST, SEEK_DTYPE,  # noqa: E402
                               SEEK_FOUND, SEEK_NONE)
from honu_amd.object import Codec  # noqa: E402
from key_merge import windows_us  # noqa: E402
from sort_keys import keys_columns  # noqa: E402

P = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
PEERS = ("identical", "disjoint", "half_behind", "digest")


def print_table(lines):
    """The points as a table: us per call, median [min, max] of the windows."""
    rows = [json.loads(ln) for ln in lines]
    print("| point | objects | rows of A | rows of B | to send | honu_key_compare us | list + seek us | "
          "compare / (list + seek) | unstaged us | ns per object | equals numpy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_us']} [{r[k + '_us_min_max'][0]}, {r[k + '_us_min_max'][1]}]"  # noqa: E731
        print(f"| {r['point']} | {r['objects']} | {r['rows_a']} | {r['rows_b']} | {r['rows_to_send']} | {cell('compare')} | "
              f"{cell('list_seek')} | {r['compare_over_list_seek']}x | "
              f"{cell('unstaged') if 'unstaged_us' in r else 'not measured'} | {r['compare_ns_per_object']} | "
              f"{'yes' if r['equals_numpy'] else 'NO'} |")
    print(json.dumps({"points": len(rows), "all_equal": all(r["equals_numpy"] for r in rows)}))


def object_ids(nobj, rng):
    """nobj distinct ULID-like IDs in byte order: a 48-bit millisecond timestamp within one hour, 80 random bits."""
    ms = np.uint64(1_760_000_000_000) + rng.integers(0, 3_600_000, nobj, dtype=np.uint64)
    oid = np.zeros((nobj, 16), np.uint8)
    oid[:, :6] = ms.astype(">u8").view(np.uint8).reshape(nobj, 8)[:, 2:]
    oid[:, 6:] = rng.integers(0, 256, (nobj, 10), dtype=np.uint8)
    w = oid.view(">u8").astype(np.uint64)
    oid = oid[np.lexsort((w[:, 1], w[:, 0]))]
    w = oid.view(">u8")
    assert ((w[1:, 0] > w[:-1, 0]) | ((w[1:, 0] == w[:-1, 0]) & (w[1:, 1] > w[:-1, 1]))).all(), "an ID twice"
    return oid


def column(oid, versions):
    """The sorted column of the objects' versions: versions[j] of object j, VID 1 .. versions[j], PID j % 4."""
    versions = np.asarray(versions, np.int64)
    which = np.repeat(np.arange(len(oid)), versions)
    start = np.concatenate([[0], np.cumsum(versions)])
    vid = (np.arange(len(which)) - start[which] + 1).astype(np.uint64)
    return keys_columns(oid[which], vid, (which % 4).astype(np.uint32)), start


def peer_and_answer(peer, V, oid, other, A, start):
    """(the peer's column B, numpy's honu_seek rows without first / latest, numpy's peer rows) for A = column(oid, V)."""
    nobj = len(oid)
    a0, a1 = start[:-1], start[1:]
    odd = np.arange(nobj) % 2 == 1
    want = np.zeros(nobj, SEEK_DTYPE)
    want["end"] = a1
    want["first"] = want["latest"] = SEEK_NONE
    if peer == "identical":
        B, bstart = A, start
        want["pos"], want["flags"] = a1, CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR
        want_peer = (bstart[1:] - 1).astype(np.uint32)
    elif peer == "disjoint":
        B, bstart = column(other, np.full(nobj, V))
        want["pos"], want["flags"] = a0, SEEK_FOUND | CMP_LATER
        want_peer = np.full(nobj, SEEK_NONE, np.uint32)
    elif peer == "half_behind":
        B, bstart = column(oid, np.where(odd, V - 1, V))
        has = bstart[1:] > bstart[:-1]
        want["pos"] = np.where(odd, a1 - 1, a1)
        want["flags"] = np.where(odd, SEEK_FOUND | CMP_LATER | (CMP_PEER_HAS | CMP_ANCESTOR if V > 1 else 0),
                                 CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR)
        want_peer = np.where(has, bstart[1:] - 1, SEEK_NONE).astype(np.uint32)
    elif peer == "digest":
        B = A[a1 - 1]
        want["pos"], want["flags"] = a1, CMP_EQUAL | CMP_PEER_HAS | CMP_ANCESTOR
        want_peer = np.arange(nobj, dtype=np.uint32)
    else:
        sys.exit(f"unknown peer {peer}")
    return B, want, want_peer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1 << 20, help="objects of the local column")
    ap.add_argument("--versions", default="1,4", help="versions per object, one set of points each")
    ap.add_argument("--peers", default=",".join(PEERS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="", help="recorded in the output")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", nargs="+", metavar="FILE", help="print the table of earlier --out files; no GPU")
    a = ap.parse_args()
    if a.summarize:
        print_table([ln for f in a.summarize for ln in open(f) if ln.strip()])
        return
    if not torch.cuda.is_available():
        sys.exit("tools/key_compare.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(a.seed)
    nobj = a.objects
    codec = Codec(0, 4096)
    L, c = codec.lib, codec.ctx
    ab = os.path.basename(_lib.LIB_PATH) != "libhonu_codec.so"  # a `make ab` library reads HONU_COMPARE_STAGE
    u8 = lambda nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731

    def up(x):
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        t = u8(x.nbytes)
        t[:x.nbytes].copy_(torch.from_numpy(x))
        return t

    def param(name):
        v = _lib.C.c_int64(0)
        _lib.check(L.honu_ctx_get_param(c, name, _lib.C.byref(v)), name.decode())
        return int(v.value)

    both = object_ids(2 * nobj, rng)  # distinct; every second one is the peer's in the disjoint points
    oid, other = both[0::2], both[1::2]
    lines = []
    for V in [int(v) for v in a.versions.split(",") if v]:
        A, start = column(oid, np.full(nobj, V))
        na = len(A)
        d_a, d_va, d_order = up(A), up(np.array([na], np.uint64)), up(np.arange(na, dtype=np.uint32)[::-1].copy())
        order_h = np.arange(na, dtype=np.uint32)[::-1]
        d_off, d_objs = up(start.astype(np.uint64)), up(np.array([nobj], np.uint64))
        cwb = int(L.honu_key_compare_workspace(na))
        d_work, d_out, d_peer, d_counts = u8(cwb), u8(20 * na), u8(4 * na), u8(64)
        # the yardstick's arrays: one range over all of A, its list rows and keys, the seek rows
        rng_all = np.zeros(1, SEEK_DTYPE)
        rng_all["end"] = na
        d_ranges, d_roff, d_total = up(rng_all), u8(16), u8(8)
        d_lrows, d_lkeys, d_seek = u8(16 * nobj), u8(29 * nobj), u8(20 * nobj)
        for peer in [p for p in a.peers.split(",") if p]:
            B, want, want_peer = peer_and_answer(peer, V, oid, other, A, start)
            found = want["pos"] < want["end"]
            want["first"][found] = order_h[want["pos"][found]]
            want["latest"][found] = order_h[want["end"][found] - 1]
            f = want["flags"]
            hasb = (f & CMP_PEER_HAS) != 0
            want_counts = [nobj, int((~hasb).sum()), int((hasb & ((f & CMP_LATER) != 0)).sum()), 0,
                           int(((f & CMP_EQUAL) != 0).sum()), int((hasb & ((f & CMP_ANCESTOR) == 0)).sum()), 0, 0]
            nb = len(B)
            d_b, d_vb = up(B), up(np.array([nb], np.uint64))

            def call():
                _lib.check(L.honu_key_compare(c, P(d_a), P(d_order), P(d_va), na, P(d_off), P(d_objs), P(d_b), P(d_vb), nb,
                                              P(d_out), P(d_peer), P(d_counts), P(d_work), cwb, codec.stream),
                           "honu_key_compare")

            def unstaged():
                os.environ["HONU_COMPARE_STAGE"] = "0"
                try:
                    call()
                finally:
                    del os.environ["HONU_COMPARE_STAGE"]

            def list_seek():
                _lib.check(L.honu_key_list(c, P(d_a), P(d_order), P(d_va), na, P(d_ranges), 1, 0, LIST_LATEST, P(d_off),
                                           P(d_objs), 0, P(d_roff), P(d_lrows), P(d_lkeys), nobj, P(d_total),
                                           codec.stream), "honu_key_list")
                _lib.check(L.honu_key_seek(c, P(d_b), P(d_vb), nb, P(d_lkeys), 0, 17, nobj, 0, 0, P(d_seek), codec.stream),
                           "honu_key_seek")

            # verified before it is timed
            fns = {"compare": call, "list_seek": list_seek}
            if ab:
                fns["unstaged"] = unstaged
            equal = True
            for name in [k for k in fns if k != "list_seek"]:
                for t in (d_out, d_peer, d_counts):
                    t.zero_()
                fns[name]()
                torch.cuda.synchronize()
                equal = equal and bool(
                    d_out[:20 * nobj].cpu().numpy().tobytes() == want.tobytes() and
                    np.array_equal(d_peer[:4 * nobj].cpu().numpy().view(np.uint32), want_peer) and
                    d_counts[:64].cpu().numpy().view(np.uint64).tolist() == want_counts)
            # the yardstick finds the same objects at the peer
            list_seek()
            torch.cuda.synchronize()
            sk = d_seek[:20 * nobj].cpu().numpy().view(SEEK_DTYPE)
            equal = equal and bool(np.array_equal((sk["flags"] & SEEK_FOUND) != 0, hasb) and
                                   np.array_equal(sk["end"][hasb] - 1, want_peer[hasb]))
            inners = {name: a.inner for name in fns}
            times = windows_us(fns, inners, {name: True for name in fns}, a.reps)
            rec = {"tool": "key_compare", "point": f"v{V}_{peer}", "objects": nobj, "versions": V, "rows_a": na,
                   "rows_b": nb, "peer": peer, "rows_to_send": int((want["end"] - want["pos"]).sum()),
                   "counts": want_counts, "with": ["d_order_a", "d_peer", "d_counts"],
                   "compare_tile": param(b"compare_tile"), "compare_stage": param(b"compare_stage"),
                   "reps": a.reps, "inner": a.inner, "equals_numpy": equal}
            for name in fns:
                med, lo_, hi_ = times[name]
                rec[name + "_us"] = round(med, 1)
                rec[name + "_us_min_max"] = [round(lo_, 1), round(hi_, 1)]
            rec["compare_over_list_seek"] = round(times["compare"][0] / times["list_seek"][0], 2)
            rec["compare_max_below_list_seek_min"] = bool(times["compare"][2] < times["list_seek"][1])
            if ab:
                rec["unstaged_over_compare"] = round(times["unstaged"][0] / times["compare"][0], 2)
            rec["compare_ns_per_object"] = round(times["compare"][0] * 1e3 / nobj, 3)
            rec["library"] = os.path.basename(_lib.LIB_PATH)
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
        sys.exit("honu_key_compare's rows differ from numpy's at: " + ", ".join(wrong))


if __name__ == "__main__":
    main()
