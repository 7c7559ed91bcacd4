"""A dict-and-list model of a store of many collections kept as one bucketed
column, and the histories the bucket-round tests run. TEST INFRASTRUCTURE ONLY.

As tests/store_model.py, the model is written from the comments in
include/honu_codec.h alone and imports neither honu_amd.keys nor the library:
only the struct layouts (honu_amd.metadata) and the record encoder it is handed
come from outside. A BucketsModel is the sorted table of collection IDs and one
store_reclaim.ReclaimModel per table row.

  put       honu_key_route's classes (the table row equal to the record's
            collection_id; k for no such row; k + 1 for a status that is not
            OK), each known bucket's records appended in arrival order, then
            what honu_key_merge_buckets leaves: every bucket tight.
  drop,     honu_key_delete over one bucket's view: the rows that went lie
  compact   behind the bucket's valid rows, in column order, in front of what
            an earlier delete left there.
  reclaim   honu_key_reclaim over one bucket's view and record state.
  squeeze   what a counted merge does to every bucket: the rows behind the
            valid ones disappear, the records stay.
  arena     the bucketed column as plain values: rows, order, off, count.

Two numberings. The model numbers a bucket's records in arrival order. The
store numbers them d_local + d_base[c]: d_local is the row's index inside its
class in the route's output, and with d_seq a key sort that is key order, equal
keys in arrival order. dev[c] maps the model's index to the store's; on_device
rewrites a bucket's expectations with it, so that indices compare as indices.
"""
from __future__ import annotations

import copy
from collections import namedtuple

import numpy as np

import store_model as sm
from honu_amd.metadata import HostBatch
from store_reclaim import ReclaimModel

NONE, OK, INPUT, KEY = sm.NONE, sm.OK, sm.INPUT, sm.KEY

Batch = namedtuple("Batch", "cids keys statuses records")
Shipment = namedtuple("Shipment", "compared visits idx")  # per bucket: StoreModel.compare's result, the visits, the records


class BucketsModel:
    def __init__(self, marshal, table):
        self.marshal = marshal
        self.table = [bytes(bytearray(t)) for t in table]
        assert self.table == sorted(set(self.table))  # ascending and distinct
        self.k = len(self.table)
        self.buckets = [ReclaimModel(marshal) for _ in self.table]
        self.dev = [[] for _ in self.table]     # per bucket: the model's record index -> the store's
        self.behind = [[] for _ in self.table]  # per bucket: [key bytes, record or None] of the rows behind the valid ones

    # ---- writes -----------------------------------------------------------
    def classes(self, cids, statuses):
        row = {t: c for c, t in enumerate(self.table)}
        return [self.k + 1 if st != OK else row.get(bytes(cid), self.k) for cid, st in zip(cids, statuses)]

    def put(self, batch: Batch, counted=True):
        """Returns (classes, per bucket the first record index of its arrivals). A merge without d_count_a
        takes every row of a bucket as valid, so it may only follow a state with nothing behind."""
        assert counted or not any(self.behind)
        cls = self.classes(batch.cids, batch.statuses)
        first = [b.n for b in self.buckets]
        for c, b in enumerate(self.buckets):
            idx = [i for i, x in enumerate(cls) if x == c]
            b.batch += 1
            b.put_raw([batch.keys[i] for i in idx], [OK] * len(idx), [batch.records[i] for i in idx])
            store = [0] * len(idx)
            for g, j in enumerate(sorted(range(len(idx)), key=lambda j: (bytes(batch.keys[idx[j]]), j))):
                store[j] = first[c] + g
            self.dev[c] += store
        self.squeeze()
        return cls, first

    def squeeze(self):
        for c, b in enumerate(self.buckets):
            self.behind[c], b.tail = [], []

    def _removed(self, c, removed):
        b = self.buckets[c]
        self.behind[c] = [[b.records[i][0], i] for i in removed] + self.behind[c]
        return removed

    def drop(self, c, prefixes, probe_len=sm.PREFIX):
        return self._removed(c, self.buckets[c].drop(prefixes, probe_len))

    def compact(self, c):
        return self._removed(c, self.buckets[c].compact())

    def reclaim(self, c):
        """ReclaimModel.reclaim's record. Both numberings keep the records that stay in their ascending old
        index; the rows behind the valid ones keep their bytes and name no record any more."""
        out = self.buckets[c].reclaim()
        old = [self.dev[c][i] for i in out["source"]]
        rank = {d: j for j, d in enumerate(sorted(old))}
        self.dev[c] = [rank[d] for d in old]
        self.behind[c] = [[key, None] for key, _ in self.behind[c]]
        return out

    # ---- the state as plain values ----------------------------------------
    def rows(self, c):
        return self.buckets[c].valid + len(self.behind[c])

    def arena(self):
        col, order, off, count = [], [], [0], []
        for c, b in enumerate(self.buckets):
            col += b.keys() + [key for key, _ in self.behind[c]]
            order += [self.dev[c][i] for i in b.column()]
            order += [NONE if i is None else self.dev[c][i] for _, i in self.behind[c]]
            count.append(b.valid)
            off.append(len(col))
        return dict(col=b"".join(col), order=order, off=off, count=count)

    def expectations(self, c, probes):
        return sm.expectations(self.buckets[c], probes)

    def on_device(self, c, exp):
        """A bucket's expectations in the store's numbering."""
        d = self.dev[c]
        to = lambda xs: [None if i is None else d[i] for i in xs]  # noqa: E731
        out = dict(exp)
        status = np.full(len(d), INPUT, np.int32)
        status[np.asarray(d, np.int64)] = exp["live_status"]
        out.update(col=to(exp["col"]), order=to(exp["order"]), live_status=status, obj_latest=to(exp["obj_latest"]),
                   retrieve=to(exp["retrieve"]), hits=[[q, p, d[i]] for q, p, i in exp["hits"]],
                   version_records=[to(w) for w in exp["version_records"]], top_records=to(exp["top_records"]))
        return out

    def records_on_device(self, c):
        """The bucket's record bytes by the store's record index."""
        out = [None] * len(self.dev[c])
        for i, d in enumerate(self.dev[c]):
            out[d] = self.buckets[c].records[i][2]
        return out

    # ---- two replicas -----------------------------------------------------
    def gather(self, peer):
        """Per bucket what compare -> list -> fetch gathers, and the buckets' shipments concatenated in
        table order: one batch of many collections mixed together."""
        ships, cids, keys, recs = [], [], [], []
        for c, (mine, theirs) in enumerate(zip(self.buckets, peer.buckets)):
            cmp = mine.compare(theirs)
            col = mine.column()
            visits = [(j, p) for j, (pos, end, _, _) in enumerate(cmp.rows) for p in range(pos, end)]
            idx = [col[p] for _, p in visits]
            ships.append(Shipment(cmp, visits, idx))
            cids += [self.table[c]] * len(idx)
            keys += [mine.records[i][0] for i in idx]
            recs += [mine.records[i][2] for i in idx]
        return ships, Batch(cids, keys, [OK] * len(keys), recs)

    def ship(self, peer, counted=True):
        ships, batch = self.gather(peer)
        return ships, batch, peer.put(batch, counted)


# --------------------------------------------------------------------------
# batches
# --------------------------------------------------------------------------
def build_batch(gen, seed, spec, ids) -> HostBatch:
    """Generator Small records of `seed` with the host's collection_id, object_id, vid, pid and tombstone
    form (an empty payload: storage version 1, data length 0) set from spec rows (collection, oid, vid,
    pid, tombstone): already-versioned records, as a sync ships them. ids: the collections' 16 bytes."""
    hb = gen(seed, len(spec))
    meta = hb.meta.copy()
    off = hb.payload_off.astype(np.int64)
    parts = []
    for i, (c, oid, vid, pid, tomb) in enumerate(spec):
        row = meta[i:i + 1]
        row["collection_id"] = np.asarray(ids[c], np.uint8)
        row["object_id"] = np.frombuffer(bytes(oid), np.uint8)
        row["vid"], row["pid"], row["tombstone"] = vid, pid, 1 if tomb else 0
        row["present"] = int(row["present"][0]) | sm.P_META | sm.P_VERSION
        parts.append(hb.payload[0:0] if tomb else hb.payload[off[i]:off[i + 1]])
    new = np.zeros(len(spec) + 1, np.uint64)
    new[1:] = np.cumsum([len(p) for p in parts])
    return HostBatch(meta, hb.var, hb.acl, hb.regions, np.concatenate(parts + [np.zeros(1, np.uint8)]), new)


def model_batch(marshal, hb: HostBatch, spoil=()) -> Batch:
    """The batch as the model takes it: the IDs and keys of the rows, the encoder's records and statuses. A
    spoiled record's bytes are overwritten before the decode, so it does not decode: its status is not OK."""
    arena, off, status = marshal(hb)
    status = [int(s) for s in status]
    for i in spoil:
        status[i] = INPUT
    keys = [sm.make_key(r["object_id"], int(r["vid"]), int(r["pid"])) for r in hb.meta]
    return Batch([r["collection_id"].tobytes() for r in hb.meta], keys, status,
                 [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(hb.meta))])


class _Book:
    """The latest version the history gave each object of each collection."""

    def __init__(self, top=None):
        self.top = dict(top or {})

    def later(self, c, oid, pid=sm.PID, tomb=False, step=1):
        key = (c, bytes(bytearray(oid)))
        self.top[key] = self.top.get(key, 0) + step
        return (c, key[1], self.top[key], pid, tomb)


def _shuffled(rng, rows):
    return [rows[i] for i in rng.permutation(len(rows))]


def _cycle(pool, count):
    return [pool[i % len(pool)] for i in range(count)]


# --------------------------------------------------------------------------
# the narrow history
# --------------------------------------------------------------------------
class Narrow:
    """k = 5 collections and an unknown ID that sorts between rows 1 and 2. Sizes come from T, the rows
    one workgroup of the merge takes. HOT (the first row, so that a tile lies wholly inside it) takes
    about 60 % of the records, SMALL is emptied and refilled, NEVER receives nothing, DUP receives stored
    keys and is compacted with HONU_DELETE_SUPERSEDED."""

    HOT, MID, SMALL, NEVER, DUP, UNKNOWN = range(6)
    K = 5
    PID_B = 9

    def __init__(self, T):
        self.T = T
        rng = np.random.default_rng(7070)
        q = lambda x: max(1, x * T // 1024)  # noqa: E731
        HOT, MID, SMALL, DUP, UNK = self.HOT, self.MID, self.SMALL, self.DUP, self.UNKNOWN
        self.table = np.array([[0x10 * (c + 1)] + [c + 1] * 15 for c in range(self.K)], np.uint8)
        unknown = self.table[1].copy()
        unknown[15] += 1  # above row 1, below row 2
        self.ids = np.concatenate([self.table, unknown[None]])
        pool = {c: [bytes(o) for o in sm._oids(rng, n, 0x10, 0xF0)] for c, n in
                ((HOT, q(400)), (MID, q(120)), (SMALL, q(30)), (DUP, q(100)), (UNK, q(60)))}
        both = [bytes(o) for o in sm._oids(rng, 3, 0x10, 0xF0)]     # one key into two collections
        absent = [bytes(o) for o in sm._oids(rng, 6, 0x10, 0xF0)]
        self.pool = pool
        book = _Book()
        L = book.later
        hot, mid, small, dup, unk = (pool[c] for c in (HOT, MID, SMALL, DUP, UNK))
        nt = q(30)                                    # the objects tombstoned in (b), per bucket
        self.tombstoned = {HOT: hot[:nt], MID: mid[:nt]}
        self.revived = {HOT: hot[:q(10)], MID: mid[:q(10)]}

        a = [L(HOT, o) for o in hot] + [L(HOT, o) for o in hot[:q(152)]]
        a += [L(MID, o) for o in mid] + [L(MID, o) for o in mid[:q(30)]]
        a += [L(SMALL, o) for o in small] + [L(SMALL, o) for o in small[:q(10)]]
        a += [L(DUP, o) for o in dup] + [L(DUP, o) for o in dup[:q(30)]]
        a += [L(UNK, o) for o in unk[:q(48)]]
        stored = [r for r in a if r[0] == HOT][:q(25)] + [r for r in a if r[0] == DUP][:q(25)]
        b = [L(HOT, o, tomb=True) for o in hot[:nt]] + [L(MID, o, tomb=True) for o in mid[:nt]] + stored
        b += [L(HOT, o) for o in _cycle(hot[nt:], q(497))] + [L(MID, o) for o in _cycle(mid[nt:], q(120))]
        b += [L(SMALL, o) for o in small[:q(20)]] + [L(DUP, o) for o in _cycle(dup, q(133))]
        b += [L(UNK, o) for o in unk[:q(40)]]
        shared = _Book(book.top)                      # what both replicas hold after (a) and (b)
        self.dropped = {HOT: hot[q(380):q(395)] + absent[:2], MID: mid[q(90):q(115)], SMALL: small + absent[2:3]}
        e = [L(HOT, o) for o in self.revived[HOT]] + [L(MID, o) for o in self.revived[MID]]
        e += [L(SMALL, o) for o in _cycle(small, q(40))]
        e += [(c, o, 1, sm.PID, False) for o in both for c in (HOT, DUP)]
        e += [L(HOT, o) for o in _cycle(hot[nt:q(300)], q(430))] + [L(MID, o) for o in _cycle(mid[nt:q(80)], q(100))]
        e += [L(DUP, o) for o in _cycle(dup[:q(90)], q(100))] + [L(UNK, o) for o in unk[:q(40)]]
        f = [L(UNK, o) for o in unk[:q(50)]] + [L(HOT, o) for o in hot[:5]] + [L(MID, o) for o in mid[:5]]
        f = _shuffled(rng, f)
        spoil = [i for i, r in enumerate(f) if r[0] != UNK]
        # the second replica's own step: forks of objects the first writes in (e), and later versions of
        # objects the first leaves alone
        B = self.PID_B
        own = [shared.later(HOT, o, B) for o in hot[nt:nt + q(20)]] + [shared.later(MID, o, B) for o in mid[nt:nt + q(15)]]
        own += [shared.later(HOT, o, B) for o in hot[q(300):q(330)]] + [shared.later(MID, o, B) for o in mid[q(80):q(90)]]
        own += [shared.later(DUP, o, B) for o in dup[q(90):q(100)]] + [shared.later(UNK, o, B) for o in unk[:q(10)]]

        P = lambda name, seed, rows, counted=False, spoil=(): dict(  # noqa: E731
            name=name, kind="put", seed=seed, spec=rows, counted=counted, spoil=list(spoil))
        D = lambda name, c, oids, seed: dict(name=name, kind="drop", bucket=c, prefixes=sm.request_rows(  # noqa: E731
            np.frombuffer(b"".join(oids), np.uint8).reshape(-1, 16), seed))
        self.base = [P("a put", 701, _shuffled(rng, a)), P("b put", 702, _shuffled(rng, b))]
        self.steps = self.base + [
            D("c1 drop", HOT, self.dropped[HOT], 711), D("c2 drop", MID, self.dropped[MID], 712),
            D("c3 drop", SMALL, self.dropped[SMALL], 713), dict(name="c4 compact", kind="compact", bucket=DUP),
        ] + [dict(name="d%d reclaim" % (j + 1), kind="reclaim", bucket=c) for j, c in enumerate((HOT, MID, SMALL, DUP))] + [
            P("e put", 705, _shuffled(rng, e), counted=True), P("f put", 706, f, counted=True, spoil=spoil)]
        self.own = [P("g own", 707, _shuffled(rng, own))]
        self.probes = [sm.request_rows(np.frombuffer(b"".join(pool.get(c, []) + both + absent), np.uint8).reshape(-1, 16),
                                       90 + c) for c in range(self.K)]
        self.next_requests = sm._spoiled(np.frombuffer(b"".join(hot[:q(60)] + hot[q(370):q(400)] + absent + both),
                                                       np.uint8).reshape(-1, 16), 731, bad=3, skipped=3)


class Wide:
    """k = 3 S collections, S the buckets a merge tile may touch and still stage its slice of offsets: a
    put spread evenly, so that every tile touches more than S buckets, drops in about 20 buckets with a
    few emptied, and a counted put that brings the arena to exactly two tiles. Every record is an object
    of its own, one row. `sample` are the buckets whose record state the store keeps and whose reads run:
    two that lose rows (they are reclaimed, the other dropped buckets are not), one emptied, one that
    never receives a record, two plain ones."""

    def __init__(self, T, S):
        self.T, self.S = T, S
        k = self.k = 3 * S
        rng = np.random.default_rng(8080)
        self.table = np.zeros((k, 16), np.uint8)
        self.table[:, 0], self.table[:, 1], self.table[:, 15] = 0x40, np.arange(k) // 256, np.arange(k) % 256
        unknown = self.table[k // 2].copy()
        unknown[14] = 1  # above row k / 2, below the next
        self.ids = np.concatenate([self.table, unknown[None]])
        never = list(range(5, k, 10))                    # k / 10 buckets that never receive a record
        late = list(range(8, k, 20))                     # and k / 20 that the last put alone fills
        first = [c for c in range(k) if c not in never and c not in late]
        last = [c for c in range(k) if c not in never and c % 10 != 2]  # the last put leaves another k / 10 out
        oid = lambda: bytes(sm._oids(rng, 1, 0x10, 0xF0)[0])  # noqa: E731
        m1 = 2 * T - T // 4
        a = [(c, oid(), 1, sm.PID, False) for c in _cycle(first, m1)] + [(k, oid(), 1, sm.PID, False) for _ in range(T // 8)]
        mine = {c: [r[1] for r in a if r[0] == c] for c in first}
        dropped = first[3::len(first) // 20][:20]
        emptied = dropped[:3]
        self.drops = {c: (mine[c] if c in emptied else mine[c][:2]) for c in dropped}
        left = m1 - sum(len(v) for v in self.drops.values())
        b = [(c, oid(), 1, sm.PID, False) for c in _cycle(last, 2 * T - left)] + [(k, oid(), 1, sm.PID, False) for _ in range(T // 16)]
        self.sample = [dropped[5], dropped[6], emptied[0], never[len(never) // 2], first[0], late[1]]
        self.reclaimed = self.sample[:3]
        self.never, self.emptied = never, emptied
        P = lambda name, seed, rows, counted=False: dict(  # noqa: E731
            name=name, kind="put", seed=seed, spec=rows, counted=counted, spoil=[])
        as_rows = lambda oids: np.frombuffer(b"".join(oids), np.uint8).reshape(-1, 16)  # noqa: E731
        self.steps = [P("1 put", 801, _shuffled(rng, a))]
        self.steps += [dict(name="2 drop %d" % c, kind="drop", bucket=c, prefixes=sm.request_rows(as_rows(v), 810 + j))
                       for j, (c, v) in enumerate(self.drops.items())]
        self.steps += [dict(name="2 reclaim %d" % c, kind="reclaim", bucket=c) for c in self.reclaimed]
        self.steps += [P("3 put", 803, _shuffled(rng, b), counted=True)]
        absent = [oid() for _ in range(3)]
        self.probes = {c: sm.request_rows(as_rows(mine.get(c, []) + [r[1] for r in b if r[0] == c] + absent), 850 + j)
                       for j, c in enumerate(self.sample)}


def apply_step(model: BucketsModel, step, gen, marshal, ids):
    """One step on the model: what it returns. A put returns (the host batch, the model's batch, classes,
    first indices)."""
    kind = step["kind"]
    if kind == "put":
        hb = build_batch(gen, step["seed"], step["spec"], ids)
        batch = model_batch(marshal, hb, step["spoil"])
        return (hb, batch) + model.put(batch, step["counted"])
    if kind == "drop":
        return model.drop(step["bucket"], step["prefixes"])
    if kind == "compact":
        return model.compact(step["bucket"])
    if kind == "reclaim":
        return model.reclaim(step["bucket"])
    raise ValueError(kind)


def tiles_touch(off, T):
    """Per output tile of T rows, the buckets that have a row in it."""
    total, out = off[-1], []
    for p0 in range(0, total, T):
        p1 = min(p0 + T, total)
        out.append([c for c in range(len(off) - 1) if max(off[c], p0) < min(off[c + 1], p1)])
    return out


class NarrowCoverage:
    """The coverage conditions of the narrow history, fed after every step; conditions, not measurements."""

    def __init__(self, hist: Narrow):
        self.h, self.at = hist, {}
        self.tombstoned, self.revived = set(), set()

    def after(self, model: BucketsModel, step, result):
        h = self.h
        a = model.arena()
        records = [b.n for b in model.buckets]
        rows = [model.rows(c) for c in range(model.k)]
        equal = sum(model.buckets[c].tail_rows_equal_to_live_keys() for c in range(model.k))
        self.at[step["name"]] = dict(hot=model.buckets[h.HOT].valid, rows=a["off"][-1], count=a["count"], bucket_rows=rows,
                                     records=records, touch=tiles_touch(a["off"], h.T), off=a["off"], equal=equal,
                                     freed=len(result["freed"]) if step["kind"] == "reclaim" else None)
        for c, b in enumerate(model.buckets):
            col = b.column()
            for pre, g in b.groups().items():
                if b.records[col[g[1] - 1]][1]:
                    self.tombstoned.add((c, pre))
                elif (c, pre) in self.tombstoned:
                    self.revived.add((c, pre))

    def check(self, model: BucketsModel):
        h, T, at = self.h, self.h.T, self.at
        names = [s["name"] for s in h.steps]
        assert at["a put"]["hot"] < T < at["b put"]["hot"]                           # crosses T upward at (b)
        assert all(at[n]["hot"] > T for n in names[1:])                              # and exceeds T from then on
        for n in ("b put", "e put", "f put"):                                        # a tile wholly inside HOT,
            s = at[n]
            assert s["touch"][0] == [h.HOT] and s["off"][1] >= T, (n, s["touch"][0])
            assert max(len(t) for t in s["touch"]) >= 3, n                           # and a tile in 3 buckets
        assert at["e put"]["rows"] > 2 * T and at["f put"]["rows"] > 2 * T           # the arena's rows exceed 2 T
        c4 = at["c4 compact"]
        short = [c for c in range(h.K) if c4["count"][c] < c4["bucket_rows"][c]]
        assert len(short) >= 3 and c4["count"][h.SMALL] == 0 < c4["bucket_rows"][h.SMALL], c4
        assert c4["equal"] >= 10, c4["equal"]                                        # removed rows equal to live keys
        for j, c in enumerate((h.HOT, h.MID, h.SMALL, h.DUP)):                       # each reclaim frees >= 20 records
            s = at["d%d reclaim" % (j + 1)]
            assert s["freed"] >= 20 and s["records"][c] == s["count"][c], (c, s)
        for n in ("e put", "f put"):                                                 # the invariant: records == rows
            assert at[n]["records"] == at[n]["bucket_rows"] == at[n]["count"], n
        assert at["e put"]["count"][h.SMALL] > 0 and at["f put"]["count"] == at["e put"]["count"]
        assert at["f put"]["records"][h.NEVER] == 0                                  # one collection receives nothing
        assert len(self.revived) >= 5, len(self.revived)                             # tombstoned and live again
        old = 0
        for b in model.buckets:
            col = b.column()
            old += sum(1 for g in b.groups().values() if not b.records[col[g[1] - 1]][1] and
                       any(b.records[col[p]][1] for p in range(g[0], g[1] - 1)))
        assert old >= 5, old                                                         # live, with an old tombstone row


CLASSES = {"only mine": lambda f: f & sm.LATER and not f & sm.PEER_HAS, "later": lambda f: f & sm.LATER and f & sm.PEER_HAS,
           "earlier": lambda f: f & sm.EARLIER, "equal": lambda f: f & sm.EQUAL,
           "fork": lambda f: f & sm.PEER_HAS and not f & sm.ANCESTOR}


def check_replica_coverage(ships, batch):
    """Every honu_key_compare class in at least two buckets, and a mixed batch of at least 3 collections."""
    for name, test in CLASSES.items():
        hit = [c for c, s in enumerate(ships) if any(test(r[2]) for r in s.compared.rows)]
        assert len(hit) >= 2, (name, hit)
    assert len(set(batch.cids)) >= 3


def check_wide_coverage(hist: Wide, before, after, batch_counts):
    """before / after: the arena's offsets around the last merge; batch_counts: the last batch's rows per bucket."""
    T, S, k = hist.T, hist.S, hist.k
    touch = tiles_touch(after, T)
    assert len(touch) >= 2 and all(len(t) > S for t in touch), [len(t) for t in touch]
    empty = [c for c in range(k) if before[c + 1] == before[c] or batch_counts[c] == 0]
    assert len(empty) >= k // 10, len(empty)
    assert any(before[c + 1] == before[c] and batch_counts[c] == 0 for c in range(k))


def run(hist, steps, marshal, gen, cover=None, model=None):
    """A history's steps on the model alone: (model, [(step, result, arena after it)])."""
    model = BucketsModel(marshal, hist.table) if model is None else model
    out = []
    for step in steps:
        result = apply_step(model, step, gen, marshal, hist.ids)
        if cover is not None:
            cover.after(model, step, result)
        out.append((step, result, model.arena()))
    return model, out


def clone(model: BucketsModel) -> BucketsModel:
    return copy.deepcopy(model)
