"""A dict-and-list model of one store, and the histories the store tests run.

TEST INFRASTRUCTURE ONLY. The model is a second, independent statement of what
a chain of honu_key_* calls leaves behind: it is written from the comments in
include/honu_codec.h alone and imports neither honu_amd.keys nor the library.
Only the struct layouts (honu_amd.metadata's numpy dtypes) and the record
encoder it is handed (oracle.marshal_batch) come from outside.

  records   a list over record index, the concatenation of all batches, of
            (key29 or None, tombstone, record bytes). A refused request's
            record exists but is never a row.
  live      the set of record indices that are live rows of the column.
  column    the live indices sorted by (key bytes, index): a merge puts equal
            keys in arrival order and b_base makes a later batch's indices
            greater, a delete is a stable compaction.
  tail      the record indices of the rows [valid, n) in the column's order:
            a delete puts the rows it removed in front of the tail it found, a
            merge appends the new batch's invalid rows in index order.

A record is a tombstone when Object.Tombstone() says so: storage version 1 and
a data length of 0 (object.go:103-112), which is what honu_record_info holds.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from honu_amd.metadata import HostBatch, NEXT_DTYPE

KEY, PREFIX = 29, 17
M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF  # HONU_SEEK_NONE
OK, INPUT = 0, 10  # HONU_OK, HONU_ERR_INPUT
CREATE, UPDATE, MERGE, DELETE = range(4)  # honu_key_next ops
(ASSIGNED, HAS_PARENT, TOMBSTONE, FOUND, LIVE, NOT_FOUND, EXISTS, BAD_KEY, SKIPPED,
 WRAPPED) = (1 << b for b in range(10))  # honu_next.flags
P_META, P_VERSION, P_PARENT = 1 << 0, 1 << 1, 1 << 2  # honu_meta.present
SEEK_FOUND = 1 << 0
PEER_HAS, LATER, EARLIER, EQUAL, ANCESTOR = (1 << b for b in range(8, 13))  # honu_key_compare's flags

Written = namedtuple("Written", "rows keys status arena off first")
Compared = namedtuple("Compared", "rows counts")  # rows: (pos, end, flags, peer row or None) per object


def make_key(oid, vid: int, pid: int) -> bytes:
    """keys.New: keyVersion | ObjectID | BE64(VID) | BE32(PID)."""
    return b"\x01" + bytes(oid) + int(vid).to_bytes(8, "big") + int(pid).to_bytes(4, "big")


def is_tombstone(rec: bytes) -> bool:
    """Object.Tombstone(): storage version 1 and a zero data length (one uvarint byte of 0)."""
    return len(rec) >= 2 and rec[0] == 1 and rec[1] == 0


def without_payloads(hb: HostBatch) -> HostBatch:
    return HostBatch(hb.meta, hb.var, hb.acl, hb.regions, np.zeros(1, np.uint8), np.zeros(len(hb.meta) + 1, np.uint64))


def _groups(keys):
    """prefix -> (pos, end) of a sorted list of keys, in the list's order."""
    out = {}
    for p, k in enumerate(keys):
        pre = k[:PREFIX]
        if pre in out:
            out[pre][1] = p + 1
        else:
            out[pre] = [p, p + 1]
    return out


class StoreModel:
    def __init__(self, marshal):
        self.marshal = marshal  # HostBatch -> (arena, off[n + 1], status[n])
        self.records = []       # (key or None, tombstone, bytes)
        self.keybytes = []      # the 29 bytes of the unsorted key column, None where they are unspecified
        self.live = set()
        self.tail = []
        self._col = None

    # ---- the column -------------------------------------------------------
    @property
    def n(self):
        return len(self.records)

    @property
    def valid(self):
        return len(self.live)

    def column(self):
        if self._col is None:
            self._col = sorted(self.live, key=lambda i: (self.records[i][0], i))
            self._keys = [self.records[i][0] for i in self._col]
            self._grp = _groups(self._keys)
        return self._col

    def keys(self):
        self.column()
        return self._keys

    def groups(self):
        self.column()
        return self._grp

    def order(self):
        """Every position's record index: the column, then the tail."""
        return list(self.column()) + list(self.tail)

    def run_of(self, oid):
        g = self.groups().get(b"\x01" + bytes(oid))
        return (g[0], g[1]) if g else None

    def tail_rows_equal_to_live_keys(self):
        have = set(self.keys())
        return sum(1 for i in self.tail if self.keybytes[i] is not None and self.keybytes[i] in have)

    def _append(self, key, rec, keybytes):
        i = len(self.records)
        self.records.append((key, is_tombstone(rec), rec))
        self.keybytes.append(keybytes)
        if key is None:
            self.tail.append(i)
        else:
            self.live.add(i)
        self._col = None

    # ---- writes -----------------------------------------------------------
    def write(self, op, requests, skip, pid, region, now, rows: HostBatch) -> Written:
        """honu_key_next's rules, then the stamping, the encoding and the
        merge. requests: uint8[m, 29]; skip: None or m statuses (not 0: the
        request is skipped); rows: the caller's batch, unchanged here."""
        m = len(requests)
        col, grp = self.column(), self.groups()
        out = np.zeros(m, NEXT_DTYPE)
        out["parent_record"] = NONE
        keys = np.zeros((m, KEY), np.uint8)
        meta = rows.meta.copy()
        rank = {}
        new_keys = [None] * m
        for i in range(m):
            req = bytes(requests[i])
            pre = req[:PREFIX]
            keys[i, :PREFIX] = requests[i, :PREFIX]
            if skip is not None and skip[i] != 0:
                out["flags"][i] = SKIPPED
                continue
            if req[0] != 1:
                out["flags"][i] = BAD_KEY
                continue
            r = rank.get(pre, 0)
            rank[pre] = r + 1
            g = grp.get(pre)
            found, live, flags = g is not None, False, 0
            if found:
                last = col[g[1] - 1]
                stored = self.records[last][0]
                V, P = int.from_bytes(stored[17:25], "big"), int.from_bytes(stored[25:29], "big")
                live = not self.records[last][1]
                flags = FOUND | (LIVE if live else 0)
            scalar = parent = None
            if op == CREATE:
                if not found and r == 0:
                    scalar = (0, 1)
                else:
                    flags |= EXISTS
            elif op == DELETE:
                if live and r == 0:
                    scalar, parent = (pid, (V + 1) & M64), (P, V)
                    flags |= TOMBSTONE
                else:
                    flags |= NOT_FOUND
            elif found and (live or op == MERGE):  # UPDATE of a live object, MERGE of a stored one
                scalar = (pid, (V + 1 + r) & M64)
                parent = (P, V) if r == 0 else (pid, (V + r) & M64)
                flags |= WRAPPED if V + 1 + r > M64 else 0
            elif op == MERGE:
                scalar, parent = (pid, 1 + r), (None if r == 0 else (pid, r))
            else:
                flags |= NOT_FOUND
            if scalar is not None:
                flags |= ASSIGNED
                out["pid"][i], out["vid"][i] = scalar
                if parent is not None:
                    flags |= HAS_PARENT
                    out["parent_pid"][i], out["parent_vid"][i] = parent
                    if r == 0 and found:
                        out["parent_record"][i] = last
                key = make_key(req[1:PREFIX], scalar[1], scalar[0])
                new_keys[i] = key
                keys[i] = np.frombuffer(key, np.uint8)
            out["flags"][i] = flags
        # the stamping: exactly the fields the header lists for d_meta, on the ASSIGNED rows alone
        a = (out["flags"] & ASSIGNED) != 0
        par = a & ((out["flags"] & HAS_PARENT) != 0)
        for f in ("vid", "pid", "parent_vid", "parent_pid"):
            meta[f][a] = out[f][a]
        meta["tombstone"][a] = 1 if op == DELETE else 0
        meta["region"][a] = region
        meta["version_created"][a] = now
        meta["modified"][a] = now
        meta["created"][a & ~par] = now
        meta["object_id"][a] = requests[a, 1:PREFIX]
        meta["present"][a] = (meta["present"][a] | np.uint32(P_META | P_VERSION)) & ~np.uint32(P_PARENT)
        meta["present"][par] |= np.uint32(P_PARENT)
        batch = HostBatch(meta, rows.var, rows.acl, rows.regions, rows.payload, rows.payload_off)
        if op == DELETE:  # a tombstone is encoded with an empty payload
            batch = without_payloads(batch)
        arena, off, _ = self.marshal(batch)
        first = self.n
        for i in range(m):
            self._append(new_keys[i], arena[int(off[i]):int(off[i + 1])].tobytes(), bytes(keys[i]))
        status = np.where((out["flags"] & ASSIGNED) != 0, OK, INPUT).astype(np.int32)
        return Written(out, keys, status, arena, off, first)

    def put_raw(self, keys, statuses, records, keybytes_known=True):
        """Already-keyed records: the shipped batch of a sync, the Put of stored keys."""
        first = self.n
        for k, st, rec in zip(keys, statuses, records):
            k = bytes(k)
            self._append(k if st == OK else None, bytes(rec), k if (st == OK or keybytes_known) else None)
        return first

    def _remove(self, removed):
        self.live -= set(removed)
        self.tail = list(removed) + self.tail
        self._col = None
        return list(removed)

    def drop(self, prefixes, probe_len=PREFIX):
        """Every live row whose first probe_len bytes are those of a prefix goes; the freed records, in column order."""
        probes = {bytes(p)[:probe_len] for p in prefixes}
        return self._remove([i for i in self.column() if self.records[i][0][:probe_len] in probes])

    def compact(self):
        """The superseded rule: of a run of equal keys only the last row stays."""
        col, keys = self.column(), self.keys()
        return self._remove([col[p] for p in range(len(col) - 1) if keys[p + 1] == keys[p]])

    # ---- reads ------------------------------------------------------------
    def retrieve(self, prefixes):
        """Per prefix the record index of the latest version, None when that is a tombstone or the object is absent."""
        col, grp = self.column(), self.groups()
        out = []
        for p in prefixes:
            g = grp.get(bytes(p)[:PREFIX])
            i = col[g[1] - 1] if g else None
            out.append(None if i is None or self.records[i][1] else i)
        return out

    def versions(self, prefixes, deleted_filter: bool):
        """(range, pos) most recent first. deleted_filter: a deleted object has
        no rows and a live one keeps its old tombstones; without it every
        tombstone row goes and nothing else."""
        col, grp = self.column(), self.groups()
        out = []
        for q, p in enumerate(prefixes):
            g = grp.get(bytes(p)[:PREFIX])
            if not g:
                continue
            if deleted_filter:
                if not self.records[col[g[1] - 1]][1]:
                    out.extend((q, pos) for pos in range(g[1] - 1, g[0] - 1, -1))
            else:
                out.extend((q, pos) for pos in range(g[1] - 1, g[0] - 1, -1) if not self.records[col[pos]][1])
        return out

    def latest_of_all(self):
        return [g[1] - 1 for g in self.groups().values()]

    def objects(self):
        """(offsets, objects + 1 of them; the latest record of each object)."""
        col = self.column()
        gs = list(self.groups().values())
        return [g[0] for g in gs] + [len(col)], [col[g[1] - 1] for g in gs]

    # ---- two replicas -----------------------------------------------------
    def compare(self, other, digest=None) -> Compared:
        """honu_key_compare's rules, self the local column, `other` the peer
        (or `digest`, a sorted list of keys, in its place)."""
        a = self.keys()
        b = other.keys() if digest is None else list(digest)
        bg = _groups(b)
        rows, counts = [], [0] * 8
        for a0, a1 in self.groups().values():
            mine = a[a1 - 1]
            g = bg.get(mine[:PREFIX])
            if g is None:
                pos, flags, peer = a0, LATER, None
                counts[1] += 1
            else:
                peer = g[1] - 1
                theirs = b[peer]
                pos = a0 + sum(1 for k in a[a0:a1] if k <= theirs)
                if mine > theirs:
                    flags = LATER | (ANCESTOR if pos > a0 and a[pos - 1] == theirs else 0)
                    counts[2] += 1
                elif mine < theirs:
                    flags = EARLIER | (ANCESTOR if mine in b[g[0]:g[1]] else 0)
                    counts[3] += 1
                else:
                    flags = EQUAL | ANCESTOR
                    counts[4] += 1
                counts[5] += 0 if flags & ANCESTOR else 1
                flags |= PEER_HAS
            rows.append((pos, a1, flags | (SEEK_FOUND if pos < a1 else 0), peer))
        counts[0] = len(rows)
        return Compared(rows, counts)

    def ship(self, peer, cap, digest=None):
        """What compare -> list -> fetch gathers, put on the peer with the empty
        records that fill the list up to cap: (visits, record indices here)."""
        col = self.column()
        visits = [(j, p) for j, (pos, end, _, _) in enumerate(self.compare(peer, digest).rows) for p in range(pos, end)]
        idx = [col[p] for _, p in visits]
        assert len(idx) <= cap
        pad = cap - len(idx)
        peer.put_raw([self.records[i][0] for i in idx] + [bytes(KEY)] * pad, [OK] * len(idx) + [INPUT] * pad,
                     [self.records[i][2] for i in idx] + [b""] * pad, keybytes_known=False)
        return visits, idx


def expectations(model: StoreModel, probes):
    """What a store in the model's state holds and answers, as plain values: the
    model may move on, these stay. probes: uint8[m, 29]."""
    col, keys, grp = model.column(), model.keys(), model.groups()
    status = np.full(model.n, INPUT, np.int32)
    status[list(model.live)] = OK
    known = np.array([p for p, i in enumerate(model.tail) if model.keybytes[i] is not None], np.int64)
    retrieve = model.retrieve(probes)
    hits = [[q, grp[bytes(probes[q][:PREFIX])][1] - 1, i] for q, i in enumerate(retrieve) if i is not None]
    versions = [model.versions(probes, True), model.versions(probes, False)]
    tops = model.latest_of_all()
    offs, last = model.objects()
    return dict(
        n=model.n, valid=model.valid, col=list(col), keys=b"".join(keys), order=model.order(), live_status=status,
        tail_known=known, tail_bytes=b"".join(model.keybytes[model.tail[p]] for p in known),
        obj_off=offs, obj_latest=last, retrieve=retrieve, hits=hits,
        hit_keys=[keys[p] for _, p, _ in hits], hit_records=[model.records[i][2] for _, _, i in hits],
        versions=[[list(v) for v in w] for w in versions], version_records=[[col[p] for _, p in w] for w in versions],
        tops=tops, top_records=[col[p] for p in tops], top_tombstones=[model.records[col[p]][1] for p in tops])


# --------------------------------------------------------------------------
# histories
# --------------------------------------------------------------------------
TILE = 1024  # the rows one workgroup of the merge, delete, list and filter takes today: the T of the first history


PID, REGION, NOW = 5, 0x00C0FFEE, 1_700_000_000_000_000_000


def _oids(rng, count, lo, hi):
    o = rng.integers(0, 256, (count, 16), dtype=np.uint8)
    o[:, 0] = rng.integers(lo, hi, count)
    return o


def request_rows(oids, seed):
    """29-byte requests: keyVersion, the ID, 12 bytes no call reads."""
    oids = np.asarray(oids, np.uint8).reshape(-1, 16)
    req = np.random.default_rng(seed).integers(0, 256, (len(oids), KEY), dtype=np.uint8)
    req[:, 0] = 1
    req[:, 1:PREFIX] = oids
    return req


def _spoiled(oids, seed, bad=0, skipped=0):
    """Shuffled requests of the IDs, `bad` more with a wrong first byte and `skipped` more with a status."""
    rng = np.random.default_rng(seed)
    oids = np.asarray(oids, np.uint8).reshape(-1, 16)
    extra = oids[rng.integers(0, len(oids), bad + skipped)]
    req = request_rows(np.concatenate([oids, extra]), seed + 1)
    status = np.zeros(len(req), np.int32)
    req[len(oids):len(oids) + bad, 0] = np.resize(np.array([0, 2, 0x81, 0xFF], np.uint8), bad)
    status[len(oids) + bad:] = np.resize(np.array([3, 10, -1, 1 << 30], np.int32), skipped)
    perm = rng.permutation(len(req))
    return req[perm], status[perm]


class Rounds:
    """The first history, built from the tile size T: the object sets and the batches in order."""

    def __init__(self, T):
        rng = np.random.default_rng(2024)
        self.T = T
        self.reg = _oids(rng, 155, 0x10, 0xE0)     # created in step 1
        self.hot = _oids(rng, 1, 0xE8, 0xE9)[0]    # sorts behind them, so its run lies where valid crosses T
        self.late = _oids(rng, 4, 0xF0, 0xFF)      # and a few objects behind it
        self.absent = _oids(rng, 30, 0x10, 0xE0)   # never created; [10, 20) come to life through MERGE
        self.created = np.concatenate([self.reg, self.hot[None], self.late])
        self.deleted = self.reg[0:40]
        self.merged = self.reg[0:15]               # deleted, then live again
        self.dropped = np.concatenate([self.hot[None], self.reg[100:115], self.reg[20:28], self.reg[0:4],
                                       self.absent[0:2]])
        self.recreated = np.concatenate([self.reg[100:115], self.reg[20:25]])
        self.probes = request_rows(np.concatenate([self.created, self.absent, np.zeros((1, 16), np.uint8),
                                                   np.full((1, 16), 0xFF, np.uint8)]), 99)
        reg, hot, late, absent = self.reg, self.hot, self.late, self.absent
        pick = lambda pool, k: pool[rng.integers(0, len(pool), k)]  # noqa: E731
        rep = lambda o, k: np.tile(np.asarray(o, np.uint8).reshape(-1, 16), (k, 1))  # noqa: E731
        others = np.concatenate([reg, late])
        W = lambda name, op, oids, seed, bad=0, skipped=0: dict(  # noqa: E731
            name=name, kind="write", op=op, seed=seed, requests=_spoiled(oids, seed, bad, skipped))
        self.steps = [
            W("1 create", CREATE, np.concatenate([self.created, pick(self.created, 12)]), 11, bad=6, skipped=6),
            W("2 update", UPDATE, np.concatenate([rep(hot, 300), rep(absent[0:10], 2), pick(others, T - 100 - 328)]),
              21, bad=4, skipped=4),
            W("3 delete", DELETE, np.concatenate([self.deleted, self.deleted[0:8], absent[0:5]]), 31),
            W("4a update", UPDATE, np.concatenate([self.created, rep(self.deleted, 5), rep(hot, 520), absent[0:5]]), 41,
              bad=3, skipped=3),
            W("4b merge", MERGE, np.concatenate([self.merged, self.merged[0:5], rep(absent[10:20], 2)]), 45),
            dict(name="5 drop", kind="drop", prefixes=request_rows(np.concatenate([self.dropped, self.dropped[0:3]]), 51)),
            W("6a create", CREATE, np.concatenate([self.recreated, self.recreated[0:3], reg[50:53]]), 61),
            W("6b update", UPDATE, rep(self.recreated, 2), 65),
            dict(name="7 put", kind="put_stored", count=50, seed=71),
            dict(name="8 compact", kind="compact"),
        ]


def stored_key_batch(model: StoreModel, count, seed, gen):
    """The Put of stored keys: `count` records that carry the keys of live,
    non-tombstone rows of the model's column, every third of them an object's
    latest row and two keys twice, but the payloads and the other metadata of
    generator records of another seed. gen(seed, n) makes the HostBatch.
    Returns (batch, keys)."""
    rng = np.random.default_rng(seed)
    col, keys = model.column(), model.keys()
    latest = [p for p in model.latest_of_all() if not model.records[col[p]][1]]
    plain = [p for p in range(len(col)) if not model.records[col[p]][1]]
    pos = [latest[j] for j in rng.choice(len(latest), count // 3, replace=False)]
    pos += [plain[j] for j in rng.choice(len(plain), count - len(pos) - 2, replace=False)]
    pos += pos[:2]
    hb = gen(seed, len(pos))
    out = []
    for i, p in enumerate(pos):
        k = keys[p]
        row = hb.meta[i:i + 1]
        row["object_id"] = np.frombuffer(k[1:PREFIX], np.uint8)
        row["vid"], row["pid"] = int.from_bytes(k[17:25], "big"), int.from_bytes(k[25:29], "big")
        row["present"] = int(row["present"][0]) | P_META | P_VERSION
        out.append(k)
    return hb, out


def apply_step(model: StoreModel, step, gen):
    """One step of a history on the model: what the step should return (a
    Written, the freed records, or (batch, keys, first index))."""
    kind = step["kind"]
    if kind == "write":
        req, status = step["requests"]
        return model.write(step["op"], req, status, step.get("pid", PID), REGION, NOW + step["seed"],
                           gen(step["seed"], len(req)))
    if kind == "drop":
        return model.drop(step["prefixes"])
    if kind == "compact":
        return model.compact()
    if kind == "put_stored":
        hb, keys = stored_key_batch(model, step["count"], step["seed"], gen)
        arena, off, _ = model.marshal(hb)
        first = model.put_raw(keys, [OK] * len(keys), [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(keys))])
        return hb, keys, first
    raise ValueError(kind)


class Coverage:
    """The coverage conditions of the first history, fed after every step."""

    def __init__(self, rounds: Rounds):
        self.r, self.valid, self.n, self.classes = rounds, [], [], {}
        self.straddles, self.tail_equal = [], {}
        self.tombstoned, self.revived = set(), set()

    def after(self, model: StoreModel, step, result):
        T = self.r.T
        self.valid.append(model.valid)
        self.n.append(model.n)
        run = model.run_of(self.r.hot)
        if run and any(run[0] < k * T < run[1] for k in range(1, model.valid // T + 1)):
            self.straddles.append(step["name"])
        self.tail_equal[step["name"]] = model.tail_rows_equal_to_live_keys()
        if step["kind"] == "write":
            f = result.rows["flags"].astype(np.int64)
            stored = result.rows["parent_record"] != NONE
            for name, mask in (("assigned", f & ASSIGNED), ("exists", f & EXISTS), ("bad key", f == BAD_KEY),
                               ("skipped", f == SKIPPED), ("tombstone", f & TOMBSTONE),
                               ("not found, found", (f & NOT_FOUND) * (f & FOUND)),
                               ("not found, absent", (f & NOT_FOUND) * ((f & FOUND) == 0)),
                               ("parent stored", (f & HAS_PARENT) * stored), ("parent in batch", (f & HAS_PARENT) * ~stored)):
                self.classes[name] = self.classes.get(name, 0) + int((np.asarray(mask) != 0).sum())
        col = model.column()
        for pre, g in model.groups().items():
            dead = model.records[col[g[1] - 1]][1]
            if dead:
                self.tombstoned.add(pre)
            elif pre in self.tombstoned:
                self.revived.add(pre)

    def check(self, model: StoreModel):
        T, names = self.r.T, [s["name"] for s in self.r.steps]
        at = {name: i for i, name in enumerate(names)}
        v, n = self.valid, self.n
        assert v[at["1 create"]] < T < v[at["2 update"]], v                     # valid crosses T upward in step 2
        assert v[at["4b merge"]] > T > v[at["5 drop"]], v                       # and downward in step 5
        assert all(x >= 2 * T + 1 for x in n[at["5 drop"]:]), n                 # n >= 2T + 1 from step 5 on
        assert len(self.straddles) >= 2, self.straddles                         # the hot run straddles a multiple of T
        assert self.tail_equal["6b update"] >= 10, self.tail_equal              # removed rows byte-equal to live keys
        assert len(self.classes) == 9 and min(self.classes.values()) >= 3, self.classes
        assert len(self.revived) >= 5                                           # deleted and later live again
        col = model.column()
        old = sum(1 for g in model.groups().values() if not model.records[col[g[1] - 1]][1] and
                  any(model.records[col[p]][1] for p in range(g[0], g[1] - 1)))
        assert old >= 5, old                                                    # live, with an old tombstone


class Replicas:
    """The second history: a base both replicas write, then what each writes alone."""

    PID_A, PID_B = 7, 9

    def __init__(self):
        rng = np.random.default_rng(4048)
        o = self.objs = _oids(rng, 300, 0x10, 0xF0)
        self.new_a, self.new_b = _oids(rng, 10, 0x10, 0xF0), _oids(rng, 10, 0x10, 0xF0)
        W = lambda name, op, oids, seed, pid: dict(name=name, kind="write", op=op, seed=seed, pid=pid,  # noqa: E731
                                                   requests=_spoiled(oids, seed))
        self.base = [W("base create", CREATE, o, 111, 3),
                     W("base update", UPDATE, np.concatenate([o[0:200], o[0:60]]), 121, 3)]
        A, B = self.PID_A, self.PID_B
        self.a = [W("a update", UPDATE, np.concatenate([o[0:60], o[40:50]]), 131, A),  # [40, 50) twice: ahead of B's fork
                  W("a delete", DELETE, o[90:120], 141, A),
                  W("a merge", MERGE, self.new_a, 151, A)]
        self.b = [W("b update", UPDATE, o[40:100], 161, B),
                  W("b merge", MERGE, self.new_b, 171, B)]
        self.probes = request_rows(np.concatenate([o, self.new_a, self.new_b, np.zeros((1, 16), np.uint8)]), 98)


def run_rounds(T, marshal, gen):
    """The first history on the model alone: (rounds, [(step, what the step returns, expectations after
    it)], the coverage record, the model at the end)."""
    rounds = Rounds(T)
    model, cover, out = StoreModel(marshal), Coverage(rounds), []
    for step in rounds.steps:
        result = apply_step(model, step, gen)
        cover.after(model, step, result)
        out.append((step, result, expectations(model, rounds.probes)))
    return rounds, out, cover, model
