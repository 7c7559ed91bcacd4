"""Host mirror of pkg/store/keys: the 29-byte object storage key.

A key is keyVersion | ObjectID (16) | BE64(VID) | BE32(PID) (keys/keys.go:27-51):
the version is serialized big endian "to maintain lexicographic sorting"
(keys.go:35-36), so bytes.Compare order of the keys of one object is
lamport.Compare order of its versions (lamport/scalar.go:50-78: VID, then
PID). Keys are bytes; the functions take what Go's methods take as receiver.
sort() is the host statement of Keys (keys.go:126-130); the batch form on the
GPU is Codec.sort_keys / Codec.key_objects (object.py, honu_sort_keys and
honu_key_objects in include/honu_codec.h). seek() and has() are the host
statement of Cursor.Seek (iterator/cursor.go:44-55) and Collection.Has
(collection.go:47-51) over such a sorted list; the batch form is
Codec.seek_keys (honu_key_seek). merge() is the host statement of a batch of
Puts into such a list (store.go:232, 395, 530); the batch form is
Codec.merge_keys (honu_key_merge). delete() is the host statement of a batch of
Deletes from such a list (the loop of Store.Drop, store.go:378-383, and its
DeleteBucket, store.go:399-404) and compact() of what a Put of a stored key
does to the row it replaces; the batch form of both is Codec.delete_keys
(honu_key_delete). scan() is the host statement of what follows a Seek on
every read path, the walk with Cursor.Next() or Cursor.Prev()
(iterator/cursor.go:57-89) that List, Versions and Retrieve
(collection.go:32-35, 97-110) and the loop of store.go:379 are made of, over a
batch of seek() ranges; the batch form is Codec.list_keys (honu_key_list).
fetch() is the host statement of what every one of those walks does at each
row, Cursor.Object() (iterator/cursor.go:31-38), over scan()'s list; the batch
form is Codec.fetch_objects (honu_key_fetch). filter() is the host statement
of what a listing leaves out, the object deleted with a tombstone version that
"will not be returned in list queries or retrieval" (collection.go:132-134),
over scan()'s list; the batch form is Codec.filter_rows (honu_key_filter).
next() is the host statement of what every write decides first, the version
it writes: pid.Next of the stored latest version (lamport/pid.go:10-15,
metadata/collection.go:56-63) for a batch of Creates, Updates, Merges or
Deletes (collection.go:75-137) over such a list; the batch form is
Codec.next_versions (honu_key_next). compare() is the host statement of what
two replicas decide when they meet, which side holds the later version of an
object under "latest writer wins" (lamport/scalar.go:15-24, 47-78), over two
such lists; the batch form is Codec.compare_keys (honu_key_compare).
reclaim() is the host statement of what a Drop is for, "to free up space in
the database" (store.go:314-322, 399-404): the records that delete() and
compact() took out of the list taken out of the records and renumbered; the
batch form is Codec.reclaim_records (honu_key_reclaim). route() is the host
statement of the bucket a write goes to, one per collection ID
(store.go:236-240, tx.go:112-120): a batch of records of many collections
partitioned stably by the store's table of collections; the batch form is
Codec.route_keys (honu_key_route). merge_buckets() is the host statement of
the write that follows, collections.Put (store.go:232, 395, 530) of the whole
routed batch, every record into its collection's bucket: merge() bucket by
bucket; the batch form is Codec.merge_bucket_keys (honu_key_merge_buckets).
"""
from __future__ import annotations

import bisect
from typing import Iterable, List, NamedTuple, Optional, Sequence

from .metadata import Scalar

KEY_SIZE = 29       # keys.go:14
KEY_VERSION = 0x01  # keys.go:18
PREFIX_SIZE = 17    # keyVersion + ObjectID: ObjectPrefix (keys.go:74-79)


class KeyError_(Exception):
    pass


class ErrBadVersion(KeyError_):  # keys.go:22
    def __init__(self):
        super().__init__("key is malformed: cannot decode specified version")


class ErrBadSize(KeyError_):  # keys.go:23
    def __init__(self):
        super().__init__("key is malformed: incorrect size")


class ErrMalformed(KeyError_):  # keys.go:24
    def __init__(self):
        super().__init__("key is malformed: cannot parse version components")


def new(oid: bytes, vers: Optional[Scalar] = None) -> bytes:
    """keys.New (keys.go:42-51). A None version leaves the object prefix
    followed by zeros: the key that sorts before every version of the object."""
    oid = bytes(oid)
    if len(oid) != 16:
        raise ValueError("an object ID is 16 bytes")
    key = bytearray(KEY_SIZE)
    key[0] = KEY_VERSION
    key[1:17] = oid
    if vers is not None:
        key[17:25] = int(vers.VID).to_bytes(8, "big")
        key[25:29] = int(vers.PID).to_bytes(4, "big")
    return bytes(key)


def check(key: bytes) -> None:
    """Key.Check (keys.go:110-120), raising where Go returns the error."""
    if len(key) != KEY_SIZE:
        raise ErrBadSize()
    if key[0] != KEY_VERSION:
        raise ErrBadVersion()


def object_id(key: bytes) -> bytes:  # keys.go:54-59 (Go panics with Check's error)
    check(key)
    return bytes(key[1:17])


def version(key: bytes) -> Scalar:  # keys.go:63-71
    check(key)
    return Scalar(PID=int.from_bytes(key[25:29], "big"), VID=int.from_bytes(key[17:25], "big"))


def object_prefix(key: bytes) -> bytes:  # keys.go:74-79
    check(key)
    return bytes(key[0:PREFIX_SIZE])


def object_limit(key: bytes) -> bytes:
    """Key.ObjectLimit (keys.go:84-92): the prefix with its last byte
    incremented, as Go's limit[16]++ does: a last byte of 0xff wraps to 0."""
    check(key)
    limit = bytearray(key[0:PREFIX_SIZE])
    limit[16] = (limit[16] + 1) & 0xFF
    return bytes(limit)


def has_version(key: bytes) -> bool:  # keys.go:97-108
    check(key)
    return any(key[PREFIX_SIZE:KEY_SIZE])


def sort(keys: Iterable[bytes]) -> List[bytes]:
    """sort.Sort(keys.Keys) (keys.go:126-130): ascending bytes.Compare, which
    is Python's order of bytes. Stable, which sort.Sort does not promise."""
    return sorted(bytes(k) for k in keys)


def _prefix_successor(probe: bytes) -> Optional[bytes]:
    """The least byte string above every string that has `probe` as prefix:
    the probe without its trailing 0xff bytes, its last byte incremented.
    None when there is none (an empty or all-0xff probe). Unlike ObjectLimit's
    limit[16]++ (keys.go:88-91) this carries instead of wrapping."""
    p = bytes(probe).rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def seek(sorted_keys: Sequence[bytes], probe: bytes):
    """Cursor.Seek (iterator/cursor.go:44-55) over a sorted list of keys, and
    where the probe's keys end: (pos, end). pos is the first position whose
    key is >= probe by bytes.Compare, which is Python's order of bytes (a key
    that has the probe as a proper prefix is greater), len(sorted_keys) where
    Seek returns nil; end is the first position >= pos whose key does not have
    the probe as prefix, so [pos, end) are the probe's keys. The batch form on
    the GPU is Codec.seek_keys (honu_key_seek in include/honu_codec.h)."""
    probe = bytes(probe)
    pos = bisect.bisect_left(sorted_keys, probe)
    nxt = _prefix_successor(probe)
    end = len(sorted_keys) if nxt is None else bisect.bisect_left(sorted_keys, nxt, lo=pos)
    return pos, end


def merge(a: Sequence[bytes], b: Sequence[bytes]) -> List[bytes]:
    """A batch of Puts into an ordered bucket (collections.Put, store.go:232,
    395; collectionsBucket.Put, store.go:530; the bkt.Put(k, value) calls of
    iterator/cursor_test.go:235), after which Cursor.Seek
    (iterator/cursor.go:44-55) and Collection.Has (collection.go:47-51) see
    the new keys: the stable merge of two sorted lists of keys by
    bytes.Compare, which is Python's order of bytes. On equal keys a's come
    before b's and each side keeps its own order, so a key's run ends on its
    latest arrival: bbolt's Put of a stored key replaces its value, and
    position end - 1 of seek() is the row that holds it. The rows returned are
    the objects given, not copies. The batch form on the GPU is
    Codec.merge_keys (honu_key_merge in include/honu_codec.h)."""
    out: List[bytes] = []
    i = j = 0
    while i < len(a) and j < len(b):
        if a[i] <= b[j]:
            out.append(a[i])
            i += 1
        else:
            out.append(b[j])
            j += 1
    out.extend(a[i:])
    out.extend(b[j:])
    return out


def delete(sorted_keys: Sequence[bytes], probes: Iterable[bytes]):
    """A batch of Deletes from an ordered bucket: (kept, removed), both in the
    list's order. A probe is a byte string of any length and removes every key
    that has it as prefix: a whole key is bucket.Delete(key); an id or an
    ObjectPrefix is the loop "Delete all collection versions" of Store.Drop
    (store.go:378-383: cursor.Seek(id[:]), then collections.Delete(key) while
    bytes.HasPrefix(key, id[:])); the empty probe is the tx.DeleteBucket behind
    it (store.go:399-404). The Go loop deletes while it walks with
    cursor.Next(), which bbolt documents as able to skip keys; this is what
    the loop states, every key with the prefix. A probe that matches nothing
    is not an error, as bbolt's Delete of an absent key returns nil; probes
    may repeat. The rows returned are the objects given, not copies. The batch
    form on the GPU is Codec.delete_keys (honu_key_delete in
    include/honu_codec.h)."""
    gone = [False] * len(sorted_keys)
    for probe in probes:
        pos, end = seek(sorted_keys, probe)
        for p in range(pos, end):
            gone[p] = True
    return ([k for k, g in zip(sorted_keys, gone) if not g], [k for k, g in zip(sorted_keys, gone) if g])


def compact(sorted_keys: Sequence[bytes]):
    """What a Put of a stored key does to the row it replaces: (kept, removed),
    both in the list's order, kept the last row of every run of equal keys.
    bbolt's Put replaces the value; merge() keeps the run, its last row the
    latest arrival, and this drops the rows before it. The rows returned are
    the objects given, not copies. The batch form on the GPU is
    Codec.delete_keys(..., superseded=True) (HONU_DELETE_SUPERSEDED)."""
    n = len(sorted_keys)
    gone = [p + 1 < n and bytes(sorted_keys[p + 1]) == bytes(sorted_keys[p]) for p in range(n)]
    return ([k for k, g in zip(sorted_keys, gone) if not g], [k for k, g in zip(sorted_keys, gone) if g])


def scan(sorted_keys: Sequence[bytes], ranges: Iterable, reverse: bool = False, limit: int = 0,
         latest: bool = False):
    """A batch of cursor walks over a sorted list of keys: for every (pos,
    end) of `ranges`, as seek() gives them, the positions a cursor visits,
    as a list of (range, pos) in output order, the ranges in the order given.
    Forward is Cursor.Next() from pos up to end (iterator/cursor.go:57-72;
    Collection.List, collection.go:32-35; the loop of store.go:379); `reverse`
    is Cursor.Prev() from end - 1 down to pos (cursor.go:74-89; Versions,
    "from the most recent version to the oldest", collection.go:106-110);
    `limit`, when not 0, stops a walk after that many steps, so reverse with
    limit 1 is Retrieve's "latest version" (collection.go:97-104) of an object
    range. With `latest` a walk visits only the rows that are the last of
    their object, the group of keys with the same first 17 bytes
    (ObjectPrefix, keys.go:74-79), so an object whose latest version lies
    outside the range is not visited. pos and end are clamped to the list
    (end to its length, pos to end); ranges may be empty, overlap, repeat and
    come in any order. Tombstones are not filtered here: filter() does. The
    batch form on the GPU is Codec.list_keys (honu_key_list in
    include/honu_codec.h)."""
    n = len(sorted_keys)
    out = []
    for q, (pos, end) in enumerate(ranges):
        end = min(int(end), n)
        pos = min(int(pos), end)
        walk = range(end - 1, pos - 1, -1) if reverse else range(pos, end)
        if latest:
            walk = [p for p in walk if p + 1 == n or
                    bytes(sorted_keys[p + 1])[:PREFIX_SIZE] != bytes(sorted_keys[p])[:PREFIX_SIZE]]
        else:
            walk = list(walk)
        out.extend((q, p) for p in (walk[:limit] if limit else walk))
    return out


def fetch(values: Sequence[bytes], visits: Iterable, order: Sequence[int], live=None):
    """Cursor.Object() (iterator/cursor.go:31-38: `obj := make([]byte,
    len(c.value)); copy(obj, c.value)`) at every row of a walk: for scan()'s
    list of (range, pos) the list of values[order[pos]], each a copy, in the
    walk's order. `order` maps a position of the sorted list to the index of
    its record (sort_keys' order), `values` holds the records. An index that
    is out of range, of `order` or of `values`, gives None, as Object() gives
    nil for a cursor without a value. `live`, when given, is a predicate on
    the record index that says False for a tombstone: such a row gives None
    too and stays in the list, the object that "will not be returned in list
    queries" (collection.go:132-134). A record named by several rows
    (overlapping ranges) is returned once per row. The batch form on the GPU
    is Codec.fetch_objects (honu_key_fetch in include/honu_codec.h)."""
    out = []
    for _, pos in visits:
        pos = int(pos)
        r = int(order[pos]) if 0 <= pos < len(order) else -1
        if not 0 <= r < len(values) or (live is not None and not live(r)):
            out.append(None)
        else:
            out.append(bytes(values[r]))
    return out


def filter(sorted_keys: Sequence[bytes], visits: Iterable, tomb, order: Optional[Sequence[int]] = None,
           deleted: bool = False):
    """What a listing leaves out: an object deleted with a tombstone version
    "will not be returned in list queries or retrieval"
    (collection.go:132-134), and Retrieve of it is "not found"
    (collection.go:97-101, 53-54). For scan()'s list of (range, pos) the
    visits that stay, in the walk's order. `tomb` is a predicate on the record
    index that says True for a tombstone; `order` maps a position of the
    sorted list to the index of its record (sort_keys' order), None where the
    position is the index. A visit goes when the record of its own row is a
    tombstone: right for a walk over latest versions (scan(latest=True), or
    reverse with limit 1 over object ranges). With `deleted` it goes when the
    record of its object's latest row is one, the last row of the group of
    keys with the same first 17 bytes (ObjectPrefix, keys.go:74-79), wherever
    that row lies: every version of a deleted object goes, its live older
    versions included, and a tombstone version of an object whose latest
    version is live stays (Versions() "includes tombstone versions",
    collection.go:106-107). A position outside the list, or outside `order`,
    names no object and stays. A visit's fate does not depend on the other
    visits, so both rules together are one call after the other. A range
    with no visit left is Retrieve's "not found". The batch form on the GPU is
    Codec.filter_rows (honu_key_filter in include/honu_codec.h)."""
    n = len(sorted_keys)
    out = []
    for q, pos in visits:
        p = int(pos)
        if 0 <= p < n and deleted:  # the object's latest row
            prefix = bytes(sorted_keys[p])[:PREFIX_SIZE]
            while p + 1 < n and bytes(sorted_keys[p + 1])[:PREFIX_SIZE] == prefix:
                p += 1
        if 0 <= p < n and (order is None or p < len(order)) and tomb(p if order is None else int(order[p])):
            continue
        out.append((q, pos))
    return out


class Next(NamedTuple):
    """One request's answer from next(): the honu_next row and its key."""
    scalar: Optional[Scalar]   # the assigned Version.Scalar, None unless NEXT_ASSIGNED
    parent: Optional[Scalar]   # Version.Parent, None without NEXT_HAS_PARENT
    parent_pos: Optional[int]  # the position of the parent in sorted_keys when it is the stored latest row
    flags: int                 # metadata.NEXT_*
    key: bytes                 # keys.New(ObjectID, scalar); the 17 request bytes and 12 zeros when not assigned


def next(sorted_keys: Sequence[bytes], requests: Sequence[bytes], op: int, pid: int, live=None,
         skip: Optional[Sequence] = None) -> List[Next]:
    """The version each of a batch of writes writes, the first thing every
    write of the reference decides: Store.Drop seeks the stored version and
    calls meta.Tombstone(lamport.ProcessID(), region) (store.go:361-395), which
    is pid.Next(&c.Version.Scalar) with the stored scalar as Parent
    (metadata/collection.go:56-63, lamport/pid.go:10-15); Store.New and
    Collection.Create start a history at Scalar{PID: 0, VID: 1}
    (store.go:192-198, collection.go:87-92). The bodies of Collection.Update,
    Merge, Delete and Retrieve are stubs upstream: what follows is their doc
    comments (collection.go:112-137) carried out with the code of Drop, New,
    Create and Tombstone, one `op` (metadata.NEXT_CREATE .. NEXT_DELETE) per
    call, the requests applied in order as the Go calls would be one after the
    other.

    A request is a byte string of which only the first 17 bytes count, the
    ObjectPrefix (keys.go:74-79). One that `skip` (a sequence of truth values)
    skips gets NEXT_SKIPPED alone; any other whose byte 0 is not keyVersion
    gets NEXT_BAD_KEY alone (Key.Check, keys.go:110-120); neither touches an
    object. For every other request the object's rows are seek()'s [pos, end)
    of the 17 bytes, FOUND = pos < end (Has, collection.go:47-51), the stored
    latest scalar is version(sorted_keys[end - 1]), and LIVE = FOUND and
    live(end - 1): `live` is a predicate on a position of sorted_keys that
    says False for a tombstone (Exists as documented, collection.go:53-54),
    None for no tombstones. FOUND and LIVE report the list as given. Then,
    with the object's state as the requests before this one left it:
      CREATE  an object that does not exist gets Scalar{0, 1} (collection.go:88,
              not the process's PID) and no parent; else NEXT_EXISTS.
      UPDATE  a live object gets pid_next(pid, latest), Parent = latest; else
              NEXT_NOT_FOUND.
      MERGE   an object that exists, deleted or not, as UPDATE; one that does
              not gets pid_next(pid, None) and no parent.
      DELETE  a live object gets pid_next(pid, latest), Parent = latest,
              NEXT_TOMBSTONE, and is deleted from then on; else NEXT_NOT_FOUND.
    So request r of an object (its rank among the counted requests with the
    same 17 bytes) with stored latest (P, V) gets VID V + 1 + r and Parent
    (P, V) for r == 0, (pid, V + r) after. VIDs are Go's uint64 and wrap as
    they do; once an object's VID has passed 2^64 - 1 in this call its rows
    carry NEXT_WRAPPED. parent_pos is end - 1 where the parent is that stored
    row. The batch form on the GPU is Codec.next_versions (honu_key_next in
    include/honu_codec.h), which equals this bit for bit."""
    from .metadata import (NEXT_ASSIGNED, NEXT_BAD_KEY, NEXT_CREATE, NEXT_DELETE, NEXT_EXISTS, NEXT_FOUND,
                           NEXT_HAS_PARENT, NEXT_LIVE, NEXT_MERGE, NEXT_NOT_FOUND, NEXT_SKIPPED, NEXT_TOMBSTONE,
                           NEXT_UPDATE, NEXT_WRAPPED, pid_next)
    if op not in (NEXT_CREATE, NEXT_UPDATE, NEXT_MERGE, NEXT_DELETE):
        raise ValueError("unknown op")
    state = {}  # prefix -> [exists, live, latest scalar, its position while it is the stored row, wrapped]
    out: List[Next] = []
    for i, req in enumerate(requests):
        prefix = bytes(req)[:PREFIX_SIZE]
        unassigned = prefix + bytes(KEY_SIZE - PREFIX_SIZE)
        if skip is not None and skip[i]:
            out.append(Next(None, None, None, NEXT_SKIPPED, unassigned))
            continue
        if len(prefix) != PREFIX_SIZE:
            raise ErrBadSize()
        if prefix[0] != KEY_VERSION:
            out.append(Next(None, None, None, NEXT_BAD_KEY, unassigned))
            continue
        pos, end = seek(sorted_keys, prefix)
        found = pos < end
        alive = found and (live is None or bool(live(end - 1)))
        flags = (NEXT_FOUND if found else 0) | (NEXT_LIVE if alive else 0)
        st = state.setdefault(prefix, [found, alive, version(bytes(sorted_keys[end - 1])) if found else None,
                                       end - 1 if found else None, False])
        if op == NEXT_CREATE:
            if st[0]:
                out.append(Next(None, None, None, flags | NEXT_EXISTS, unassigned))
                continue
            scalar, parent, parent_pos = Scalar(PID=0, VID=1), None, None
        elif op == NEXT_MERGE or st[1]:
            scalar, parent, parent_pos = pid_next(pid, st[2]), st[2], st[3]
            st[4] = st[4] or (parent is not None and scalar.VID < parent.VID)
        else:
            out.append(Next(None, None, None, flags | NEXT_NOT_FOUND, unassigned))
            continue
        st[0], st[1], st[2], st[3] = True, op != NEXT_DELETE, scalar, None
        flags |= NEXT_ASSIGNED | (NEXT_HAS_PARENT if parent is not None else 0)
        flags |= (NEXT_TOMBSTONE if op == NEXT_DELETE else 0) | (NEXT_WRAPPED if st[4] else 0)
        out.append(Next(scalar, parent, parent_pos, flags, new(prefix[1:], scalar)))
    return out


class Compare(NamedTuple):
    """One object's answer from compare(): the honu_seek row and the peer's row."""
    pos: int             # [pos, end) of a: the object's versions later than anything the peer holds
    end: int             # one past the object's latest row in a
    flags: int           # metadata.SEEK_FOUND (pos < end) | metadata.CMP_*
    peer: Optional[int]  # the position of the peer's latest row of the object in b, None without CMP_PEER_HAS


def compare(a: Sequence[bytes], b: Sequence[bytes]) -> List[Compare]:
    """The versions of two sorted lists of keys compared object by object:
    what two replicas decide when they meet. A lamport.Scalar "uses a 'latest
    writer wins' policy to determine how to solve conflicts"
    (lamport/scalar.go:15-24), lamport.Compare is the happens-before test
    (scalar.go:47-78), and a key stores its version big endian "to maintain
    lexicographic sorting" (keys.go:35-36), so the order of two keys of one
    object, Python's order of bytes, is lamport.Compare of their versions
    (metadata.scalar_compare). `a` is the local list, `b` the peer's: its
    whole list, or a digest of one key per object, its latest.

    One answer per object of `a`, the groups of keys with the same first 17
    bytes (ObjectPrefix, keys.go:74-79) in the list's order. For an object
    with rows [a0, a1) and latest key K = a[a1 - 1], the peer's rows [b0, b1)
    are seek(b, K[:17]), found by prefix equality and not by ObjectLimit's
    wrapping limit[16]++ (keys.go:88-91), and only b[b1 - 1], the peer's
    latest, decides:
      end    a1.
      pos    the first row of [a0, a1) whose key is greater than b[b1 - 1]
             when the peer has the object, else a0: [pos, end) is what
             latest-writer-wins sends, empty for an object equal or behind.
      flags  SEEK_FOUND when pos < end; CMP_PEER_HAS when b0 < b1; one of
             CMP_LATER (K > b[b1 - 1], or the peer has none), CMP_EARLIER and
             CMP_EQUAL; CMP_ANCESTOR, with PEER_HAS only, when the older
             side's latest key is a row of the newer side's range: a[pos - 1]
             == b[b1 - 1] with pos > a0 for LATER, K in b[b0:b1] for EARLIER,
             always for EQUAL. PEER_HAS without ANCESTOR is a forked write,
             the branch that "can be detected later" (collection.go:77-79);
             for EARLIER that is meaningful only when `b` is a whole list.
    Equal keys form runs, as after merge(); the bounds above say which row of
    a run counts. The objects only the peer has are the rows without
    CMP_PEER_HAS of compare(b, a). The batch form on the GPU is
    Codec.compare_keys (honu_key_compare in include/honu_codec.h), which
    equals this."""
    from .metadata import CMP_ANCESTOR, CMP_EARLIER, CMP_EQUAL, CMP_LATER, CMP_PEER_HAS, SEEK_FOUND
    a = [bytes(k) for k in a]
    b = [bytes(k) for k in b]
    out: List[Compare] = []
    a0 = 0
    while a0 < len(a):
        _, a1 = seek(a, a[a0][:PREFIX_SIZE])
        mine = a[a1 - 1]
        b0, b1 = seek(b, mine[:PREFIX_SIZE])
        pos, flags, peer = a0, 0, None
        if b0 < b1:
            peer = b1 - 1
            theirs = b[peer]
            pos = bisect.bisect_right(a, theirs, a0, a1)
            if mine > theirs:
                flags = CMP_LATER | (CMP_ANCESTOR if pos > a0 and a[pos - 1] == theirs else 0)
            elif mine < theirs:
                at = bisect.bisect_left(b, mine, b0, b1)
                flags = CMP_EARLIER | (CMP_ANCESTOR if at < b1 and b[at] == mine else 0)
            else:
                flags = CMP_EQUAL | CMP_ANCESTOR
            flags |= CMP_PEER_HAS
        else:
            flags = CMP_LATER
        out.append(Compare(pos, a1, flags | (SEEK_FOUND if pos < a1 else 0), peer))
        a0 = a1
    return out


def reclaim(order: Sequence[int], valid: int, values: Sequence[bytes], keys: Optional[Sequence] = None,
            statuses: Optional[Sequence] = None, info: Optional[Sequence] = None):
    """The space a Drop frees: Store.Drop exists "to free up space in the
    database" (store.go:314-322), and after the DeleteBucket behind it bbolt
    "marks the pages as free" (store.go:399-404). delete() and compact() take
    rows out of the sorted list; this takes the records they named out of
    `values`, the list of records that `order` indexes (sort_keys' order: the
    position of a sorted row -> the index of its record), and out of the
    per-record lists beside it (`keys`, `statuses`, `info`, each optional).

    A record r stays when order[p] == r for some p < v, v = min(valid,
    len(order)): the rows at or past v are the removed rows of a delete or the
    invalid rows of a batch, and the records only they name are freed. The
    records that stay are renumbered 0 .. kept - 1 in ascending old index, so
    arrival order survives, which merge()'s tie rule and compact() rest on.
    Returns (order_out, remap, source, values_out, keys_out, statuses_out,
    info_out):
      order_out   len(order) entries: the new index of order[p] for p < v,
                  SEEK_NONE for an index that names no record and for p >= v;
      remap       per old record its new index, or SEEK_NONE when freed;
      source      per new record its old index, ascending;
      values_out  [bytes(values[r]) for r in source], copies;
      keys_out, statuses_out, info_out  the lists given, gathered by source;
                  None for a list not given.
    An index repeated in order[:v] keeps its record once and both positions
    get the same new index; a `valid` above len(order) is clamped; an index
    that is negative or not below len(values) names no record. The first kept
    rows of the sorted list stand as they are: with them, order_out[:v] and
    values_out the state is what seek(), scan(), fetch(), filter(), next(),
    compare(), delete() and merge() take. The batch form on the GPU is
    Codec.reclaim_records (honu_key_reclaim in include/honu_codec.h), which
    equals this."""
    from .metadata import SEEK_NONE
    n, nrec = len(order), len(values)
    v = min(max(int(valid), 0), n)
    named = {int(order[p]) for p in range(v)}
    source = [r for r in range(nrec) if r in named]
    remap = [SEEK_NONE] * nrec
    for j, r in enumerate(source):
        remap[r] = j
    order_out = [remap[int(order[p])] if 0 <= int(order[p]) < nrec else SEEK_NONE for p in range(v)]
    order_out += [SEEK_NONE] * (n - v)

    def gather(rows):
        return None if rows is None else [rows[r] for r in source]

    return (order_out, remap, source, [bytes(values[r]) for r in source], gather(keys), gather(statuses),
            gather(info))


class Route(NamedTuple):
    """What route() returns. Class c < k is row c of the table, k the records
    of no known collection, k + 1 the positions that do not take part."""
    buckets: List[Optional[int]]  # per record: its table row, SEEK_NONE for none, None for a record no position names
    rows: List[tuple]             # per output row: (class, position, record or SEEK_NONE, flags)
    local: List[int]              # per output row: its index inside its class
    keys: Optional[List[bytes]]   # per output row: the record's key, 29 zero bytes for no record; None without keys
    offsets: List[int]            # k + 3: the first output row of each class, then m
    counts: List[int]             # k + 2


def route(ids: Sequence[bytes], table: Sequence[bytes], statuses: Optional[Sequence[int]] = None,
          seq: Optional[Sequence[int]] = None, keys: Optional[Sequence[bytes]] = None) -> Route:
    """A batch taken apart by collection. The store has one bbolt bucket per
    collection, named by the 16-byte collection ID:
    tx.CreateBucketIfNotExists(info.ID[:]) (store.go:236-240),
    t.tx.Bucket(collectionID[:]) with a nil bucket ErrRepairCollection
    (tx.go:112-120), Tx.Has and Tx.Exists (tx.go:141-158); every object
    carries its collection (meta.CollectionID = c.ID, collection.go:86).

    `ids` are the m records' collection IDs, `table` the store's k bucket
    names, ascending by bytes.Compare and distinct. Position p < m stands for
    record i = seq[p], or i = p without `seq`. Its class c is
      the row of `table` that equals ids[i], when record i takes part
            (`statuses` is None or statuses[i] == 0): the first such row;
      k     when it takes part and no row does: the nil bucket;
      k + 1 when it does not take part, or seq[p] names no record (not in
            [0, m)).
    Output row g is the g-th position when positions are ordered by (class,
    p): a stable partition, Python's sorted(). With `seq` a key sort of the
    batch (stable, the records that do not take part anywhere), every class's
    rows stand in key order with equal keys in arrival order: what sort() of
    that collection's keys alone gives, and so, as it stands, the B side of a
    merge() into that collection's list.
    Returns Route(buckets, rows, local, keys, offsets, counts): offsets[c] is
    the first row of class c and offsets[k + 2] = m; counts[c] = offsets[c +
    1] - offsets[c]; a row is (c, p, i or SEEK_NONE, LIST_ROW_HEAD on the
    first row of every class that has rows, else 0); local[g] = g -
    offsets[c]; keys[g] = bytes(keys[i]), or 29 zero bytes for a position
    that names no record; buckets[i] = c for c < k, else SEEK_NONE, for every
    record some position names. The batch form on the GPU is Codec.route_keys
    (honu_key_route in include/honu_codec.h), which equals this."""
    from .metadata import LIST_ROW_HEAD, SEEK_NONE
    table = [bytes(t) for t in table]
    m, k = len(ids), len(table)
    buckets: List[Optional[int]] = [None] * m
    classes = []
    for p in range(m):
        i = p if seq is None else int(seq[p])
        if not 0 <= i < m:
            classes.append((k + 1, p, SEEK_NONE))
            continue
        if statuses is not None and int(statuses[i]) != 0:
            c = k + 1
        else:
            c = bisect.bisect_left(table, bytes(ids[i]))
            if c == k or table[c] != bytes(ids[i]):
                c = k
        buckets[i] = c if c < k else SEEK_NONE
        classes.append((c, p, i))
    placed = sorted(classes, key=lambda row: row[0])  # stable: (class, p)
    ascending = [row[0] for row in placed]
    offsets = [bisect.bisect_left(ascending, c) for c in range(k + 3)]  # the rows of a class below c
    counts = [offsets[c + 1] - offsets[c] for c in range(k + 2)]
    rows, local, keys_out = [], [], None if keys is None else []
    for g, (c, p, i) in enumerate(placed):
        rows.append((c, p, i, LIST_ROW_HEAD if g == offsets[c] else 0))
        local.append(g - offsets[c])
        if keys is not None:
            keys_out.append(bytes(KEY_SIZE) if i == SEEK_NONE else bytes(keys[i]))
    return Route(buckets, rows, local, keys_out, offsets, counts)


class BucketRow(NamedTuple):
    key: bytes
    side: int   # 0: the row came from a, 1: from b
    index: int  # its index inside that side's bucket


def merge_buckets(a: Sequence[Sequence[bytes]], b: Sequence[Sequence[bytes]],
                  counts: Optional[Sequence[int]] = None) -> List[List[BucketRow]]:
    """A routed batch of Puts into every collection's bucket at once
    (collections.Put, store.go:232, 395, 530, into the bucket
    tx.Bucket(collectionID[:]) names, store.go:236-240, tx.go:112-120): `a`
    and `b` are k buckets each, bucket c a sorted list of keys, a's the
    resident rows and b's what route() left for row c of the table;
    `counts[c]`, when given, says how many of a[c]'s rows are valid, its first
    min(counts[c], len(a[c])). Bucket c of the result is merge() of a[c]'s
    valid rows and b[c]: on equal keys a's rows before b's, each side in its
    own order; invalid rows are dropped, so the result is tight. Every row is
    (key, side, index): where it came from. Concatenated, the buckets are the
    rows Codec.merge_bucket_keys (honu_key_merge_buckets in
    include/honu_codec.h) writes, and the lengths its counts."""
    if len(a) != len(b) or (counts is not None and len(counts) != len(a)):
        raise ValueError("a, b and counts have one entry per bucket")
    out = []
    for c in range(len(a)):
        va = len(a[c]) if counts is None else min(int(counts[c]), len(a[c]))
        # (key, side, index) orders as the key, then a before b: merge()'s own tie rule
        rows = merge([(bytes(key), 0, i) for i, key in enumerate(a[c][:va])],
                     [(bytes(key), 1, i) for i, key in enumerate(b[c])])
        out.append([BucketRow(*row) for row in rows])
    return out


def has(sorted_keys: Sequence[bytes], probe: bytes) -> bool:
    """Collection.Has (collection.go:47-51): key != nil && bytes.HasPrefix(key, probe)
    of the key Seek lands on."""
    pos, _ = seek(sorted_keys, probe)
    return pos < len(sorted_keys) and bytes(sorted_keys[pos]).startswith(bytes(probe))
