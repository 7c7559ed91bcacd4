"""Inputs of the system-object write-set tests (test_system_bounds_host.py,
test_gpu_system_bounds.py), built once per process on the CPU: collections
that each isolate one edge of MarshalSystem (object/system.go:10-31,
collection.go:137-237), and records that each isolate one edge of
UnmarshalSystem / lani.Unmarshal(raw, &Collection{}) (system.go:33-45,
collection.go:240-356, lani/decode.go). A plain helper module, not a conftest."""
import copy
import functools

import numpy as np

from fixtures import py_marshal_system, py_uvarint
from honu_amd.metadata import AccessControl, Compression, Encryption, Publisher, Scalar, SchemaVersion, Version
from honu_amd.system import Collection, Field, Index, pack_system_batch

U32, I64_MIN, I64_MAX = 2**32 - 1, -2**63, 2**63 - 1


def u(k: int) -> bytes:
    """The k-th deterministic ULID."""
    return bytes((37 * k + 11 * j + 3) & 0xFF for j in range(16))


def _acl(n, nil=()):
    return [None if j in nil else AccessControl(u(100 + j), (j * 29) & 0xFF) for j in range(n)]


def _index(j, name="ix", field="f", ref="r"):
    return Index(u(200 + j), name, j % 8, None if field is None else Field(field, j % 9, u(300 + j)),
                 None if ref is None else Field(ref, (j + 1) % 9, u(400 + j)))


def full_collection() -> Collection:
    """Every optional struct present, all three lists with a nil entry, every
    varint one byte long: a cut of its encoding falls either on the start of
    a field or inside a ULID or a frame (full_atoms)."""
    return Collection(
        ID=u(1), Name="edge", Version=Version(Scalar(3, 9), 7, Scalar(2, 8), True, 11), Owner=u(2), Group=u(3),
        Permissions=0o44, ACL=[AccessControl(u(4), 1), None, AccessControl(u(5), 255)], WriteRegions=[1, 100],
        Publisher=Publisher(u(6), u(7), b"\x7f\x00\x00\x01", "agent"), Schema=SchemaVersion("sch", 1, 2, 3),
        Encryption=Encryption("pk", b"ek!", b"hm", b"sig12", 1, 2, 3), Compression=Compression(2, -3), Flags=5,
        Indexes=[_index(0), None, Index(u(11), "", 2, None, None)], Created=21, Modified=-22)


def full_atoms():
    """The lengths of the indivisible reads of full_collection()'s system
    object after its version byte, in order: 1 for a flag, a byte or a
    one-byte varint, 16 for a ULID, 1 + k for a frame of k bytes."""
    c = full_collection()
    fr = lambda b: [1 + len(b)]  # noqa: E731
    a = [1, 16] + fr(c.Name)                                   # struct flag, ID, Name
    a += [1, 1, 1, 1, 1, 1, 1, 1, 1]                           # Version: flag pid vid region flag pid vid tomb created
    a += [16, 16, 1, 1]                                        # Owner, Group, Permissions, len(ACL)
    for e in c.ACL:
        a += [1] if e is None else [1, 16, 1]
    a += [1] + [1] * len(c.WriteRegions)
    a += [1, 16, 16] + fr(c.Publisher.IPAddress) + fr(c.Publisher.UserAgent)
    a += [1] + fr(c.Schema.Name) + [1, 1, 1]
    e = c.Encryption
    a += [1] + fr(e.PublicKeyID) + fr(e.EncryptionKey) + fr(e.HMACSecret) + fr(e.Signature) + [1, 1, 1]
    a += [1, 1, 1]                                             # Compression
    a += [1, 1]                                                # Flags, len(Indexes)
    for x in c.Indexes:
        if x is None:
            a += [1]
            continue
        a += [1, 16] + fr(x.Name) + [1]
        for f in (x.Field, x.Ref):
            a += [1] if f is None else [1] + fr(f.Name) + [1, 16]
    a += [1, 1]                                                # Created, Modified
    assert sum(a) + 2 == len(py_marshal_system(c))
    return a


@functools.lru_cache(maxsize=None)
def _edge_collections():
    out = [None, Collection()]
    base = dict(ID=u(20), Owner=u(21), Group=u(22))
    # each optional struct alone, all of them
    out += [Collection(Version=Version(Scalar(5, 6), 7, None, False, 8), **base),
            Collection(Version=Version(Scalar(5, 6), 7, Scalar(9, 10), False, 8), **base),
            Collection(Publisher=Publisher(u(23), u(24), b"\x0a\x00\x00\x01", "ua"), **base),
            Collection(Schema=SchemaVersion("schema", 1, 2, 3), **base),
            Collection(Encryption=Encryption("key", b"e" * 32, b"h" * 32, b"s" * 64, 1, 2, 3), **base),
            Collection(Compression=Compression(3, 9), **base),
            full_collection()]
    # uvarint length boundaries of a frame, and the 64-byte step of the writer's run()
    out += [Collection(Name="n" * k, **base) for k in (0, 1, 63, 64, 65, 127, 128, 129, 16383, 16384)]
    # the other frames at the same boundaries, nil and empty byte slices
    out += [Collection(Publisher=Publisher(u(23), u(24), ip, "a" * k), **base)
            for ip, k in ((None, 0), (b"", 127), (bytes(range(16)), 128), (b"\x0a\x00\x00\x02", 16384))]
    out += [Collection(Schema=SchemaVersion("s" * k, k, 1, 0), **base) for k in (0, 63, 64, 65, 127, 128)]
    out += [Collection(Encryption=Encryption("k" * a, b"e" * b or None, b"h" * c or None, b"s" * d or None, 1, 2, 3),
                       **base)
            for a, b, c, d in ((0, 0, 0, 0), (127, 128, 63, 64), (128, 127, 65, 129), (1, 16383, 1, 1),
                               (1, 1, 16384, 1), (64, 64, 64, 16383))]
    # ACL
    out += [Collection(ACL=_acl(1), **base), Collection(ACL=_acl(127), **base), Collection(ACL=_acl(128), **base),
            Collection(ACL=_acl(3, nil=(0,)), **base), Collection(ACL=_acl(3, nil=(2,)), **base),
            Collection(ACL=_acl(127, nil=range(127)), **base), Collection(ACL=_acl(128, nil=range(0, 128, 2)), **base)]
    # WriteRegions: nil and empty (both len 0 on the wire), every uvarint width, the count's boundaries
    out += [Collection(WriteRegions=None, **base), Collection(WriteRegions=[], **base),
            Collection(WriteRegions=[0, 127, 128, 16383, 16384, U32], **base),
            Collection(WriteRegions=[U32], **base), Collection(WriteRegions=[0], **base),
            Collection(WriteRegions=[(j * 2654435761) & U32 for j in range(127)], **base),
            Collection(WriteRegions=[(j * 40503) & U32 for j in range(128)], **base)]
    # Indexes
    out += [Collection(Indexes=[_index(0)], **base),
            Collection(Indexes=[_index(j) for j in range(127)], **base),
            Collection(Indexes=[_index(j, field=None if j % 3 == 0 else "f", ref=None if j % 2 else "r")
                                for j in range(128)], **base),
            Collection(Indexes=[None, _index(1), None], **base), Collection(Indexes=[None] * 5, **base),
            Collection(Indexes=[_index(0, field=None, ref=None), _index(1, field="only", ref=None),
                                _index(2, field=None, ref="only")], **base),
            Collection(Indexes=[_index(j, name="i" * k, field="f" * k, ref="r" * k)
                                for j, k in enumerate((0, 127, 128))], **base)]
    # u32 and u64 fields at their ends
    out += [Collection(Version=Version(Scalar(0, 0), 0, Scalar(0, 0), False, 0),
                       Schema=SchemaVersion("", 0, 0, 0), **base),
            Collection(Version=Version(Scalar(U32, 2**64 - 1), U32, Scalar(U32, 2**63), False, 1),
                       Schema=SchemaVersion("s", U32, U32, U32), **base),
            Collection(Version=Version(Scalar(1, 2**63), 1, Scalar(1, 2**64 - 1), False, 1), **base)]
    # zig-zag varints at their ends
    out += [Collection(Created=t, Modified=t, Version=Version(Scalar(1, 1), 1, None, False, t),
                       Compression=Compression(1, t), **base) for t in (0, -1, I64_MIN, I64_MAX)]
    # bytes at their ends, tombstone
    out += [Collection(Permissions=0, Flags=0, **base), Collection(Permissions=255, Flags=255, **base),
            Collection(Permissions=255, Flags=255, ACL=[AccessControl(u(30), 0), AccessControl(u(31), 255)],
                       Encryption=Encryption("", None, None, None, 255, 255, 255), Compression=Compression(255, 0),
                       Version=Version(Scalar(1, 1), 1, None, True, 1), **base)]
    return tuple(out)


def edge_collections():
    """Collections (or None) that each isolate one edge of the encoder."""
    return [copy.deepcopy(c) for c in _edge_collections()]


def edge_objects(oracle):
    """The system objects of edge_collections(), by the oracle."""
    out, off, st = oracle.system_marshal_batch(pack_system_batch(edge_collections()))
    assert (st == 0).all()
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(st))]


def _pos(c, change):
    """Where the system object of `c` first differs from that of `c` after
    change(c): the byte a one-field change lands on."""
    d = copy.deepcopy(c)
    change(d)
    a, b = py_marshal_system(c), py_marshal_system(d)
    return next(i for i in range(min(len(a), len(b))) if a[i] != b[i])


def _set(path, value):
    def change(c):
        *head, last = path
        for p in head:
            c = c[p] if isinstance(p, int) else getattr(c, p)
        if isinstance(last, int):
            c[last] = value
        else:
            setattr(c, last, value)
    return change


def boolean_positions():
    """Every byte of full_collection()'s system object that DecodeBool reads
    (the struct flag, the nil flags of Version, Parent, each ACL entry,
    Publisher, Schema, Encryption, Compression, each Index, its Field and Ref;
    Tombstone), found by flipping each in turn."""
    c = full_collection()
    pos = [1]
    pos += [_pos(c, _set(p, v)) for p, v in [
        (("Version",), None), (("Version", "Parent"), None), (("Version", "Tombstone"), False),
        (("ACL", 0), None), (("ACL", 1), AccessControl()), (("ACL", 2), None),
        (("Publisher",), None), (("Schema",), None), (("Encryption",), None), (("Compression",), None),
        (("Indexes", 0), None), (("Indexes", 0, "Field"), None), (("Indexes", 0, "Ref"), None),
        (("Indexes", 1), Index()), (("Indexes", 2), None), (("Indexes", 2, "Field"), Field()),
        (("Indexes", 2, "Ref"), Field())]]
    assert len(set(pos)) == len(pos) == 18
    return pos


def engineered_records():
    """(label, headed record, UnmarshalSystem status) of the hand-made bad
    records; the statuses are literals from the Go reference:
    - a flag byte of 2: ErrParseBoolean (decode.go:111-118) -> 6;
    - DecodeUint32 over uvarint(2^32): five bytes fit MaxVarintLen32 and
      uint32(v) truncates (decode.go:133-145) -> 0, pid 0;
    - five / ten continuation bytes, or a tenth byte above 1: binary.Uvarint
      gives k <= 0 (decode.go:139-141, 161-163) -> 7; in a frame's length
      ErrNoLength (decode.go:274-277) -> 5;
    - len(ACL), len(Indexes) above 2^45 and len(WriteRegions) above 2^46:
      make() panics over maxAlloc = 2^48 bytes (collection.go:283, :335,
      region.go:160) -> 8; at the limit make() is let through and the first
      entry's read meets the window's end: io.EOF (decode.go:95, :128) -> 3;
    - records of 0 and 1 bytes: obj[1:len(obj)-1] panics (system.go:40) -> 8;
      2 bytes: an empty window, io.EOF -> 3; 3 bytes: a nil collection -> 0."""
    c = full_collection()
    obj = py_marshal_system(c)
    out = [(f"bool2@{p}", obj[:p] + b"\x02" + obj[p + 1:], 6) for p in boolean_positions()]
    pid = _pos(c, _set(("Version", "Scalar", "PID"), 4))
    vid = _pos(c, _set(("Version", "Scalar", "VID"), 10))
    name = _pos(c, _set(("Name",), "edge+"))
    out += [("pid=uvarint(2^32)", obj[:pid] + py_uvarint(2**32) + obj[pid + 1:], 0),
            ("pid 5 continuation bytes", obj[:pid] + b"\xff" * 5 + b"\x01" + obj[pid + 1:], 7),
            ("vid 10-byte overflow", obj[:vid] + b"\xff" * 9 + b"\x02" + obj[vid + 1:], 7),
            ("vid 11 bytes", obj[:vid] + b"\xff" * 10 + b"\x01" + obj[vid + 1:], 7),
            ("vid 2^64-1", obj[:vid] + b"\xff" * 9 + b"\x01" + obj[vid + 1:], 0),
            ("name length overflows", obj[:name] + b"\xff" * 10 + b"\x00", 5)]
    nacl = _pos(c, lambda d: d.ACL.append(None))
    nreg = _pos(c, lambda d: d.WriteRegions.append(1))
    nidx = _pos(c, lambda d: d.Indexes.append(None))
    for label, p, lim in (("ACL", nacl, 2**45), ("WriteRegions", nreg, 2**46), ("Indexes", nidx, 2**45)):
        out += [(f"len({label})=limit", obj[:p] + py_uvarint(lim) + b"\x00", 3),
                (f"len({label})=limit+1", obj[:p] + py_uvarint(lim + 1) + b"\x00", 8)]
    out += [("len 0", b"", 8), ("len 1", b"\x01", 8), ("len 2", b"\x01\x00", 3), ("len 3", b"\x01\x00\x00", 0)]
    return out


def prefix_status(window_len, atoms):
    """The error of a decode whose window ends after window_len bytes of the
    reads `atoms`: io.EOF (3) where the next read starts at the window's end
    (decode.go:95, :128, :150, :172, :210, :263), io.ErrUnexpectedEOF (4)
    inside a ULID or a frame (decode.go:214-216, :45-47), 0 for all of it."""
    at = 0
    for a in atoms:
        if window_len == at:
            return 3
        if window_len < at + a:
            return 4
        at += a
    assert window_len == at
    return 0


def prefix_records():
    """Every prefix of full_collection()'s system object (headed) and of its
    lani.Marshal body obj[2:-1] (headless), with the status each decodes to
    through its own entry point: [(record, status)], [(record, status)]."""
    obj = py_marshal_system(full_collection())
    atoms = full_atoms()
    headed = []
    for k in range(len(obj) + 1):  # the window is obj[1:k-1]
        headed.append((obj[:k], 8 if k < 2 else prefix_status(k - 2, atoms)))
    body = obj[2:-1]
    headless = [(body[:k], prefix_status(k, atoms[1:])) for k in range(len(body) + 1)]
    return headed, headless


def edge_records(oracle, headless=False):
    """The records of the decode tests: the encoded edge set (headless: their
    lani.Marshal bodies, which is what that entry point decodes), every prefix
    of the all-present object headed and as its body, and the engineered bad
    records. The edge set, cycled, alternates with the others, so that
    failing rows sit between rows with lists throughout."""
    good = edge_objects(oracle)
    if headless:
        good = [o[2:-1] for o in good]
    headed, bodies = prefix_records()
    bad = [r for _, r, _ in engineered_records()] + [r for r, _ in headed] + [r for r, _ in bodies]
    assert len(bad) >= len(good)
    out = []
    for i, b in enumerate(bad):  # the edge set cycles among the others
        out += [good[i % len(good)], b]
    return out


def lists_record(headless=False):
    obj = py_marshal_system(full_collection())
    return obj[2:-1] if headless else obj


def batch_of(records, n, headless=False):
    """`records` cycled to n rows; rows 1023 and 1024 (the last row of the
    three-column scan's first short tile and the first of its second) carry
    all three lists."""
    rows = [records[i % len(records)] for i in range(n)]
    for i in (1023, 1024):
        if i < n:
            rows[i] = lists_record(headless)
    return rows


def arena(records):
    """(rec, off): the records back to back and their n + 1 offsets."""
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    rec = np.frombuffer(b"".join(records) + b"\0", np.uint8)[: int(off[-1])]
    return rec, off


COLLECTION_SPANS = (("name", 1 << 0), ("schema_name", 1 << 3), ("ip_address", 1 << 4), ("user_agent", 1 << 4),
                    ("public_key_id", 1 << 5), ("encryption_key", 1 << 5), ("hmac_secret", 1 << 5),
                    ("signature", 1 << 5))


def wild_spans(var_len):
    """off > var_len; len > var_len - off; off = 2^64 - 1 with len = 2 (off + len wraps)."""
    return [(var_len + 1, 1), (var_len - 1, 2), (2**64 - 1, 2)]


def input_error_batch():
    """(batch, statuses): rows of the all-present collection with one defect
    each, and what honu_system_sizes gives them (HONU_ERR_INPUT = 10 where a
    live span or a list lies outside its arena, else 0): each of the eight
    collection spans out of range under a set presence bit and under a clear
    one (name's bit is HONU_HAS_COLLECTION: the row is then a nil collection),
    spans of no bytes at a wild offset, each index span gated by present /
    has_field / has_ref, each list's offset past its table, its count past
    the table's end, and offset + count wrapping."""
    n = 1 + 8 + 8 + 2 + 6 + 9 + 1
    hb = pack_system_batch([full_collection()] * n)
    r, want = hb.rows, [0] * n
    wild = wild_spans(len(hb.var))
    i = 1
    for k, (field, bit) in enumerate(COLLECTION_SPANS):  # under a set bit
        r[i][field] = wild[k % 3]
        want[i] = 10
        i += 1
    for k, (field, bit) in enumerate(COLLECTION_SPANS):  # under a clear bit
        r[i][field] = wild[(k + 1) % 3]
        r[i]["present"] &= ~np.uint32(bit)
        i += 1
    r[i]["name"] = (2**64 - 1, 0)
    r[i + 1]["signature"] = (len(hb.var) + 5, 0)
    i += 2
    for k, (field, gate) in enumerate((("name", "present"), ("field_name", "has_field"), ("ref_name", "has_ref"))):
        x = int(r[i]["index_off"])  # the row's first Index: present, with Field and Ref
        assert hb.index[x]["present"] and hb.index[x]["has_field"] and hb.index[x]["has_ref"]
        hb.index[x][field] = wild[k]
        want[i] = 10
        x = int(r[i + 1]["index_off"])
        hb.index[x][field] = wild[(k + 1) % 3]
        hb.index[x][gate] = 0
        i += 2
    for f, table in (("acl", hb.acl), ("regions", hb.regions), ("index", hb.index)):
        r[i][f + "_off"] = len(table) + 1
        r[i + 1][f + "_count"] = len(table) - int(r[i + 1][f + "_off"]) + 1
        r[i + 2][f + "_off"], r[i + 2][f + "_count"] = 2**64 - 1, 2
        want[i:i + 3] = [10, 10, 10]
        i += 3
    assert i == n - 1
    return hb, want


def cycled(cols, n):
    return [copy.deepcopy(cols[i % len(cols)]) for i in range(n)]


def decode_caps(full):
    """The capacity settings of the GPU decode test for a batch decoded
    without capacities (`full`): each table's capacity alone at need, need - 1,
    a cut inside a mid-batch row's list, half and 0, and all three at 0."""
    rows, st, _, _, _, tot = full
    need = [int(v) for v in tot]
    names = ("acl_cap", "regions_cap", "index_cap")
    out = []
    for k, (name, f) in enumerate(zip(names, ("acl", "regions", "index"))):
        mid = [i for i in range(len(st) // 3, len(st)) if st[i] == 0 and int(rows[i][f + "_count"]) >= 2][0]
        inside = int(rows[mid][f + "_off"]) + 1
        out += [{name: c} for c in (need[k], need[k] - 1, inside, need[k] // 2, 0)]
    out.append({name: 0 for name in names})
    return out


def cap_batch(oracle_lib, headless=False, n=257):
    return arena(batch_of(edge_records(oracle_lib, headless), n, headless))


def out_caps(hb, ooff, ost, oout):
    """out_cap inside a mid-batch record's ID, its name and its ACL list,
    exactly at a record's end, and 0."""
    n = len(ost)
    r = hb.rows
    j = [i for i in range(n // 3, n) if ost[i] == 0 and int(r[i]["acl_count"]) >= 2 and int(r[i]["name"]["len"]) >= 2 and
         hb.acl[int(r[i]["acl_off"])]["present"]][0]
    b, nl = int(ooff[j]), int(r[j]["name"]["len"])
    first = b"\x01" + hb.acl[int(r[j]["acl_off"])]["client_id"].tobytes()
    lst = b + oout[b:int(ooff[j + 1])].tobytes().index(first)
    return {"id": b + 2 + 8, "name": b + 2 + 16 + 1 + nl // 2, "acl_list": lst + 18 + 7, "record_end": int(ooff[j + 1]),
            "zero": 0}


def encode_cap_batch():
    """257 rows: the edge set cycled (the all-present collection, with a name
    and all three lists, comes round in the middle third)."""
    return cycled(edge_collections(), 257)
