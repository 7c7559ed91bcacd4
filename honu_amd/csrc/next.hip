// next.hip — the version a write writes, for a batch of requests over the
// sorted key column: what every write of the reference decides first.
// Store.Drop seeks the stored version and calls meta.Tombstone(pid, region)
// (store.go:361-395), which is pid.Next(&Version.Scalar) with the stored scalar
// as Parent (metadata/collection.go:56-63, lamport/pid.go:10-15); Store.New and
// Collection.Create start a history at Scalar{PID 0, VID 1} (store.go:192-198,
// collection.go:87-92). The bodies of Collection.Update, Merge and Delete are
// stubs upstream: their ops are their doc comments (collection.go:112-137)
// carried out with the code of Drop, New, Create and Tombstone.
//
// A request is the 17-byte ObjectPrefix (keys.go:74-79) of a 29-byte row. A
// request names its object's rows [pos, end) in the column (seek_bounds, as
// honu_key_seek's 17-byte probe), the stored latest scalar (P, V) in bytes
// [17, 29) of row end - 1, and its rank r: the earlier requests of the call
// that name the same object. The call then answers as the Go calls would one
// after the other: request r of an object meets what requests 0 .. r - 1 left.
//
// Ranks need the requests grouped. Three steps on one stream:
//   pack    a thread per request: its 17 bytes and 12 zero bytes into the
//           workspace, with a status column (HONU_OK, or not for a request that
//           is skipped or whose byte 0 is not keyVersion). A request that does
//           not count is finished here: its SKIPPED / BAD_KEY row, its key and
//           its key status are written by the thread that saw why;
//   sort    launch_sort_keys over that column: stable, and the version bytes
//           are zero, so the requests of one object stand in request order and
//           the requests that do not count behind the valid count;
//   assign  a thread per sorted position p below the valid count: r = p - the
//           lower bound of its own prefix in the sorted requests (the row
//           before it answers for a run of one; thread_bound for the rest),
//           both bounds in the resident column, the op's row of the table
//           (include/honu_codec.h), the result through the order to its row i.
// Every row i is written by exactly one thread. The new kernels have no
// atomics, no spin-wait and no state outside the launch; the grids come from
// m. Every index read from device memory is clamped (keycol.h).
#include "kernels.h"
#include "keycol.h"

namespace honu {

// the sort's workspace, then the packed requests, their sorted column, the order, the status column and
// the valid count
uint64_t next_workspace_bytes(uint64_t m) {
    if (m == 0) return 0;
    return sort_workspace_bytes(m) + 2 * up256(HONU_KEY_LEN * m) + 2 * up256(4 * m) + up256(8);
}

struct NextWork {
    void *sort;
    uint8_t *packed;
    uint8_t *sorted;
    uint32_t *order;
    int32_t *status;
    uint64_t *count;
};

static NextWork next_carve(void *work, uint64_t m) {
    NextWork w;
    uint8_t *p = (uint8_t *)work;
    w.sort = p;
    p += sort_workspace_bytes(m);
    w.packed = p;
    p += up256(HONU_KEY_LEN * m);
    w.sorted = p;
    p += up256(HONU_KEY_LEN * m);
    w.order = (uint32_t *)p;
    p += up256(4 * m);
    w.status = (int32_t *)p;
    p += up256(4 * m);
    w.count = (uint64_t *)p;
    return w;
}

// one result row as two 8-byte and four 4-byte stores (d_out is 8-byte aligned, a row 32 bytes)
HONU_DEV void next_store(honu_next *out, uint64_t vid, uint64_t parent_vid, uint32_t pid, uint32_t parent_pid,
                         uint32_t parent_record, uint32_t flags) {
    uint64_t *q = reinterpret_cast<uint64_t *>(out);
    q[0] = vid;
    q[1] = parent_vid;
    uint32_t *w = reinterpret_cast<uint32_t *>(out) + 4;
    w[0] = pid;
    w[1] = parent_pid;
    w[2] = parent_record;
    w[3] = flags;
}

// the object prefix of a request, bytes [0, 17) and no byte more: as a key's two loads, bytes past 16 zero
HONU_DEV void load_prefix(const uint8_t *k, u32x4 &a, u32x4 &b) {
    a = *reinterpret_cast<const u32x4u *>(k);
    b = u32x4{(a.w >> 8) | ((uint32_t)k[16] << 24), 0u, 0u, 0u};
}

__global__ __launch_bounds__(HONU_BLOCK) void k_next_pack(
    const uint8_t *__restrict__ req, const int32_t *__restrict__ rstatus, uint32_t m, honu_next *__restrict__ out,
    uint8_t *__restrict__ keys_out, int32_t *__restrict__ key_status, NextWork W) {
    const uint32_t i = blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (i >= m) return;
    const bool skipped = rstatus && rstatus[i] != HONU_OK;
    u32x4 a, b;
    load_prefix(req + (uint64_t)HONU_KEY_LEN * i, a, b);
    store_key(W.packed + (uint64_t)HONU_KEY_LEN * i, a, b);
    const bool counts = !skipped && (a.x & 0xFFu) == 0x01u;  // Key.Check (keys.go:110-120)
    W.status[i] = counts ? HONU_OK : HONU_ERR_INPUT;
    if (counts) return;
    next_store(out + i, 0, 0, 0, 0, HONU_SEEK_NONE, skipped ? (uint32_t)HONU_NEXT_SKIPPED : (uint32_t)HONU_NEXT_BAD_KEY);
    store_key(keys_out + (uint64_t)HONU_KEY_LEN * i, a, b);
    key_status[i] = HONU_ERR_INPUT;
}

// what the call was given besides the requests
struct NextArgs {
    const uint8_t *sorted;  // the resident column
    const uint64_t *valid;
    uint64_t n;
    const uint32_t *order;
    const honu_record_info *info;
    uint32_t op, pid, region;
    int64_t now;
};

// the stamping Create describes (collection.go:81-92) into the caller's row: the named fields and no other byte
HONU_DEV void next_stamp(honu_meta *row, const NextArgs &A, uint64_t vid, uint32_t pid, bool has_parent,
                         uint64_t parent_vid, uint32_t parent_pid, const u32x4 &a, const u32x4 &b) {
    const uint32_t has = HONU_HAS_META | HONU_HAS_VERSION;
    row->present = ((row->present | has) & ~(uint32_t)HONU_HAS_PARENT) | (has_parent ? (uint32_t)HONU_HAS_PARENT : 0u);
    row->tombstone = A.op == HONU_NEXT_DELETE;
    row->region = A.region;
    row->vid = vid;
    row->pid = pid;
    row->parent_pid = parent_pid;
    row->parent_vid = parent_vid;
    row->version_created = A.now;
    if (!has_parent) row->created = A.now;
    row->modified = A.now;
    // ObjectID = request[1, 17): the row is 8-byte aligned, object_id at 96
    uint64_t *id = reinterpret_cast<uint64_t *>(row->object_id);
    const uint32_t o0 = (a.x >> 8) | (a.y << 24), o1 = (a.y >> 8) | (a.z << 24), o2 = (a.z >> 8) | (a.w << 24),
                   o3 = b.x;  // (b: the key's bytes [13, 29))
    id[0] = (uint64_t)o0 | ((uint64_t)o1 << 32);
    id[1] = (uint64_t)o2 | ((uint64_t)o3 << 32);
}

__global__ __launch_bounds__(HONU_BLOCK) void k_next_assign(NextArgs A, SeekMask M, uint32_t m,
                                                            honu_next *__restrict__ out,
                                                            uint8_t *__restrict__ keys_out,
                                                            int32_t *__restrict__ key_status,
                                                            honu_meta *__restrict__ meta, NextWork W) {
    const uint32_t p = blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= m || p >= valid_rows(W.count, m)) return;
    const uint32_t i = order_index(W.order[p], m);
    const uint8_t *row = W.sorted + (uint64_t)HONU_KEY_LEN * p;
    u32x4 a, b;
    load_key(row, a, b);
    uint32_t x[SORT_KEY_WORDS];
    load_masked(row, M, x);
    auto request = [&](uint32_t j, uint32_t k[SORT_KEY_WORDS]) { load_masked(W.sorted + (uint64_t)HONU_KEY_LEN * j, M, k); };
    auto before = [&](uint32_t j) {
        uint32_t k[SORT_KEY_WORDS];
        request(j, k);
        return packed_before(k, x, false);
    };
    // the earlier requests of the same object: the run's start is the lower bound of x over [0, p]
    uint32_t r = 0;
    if (p && !before(p - 1)) r = p - thread_bound(0, p - 1, before);

    const uint32_t v = (uint32_t)valid_rows(A.valid, A.n);
    uint32_t pos, end;
    seek_bounds([&](uint32_t j, uint32_t k[SORT_KEY_WORDS]) { load_masked(A.sorted + (uint64_t)HONU_KEY_LEN * j, M, k); },
                x, 0, v, 0, v, pos, end);
    const bool found = pos < end;
    uint64_t V = 0;
    uint32_t P = 0, latest = HONU_SEEK_NONE;
    bool live = found;
    if (found) {  // the stored latest scalar: BE64(VID) | BE32(PID) in bytes [17, 29), packed bytes [18, 30)
        uint32_t k[SORT_KEY_WORDS];
        pack_key(A.sorted + (uint64_t)HONU_KEY_LEN * (end - 1), true, k);
        V = ((uint64_t)(k[4] & 0xFFFFu) << 48) | ((uint64_t)k[5] << 16) | (k[6] >> 16);
        P = (k[6] << 16) | (k[7] >> 16);
        if (A.order) {
            latest = A.order[end - 1];
            if (A.info) live = !A.info[order_index(latest, A.n)].tombstone;
        }
    }

    bool assigned = false, has_parent = false, stored_parent = false;
    uint64_t vid = 0, parent_vid = 0;
    uint32_t pid = 0, parent_pid = 0, flags = (found ? (uint32_t)HONU_NEXT_FOUND : 0u) | (live ? (uint32_t)HONU_NEXT_LIVE : 0u);
    if (A.op == HONU_NEXT_CREATE) {
        assigned = !found && r == 0;
        vid = 1;  // Scalar{PID: 0, VID: 1}, not the process's PID (collection.go:88)
        if (!assigned) flags |= HONU_NEXT_EXISTS;
    } else {
        const bool del = A.op == HONU_NEXT_DELETE;
        assigned = A.op == HONU_NEXT_MERGE ? true : (live && (!del || r == 0));
        if (!assigned) flags |= HONU_NEXT_NOT_FOUND;
        pid = A.pid;
        vid = V + 1 + r;  // pid.Next r + 1 times over (uint64, wrapping as Go's)
        if (assigned && vid <= r) flags |= HONU_NEXT_WRAPPED;  // V + 1 + r passed 2^64 - 1
        has_parent = found || r;
        stored_parent = found && r == 0;
        parent_vid = stored_parent ? V : V + r;
        parent_pid = stored_parent ? P : A.pid;
        if (del) flags |= assigned ? (uint32_t)HONU_NEXT_TOMBSTONE : 0u;
    }
    uint8_t *key = keys_out + (uint64_t)HONU_KEY_LEN * i;
    if (!assigned) {
        next_store(out + i, 0, 0, 0, 0, HONU_SEEK_NONE, flags);
        store_key(key, a, b);
        key_status[i] = HONU_ERR_INPUT;
        return;
    }
    if (!has_parent) parent_vid = 0, parent_pid = 0;
    flags |= HONU_NEXT_ASSIGNED | (has_parent ? (uint32_t)HONU_NEXT_HAS_PARENT : 0u);
    next_store(out + i, vid, parent_vid, pid, parent_pid, stored_parent ? latest : HONU_SEEK_NONE, flags);
    // keys.New (keys.go:42-51): the prefix, BE64(VID), BE32(PID)
    x[4] |= (uint32_t)(vid >> 48);
    x[5] = (uint32_t)(vid >> 16);
    x[6] = ((uint32_t)vid << 16) | (pid >> 16);
    x[7] = pid << 16;
    unpack_key(key, x);
    key_status[i] = HONU_OK;
    if (meta) next_stamp(meta + i, A, vid, pid, has_parent, parent_vid, parent_pid, a, b);
}

hipError_t launch_key_next(const uint8_t *sorted, const uint64_t *valid, uint64_t n, const uint32_t *order,
                           const honu_record_info *info, const uint8_t *req, const int32_t *rstatus, uint64_t m,
                           uint32_t op, uint32_t pid, uint32_t region, int64_t now, honu_next *out, uint8_t *keys_out,
                           int32_t *key_status, honu_meta *meta, void *work, const ScanState &S, uint64_t scan_rows,
                           hipStream_t s) {
    if (m == 0) return hipSuccess;
    const NextWork W = next_carve(work, m);
    const unsigned blocks = (unsigned)((m + HONU_BLOCK - 1) / HONU_BLOCK);
    hipLaunchKernelGGL(k_next_pack, dim3(blocks), dim3(HONU_BLOCK), 0, s, req, rstatus, (uint32_t)m, out, keys_out,
                       key_status, W);
    const hipError_t e = launch_sort_keys(W.packed, W.status, m, W.order, W.sorted, W.count, W.sort, S, scan_rows, s);
    if (e != hipSuccess) return e;
    const NextArgs A = {sorted, valid, n, order, info, op, pid, region, now};
    hipLaunchKernelGGL(k_next_assign, dim3(blocks), dim3(HONU_BLOCK), 0, s, A, seek_mask(17), (uint32_t)m, out, keys_out,
                       key_status, meta, W);
    return hipGetLastError();
}

}  // namespace honu
