// route.hip — a batch taken apart by collection: the bucket each record's
// write goes to. The reference store has one bbolt bucket per collection,
// named by the 16-byte collection ID: tx.CreateBucketIfNotExists(info.ID[:])
// (store.go:236-240), t.tx.Bucket(collectionID[:]) with a nil bucket
// ErrRepairCollection (tx.go:112-120), Tx.Has and Tx.Exists (tx.go:141-158);
// every object carries its collection (meta.CollectionID = c.ID,
// collection.go:86; honu_meta.collection_id).
//
// A position p of the batch stands for record i (d_seq[p], or p). Its class
// is the row of the table of collections that equals the record's ID, k for
// an ID the table does not hold, k + 1 for a position that does not take
// part (route_find.h). The output is the stable partition of the positions by
// class. Three steps on one stream:
//   find   a thread per position: the ID (16 bytes at any address, one load,
//          four big-endian words), its lower bound in the table and the test
//          for equality; the table staged in LDS by every workgroup when it
//          has no more than ROUTE_STAGE rows, read from memory otherwise, one
//          loop in two forms (route_find.h). The thread writes d_bucket and
//          packs the class into a 29-byte sort row of the workspace;
//   sort   launch_sort_keys over those rows: stable, and only the digits in
//          which the classes differ run a pass (sort.hip's plan);
//   emit   a thread per sorted row g: its class out of the sorted rows, its
//          position out of the order, the start of its class (the row before
//          it answers for a head; a bisection over the rows before it for the
//          rest) for d_local, the row, the key; and a thread per class
//          c <= k + 2: d_bucket_off[c] as a bound over the sorted classes and
//          the count as the next bound less this one.
// The new kernels have no atomics, no spin-wait and no state outside the
// launch; the grids come from m and k. Every index read from device memory is
// clamped (keycol.h; route_row_class).
#include "kernels.h"
#include "keycol.h"

namespace honu {

typedef uint32_t u32u __attribute__((aligned(1)));

// 16 bytes at any byte address as four big-endian words: one load (common.h u32x4u)
HONU_DEV void route_load_id(const uint8_t *p, uint32_t w[4]) {
    const u32x4 v = *reinterpret_cast<const u32x4u *>(p);
    w[0] = __builtin_bswap32(v.x);
    w[1] = __builtin_bswap32(v.y);
    w[2] = __builtin_bswap32(v.z);
    w[3] = __builtin_bswap32(v.w);
}

HONU_DEV uint32_t route_load_be32(const uint8_t *p) { return __builtin_bswap32(*reinterpret_cast<const u32u *>(p)); }

}  // namespace honu

#define HONU_ROUTE_FN HONU_DEV
#define HONU_ROUTE_LOAD_ID(p, w) honu::route_load_id((p), (w))
#define HONU_ROUTE_LOAD_BE32(p) honu::route_load_be32(p)
#include "route_find.h"

namespace honu {

// table rows a workgroup stages: 2048 rows are 32 KiB of LDS, the trade seek's fence makes
constexpr uint32_t ROUTE_STAGE = 2048;

uint32_t route_stage() { return ROUTE_STAGE; }

// the sort's workspace, then the packed classes, their sorted column, the order and the sort's valid count
uint64_t route_workspace_bytes(uint64_t m) {
    if (m == 0) return 0;
    return sort_workspace_bytes(m) + 2 * up256(HONU_KEY_LEN * m) + up256(4 * m) + up256(8);
}

struct RouteWork {
    void *sort;
    uint8_t *packed;
    uint8_t *sorted;
    uint32_t *order;
    uint64_t *count;
};

static RouteWork route_carve(void *work, uint64_t m) {
    RouteWork w;
    uint8_t *p = (uint8_t *)work;
    w.sort = p;
    p += sort_workspace_bytes(m);
    w.packed = p;
    p += up256(HONU_KEY_LEN * m);
    w.sorted = p;
    p += up256(HONU_KEY_LEN * m);
    w.order = (uint32_t *)p;
    p += up256(4 * m);
    w.count = (uint64_t *)p;
    return w;
}

// what the call was given
struct RouteArgs {
    const uint8_t *ids;
    uint64_t id_stride;
    const int32_t *status;
    const uint32_t *seq;
    const uint8_t *table;
    const uint8_t *keys;
    uint32_t m, k;
};

template <bool STAGED>
__global__ __launch_bounds__(HONU_BLOCK) void k_route_find(RouteArgs A, uint32_t *__restrict__ bucket, RouteWork W) {
    __shared__ uint32_t rows[STAGED ? ROUTE_STAGE * ROUTE_ID_WORDS : ROUTE_ID_WORDS];
    if (STAGED) {  // (A.k <= ROUTE_STAGE: launch_key_route)
        for (uint32_t r = threadIdx.x; r < A.k; r += HONU_BLOCK)
            route_load_id(A.table + (uint64_t)ROUTE_ID_LEN * r, rows + ROUTE_ID_WORDS * r);
        __syncthreads();
    }
    const uint32_t p = blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= A.m) return;
    const uint32_t i = A.seq ? A.seq[p] : p;
    const bool named = i < A.m;
    const bool part = named && (!A.status || A.status[i] == HONU_OK);
    uint32_t lb = A.k;
    bool same = false;
    if (part) {
        uint32_t id[ROUTE_ID_WORDS], row[ROUTE_ID_WORDS];
        route_load_id(A.ids + A.id_stride * i, id);
        lb = STAGED ? route_lower_bound_words(rows, A.k, id) : route_lower_bound_bytes(A.table, A.k, id);
        if (lb < A.k) {
            if (STAGED) {
#pragma unroll
                for (int j = 0; j < ROUTE_ID_WORDS; j++) row[j] = rows[ROUTE_ID_WORDS * lb + j];
            } else {
                route_load_id(A.table + (uint64_t)ROUTE_ID_LEN * lb, row);
            }
            same = route_id_same(row, id);
        }
    }
    const uint32_t c = route_class(part, lb, same, A.k);
    if (named && bucket) bucket[i] = c < A.k ? c : HONU_SEEK_NONE;
    store_key(W.packed + (uint64_t)HONU_KEY_LEN * p, u32x4{route_row_word0(c), route_row_word1(c), 0u, 0u},
              u32x4{0u, 0u, 0u, 0u});
}

// thread t: sorted row t (t < m) and class t (t <= k + 2)
__global__ __launch_bounds__(HONU_BLOCK) void k_route_emit(RouteArgs A, honu_list_row *__restrict__ rows_out,
                                                           uint32_t *__restrict__ local,
                                                           uint8_t *__restrict__ keys_out,
                                                           uint64_t *__restrict__ bucket_off,
                                                           uint64_t *__restrict__ bucket_count, RouteWork W) {
    const uint64_t t = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    const uint32_t m = A.m, k = A.k;
    if (t <= (uint64_t)k + 2) {
        const uint32_t c = (uint32_t)t;
        const uint32_t lo = route_offset(W.sorted, 0, m, c, k);  // (m == 0: no row is read)
        bucket_off[c] = lo;
        if (c < k + 2) bucket_count[c] = route_offset(W.sorted, lo, m, c + 1, k) - lo;
    }
    if (t >= m) return;
    const uint32_t g = (uint32_t)t;
    const uint32_t c = route_row_class(W.sorted + (uint64_t)HONU_KEY_LEN * g, k);
    const uint32_t p = order_index(W.order[g], m);
    const uint32_t i = A.seq ? A.seq[p] : p;
    const uint32_t record = i < m ? i : HONU_SEEK_NONE;
    const bool head = g == 0 || route_row_class(W.sorted + (uint64_t)HONU_KEY_LEN * (g - 1), k) != c;
    if (rows_out)
        *reinterpret_cast<u32x4 *>(rows_out + g) = u32x4{c, p, record, head ? (uint32_t)HONU_LIST_ROW_HEAD : 0u};
    if (local) local[g] = head ? 0u : g - route_offset(W.sorted, 0, g - 1, c, k);
    if (keys_out) {
        uint8_t *out = keys_out + (uint64_t)HONU_KEY_LEN * g;
        if (record != HONU_SEEK_NONE) copy_key(out, A.keys + (uint64_t)HONU_KEY_LEN * record);
        else store_key(out, u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u});
    }
}

hipError_t launch_key_route(const uint8_t *ids, uint64_t id_stride, const int32_t *status, uint64_t m,
                            const uint32_t *seq, const uint8_t *table, uint64_t k, const uint8_t *keys,
                            uint32_t *bucket, honu_list_row *rows, uint32_t *local, uint8_t *keys_out,
                            uint64_t *bucket_off, uint64_t *bucket_count, void *work, const ScanState &S,
                            uint64_t scan_rows, hipStream_t s) {
    const RouteArgs A = {ids, id_stride, status, seq, table, keys, (uint32_t)m, (uint32_t)k};
    RouteWork W = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (m) {
        W = route_carve(work, m);
        const unsigned blocks = (unsigned)((m + HONU_BLOCK - 1) / HONU_BLOCK);
        if (k <= ROUTE_STAGE) hipLaunchKernelGGL(k_route_find<true>, dim3(blocks), dim3(HONU_BLOCK), 0, s, A, bucket, W);
        else hipLaunchKernelGGL(k_route_find<false>, dim3(blocks), dim3(HONU_BLOCK), 0, s, A, bucket, W);
        const hipError_t e = launch_sort_keys(W.packed, nullptr, m, W.order, W.sorted, W.count, W.sort, S, scan_rows, s);
        if (e != hipSuccess) return e;
    }
    const uint64_t threads = m > k + 3 ? m : k + 3;
    hipLaunchKernelGGL(k_route_emit, dim3((unsigned)((threads + HONU_BLOCK - 1) / HONU_BLOCK)), dim3(HONU_BLOCK), 0, s,
                       A, rows, local, keys_out, bucket_off, bucket_count, W);
    return hipGetLastError();
}

}  // namespace honu
