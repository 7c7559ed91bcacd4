// list.hip — a batch of cursor walks over the sorted key column: what follows
// the Seek on every read path, Cursor.Next() / Cursor.Prev()
// (iterator/cursor.go:57-89) as Collection.List() (collection.go:32-35),
// Versions() ("from the most recent version to the oldest",
// collection.go:106-110), Retrieve() ("the latest version",
// collection.go:97-104) and the loop of store.go:379 use them. The ranges are
// honu_key_seek's rows, [pos, end) each; the rows a cursor would visit come
// out packed, the ranges in order, and every count stays on the device.
//
// Three launches, no workspace:
//   count   a thread per range: c_q = end' - pos' (plain), or the objects whose
//           latest row lies in [pos', end') by two binary searches over
//           d_obj_off[1..objects] (HONU_LIST_LATEST), capped at limit; c_q to
//           d_range_off[q], 0 to d_range_off[m];
//   scan    launch_scan in place over the m + 1 values, the total to d_total
//           (the context's scan state covers max_records rows:
//           honu_key_list refuses m + 1 above that). The extra value makes
//           d_range_off[m] come out of the scan, whether or not an expand
//           grid follows;
//   expand  a load-balanced segmented expansion, a workgroup per LIST_TILE
//           output rows (the grid is sized from cap and strides over the
//           tiles; a tile at or past min(total, cap) ends the workgroup). The
//           ranges of the tile's first and last row are two upper bounds over
//           d_range_off, a wave each (wave_bound, keycol.h). A slice of at
//           most LIST_STAGE ranges is staged in LDS, per range its 32-bit
//           offset from the tile's first row and where its walk starts (pos',
//           end', or with LATEST the object found by one binary search per
//           non-empty range, not per row), and every row searches the offsets
//           there (thread_bound); a longer slice (a run of empty ranges inside
//           one tile) is searched in global memory. A row then has its range
//           q and its index k in it: its position is
//           pos' + k, end' - 1 - k, or through d_obj_off for LATEST. The
//           16-byte row goes out in one vector store, the key as its bytes
//           (copy_key).
// The kernels have no atomics, no spin-wait and no state outside the launch;
// launch_scan is the only step in which workgroups depend on each other. Every
// position derived from a count or offset read on the device is clamped to the
// n / m / v rows: garbage in d_ranges or d_obj_off may give wrong rows, never
// an access out of bounds or a search that does not end.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t LIST_TILE = 1024;                        // output rows per workgroup
constexpr uint32_t LIST_ROUNDS = LIST_TILE / HONU_BLOCK;    // rows per thread
constexpr uint32_t LIST_STAGE = 2048;                       // range offsets a workgroup stages
// 2048 x (4 + 4) bytes, the offset and the walk's start of each range: 16 KiB, so LDS is not what bounds the
// workgroups per CU (eight would take 128 KiB of its 160 KiB; the expand kernel's 90 SGPRs admit seven, and a
// stage of 4096 would leave five). 32-bit offsets from the tile's first
// row, clamped to LIST_TILE, say all a row of the tile asks. A slice longer than the tile has rows holds empty
// ranges in between; twice the tile keeps a call with every other range empty on the staged path
static_assert(LIST_TILE % HONU_BLOCK == 0, "a thread takes whole rounds");
static_assert(HONU_WAVES_PER_BLOCK >= 2, "a wave for each end of the tile");

uint32_t list_tile() { return LIST_TILE; }
uint32_t list_stage() { return LIST_STAGE; }

struct ListRange {
    uint32_t pos, end;  // pos <= end <= v
};

// range q clamped to the valid rows; empty when the seek skipped the probe
HONU_DEV ListRange list_range(const honu_seek *__restrict__ ranges, uint32_t q, uint32_t v) {
    const uint32_t pos = ranges[q].pos, end = ranges[q].end, skipped = ranges[q].flags & HONU_SEEK_SKIPPED;
    ListRange R;
    R.end = end < v ? end : v;
    R.pos = pos < R.end ? pos : R.end;
    if (skipped) R.pos = R.end = 0;
    return R;
}

// How many of the objects [0, objects) have their end, d_obj_off[j + 1] clamped to v, at or below x: the
// object whose latest row is the first at or past x
HONU_DEV uint32_t list_objects_below(const uint64_t *__restrict__ obj_off, uint32_t objects, uint32_t v, uint32_t x) {
    return thread_bound(0, objects, [&](uint32_t mid) {
        const uint64_t e = obj_off[(uint64_t)mid + 1];
        return (e < v ? (uint32_t)e : v) <= x;
    });
}

// Where the walk of range R starts: the row pos (forward) or the row before end (REVERSE: end itself is
// kept, the k-th row is end - 1 - k). With LATEST it counts objects instead: the first object whose latest
// row is at or past pos, or one past the last whose latest row is below end
HONU_DEV uint32_t list_base(const ListRange R, uint32_t flags, const uint64_t *__restrict__ obj_off, uint32_t objs,
                            uint32_t v) {
    const uint32_t x = flags & HONU_LIST_REVERSE ? R.end : R.pos;
    return flags & HONU_LIST_LATEST ? list_objects_below(obj_off, objs, v, x) : x;
}

__global__ __launch_bounds__(HONU_BLOCK) void k_list_count(
    const uint64_t *__restrict__ valid, uint32_t n, const honu_seek *__restrict__ ranges, uint32_t m, uint32_t limit,
    uint32_t flags, const uint64_t *__restrict__ obj_off, const uint64_t *__restrict__ objects,
    uint64_t *__restrict__ range_off) {
    const uint64_t q = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (q > m) return;
    uint32_t c = 0;
    if (q < m) {
        const uint32_t v = valid_rows(valid, n);
        const ListRange R = list_range(ranges, (uint32_t)q, v);
        if (flags & HONU_LIST_LATEST) {
            // the latest rows L_j = off[j + 1] - 1 with pos <= L_j < end: pos < off[j + 1] <= end
            const uint32_t objs = valid_rows(objects, n);
            const uint32_t a = list_objects_below(obj_off, objs, v, R.pos), b = list_objects_below(obj_off, objs, v, R.end);
            c = b > a ? b - a : 0;
        } else {
            c = R.end - R.pos;
        }
        if (limit && c > limit) c = limit;
    }
    range_off[q] = c;
}

// How many of off[0, m) are at or below g, by a whole wave with one g
HONU_DEV uint32_t list_bound(const uint64_t *__restrict__ off, uint32_t m, uint64_t g) {
    return wave_bound(0, m, [&](uint32_t mid) { return off[mid] <= g; });
}

// range_off scanned (range_off[q] the rows before range q), *total_p the total
__global__ __launch_bounds__(HONU_BLOCK) void k_list_expand(
    const uint8_t *__restrict__ sorted, const uint32_t *__restrict__ order, const uint64_t *__restrict__ valid,
    uint32_t n, const honu_seek *__restrict__ ranges, uint32_t m, uint32_t flags,
    const uint64_t *__restrict__ obj_off, const uint64_t *__restrict__ objects,
    const honu_record_info *__restrict__ info, const uint64_t *__restrict__ range_off,
    honu_list_row *__restrict__ rows, uint8_t *__restrict__ keys_out, uint32_t cap,
    const uint64_t *__restrict__ total_p) {
    __shared__ uint32_t rel[LIST_STAGE];   // the slice's offsets less the tile's first row, within [0, LIST_TILE]
    __shared__ uint32_t base[LIST_STAGE];  // where each of the slice's walks starts (list_base)
    __shared__ uint32_t ends[2];
    const uint32_t v = valid_rows(valid, n);
    const uint64_t total = *total_p;
    const uint32_t w = (uint32_t)(total < cap ? total : cap);  // rows written
    const uint32_t objs = flags & HONU_LIST_LATEST ? valid_rows(objects, n) : 0;
    const uint32_t wv = wave_in_block(), lane = lane_id();
    for (uint64_t tile = blockIdx.x; tile * LIST_TILE < w; tile += gridDim.x) {  // (block-uniform; n, m >= 1 here)
        const uint32_t g0 = (uint32_t)(tile * LIST_TILE);
        const uint32_t len = w - g0 < LIST_TILE ? w - g0 : LIST_TILE;
        // the ranges [q0, q1] of the tile's first and last row: the last range that starts at or before the row
        if (threadIdx.x < 2 * HONU_WAVE) {
            const uint32_t b = list_bound(range_off, m, wv ? g0 + len - 1 : g0);
            if (lane == 0) ends[wv] = b ? b - 1 : 0;  // < m
        }
        __syncthreads();
        const uint32_t q0 = ends[0];
        const uint32_t q1 = ends[1] < q0 ? q0 : ends[1];  // (q0 <= q1 over scanned offsets)
        const uint32_t qn = q1 - q0 + 1;
        const bool staged = qn <= LIST_STAGE;
        const uint64_t before0 = range_off[q0];  // at or below g0 over scanned offsets
        if (staged) {  // (block-uniform) an empty range of the slice takes no row: its walk's start is not looked up
            for (uint32_t i = threadIdx.x; i < qn; i += HONU_BLOCK) {
                const uint64_t o = range_off[q0 + i], next = range_off[q0 + i + 1];  // (q0 + i + 1 <= m)
                rel[i] = o > g0 ? (o - g0 < LIST_TILE ? (uint32_t)(o - g0) : LIST_TILE) : 0;
                base[i] = next > o ? list_base(list_range(ranges, q0 + i, v), flags, obj_off, objs, v) : 0;
            }
        }
        __syncthreads();
        for (uint32_t r = 0; r < LIST_ROUNDS; r++) {
            const uint32_t t = r * HONU_BLOCK + threadIdx.x;
            if (t >= len) break;
            const uint32_t g = g0 + t;
            // the last i in [0, qn) with offset <= g (entry 0 is: the tile's first row lies in range q0)
            const uint32_t a = thread_bound(
                1, qn, [&](uint32_t mid) { return staged ? rel[mid] <= t : range_off[q0 + mid] <= g; });
            const uint32_t i = a - 1, q = q0 + i;  // q < m
            // the row's index in its range (rel[i] is exact for i > 0: q0 is the last range that starts at or before g0)
            const uint64_t before = i == 0 ? before0 : (staged ? (uint64_t)g0 + rel[i] : range_off[q]);
            const uint32_t k = before < g ? g - (uint32_t)before : 0;
            const uint32_t from = staged ? base[i] : list_base(list_range(ranges, q, v), flags, obj_off, objs, v);
            uint64_t p = flags & HONU_LIST_REVERSE ? (from > k ? from - 1 - k : 0) : (uint64_t)from + k;
            if (flags & HONU_LIST_LATEST) {  // p counts objects: the object's last row
                const uint64_t j = p < objs ? p : (objs ? objs - 1 : 0);
                const uint64_t e = obj_off[j + 1];  // (j + 1 <= n: d_obj_off has n + 1 values)
                p = e < v ? e : v;
                p = p ? p - 1 : 0;
            }
            p = p < n ? p : n - 1;
            u32x4 row;
            row[0] = q;
            row[1] = (uint32_t)p;
            row[2] = HONU_SEEK_NONE;
            row[3] = k == 0 ? (uint32_t)HONU_LIST_ROW_HEAD : 0u;
            if (order) {
                const uint32_t rec = order[p];
                row[2] = rec;
                if (info && info[order_index(rec, n)].tombstone) row[3] |= HONU_LIST_ROW_TOMBSTONE;
            }
            *reinterpret_cast<u32x4 *>(rows + g) = row;
            if (keys_out) copy_key(keys_out + (uint64_t)HONU_KEY_LEN * g, sorted + (uint64_t)HONU_KEY_LEN * p);
        }
        __syncthreads();  // rel and ends are rewritten by the next tile
    }
}

hipError_t launch_key_list(int num_cu, const uint8_t *sorted, const uint32_t *order, const uint64_t *valid, uint64_t n,
                           const honu_seek *ranges, uint64_t m, uint32_t limit, uint32_t flags,
                           const uint64_t *obj_off, const uint64_t *objects, const honu_record_info *info,
                           uint64_t *range_off, honu_list_row *rows, uint8_t *keys_out, uint64_t cap,
                           uint64_t *total, const ScanState &S, hipStream_t s) {
    const uint64_t cb = (m + 1 + HONU_BLOCK - 1) / HONU_BLOCK;
    hipLaunchKernelGGL(k_list_count, dim3((unsigned)cb), dim3(HONU_BLOCK), 0, s, valid, (uint32_t)n, ranges,
                       (uint32_t)m, limit, flags, obj_off, objects, range_off);
    const hipError_t e = launch_scan(range_off, m + 1, 1, range_off, total, S, s);  // (m + 1 <= the state's rows: the caller)
    if (e != hipSuccess) return e;
    if (cap == 0 || n == 0 || m == 0) return hipGetLastError();  // (no row can be written: every count is 0)
    // from cap alone, never from a count on the device; eight workgroups per CU stride over the tiles beyond that
    const uint64_t tiles = (cap + LIST_TILE - 1) / LIST_TILE;
    const uint64_t resident = 8ull * (uint64_t)(num_cu > 0 ? num_cu : 1);
    hipLaunchKernelGGL(k_list_expand, dim3((unsigned)(tiles < resident ? tiles : resident)), dim3(HONU_BLOCK), 0, s,
                       sorted, order, valid, (uint32_t)n, ranges, (uint32_t)m, flags, obj_off, objects, info, range_off,
                       rows, keys_out, (uint32_t)cap, total);
    return hipGetLastError();
}

}  // namespace honu
