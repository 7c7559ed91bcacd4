// filter.hip — the live-object filter over listed rows: "an object with a
// tombstone version will not be returned in list queries or retrieval"
// (collection.go:132-134), Retrieve of it "not found" (collection.go:97-101,
// 53-54). A stable stream compaction of honu_key_list's rows: the rows that
// stay, in list order, with the ranges' offsets and HEAD flags recomputed, so
// the result is a list again (honu_key_fetch and the decoders take it as it
// is).
//
// Four launches, a workgroup per FILTER_TILE rows of the list (the grid from
// cap, never from a count on the device), on compact.h's mark / scan / place
// with a launch for the offsets between:
//   mark     a thread loads its 16-byte row once and decides it. A row at or
//            past w = min(total, cap) is no row. HONU_FILTER_TOMBSTONE: the row
//            goes when its flags carry HONU_LIST_ROW_TOMBSTONE.
//            HONU_FILTER_DELETED: the row's object j is an upper bound of pos
//            over d_obj_off[1..objects] (thread_bound, every offset clamped to
//            v, as the list's LATEST mode reads them); the row goes when the
//            info row of d_latest[j] is a tombstone;
//   scan     launch_scan over the tiles' kept counts, the total to
//            d_total_out (the context's scan state covers max_records rows:
//            honu_key_filter refuses a cap of more tiles than that);
//   offsets  a thread per range offset: the kept rows below min(off, w), the
//            row's rank out of global memory (compact_rank_row); entry m is
//            the total;
//   place    a kept row goes to its rank as one 16-byte load and store, its
//            key as its bytes (copy_key). HEAD is set when the row lands on
//            its range's new offset, which the launch before wrote.
// The offsets are a launch of their own so that place reads HEAD's answer, one
// 8-byte load per kept row, in place of a rank of its range's first row out of
// another tile's masks. launch_scan is the only step in which workgroups
// depend on each other. Every index derived from device data is clamped to
// the cap / m / n / v rows.
#include "compact.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t FILTER_TILE = 1024;  // list rows per workgroup

uint32_t filter_tile() { return FILTER_TILE; }
uint64_t filter_tiles(uint64_t cap) { return compact_tiles<FILTER_TILE>(cap); }
uint64_t filter_workspace_bytes(uint64_t cap) { return compact_workspace_bytes<FILTER_TILE>(cap); }

// the column and its objects as HONU_FILTER_DELETED reads them (all null without the flag)
struct FilterColumn {
    const uint64_t *valid;
    uint32_t n;
    const uint64_t *obj_off;
    const uint32_t *latest;
    const uint64_t *objects;
    const honu_record_info *info;
};

// the rows of the list that take part: min(total, cap)
HONU_DEV uint32_t filter_rows(const uint64_t *total, uint32_t cap) { return valid_rows(total, cap); }

__global__ __launch_bounds__(HONU_BLOCK) void k_filter_mark(
    const honu_list_row *__restrict__ rows, const uint64_t *__restrict__ total, uint32_t cap, uint32_t flags,
    FilterColumn C, CompactWork W) {
    const uint32_t w = filter_rows(total, cap);
    const uint32_t g0 = blockIdx.x * FILTER_TILE;  // below cap
    const uint32_t len = g0 < w ? (w - g0 < FILTER_TILE ? w - g0 : FILTER_TILE) : 0;  // the tile's rows: its first len
    uint32_t v = 0, objs = 0;
    if (flags & HONU_FILTER_DELETED) {
        v = valid_rows(C.valid, C.n);
        objs = valid_rows(C.objects, C.n);
    }
    compact_mark<FILTER_TILE>(W, blockIdx.x, [&](uint32_t, uint32_t t) {
        bool keep = t < len;
        if (keep && flags) {
            const u32x4 row = *reinterpret_cast<const u32x4 *>(rows + g0 + t);
            bool drop = (flags & HONU_FILTER_TOMBSTONE) && (row[3] & HONU_LIST_ROW_TOMBSTONE);
            const uint32_t pos = row[1];
            if ((flags & HONU_FILTER_DELETED) && pos < v && objs) {  // (v, objs <= n: n >= 1 here)
                // the objects whose end is at or below pos: the object that holds pos, the last one at most
                uint32_t o = thread_bound(0, objs, [&](uint32_t mid) {
                    const uint64_t e = C.obj_off[(uint64_t)mid + 1];
                    return (e < v ? (uint32_t)e : v) <= pos;
                });
                o = o < objs ? o : objs - 1;
                drop = drop || C.info[order_index(C.latest[o], C.n)].tombstone != 0;
            }
            keep = !drop;
        }
        return keep;
    });
}

// W.kept scanned (the rows kept before the tile), *kept_total the total: range_off_out[q] the kept rows
// below min(range_off[q], w), range_off_out[m] the total
__global__ __launch_bounds__(HONU_BLOCK) void k_filter_offsets(
    const uint64_t *__restrict__ range_off, uint32_t m, const uint64_t *__restrict__ total, uint32_t cap,
    const uint64_t *__restrict__ kept_total, uint64_t *__restrict__ range_off_out, CompactWork W) {
    const uint64_t q = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (q > m) return;
    const uint32_t w = filter_rows(total, cap);
    uint64_t k = filter_rows(kept_total, w);
    const uint64_t off = q < m ? range_off[q] : w;
    if (off < w) {  // a row of the list: its tile is one of the cap's
        const uint32_t x = (uint32_t)off, tile = x / FILTER_TILE;
        const uint64_t *msk = W.mask + (uint64_t)tile * CompactTile<FILTER_TILE>::WORDS;
        k = compact_at_most(compact_rank_row(W.kept[tile], msk, x % FILTER_TILE), k);
    }
    range_off_out[q] = k;
}

// range_off_out as k_filter_offsets wrote it
__global__ __launch_bounds__(HONU_BLOCK) void k_filter_place(
    const honu_list_row *__restrict__ rows, const uint8_t *__restrict__ keys, const uint64_t *__restrict__ total,
    uint32_t cap, uint32_t m, const uint64_t *__restrict__ range_off_out, honu_list_row *__restrict__ rows_out,
    uint8_t *__restrict__ keys_out, CompactWork W) {
    const uint32_t w = filter_rows(total, cap);
    const uint32_t g0 = blockIdx.x * FILTER_TILE;  // below cap
    if (g0 >= w) return;  // (block-uniform)
    const CompactRanks K = compact_ranks<FILTER_TILE>(W, blockIdx.x);
    const uint32_t wv = wave_in_block(), lane = lane_id();
    for (uint32_t r = 0; r < CompactTile<FILTER_TILE>::ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;
        const uint32_t g = g0 + j * HONU_WAVE + lane;
        if (g >= w || !K.kept_bit(j, lane)) continue;
        const uint64_t dst = compact_at_most(K.kept_before(j, lane), g);  // a kept row never moves up
        u32x4 row = *reinterpret_cast<const u32x4 *>(rows + g);
        const uint32_t q = row[0] < m ? row[0] : m - 1;  // (m == 0: no range, no HEAD)
        const bool head = m && range_off_out[q] == dst;
        row[3] = (row[3] & ~(uint32_t)HONU_LIST_ROW_HEAD) | (head ? (uint32_t)HONU_LIST_ROW_HEAD : 0u);
        *reinterpret_cast<u32x4 *>(rows_out + dst) = row;
        if (keys_out) copy_key(keys_out + (uint64_t)HONU_KEY_LEN * dst, keys + (uint64_t)HONU_KEY_LEN * g);
    }
}

hipError_t launch_key_filter(const honu_list_row *rows, const uint8_t *keys, const uint64_t *range_off, uint64_t m,
                             const uint64_t *total, uint64_t cap, uint32_t flags, const uint64_t *valid, uint64_t n,
                             const uint64_t *obj_off, const uint32_t *latest, const uint64_t *objects,
                             const honu_record_info *info, honu_list_row *rows_out, uint8_t *keys_out,
                             uint64_t *range_off_out, uint64_t *total_out, void *work, const ScanState &S,
                             hipStream_t s) {
    if (cap == 0) {  // no row takes part: every offset and the total are 0
        hipError_t e = hipMemsetAsync(total_out, 0, sizeof(uint64_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(range_off_out, 0, sizeof(uint64_t) * (m + 1), s);
        return e;
    }
    if (n == 0) flags &= ~(uint32_t)HONU_FILTER_DELETED;  // (no row of the column: no pos names an object)
    const bool del = flags & HONU_FILTER_DELETED;
    const FilterColumn C = {del ? valid : nullptr,  (uint32_t)n,           del ? obj_off : nullptr,
                            del ? latest : nullptr, del ? objects : nullptr, del ? info : nullptr};
    const CompactWork W = compact_carve<FILTER_TILE>(work, cap);
    const uint64_t tiles = filter_tiles(cap);
    hipLaunchKernelGGL(k_filter_mark, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, rows, total, (uint32_t)cap, flags,
                       C, W);
    const hipError_t e = launch_scan(W.kept, tiles, 1, W.kept, total_out, S, s);  // (tiles <= the state's rows: the caller)
    if (e != hipSuccess) return e;
    const uint64_t ob = (m + 1 + HONU_BLOCK - 1) / HONU_BLOCK;
    hipLaunchKernelGGL(k_filter_offsets, dim3((unsigned)ob), dim3(HONU_BLOCK), 0, s, range_off, (uint32_t)m, total,
                       (uint32_t)cap, total_out, range_off_out, W);
    hipLaunchKernelGGL(k_filter_place, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, rows,
                       keys_out ? keys : nullptr, total, (uint32_t)cap, (uint32_t)m, range_off_out, rows_out, keys_out,
                       W);
    return hipGetLastError();
}

}  // namespace honu
