// filter.hip — the live-object filter over listed rows: "an object with a
// tombstone version will not be returned in list queries or retrieval"
// (collection.go:132-134), Retrieve of it "not found" (collection.go:97-101,
// 53-54). A stable stream compaction of honu_key_list's rows: the rows that
// stay, in list order, with the ranges' offsets and HEAD flags recomputed, so
// the result is a list again (honu_key_fetch and the decoders take it as it
// is). delete.hip's shape over list rows instead of column rows.
//
// Four launches, a workgroup per FILTER_TILE rows of the list (the grid from
// cap, never from a count on the device):
//   mark     a thread loads its 16-byte row once and decides it. A row at or
//            past w = min(total, cap) is no row. HONU_FILTER_TOMBSTONE: the row
//            goes when its flags carry HONU_LIST_ROW_TOMBSTONE.
//            HONU_FILTER_DELETED: the row's object j is an upper bound of pos
//            over d_obj_off[1..objects] (thread_bound, every offset clamped to
//            v, as the list's LATEST mode reads them); the row goes when the
//            info row of d_latest[j] is a tombstone. The tile writes its keep
//            mask, one ballot per 64 rows, and its kept count;
//   scan     launch_scan over the tiles' kept counts, the total to
//            d_total_out (the context's scan state covers max_records rows:
//            honu_key_filter refuses a cap of more tiles than that);
//   offsets  a thread per range offset: the kept rows below min(off, w) are
//            the tile's scanned count plus a popcount of its masks below the
//            row; entry m is the total;
//   place    a kept row's rank in its tile is a popcount of the mask below it:
//            it goes to kept_before_tile + rank as one 16-byte load and store,
//            its key as its bytes (copy_key). HEAD is set when the row lands
//            on its range's new offset, which the launch before wrote.
// The offsets are a launch of their own so that place reads HEAD's answer, one
// 8-byte load per kept row, in place of a rank of its range's first row out of
// another tile's masks. The new kernels have no atomics, no spin-wait and no
// state outside the launch; launch_scan is the only step in which workgroups
// depend on each other. Every index derived from device data is clamped to
// the cap / m / n / v rows.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t FILTER_TILE = 1024;                                   // list rows per workgroup
constexpr uint32_t FILTER_WORDS = FILTER_TILE / HONU_WAVE;               // ballots per tile
constexpr uint32_t FILTER_ROUNDS = FILTER_WORDS / HONU_WAVES_PER_BLOCK;  // ballots per wave
static_assert(FILTER_TILE % (HONU_WAVE * HONU_WAVES_PER_BLOCK) == 0, "a wave takes whole ballots");
static_assert(FILTER_WORDS <= HONU_BLOCK, "a thread per ballot in the place kernel");

uint32_t filter_tile() { return FILTER_TILE; }
uint64_t filter_tiles(uint64_t cap) { return (cap + FILTER_TILE - 1) / FILTER_TILE; }

// the keep masks (FILTER_WORDS words per tile), then the kept counts (a word per tile)
uint64_t filter_workspace_bytes(uint64_t cap) {
    const uint64_t tiles = filter_tiles(cap);
    return up256(8 * FILTER_WORDS * tiles) + up256(8 * tiles);
}

struct FilterWork {
    uint64_t *mask;
    uint64_t *kept;
};

static FilterWork filter_carve(void *work, uint64_t cap) {
    FilterWork w;
    w.mask = (uint64_t *)work;
    w.kept = (uint64_t *)((uint8_t *)work + up256(8 * FILTER_WORDS * filter_tiles(cap)));
    return w;
}

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
    FilterColumn C, FilterWork W) {
    __shared__ uint32_t cnt[HONU_WAVES_PER_BLOCK];
    const uint32_t w = filter_rows(total, cap);
    const uint32_t g0 = blockIdx.x * FILTER_TILE;  // below cap
    const uint32_t len = g0 < w ? (w - g0 < FILTER_TILE ? w - g0 : FILTER_TILE) : 0;  // the tile's rows: its first len
    const uint32_t wv = wave_in_block(), lane = lane_id();
    uint32_t v = 0, objs = 0;
    if (flags & HONU_FILTER_DELETED) {
        v = valid_rows(C.valid, C.n);
        objs = valid_rows(C.objects, C.n);
    }
    uint32_t kept = 0;
    for (uint32_t r = 0; r < FILTER_ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;  // the tile's ballot: rows [64 j, 64 j + 64)
        const uint32_t t = j * HONU_WAVE + lane;
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
        const uint64_t bits = __ballot(keep);
        if (lane == 0) W.mask[(uint64_t)blockIdx.x * FILTER_WORDS + j] = bits;
        kept += (uint32_t)__popcll(bits);
    }
    if (lane == 0) cnt[wv] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < HONU_WAVES_PER_BLOCK; i++) sum += cnt[i];
        W.kept[blockIdx.x] = sum;
    }
}

// W.kept scanned (the rows kept before the tile), *kept_total the total: range_off_out[q] the kept rows
// below min(range_off[q], w), range_off_out[m] the total
__global__ __launch_bounds__(HONU_BLOCK) void k_filter_offsets(
    const uint64_t *__restrict__ range_off, uint32_t m, const uint64_t *__restrict__ total, uint32_t cap,
    const uint64_t *__restrict__ kept_total, uint64_t *__restrict__ range_off_out, FilterWork W) {
    const uint64_t q = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (q > m) return;
    const uint32_t w = filter_rows(total, cap);
    uint64_t k = filter_rows(kept_total, w);
    const uint64_t off = q < m ? range_off[q] : w;
    if (off < w) {  // a row of the list: its tile is one of the cap's
        const uint32_t x = (uint32_t)off, tile = x / FILTER_TILE, j = (x % FILTER_TILE) / HONU_WAVE, b = x % HONU_WAVE;
        const uint64_t *msk = W.mask + (uint64_t)tile * FILTER_WORDS;
        uint64_t s = W.kept[tile];
        for (uint32_t i = 0; i < j; i++) s += (uint32_t)__popcll(msk[i]);
        s += (uint32_t)__popcll(msk[j] & (b ? (~0ull >> (64 - b)) : 0));
        k = s < k ? s : k;
    }
    range_off_out[q] = k;
}

// range_off_out as k_filter_offsets wrote it
__global__ __launch_bounds__(HONU_BLOCK) void k_filter_place(
    const honu_list_row *__restrict__ rows, const uint8_t *__restrict__ keys, const uint64_t *__restrict__ total,
    uint32_t cap, uint32_t m, const uint64_t *__restrict__ range_off_out, honu_list_row *__restrict__ rows_out,
    uint8_t *__restrict__ keys_out, FilterWork W) {
    __shared__ uint64_t msk[FILTER_WORDS];
    __shared__ uint32_t pre[FILTER_WORDS];  // rows kept in the tile's ballots before ballot j
    const uint32_t w = filter_rows(total, cap);
    const uint32_t g0 = blockIdx.x * FILTER_TILE;  // below cap
    if (g0 >= w) return;  // (block-uniform)
    if (threadIdx.x < FILTER_WORDS) msk[threadIdx.x] = W.mask[(uint64_t)blockIdx.x * FILTER_WORDS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < FILTER_WORDS) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < threadIdx.x; j++) s += (uint32_t)__popcll(msk[j]);
        pre[threadIdx.x] = s;
    }
    __syncthreads();
    const uint64_t base = W.kept[blockIdx.x];
    const uint32_t wv = wave_in_block(), lane = lane_id();
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0;
    for (uint32_t r = 0; r < FILTER_ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;
        const uint32_t g = g0 + j * HONU_WAVE + lane;
        if (g >= w || !((msk[j] >> lane) & 1ull)) continue;
        uint64_t dst = base + pre[j] + (uint32_t)__popcll(msk[j] & below);
        dst = dst < g ? dst : g;  // (a mask or a count that is not the mark's: inside the rows all the same)
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
    const FilterWork W = filter_carve(work, cap);
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
