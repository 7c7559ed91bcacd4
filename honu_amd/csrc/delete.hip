// delete.hip — a batch of Deletes from the sorted key column: the loop "Delete
// all collection versions" of Store.Drop (store.go:378-383: Seek(id), then
// collections.Delete(key) while bytes.HasPrefix(key, id)), the DeleteBucket
// behind it (store.go:399-404), and the rows a Put of a stored key supersedes
// (bbolt replaces the value; honu_key_merge keeps the run). A stable stream
// compaction: the rows that stay in column order, then the rows that go in
// column order, then the invalid tail as it stands.
//
// Three launches, a workgroup per DELETE_TILE positions of the column, on
// compact.h's mark / scan / place:
//   mark   a row goes when its probe_len-byte prefix is in the delete list, or
//          (HONU_DELETE_SUPERSEDED) when the next valid row has its 29 bytes.
//          The delete rows that can match any row of the tile are one range
//          of the list (keycol.h's peer_range), staged masked in LDS when it
//          has no more than DELETE_STAGE rows; a longer one is searched in
//          global memory. A row's lower bound in the range (thread_bound)
//          decides it. The successor comes from the next lane, for lane 63
//          from memory (it may be the next tile's);
//   scan   launch_scan over the tiles' kept counts, the total to d_valid_out
//          (the context's scan state covers max_records rows: honu_key_delete
//          refuses a column of more tiles than that);
//   place  a kept row goes to its rank, a removed row p to
//          kept + (p - kept_before_p), a tail row stays. Rows move as their
//          bytes (copy_key).
// launch_scan is the only step in which workgroups depend on each other.
// Every position derived from a count on the device is clamped to the n / m
// rows.
#include "compact.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t DELETE_TILE = 1024;   // column positions per workgroup
constexpr uint32_t DELETE_STAGE = 1024;  // delete rows a workgroup stages
// 1024 x 36 bytes: 36 KiB, four workgroups per CU (measured against 2048 rows, two workgroups per CU,
// and against no stage at all: DESIGN §6.4)

uint32_t delete_tile() { return DELETE_TILE; }
uint64_t delete_tiles(uint64_t n) { return compact_tiles<DELETE_TILE>(n); }
uint64_t delete_workspace_bytes(uint64_t n) { return compact_workspace_bytes<DELETE_TILE>(n); }

HONU_DEV void delete_load(const uint8_t *col, uint32_t i, const SeekMask &M, uint32_t w[SORT_KEY_WORDS]) {
    load_masked(col + (uint64_t)HONU_KEY_LEN * i, M, w);
}

__global__ __launch_bounds__(HONU_BLOCK) void k_delete_mark(
    const uint8_t *__restrict__ sorted, const uint64_t *__restrict__ valid, uint32_t n,
    const uint8_t *__restrict__ del, const uint64_t *__restrict__ valid_del, uint32_t m, SeekMask M,
    uint32_t flags, CompactWork W) {
    __shared__ uint32_t rows[DELETE_STAGE * KEY_ROW_WORDS];
    const uint32_t v = valid_rows(valid, n), vd = m ? valid_rows(valid_del, m) : 0;
    const uint32_t p0 = blockIdx.x * DELETE_TILE;  // below n
    const uint32_t len = n - p0 < DELETE_TILE ? n - p0 : DELETE_TILE;
    const uint32_t vlen = p0 < v ? (v - p0 < len ? v - p0 : len) : 0;  // the tile's valid rows: its first vlen
    const uint32_t lane = lane_id();

    // the delete rows that a row of the tile can match, staged as their masked keys
    const auto R = peer_range(
        [&](bool last, uint32_t k[SORT_KEY_WORDS]) { delete_load(sorted, last ? p0 + vlen - 1 : p0, M, k); }, del,
        vlen ? vd : 0, M, [&](uint32_t at, uint32_t d[SORT_KEY_WORDS]) { delete_load(del, at, M, d); }, DELETE_STAGE,
        rows);

    compact_mark<DELETE_TILE>(W, blockIdx.x, [&](uint32_t j, uint32_t t) {
        bool keep = false;
        if (j * HONU_WAVE < vlen) {  // (wave-uniform) the ballot has a valid row
            const bool in = t < vlen;
            uint32_t w[SORT_KEY_WORDS];
#pragma unroll
            for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] = 0;
            if (in) pack_key(sorted + (uint64_t)HONU_KEY_LEN * (p0 + t), true, w);
            bool drop = false;
            if (in && R.dn) {
                uint32_t k[SORT_KEY_WORDS], d[SORT_KEY_WORDS];
#pragma unroll
                for (int i = 0; i < SORT_KEY_WORDS; i++) k[i] = w[i] & M.w[i];
                const uint32_t a = thread_bound(0, R.dn, [&](uint32_t mid) {  // the lower bound of k in the range
                    R.load(mid, d);
                    return packed_before(d, k, false);
                });
                if (a < R.dn) {
                    R.load(a, d);
                    drop = packed_same(d, k);
                }
            }
            if (flags & HONU_DELETE_SUPERSEDED) {
                // row p + 1: the next lane's, for lane 63 read from memory (the next ballot's or the next tile's)
                uint32_t nx[SORT_KEY_WORDS];
#pragma unroll
                for (int i = 0; i < SORT_KEY_WORDS; i++) nx[i] = (uint32_t)__shfl_down((int)w[i], 1, HONU_WAVE);
                const bool has_next = in && v - p0 - t > 1;  // p + 1 < v
                if (lane == HONU_WAVE - 1 && has_next)
                    pack_key(sorted + (uint64_t)HONU_KEY_LEN * (p0 + t + 1), true, nx);
                drop = drop || (has_next && packed_same(w, nx));
            }
            keep = in && !drop;
        }
        return keep;
    });
}

// W.kept scanned (the rows kept before the tile), *kept_total the total
__global__ __launch_bounds__(HONU_BLOCK) void k_delete_place(
    const uint8_t *__restrict__ sorted, const uint32_t *__restrict__ order, const uint64_t *__restrict__ valid,
    uint32_t n, uint8_t *__restrict__ out, uint32_t *__restrict__ order_out,
    const uint64_t *__restrict__ kept_total, uint64_t *__restrict__ removed, CompactWork W) {
    const uint32_t v = valid_rows(valid, n);
    const uint64_t kept = *kept_total < v ? *kept_total : v;
    if (blockIdx.x == 0 && threadIdx.x == 0 && removed) *removed = v - kept;
    const uint32_t p0 = blockIdx.x * DELETE_TILE;  // below n
    const uint32_t len = n - p0 < DELETE_TILE ? n - p0 : DELETE_TILE;
    const CompactRanks K = compact_ranks<DELETE_TILE>(W, blockIdx.x);
    const uint32_t wv = wave_in_block(), lane = lane_id();
    for (uint32_t r = 0; r < CompactTile<DELETE_TILE>::ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;
        const uint32_t t = j * HONU_WAVE + lane;
        if (t >= len) continue;
        const uint32_t p = p0 + t;
        uint64_t dst = p;  // a row of the invalid tail stays
        if (p < v) {
            const uint64_t kept_before = K.kept_before(j, lane);
            dst = K.kept_bit(j, lane) ? kept_before : compact_removed_dst(kept, p, kept_before);
            dst = compact_dst_or_stay(dst, v, p);
        }
        copy_key(out + (uint64_t)HONU_KEY_LEN * dst, sorted + (uint64_t)HONU_KEY_LEN * p);
        if (order_out) order_out[dst] = order[p];
    }
}

hipError_t launch_key_delete(const uint8_t *sorted, const uint32_t *order, const uint64_t *valid, uint64_t n,
                             const uint8_t *del, const uint64_t *valid_del, uint64_t m, uint32_t probe_len,
                             uint32_t flags, uint8_t *out, uint32_t *order_out, uint64_t *valid_out,
                             uint64_t *removed, void *work, const ScanState &S, hipStream_t s) {
    if (n == 0) {
        hipError_t e = hipMemsetAsync(valid_out, 0, sizeof(uint64_t), s);
        if (e == hipSuccess && removed) e = hipMemsetAsync(removed, 0, sizeof(uint64_t), s);
        return e;
    }
    const CompactWork W = compact_carve<DELETE_TILE>(work, n);
    const uint64_t tiles = delete_tiles(n);
    hipLaunchKernelGGL(k_delete_mark, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, sorted, valid, (uint32_t)n, del,
                       valid_del, (uint32_t)m, seek_mask(probe_len), flags, W);
    const hipError_t e = launch_scan(W.kept, tiles, 1, W.kept, valid_out, S, s);  // (tiles <= the state's rows: the caller)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_delete_place, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, sorted,
                       order_out ? order : nullptr, valid, (uint32_t)n, out, order_out, valid_out, removed, W);
    return hipGetLastError();
}

}  // namespace honu
