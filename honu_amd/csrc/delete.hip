// delete.hip — a batch of Deletes from the sorted key column: the loop "Delete
// all collection versions" of Store.Drop (store.go:378-383: Seek(id), then
// collections.Delete(key) while bytes.HasPrefix(key, id)), the DeleteBucket
// behind it (store.go:399-404), and the rows a Put of a stored key supersedes
// (bbolt replaces the value; honu_key_merge keeps the run). A stable stream
// compaction: the rows that stay in column order, then the rows that go in
// column order, then the invalid tail as it stands.
//
// Three launches, a workgroup per DELETE_TILE positions of the column:
//   mark   a row goes when its probe_len-byte prefix is in the delete list, or
//          (HONU_DELETE_SUPERSEDED) when the next valid row has its 29 bytes.
//          The tile's rows are a contiguous key range, so the delete rows that
//          can match any of them are one range of the list: its two ends are
//          found once per workgroup, a wave each (wave_bound), and the
//          range is staged packed and masked in LDS (keycol.h's 9-word row)
//          when it has no more than DELETE_STAGE rows; a longer one is
//          searched in global memory. A row's lower bound in the range
//          (thread_bound) decides it. The successor comes from the next
//          lane, for lane 63 from memory (it may be the next tile's). The
//          tile writes its keep mask, one ballot per 64 rows, and its kept
//          count;
//   scan   launch_scan over the tiles' kept counts, the total to d_valid_out
//          (the context's scan state covers max_records rows: honu_key_delete
//          refuses a column of more tiles than that);
//   place  a row's rank in its tile is a popcount of the mask below it; a
//          kept row goes to kept_before_tile + rank, a removed row p to
//          kept + (p - kept_before_p), a tail row stays. Rows move as their
//          bytes (copy_key).
// The new kernels have no atomics, no spin-wait and no state outside the
// launch; launch_scan is the only step in which workgroups depend on each
// other. Every position derived from a count on the device is clamped to the
// n / m rows.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t DELETE_TILE = 1024;                                   // column positions per workgroup
constexpr uint32_t DELETE_WORDS = DELETE_TILE / HONU_WAVE;               // ballots per tile
constexpr uint32_t DELETE_ROUNDS = DELETE_WORDS / HONU_WAVES_PER_BLOCK;  // ballots per wave
constexpr uint32_t DELETE_STAGE = 1024;                                  // delete rows a workgroup stages
// 1024 x 36 bytes: 36 KiB, four workgroups per CU (measured against 2048 rows, two workgroups per CU,
// and against no stage at all: DESIGN §6.4)
static_assert(DELETE_TILE % (HONU_WAVE * HONU_WAVES_PER_BLOCK) == 0, "a wave takes whole ballots");
static_assert(DELETE_WORDS <= HONU_BLOCK, "a thread per ballot in the place kernel");

uint32_t delete_tile() { return DELETE_TILE; }
uint64_t delete_tiles(uint64_t n) { return (n + DELETE_TILE - 1) / DELETE_TILE; }

// the keep masks (DELETE_WORDS words per tile), then the kept counts (a word per tile)
uint64_t delete_workspace_bytes(uint64_t n) {
    const uint64_t tiles = delete_tiles(n);
    return up256(8 * DELETE_WORDS * tiles) + up256(8 * tiles);
}

struct DeleteWork {
    uint64_t *mask;
    uint64_t *kept;
};

static DeleteWork delete_carve(void *work, uint64_t n) {
    DeleteWork w;
    w.mask = (uint64_t *)work;
    w.kept = (uint64_t *)((uint8_t *)work + up256(8 * DELETE_WORDS * delete_tiles(n)));
    return w;
}

HONU_DEV void delete_load(const uint8_t *col, uint32_t i, const SeekMask &M, uint32_t w[SORT_KEY_WORDS]) {
    load_masked(col + (uint64_t)HONU_KEY_LEN * i, M, w);
}

// How many of the delete rows [0, vd) are below k (upper: below or equal) over
// the masked prefixes: the lower (upper) bound of k in the list, by a whole
// wave with one k
HONU_DEV uint32_t delete_bound(const uint8_t *__restrict__ del, uint32_t vd, const SeekMask &M,
                               const uint32_t k[SORT_KEY_WORDS], bool upper) {
    return wave_bound(0, vd, [&](uint32_t mid) {
        uint32_t d[SORT_KEY_WORDS];
        delete_load(del, mid, M, d);
        return packed_before(d, k, upper);
    });
}

__global__ __launch_bounds__(HONU_BLOCK) void k_delete_mark(
    const uint8_t *__restrict__ sorted, const uint64_t *__restrict__ valid, uint32_t n,
    const uint8_t *__restrict__ del, const uint64_t *__restrict__ valid_del, uint32_t m, SeekMask M,
    uint32_t flags, DeleteWork W) {
    __shared__ uint32_t rows[DELETE_STAGE * KEY_ROW_WORDS];
    __shared__ uint32_t range[2];
    __shared__ uint32_t cnt[HONU_WAVES_PER_BLOCK];
    const uint32_t v = valid_rows(valid, n), vd = m ? valid_rows(valid_del, m) : 0;
    const uint32_t p0 = blockIdx.x * DELETE_TILE;  // below n
    const uint32_t len = n - p0 < DELETE_TILE ? n - p0 : DELETE_TILE;
    const uint32_t vlen = p0 < v ? (v - p0 < len ? v - p0 : len) : 0;  // the tile's valid rows: its first vlen
    const uint32_t wv = wave_in_block(), lane = lane_id();

    // the delete rows [lo, hi) that a row of the tile can match
    uint32_t lo = 0, hi = 0;
    if (vlen && vd) {  // (block-uniform)
        if (threadIdx.x < 2 * HONU_WAVE) {
            uint32_t k[SORT_KEY_WORDS];
            delete_load(sorted, wv ? p0 + vlen - 1 : p0, M, k);
            const uint32_t b = delete_bound(del, vd, M, k, wv != 0);
            if (lane == 0) range[wv] = b;
        }
        __syncthreads();
        lo = range[0];                        // <= vd
        hi = range[1] < lo ? lo : range[1];   // <= vd (lo <= hi over sorted columns)
    }
    const uint32_t dn = hi - lo;
    const bool staged = dn <= DELETE_STAGE;
    if (dn && staged) {  // (block-uniform)
        for (uint32_t r = threadIdx.x; r < dn; r += HONU_BLOCK) {
            uint32_t d[SORT_KEY_WORDS];
            delete_load(del, lo + r, M, d);
            lds_row_store(rows, r, d);
        }
        __syncthreads();
    }

    uint32_t kept = 0;
    for (uint32_t r = 0; r < DELETE_ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;  // the tile's ballot: rows [64 j, 64 j + 64)
        const uint32_t t = j * HONU_WAVE + lane;
        bool keep = false;
        if (j * HONU_WAVE < vlen) {  // (wave-uniform) the ballot has a valid row
            const bool in = t < vlen;
            uint32_t w[SORT_KEY_WORDS];
#pragma unroll
            for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] = 0;
            if (in) pack_key(sorted + (uint64_t)HONU_KEY_LEN * (p0 + t), true, w);
            bool drop = false;
            if (in && dn) {
                uint32_t k[SORT_KEY_WORDS], d[SORT_KEY_WORDS];
#pragma unroll
                for (int i = 0; i < SORT_KEY_WORDS; i++) k[i] = w[i] & M.w[i];
                auto load = [&](uint32_t at) {
                    if (staged) lds_row_load(rows, at, d);
                    else delete_load(del, lo + at, M, d);
                };
                const uint32_t a = thread_bound(0, dn, [&](uint32_t mid) {  // the lower bound of k in the range
                    load(mid);
                    return packed_before(d, k, false);
                });
                if (a < dn) {
                    load(a);
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
        const uint64_t bits = __ballot(keep);
        if (lane == 0) W.mask[(uint64_t)blockIdx.x * DELETE_WORDS + j] = bits;
        kept += (uint32_t)__popcll(bits);
    }
    if (lane == 0) cnt[wv] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) sum += cnt[w];
        W.kept[blockIdx.x] = sum;
    }
}

// W.kept scanned (the rows kept before the tile), *kept_total the total
__global__ __launch_bounds__(HONU_BLOCK) void k_delete_place(
    const uint8_t *__restrict__ sorted, const uint32_t *__restrict__ order, const uint64_t *__restrict__ valid,
    uint32_t n, uint8_t *__restrict__ out, uint32_t *__restrict__ order_out,
    const uint64_t *__restrict__ kept_total, uint64_t *__restrict__ removed, DeleteWork W) {
    __shared__ uint64_t msk[DELETE_WORDS];
    __shared__ uint32_t pre[DELETE_WORDS];  // rows kept in the tile's ballots before ballot j
    const uint32_t v = valid_rows(valid, n);
    const uint64_t kept = *kept_total < v ? *kept_total : v;
    if (blockIdx.x == 0 && threadIdx.x == 0 && removed) *removed = v - kept;
    const uint32_t p0 = blockIdx.x * DELETE_TILE;  // below n
    const uint32_t len = n - p0 < DELETE_TILE ? n - p0 : DELETE_TILE;
    if (threadIdx.x < DELETE_WORDS) msk[threadIdx.x] = W.mask[(uint64_t)blockIdx.x * DELETE_WORDS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < DELETE_WORDS) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < threadIdx.x; j++) s += (uint32_t)__popcll(msk[j]);
        pre[threadIdx.x] = s;
    }
    __syncthreads();
    const uint64_t base = W.kept[blockIdx.x];
    const uint32_t wv = wave_in_block(), lane = lane_id();
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0;
    for (uint32_t r = 0; r < DELETE_ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;
        const uint32_t t = j * HONU_WAVE + lane;
        if (t >= len) continue;
        const uint32_t p = p0 + t;
        uint64_t dst = p;  // a row of the invalid tail stays
        if (p < v) {
            const uint64_t kept_before = base + pre[j] + (uint32_t)__popcll(msk[j] & below);
            dst = (msk[j] >> lane) & 1ull ? kept_before : kept + ((uint64_t)p - kept_before);
            dst = dst < v ? dst : p;  // (a mask or a count that is not the mark's: inside the rows all the same)
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
    const DeleteWork W = delete_carve(work, n);
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
