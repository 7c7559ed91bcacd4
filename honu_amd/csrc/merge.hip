// merge.hip — a batch of Puts into the sorted key column (collections.Put,
// store.go:232, 395, 530; the bkt.Put(k, value) calls of
// iterator/cursor_test.go:235): the stable merge of two of honu_sort_keys'
// outputs, A's rows before B's on equal keys, which is what the sort returns
// for the concatenated columns.
//
// One launch, one workgroup per MERGE_TILE output positions. The valid counts
// are on the device, so a workgroup decides there what its tile is: positions
// below va + vb are merged, the rest copied from the two invalid tails.
//   partition  the tile's first and last diagonal are split by a search over
//              global memory (merge path, a wave_bound), each workgroup its
//              own two, a wave each: nothing passes between workgroups;
//   stage      the A range and the B range of the tile packed into LDS, the
//              index beside the key (keycol.h's 9-word row);
//   rank       a row's output position is its offset in its own range plus
//              the rows of the other range that go before it, one
//              thread_bound in LDS: strictly below it for an A row, below or
//              equal for a B row, the partition's tie rule;
//   emit       the ranks turned round in LDS (rank -> staged row), so that
//              consecutive lanes store consecutive output rows.
// (Measured against a per-thread serial merge of four consecutive outputs
// from a split of the thread's own diagonal in LDS: equal within the windows'
// spread at 64 K and 1 M keys per batch, 21 us against 29 us at 1 K, where
// nearly every tile is A's alone. DESIGN §6.3.)
// No atomics, no spin-wait, no state outside the launch.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t MERGE_TILE = 1024;                 // output positions per workgroup
// 1024 x 36 bytes of rows + 2 KiB of ranks + the splits: 38 KiB, four workgroups per CU
static_assert(MERGE_TILE <= 65536, "the ranks are 16-bit");
static_assert(MERGE_TILE % HONU_BLOCK == 0, "a thread takes MERGE_TILE / HONU_BLOCK positions");

uint32_t merge_tile() { return MERGE_TILE; }

HONU_DEV void load_packed(const uint8_t *col, uint32_t i, uint32_t w[SORT_KEY_WORDS]) {
    pack_key(col + (uint64_t)HONU_KEY_LEN * i, true, w);
}

// How many of the first d merged rows (d <= va + vb) come from A: the i with
// A[i - 1] <= B[d - i] and B[d - i - 1] < A[i], rows out of range counting as
// -inf / +inf. A[mid] is among the first d exactly when it goes before
// B[d - 1 - mid], and on equal keys it does; the mids that say yes are the
// ones below i. Called by a whole wave with one d: four round trips over 1M
// rows (measured against the one-lane bisection: DESIGN §6.3).
HONU_DEV uint32_t merge_split(const uint8_t *__restrict__ a, uint32_t va, const uint8_t *__restrict__ b,
                              uint32_t vb, uint32_t d) {
    return wave_bound(d > vb ? d - vb : 0, d < va ? d : va, [&](uint32_t mid) {  // mid < va, 0 <= d - 1 - mid < vb
        uint32_t ka[SORT_KEY_WORDS], kb[SORT_KEY_WORDS];
        load_packed(a, mid, ka);
        load_packed(b, d - 1 - mid, kb);
        return packed_before(ka, kb, true);
    });
}

__global__ __launch_bounds__(HONU_BLOCK) void k_key_merge(
    const uint8_t *__restrict__ sa, const uint32_t *__restrict__ oa, const uint64_t *__restrict__ valid_a,
    uint32_t na, const uint8_t *__restrict__ sb, const uint32_t *__restrict__ ob,
    const uint64_t *__restrict__ valid_b, uint32_t nb, uint32_t b_base, uint8_t *__restrict__ out,
    uint32_t *__restrict__ order, uint64_t *__restrict__ valid_out) {
    __shared__ uint32_t rows[MERGE_TILE * KEY_ROW_WORDS];  // the packed key, the index beside it
    __shared__ uint16_t at[MERGE_TILE];  // rank in the tile -> staged row
    __shared__ uint32_t split[2];
    const uint32_t va = valid_rows(valid_a, na), vb = valid_rows(valid_b, nb);
    const uint32_t v = va + vb, n = na + nb;  // n <= 2^32 - 1 (launch_key_merge's caller)
    if (blockIdx.x == 0 && threadIdx.x == 0) *valid_out = v;
    const uint32_t p0 = blockIdx.x * MERGE_TILE;  // below n
    const uint32_t p1 = n - p0 < MERGE_TILE ? n : p0 + MERGE_TILE;
    const uint32_t d0 = p0 < v ? p0 : v, d1 = p1 < v ? p1 : v;

    if (d0 < d1) {  // (block-uniform)
        // the two splits, each by a wave of its own
        if (threadIdx.x < 2 * HONU_WAVE) {
            const uint32_t w = wave_in_block();
            const uint32_t i = merge_split(sa, va, sb, vb, w ? d1 : d0);
            if (lane_id() == 0) split[w] = i;
        }
        __syncthreads();
        const uint32_t i0 = split[0], len = d1 - d0;  // len <= MERGE_TILE
        // (i0 <= i1 <= i0 + len over sorted columns; over anything else the clamp keeps every read inside them)
        const uint32_t i1 = split[1] < i0 ? i0 : (split[1] - i0 > len ? i0 + len : split[1]);
        const uint32_t j0 = d0 - i0, la = i1 - i0;  // la A rows, then len - la B rows
        for (uint32_t r = threadIdx.x; r < len; r += HONU_BLOCK) {
            const bool from_a = r < la;
            const uint32_t src = from_a ? i0 + r : j0 + (r - la);
            uint32_t w[SORT_KEY_WORDS];
            load_packed(from_a ? sa : sb, src, w);
            lds_row_store(rows, r, w);
            rows[r * KEY_ROW_WORDS + SORT_KEY_WORDS] = order ? (from_a ? oa[src] : ob[src] + b_base) : 0;
        }
        __syncthreads();
        for (uint32_t r = threadIdx.x; r < len; r += HONU_BLOCK) {
            const bool from_a = r < la;
            uint32_t w[SORT_KEY_WORDS];
            lds_row_load(rows, r, w);
            // an A row: the B rows below it; a B row: the A rows below or equal to it
            const uint32_t first = from_a ? la : 0;
            const uint32_t bound = thread_bound(first, from_a ? len : la, [&](uint32_t mid) {
                uint32_t k[SORT_KEY_WORDS];
                lds_row_load(rows, mid, k);
                return packed_before(k, w, !from_a);
            });
            at[(from_a ? r : r - la) + (bound - first)] = (uint16_t)r;
        }
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < len; q += HONU_BLOCK) {
            const uint32_t r = at[q], p = d0 + q;
            uint32_t w[SORT_KEY_WORDS];
            lds_row_load(rows, r, w);
            unpack_key(out + (uint64_t)HONU_KEY_LEN * p, w);
            if (order) order[p] = rows[r * KEY_ROW_WORDS + SORT_KEY_WORDS];
        }
    }

    // the invalid rows behind the merged ones: A's [va, na), then B's [vb, nb), as they stand
    const uint32_t ta = na - va;
    // (t counts from the tile's first position, behind its d1 - d0 merged ones: at most MERGE_TILE, where
    // a position plus HONU_BLOCK could wrap past 2^32 on the last tile)
    for (uint32_t t = (d1 - d0) + threadIdx.x; t < p1 - p0; t += HONU_BLOCK) {
        const uint32_t p = p0 + t, q = p - v;
        const bool from_a = q < ta;
        const uint32_t src = from_a ? va + q : vb + (q - ta);
        copy_key(out + (uint64_t)HONU_KEY_LEN * p, (from_a ? sa : sb) + (uint64_t)HONU_KEY_LEN * src);
        if (order) order[p] = from_a ? oa[src] : ob[src] + b_base;
    }
}

hipError_t launch_key_merge(const uint8_t *sa, const uint32_t *oa, const uint64_t *valid_a, uint64_t na,
                            const uint8_t *sb, const uint32_t *ob, const uint64_t *valid_b, uint64_t nb,
                            uint32_t b_base, uint8_t *out, uint32_t *order, uint64_t *valid_out, hipStream_t s) {
    const uint64_t n = na + nb;  // <= 2^32 - 1
    if (n == 0) return hipMemsetAsync(valid_out, 0, sizeof(uint64_t), s);
    hipLaunchKernelGGL(k_key_merge, dim3((unsigned)((n + MERGE_TILE - 1) / MERGE_TILE)), dim3(HONU_BLOCK), 0, s, sa,
                       order ? oa : nullptr, valid_a, (uint32_t)na, sb, order ? ob : nullptr, valid_b, (uint32_t)nb,
                       b_base, out, order, valid_out);
    return hipGetLastError();
}

}  // namespace honu
