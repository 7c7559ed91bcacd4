// merge_buckets.hip — a routed batch of Puts into every collection's bucket at
// once (collections.Put, store.go:232, 395, 530, into the bucket
// tx.Bucket(collectionID[:]) names, store.go:236-240, tx.go:112-120): k
// buckets' sorted columns lie end to end in one arena (bucket_off.h), the
// batch as honu_key_route leaves it is a second such arena, and the output is
// the third: per bucket the stable merge of its valid A rows and its B rows,
// A's before B's on equal keys, the buckets tight behind each other. What
// merge.hip does for one column, for all of them in one launch: the offsets
// are read on the device, so nothing is read on the host between the route
// and this.
//
// The output is bucket-major and so are both inputs, so the MERGE_TILE output
// rows of a workgroup come from one run of A's valid rows and one run of B's
// rows (bucket_off.h: A's valid rows numbered end to end by pa).
//   offsets    without counts d_off_out[c] = ea[c] + eb[c], no scan: a
//              grid-stride part of the merge's own launch. With d_count_a the
//              buckets' rows va + vb go through launch_scan first (k values
//              in place, the total to d_off_out[k]) and the merge reads what
//              the scan wrote;
//   partition  two waves, one per end of the tile: the bucket of the end (a
//              wave_bound over c on the output offsets, computed as they are
//              read), then the split of the local diagonal inside that bucket
//              (merge path over the bucket's two views, a wave_bound over
//              global memory). Nothing passes between workgroups;
//   stage      both runs packed into LDS, the index beside the key (keycol.h's
//              9-word row); the tile's slice of offsets too when the tile
//              touches no more than MERGE_BUCKETS_STAGE buckets, read from
//              memory above that. A row's bucket is the last one of the slice
//              that starts at or below it (empty buckets give equal offsets);
//   rank       by (bucket, key): a row's rank is its offset in its own run
//              plus the rows of the other run that go before it, which are the
//              other run's rows of earlier buckets and, inside the row's own
//              bucket, one thread_bound in LDS over that bucket's part of the
//              run alone: strictly below it for an A row, below or equal for a
//              B row, the merge's tie rule. The bucket bounds the bracket, so
//              no key of another bucket is ever compared;
//   emit       the ranks turned round in LDS (rank -> staged row), so that
//              consecutive lanes store consecutive output rows.
// LDS: 1024 x 36 bytes of rows + 2 KiB of ranks + 3 x 161 words of offsets +
// the two cuts: 40,904 bytes as laid out, four workgroups per CU (160 KiB),
// as merge.hip.
// No atomics and no spin-wait of its own (launch_scan's are the context's),
// no state outside the launch, plain C++ stores. Every row read lies below na
// or nb, every offset entry read in [0, k], whatever the arrays hold.
#include "kernels.h"
#include "keycol.h"

#define HONU_BUCKET_FN HONU_DEV
#include "bucket_off.h"

namespace honu {

constexpr uint32_t MB_TILE = 1024;  // output rows per workgroup, merge.hip's
// buckets a tile touches at most for its slice of offsets to be staged (chosen so that the LDS stays
// at four workgroups per CU, not measured: DESIGN §6.12)
constexpr uint32_t MERGE_BUCKETS_STAGE = 160;
static_assert(MB_TILE <= 65536, "the ranks are 16-bit");
static_assert(MB_TILE * KEY_ROW_WORDS * 4 + MB_TILE * 2 + 3 * (MERGE_BUCKETS_STAGE + 1) * 4 + 6 * 4 <= 40960,
              "four workgroups per CU");

uint32_t merge_buckets_stage() { return MERGE_BUCKETS_STAGE; }

// row min(i, n - 1) of a column of n rows packed, zeros for a column without rows
HONU_DEV void load_row_clamped(const uint8_t *col, uint32_t i, uint32_t n, uint32_t w[SORT_KEY_WORDS]) {
    if (n) pack_key(col + (uint64_t)HONU_KEY_LEN * (i < n ? i : n - 1), true, w);
    else pack_key(col, false, w);
}

// what the call writes for bucket c <= k beside the rows. Without counts the offset itself; with them
// the bucket's rows, which launch_scan turns into offsets in place (d_off_out[k] is the scan's total)
HONU_DEV void bucket_write(const bucket_cols &B, uint32_t c, uint64_t *__restrict__ off_out,
                           uint64_t *__restrict__ count_out) {
    const uint32_t rows = c < B.k ? bucket_va(&B, c) + bucket_vb(&B, c) : 0;
    if (c < B.k && count_out) count_out[c] = rows;
    if (B.count_a) {
        if (c < B.k) off_out[c] = rows;
    } else {
        off_out[c] = bucket_out(&B, c);
    }
}

__global__ __launch_bounds__(HONU_BLOCK) void k_bucket_off(bucket_cols B, uint64_t *__restrict__ off_out,
                                                           uint64_t *__restrict__ count_out) {
    const uint64_t c = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (c <= B.k) bucket_write(B, (uint32_t)c, off_out, count_out);
}

// the rows of the two sides and the record numbering of B's
struct BucketRows {
    const uint8_t *sa;
    const uint32_t *oa;
    const uint8_t *sb;
    const uint32_t *ob;
    const uint32_t *base;  // per bucket, or null: b_base
    uint32_t b_base;
};

__global__ __launch_bounds__(HONU_BLOCK) void k_merge_buckets(bucket_cols B, BucketRows R, uint8_t *__restrict__ out,
                                                              uint32_t *__restrict__ order,
                                                              uint64_t *__restrict__ off_out,
                                                              uint64_t *__restrict__ count_out) {
    __shared__ uint32_t rows[MB_TILE * KEY_ROW_WORDS];  // the packed key, the index beside it
    __shared__ uint16_t at[MB_TILE];                    // rank in the tile -> staged row
    // the tile's slice of offsets, entry j for bucket c0 + j: pa, eb, and with counts ea
    __shared__ uint32_t s_pa[MERGE_BUCKETS_STAGE + 1], s_eb[MERGE_BUCKETS_STAGE + 1], s_ea[MERGE_BUCKETS_STAGE + 1];
    __shared__ uint32_t cut[6];  // per end of the tile: A's valid rows before it, B's rows before it, its bucket
    const bool counted = B.count_a != nullptr;
    const uint32_t k = B.k, n = B.na + B.nb;  // n <= 2^32 - 1 (launch_merge_buckets' caller)

    if (!counted)  // the offsets and counts: k can exceed the rows by orders of magnitude
        for (uint64_t c = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x; c <= k; c += (uint64_t)gridDim.x * HONU_BLOCK)
            bucket_write(B, (uint32_t)c, off_out, count_out);

    const uint32_t total = bucket_out(&B, k);  // <= n
    const uint32_t p0 = blockIdx.x * MB_TILE;  // below n
    const uint32_t p1 = n - p0 < MB_TILE ? n : p0 + MB_TILE;
    const uint32_t d0 = p0 < total ? p0 : total, d1 = p1 < total ? p1 : total;
    if (d0 >= d1) return;  // (block-uniform; k >= 1 from here on, as total > 0)

    // the two cuts, each by a wave of its own: the first row's bucket and the rows of it before the tile,
    // the last row's bucket and the rows of it up to the tile's end
    if (threadIdx.x < 2 * HONU_WAVE) {
        const uint32_t w = wave_in_block();
        const uint32_t d = w ? d1 : d0, at_row = w ? d1 - 1 : d0;
        uint32_t c = wave_bound(1, k + 1, [&](uint32_t mid) { return bucket_starts_by(&B, mid, at_row) != 0; }) - 1;
        c = c < k ? c : k - 1;
        const uint32_t ea = bucket_ea(&B, c), eb = bucket_eb(&B, c);
        const uint32_t va = bucket_va(&B, c), vb = bucket_vb(&B, c);  // ea + va <= na, eb + vb <= nb
        const uint32_t l = bucket_diag(&B, c, d);                     // <= va + vb
        const uint8_t *a = R.sa + (uint64_t)HONU_KEY_LEN * ea, *b = R.sb + (uint64_t)HONU_KEY_LEN * eb;
        // how many of the bucket's first l merged rows come from A (merge.hip's merge_split over the two views)
        const uint32_t i = wave_bound(bucket_split_lo(l, vb), bucket_split_hi(l, va), [&](uint32_t mid) {
            uint32_t ka[SORT_KEY_WORDS], kb[SORT_KEY_WORDS];  // mid < va, 0 <= l - 1 - mid < vb
            pack_key(a + (uint64_t)HONU_KEY_LEN * mid, true, ka);
            pack_key(b + (uint64_t)HONU_KEY_LEN * (l - 1 - mid), true, kb);
            return packed_before(ka, kb, true);
        });
        if (lane_id() == 0) {
            cut[3 * w] = bucket_pa(&B, c) + i;
            cut[3 * w + 1] = eb + (l - i);
            cut[3 * w + 2] = c;
        }
    }
    __syncthreads();
    const uint32_t len = d1 - d0;  // <= MB_TILE
    const uint32_t u0 = cut[0], v0 = cut[1], c0 = cut[2];
    // (u0 <= u1 <= u0 + len and c0 <= c1 over ascending offsets and sorted buckets; over anything else the
    // clamps keep every read inside the arrays)
    const uint32_t la = bucket_min(bucket_sub(cut[3], u0), len), lb = len - la;  // la A rows, then lb B rows
    const uint32_t nbk = (cut[5] > c0 ? cut[5] - c0 : 0) + 1;                    // c0 + nbk <= k
    const bool staged = nbk <= MERGE_BUCKETS_STAGE;                              // (block-uniform)
    if (staged) {
        for (uint32_t j = threadIdx.x; j <= nbk; j += HONU_BLOCK) {
            s_pa[j] = bucket_pa(&B, c0 + j);
            s_eb[j] = bucket_eb(&B, c0 + j);
            if (counted) s_ea[j] = bucket_ea(&B, c0 + j);
        }
        __syncthreads();
    }
    // the bucket (less c0) of A's valid row u or of B's row v of the tile
    auto bucket_a = [&](uint32_t u) { return staged ? bucket_of_row_words(s_pa, nbk, u) : bucket_of_row(&B, 0, c0, nbk, u); };
    auto bucket_b = [&](uint32_t v) { return staged ? bucket_of_row_words(s_eb, nbk, v) : bucket_of_row(&B, 1, c0, nbk, v); };

    for (uint32_t r = threadIdx.x; r < len; r += HONU_BLOCK) {
        const bool from_a = r < la;
        uint32_t w[SORT_KEY_WORDS], idx = 0;
        if (from_a) {
            uint32_t src = u0 + r;
            if (counted) {  // the valid rows of a bucket are its first, the invalid ones lie between the buckets
                const uint32_t j = bucket_a(src);
                const uint32_t ea = staged ? s_ea[j] : bucket_ea(&B, c0 + j), pa = staged ? s_pa[j] : bucket_pa(&B, c0 + j);
                src = ea + bucket_sub(src, pa);
            }
            load_row_clamped(R.sa, src, B.na, w);
            if (order && B.na) idx = R.oa[src < B.na ? src : B.na - 1];
        } else {
            const uint32_t v = v0 + (r - la), src = v < B.nb ? v : bucket_sub(B.nb, 1);
            load_row_clamped(R.sb, v, B.nb, w);
            if (order) idx = bucket_b_index(R.ob && B.nb ? R.ob[src] : v, R.base ? R.base[c0 + bucket_b(v)] : R.b_base);
        }
        lds_row_store(rows, r, w);
        rows[r * KEY_ROW_WORDS + SORT_KEY_WORDS] = idx;
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < len; r += HONU_BLOCK) {
        const bool from_a = r < la;
        uint32_t w[SORT_KEY_WORDS], lo, hi;
        lds_row_load(rows, r, w);
        // the other run's rows of this row's bucket: [lo, hi) of that run
        if (from_a) {
            const uint32_t j = bucket_a(u0 + r);
            bucket_span(staged ? s_eb[j] : bucket_eb(&B, c0 + j), staged ? s_eb[j + 1] : bucket_eb(&B, c0 + j + 1), v0, lb,
                        &lo, &hi);
        } else {
            const uint32_t j = bucket_b(v0 + (r - la));
            bucket_span(staged ? s_pa[j] : bucket_pa(&B, c0 + j), staged ? s_pa[j + 1] : bucket_pa(&B, c0 + j + 1), u0, la,
                        &lo, &hi);
        }
        // an A row: the B rows below it; a B row: the A rows below or equal to it
        const uint32_t first = from_a ? la : 0;
        const uint32_t bound = thread_bound(first + lo, first + hi, [&](uint32_t mid) {
            uint32_t key[SORT_KEY_WORDS];
            lds_row_load(rows, mid, key);
            return packed_before(key, w, !from_a);
        });
        at[(from_a ? r : r - la) + (bound - first)] = (uint16_t)r;
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < len; q += HONU_BLOCK) {
        const uint32_t r = at[q] < len ? at[q] : len - 1, p = d0 + q;  // (a permutation over sorted buckets)
        uint32_t w[SORT_KEY_WORDS];
        lds_row_load(rows, r, w);
        unpack_key(out + (uint64_t)HONU_KEY_LEN * p, w);
        if (order) order[p] = rows[r * KEY_ROW_WORDS + SORT_KEY_WORDS];
    }
}

hipError_t launch_merge_buckets(uint64_t k, const uint8_t *sa, const uint32_t *oa, const uint64_t *off_a,
                                const uint64_t *count_a, uint64_t na, const uint8_t *sb, const uint32_t *ob,
                                const uint64_t *off_b, uint64_t nb, const uint32_t *base, uint32_t b_base, uint8_t *out,
                                uint32_t *order, uint64_t *off_out, uint64_t *count_out, const ScanState &S,
                                hipStream_t s) {
    const uint64_t n = na + nb;  // <= 2^32 - 1
    const bucket_cols B = {off_a, count_a, off_b, off_out, (uint32_t)na, (uint32_t)nb, (uint32_t)k};
    if (count_a || n == 0) {
        hipLaunchKernelGGL(k_bucket_off, dim3((unsigned)((k + 1 + HONU_BLOCK - 1) / HONU_BLOCK)), dim3(HONU_BLOCK), 0, s,
                           B, off_out, count_out);
        if (count_a) {  // (k <= the state's rows: the caller; k == 0 stores the total, 0, alone)
            const hipError_t e = launch_scan(off_out, k, 1, off_out, off_out + k, S, s);
            if (e != hipSuccess) return e;
        }
    }
    if (n == 0) return hipGetLastError();
    const BucketRows R = {sa, order ? oa : nullptr, sb, order ? ob : nullptr, order ? base : nullptr, b_base};
    hipLaunchKernelGGL(k_merge_buckets, dim3((unsigned)((n + MB_TILE - 1) / MB_TILE)), dim3(HONU_BLOCK), 0, s, B, R, out,
                       order, off_out, count_out);
    return hipGetLastError();
}

}  // namespace honu
