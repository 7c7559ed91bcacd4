// bucket_off.h — the arithmetic of the bucketed column (merge_buckets.hip) as
// plain functions: no HIP, <stdint.h> alone, the qualifier and the load from
// macros, so the host program of tests/test_key_bucket_off_host.py runs what
// the kernels run. A bucketed column is k buckets end to end in one arena of
// n rows: d_off is uint64[k + 1], bucket c the rows [d_off[c], d_off[c + 1]).
// A merge has two of them, A (with an optional count of valid rows per
// bucket) and B, and writes a third. Per bucket c, all in rows:
//   ea, eb   the offsets clamped to their arenas (bucket_clamp);
//   va, vb   the rows that take part: the clamped difference, never negative,
//            A's also capped by its count;
//   out      the bucket's first output row: ea + eb without counts (0 for
//            c = 0), d_off_out[c] as the scan wrote it with them;
//   pa       the valid A rows before the bucket: ea without counts, out - eb
//            with them. A's valid rows numbered this way lie end to end, as
//            B's rows do in their arena.
// Whatever the arrays hold, every entry read lies in [0, k], every result is
// clamped to its arena and every bracket shrinks at each step.
#pragma once

#include <stdint.h>

#ifndef HONU_BUCKET_FN
#define HONU_BUCKET_FN static inline
#endif
// one uint64 of an offset or count array (merge_buckets.hip loads it as it is)
#ifndef HONU_BUCKET_LOAD
#define HONU_BUCKET_LOAD(p) (*(p))
#endif

typedef struct {
    const uint64_t *off_a;    // k + 1
    const uint64_t *count_a;  // k, or null: every row of a bucket is valid
    const uint64_t *off_b;    // k + 1
    const uint64_t *off_out;  // k + 1, read only with count_a: the scanned output offsets
    uint32_t na, nb, k;       // na + nb <= 2^32 - 1
} bucket_cols;

// an offset clamped to the n rows of its arena
HONU_BUCKET_FN uint32_t bucket_clamp(uint64_t off, uint32_t n) { return off < n ? (uint32_t)off : n; }

// a - b, 0 where b is the larger (offsets that do not ascend)
HONU_BUCKET_FN uint32_t bucket_sub(uint32_t a, uint32_t b) { return a > b ? a - b : 0; }

HONU_BUCKET_FN uint32_t bucket_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// c <= k
HONU_BUCKET_FN uint32_t bucket_ea(const bucket_cols *B, uint32_t c) {
    return bucket_clamp(HONU_BUCKET_LOAD(B->off_a + c), B->na);
}
HONU_BUCKET_FN uint32_t bucket_eb(const bucket_cols *B, uint32_t c) {
    return bucket_clamp(HONU_BUCKET_LOAD(B->off_b + c), B->nb);
}

// c < k: ea + va <= na and eb + vb <= nb, so the views (ea, va) and (eb, vb) lie inside the arenas
HONU_BUCKET_FN uint32_t bucket_va(const bucket_cols *B, uint32_t c) {
    const uint32_t rows = bucket_sub(bucket_ea(B, c + 1), bucket_ea(B, c));
    if (!B->count_a) return rows;
    return bucket_clamp(HONU_BUCKET_LOAD(B->count_a + c), rows);
}
HONU_BUCKET_FN uint32_t bucket_vb(const bucket_cols *B, uint32_t c) {
    return bucket_sub(bucket_eb(B, c + 1), bucket_eb(B, c));
}

// c <= k: the first output row of bucket c, no more than na + nb
HONU_BUCKET_FN uint32_t bucket_out(const bucket_cols *B, uint32_t c) {
    if (B->count_a) return bucket_clamp(HONU_BUCKET_LOAD(B->off_out + c), B->na + B->nb);
    return c ? bucket_ea(B, c) + bucket_eb(B, c) : 0;
}

// c <= k: the valid A rows before bucket c
HONU_BUCKET_FN uint32_t bucket_pa(const bucket_cols *B, uint32_t c) {
    return B->count_a ? bucket_sub(bucket_out(B, c), bucket_eb(B, c)) : bucket_ea(B, c);
}

// An output position's bucket: the last c with out(c) <= d. Empty buckets
// give equal offsets, so this is the bucket that holds row d when one does.
// The predicate of the search, asked for 1 <= c <= k ...
HONU_BUCKET_FN int bucket_starts_by(const bucket_cols *B, uint32_t c, uint32_t d) { return bucket_out(B, c) <= d; }

// ... and the search by one thread (the kernel asks 64 c's a step, keycol.h's
// wave_bound over the same bracket [1, k + 1) less one): below k for k >= 1,
// whatever the offsets hold
HONU_BUCKET_FN uint32_t bucket_of_pos(const bucket_cols *B, uint32_t d) {
    uint32_t lo = 1, hi = B->k + 1;  // (k <= 2^32 - 4)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bucket_starts_by(B, mid, d)) lo = mid + 1;
        else hi = mid;
    }
    return bucket_min(lo - 1, bucket_sub(B->k, 1));
}

// The local diagonal of output position d in bucket c < k: the rows of the
// bucket before d, no more than the bucket has ...
HONU_BUCKET_FN uint32_t bucket_diag(const bucket_cols *B, uint32_t c, uint32_t d) {
    return bucket_min(bucket_sub(d, bucket_out(B, c)), bucket_va(B, c) + bucket_vb(B, c));
}

// ... and the bracket of its split, the A rows among the first l merged rows
// of views of va and vb rows (l <= va + vb): lo <= hi <= va, and for a mid in
// [lo, hi) B's row l - 1 - mid lies in [0, vb)
HONU_BUCKET_FN uint32_t bucket_split_lo(uint32_t l, uint32_t vb) { return bucket_sub(l, vb); }
HONU_BUCKET_FN uint32_t bucket_split_hi(uint32_t l, uint32_t va) { return bucket_min(l, va); }

// A row's bucket among the nbk >= 1 buckets a tile touches: off holds the
// tile's slice of pa (A) or eb (B), off[j] for bucket c0 + j; x is the row's
// number, at or above off[0]. The last j < nbk with off[j] <= x. Two forms of
// one loop: the slice staged as words ...
HONU_BUCKET_FN uint32_t bucket_of_row_words(const uint32_t *off, uint32_t nbk, uint32_t x) {
    uint32_t lo = 1, hi = nbk;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// ... and read from the arrays (side_b: eb, else pa), c0 + nbk <= k
HONU_BUCKET_FN uint32_t bucket_of_row(const bucket_cols *B, int side_b, uint32_t c0, uint32_t nbk, uint32_t x) {
    uint32_t lo = 1, hi = nbk;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((side_b ? bucket_eb(B, c0 + mid) : bucket_pa(B, c0 + mid)) <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// The rows of a bucket inside a tile's staged range: the bucket is the rows
// [first, next) of its side, the range the len rows from start. *lo <= *hi <= len
HONU_BUCKET_FN void bucket_span(uint32_t first, uint32_t next, uint32_t start, uint32_t len, uint32_t *lo,
                                uint32_t *hi) {
    const uint32_t l = bucket_min(bucket_sub(first, start), len);
    const uint32_t h = bucket_min(bucket_sub(next, start), len);
    *lo = l;
    *hi = h > l ? h : l;
}

// The record index of B's row g: its own (order is d_order_b[g], or g without
// d_order_b) plus the bucket's base, modulo 2^32
HONU_BUCKET_FN uint32_t bucket_b_index(uint32_t order, uint32_t base) { return order + base; }
