// route_find.h — the arithmetic of the route (route.hip) as plain functions:
// no HIP, <stdint.h> alone, the qualifier and the two loads from macros, so
// the host program of tests/test_key_route_find_host.py runs what the kernels
// run. A collection ID is 16 bytes compared with bytes.Compare: four
// big-endian words, word 0 the most significant. The table of collections is
// k such IDs, ascending and distinct; a class is a table row (< k), k for an
// ID the table does not hold (the nil bucket, tx.go:117-120) and k + 1 for a
// position that does not take part.
#pragma once

#include <stdint.h>

#ifndef HONU_ROUTE_FN
#define HONU_ROUTE_FN static inline
#endif

#define ROUTE_ID_LEN 16u
#define ROUTE_ID_WORDS 4

// the big-endian word of the 4 bytes at p, any byte address
HONU_ROUTE_FN uint32_t route_bytes_be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// the four big-endian words of the 16 bytes at p, any byte address
HONU_ROUTE_FN void route_bytes_id(const uint8_t *p, uint32_t w[ROUTE_ID_WORDS]) {
    for (int i = 0; i < ROUTE_ID_WORDS; i++) w[i] = route_bytes_be32(p + 4 * i);
}

// The kernels load with one instruction each (route.hip defines both before
// it includes this header); the host program takes the bytes one by one.
#ifndef HONU_ROUTE_LOAD_ID
#define HONU_ROUTE_LOAD_ID(p, w) route_bytes_id((p), (w))
#endif
#ifndef HONU_ROUTE_LOAD_BE32
#define HONU_ROUTE_LOAD_BE32(p) route_bytes_be32(p)
#endif

// a < b by bytes.Compare
HONU_ROUTE_FN int route_id_before(const uint32_t a[ROUTE_ID_WORDS], const uint32_t b[ROUTE_ID_WORDS]) {
    int lt = 0;
    for (int i = ROUTE_ID_WORDS - 1; i >= 0; i--) lt = a[i] != b[i] ? a[i] < b[i] : lt;
    return lt;
}

HONU_ROUTE_FN int route_id_same(const uint32_t a[ROUTE_ID_WORDS], const uint32_t b[ROUTE_ID_WORDS]) {
    int eq = 1;
    for (int i = 0; i < ROUTE_ID_WORDS; i++) eq = eq && a[i] == b[i];
    return eq;
}

// The lower bound of id in the table: the first row that is not before id, k
// when every row is. Whatever the rows hold, lo <= the result <= k, every row
// asked lies in [0, k) and the bracket shrinks at every step. Two forms of one
// loop: the table as it lies in memory (16-byte rows at any byte address) ...
HONU_ROUTE_FN uint32_t route_lower_bound_bytes(const uint8_t *table, uint32_t k, const uint32_t id[ROUTE_ID_WORDS]) {
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t row[ROUTE_ID_WORDS];
        HONU_ROUTE_LOAD_ID(table + (uint64_t)ROUTE_ID_LEN * mid, row);
        if (route_id_before(row, id)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ... and as a workgroup stages it: four big-endian words per row
HONU_ROUTE_FN uint32_t route_lower_bound_words(const uint32_t *rows, uint32_t k, const uint32_t id[ROUTE_ID_WORDS]) {
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (route_id_before(rows + ROUTE_ID_WORDS * mid, id)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The class of a position: `part` says the position names a record that takes
// part, lb is the lower bound of its ID and `same` whether row lb (lb < k)
// equals it. Over an ascending table the lower bound is the only row that
// can; over garbage it is the first such row the search can see.
HONU_ROUTE_FN uint32_t route_class(int part, uint32_t lb, int same, uint32_t k) {
    if (!part) return k + 1;
    return lb < k && same ? lb : k;
}

// The sort row of a class: 29 bytes, a constant byte 0, the class big-endian
// in bytes [1, 5), zeros behind it. As the two little-endian words that hold
// bytes [0, 8):
#define ROUTE_ROW_BYTE0 0x01u
HONU_ROUTE_FN uint32_t route_row_word0(uint32_t c) {
    return ROUTE_ROW_BYTE0 | ((c >> 24) << 8) | (((c >> 16) & 0xFFu) << 16) | (((c >> 8) & 0xFFu) << 24);
}
HONU_ROUTE_FN uint32_t route_row_word1(uint32_t c) { return c & 0xFFu; }

// the class a sort row holds, no more than k + 1 whatever the row holds
HONU_ROUTE_FN uint32_t route_row_class(const uint8_t *row, uint32_t k) {
    const uint32_t c = HONU_ROUTE_LOAD_BE32(row + 1);
    return c < k + 1 ? c : k + 1;
}

// An offset as a bound over the classes: the first row of [lo, hi) of the
// sorted rows (29 bytes each) whose class is not below c, hi when none is.
// With lo = 0 and hi = m this is d_bucket_off[c], and m for c = k + 2.
HONU_ROUTE_FN uint32_t route_offset(const uint8_t *sorted, uint32_t lo, uint32_t hi, uint32_t c, uint32_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (route_row_class(sorted + (uint64_t)29 * mid, k) < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
