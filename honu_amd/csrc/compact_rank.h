// compact_rank.h — the arithmetic of the stable stream compaction (compact.h)
// as plain functions: no HIP, <stdint.h> alone, the qualifier from a macro, so
// the host program of tests/test_key_compact_host.py runs what the kernels
// run. A tile's keep masks are its ballots, bit l of word j row 64 j + l; a
// row's rank is the kept rows before it.
#pragma once

#include <stdint.h>

#ifndef HONU_COMPACT_FN
#define HONU_COMPACT_FN static inline
#endif

// the lanes of a ballot below `lane` (lane < 64; a shift by 64 is no shift)
HONU_COMPACT_FN uint64_t compact_lanes_below(uint32_t lane) { return lane ? ~0ull >> (64 - lane) : 0; }

// the rows kept in the tile's ballots before ballot j
HONU_COMPACT_FN uint32_t compact_words_before(const uint64_t *msk, uint32_t j) {
    uint32_t s = 0;
    for (uint32_t i = 0; i < j; i++) s += (uint32_t)__builtin_popcountll(msk[i]);
    return s;
}

// the rank of lane `lane` of a ballot, `before` the rows kept before the ballot
HONU_COMPACT_FN uint64_t compact_rank_lane(uint64_t before, uint64_t word, uint32_t lane) {
    return before + (uint32_t)__builtin_popcountll(word & compact_lanes_below(lane));
}

// the rank of row x of a tile out of its scanned count and its masks alone
HONU_COMPACT_FN uint64_t compact_rank_row(uint64_t base, const uint64_t *msk, uint32_t x) {
    return compact_rank_lane(base + compact_words_before(msk, x / 64), msk[x / 64], x % 64);
}

// where a removed row p goes: behind the `kept` rows, in row order
HONU_COMPACT_FN uint64_t compact_removed_dst(uint64_t kept, uint64_t p, uint64_t kept_before) {
    return kept + (p - kept_before);
}

// The clamps. The mark's own masks and counts never meet them: a mask or a
// count that is not the mark's may give wrong rows, never one outside the rows.
// a destination inside the rows, else the row stays where it is
HONU_COMPACT_FN uint64_t compact_dst_or_stay(uint64_t dst, uint64_t rows, uint64_t p) { return dst < rows ? dst : p; }
// a rank is no more than its bound (a kept row's own position, the kept total)
HONU_COMPACT_FN uint64_t compact_at_most(uint64_t rank, uint64_t bound) { return rank < bound ? rank : bound; }
// a slot that is written at all
HONU_COMPACT_FN int compact_inside(uint64_t slot, uint64_t rows) { return slot < rows; }
