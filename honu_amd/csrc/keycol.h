// keycol.h — what the kernels over the ordered key column share: the sort
// (sort.hip), the seek (seek.hip), the merge (merge.hip), the delete
// (delete.hip), the list (list.hip), the filter (filter.hip), the version
// assignment (next.hip), the comparison of two columns (compare.hip) and the
// reclaim (reclaim.hip). The compaction that delete, filter and reclaim share
// is compact.h's.
//   the packed key  a 29-byte key as 32 bytes read as eight big-endian words,
//                   byte 0 the validity (0 valid, 1 not), bytes 1-29 the key,
//                   bytes 30-31 zero. An unsigned compare of the words from
//                   word 0 down is bytes.Compare of the keys;
//   rows            a key moved as its bytes, the counts and indices read on
//                   the device clamped to the rows, the 9-word row in LDS;
//   searches        the leading positions of a bracket that say yes to a
//                   predicate, by a wave (64 mids per step) or by a thread;
//   the peer range  the rows of a second sorted column that a workgroup's
//                   tile can match, found once per workgroup and staged in
//                   LDS when short (peer_range: delete.hip, compare.hip).
#pragma once

#include "common.h"

#define HONU_BRACKET_FN HONU_DEV
#include "bracket.h"

namespace honu {

constexpr int SORT_KEY_WORDS = 8;

// byte j (0..28) of a key loaded as its bytes [0,16) in a and [13,29) in b
HONU_DEV uint32_t key_byte(const u32x4 &a, const u32x4 &b, int j) {
    return j < 16 ? (a[j >> 2] >> (8 * (j & 3))) & 0xFFu : (b[(j - 13) >> 2] >> (8 * ((j - 13) & 3))) & 0xFFu;
}

// the key at k (any byte address): two overlapping 16-byte loads, bytes [0,16)
// and [13,29), cover the 29 bytes and not one more; stored the same way
HONU_DEV void load_key(const uint8_t *k, u32x4 &a, u32x4 &b) {
    a = *reinterpret_cast<const u32x4u *>(k);
    b = *reinterpret_cast<const u32x4u *>(k + 13);
}

HONU_DEV void store_key(uint8_t *out, const u32x4 &a, const u32x4 &b) {
    *reinterpret_cast<u32x4u *>(out) = a;
    *reinterpret_cast<u32x4u *>(out + 13) = b;
}

// a row moved as its bytes, both loads before the stores
HONU_DEV void copy_key(uint8_t *dst, const uint8_t *src) {
    u32x4 a, b;
    load_key(src, a, b);
    store_key(dst, a, b);
}

// the packed form of the key at k
HONU_DEV void pack_key(const uint8_t *k, bool valid, uint32_t w[SORT_KEY_WORDS]) {
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] = 0;
    if (!valid) {  // equal among themselves, so they keep their index order, and after every valid key
        w[0] = 1u << 24;
        return;
    }
    u32x4 a, b;
    load_key(k, a, b);
#pragma unroll
    for (int j = 0; j < HONU_KEY_LEN; j++) {
        const int pb = j + 1;  // packed byte
        w[pb >> 2] |= key_byte(a, b, j) << (8 * (3 - (pb & 3)));
    }
}

// the packed key -> its 29 bytes at out: key bytes [0,16) and [13,29) as
// little-endian words (key byte j is packed byte j + 1)
HONU_DEV void unpack_key(uint8_t *out, const uint32_t w[SORT_KEY_WORDS]) {
    uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int pa = j + 1, pb = j + 14;
        a[j >> 2] |= ((w[pa >> 2] >> (8 * (3 - (pa & 3)))) & 0xFFu) << (8 * (j & 3));
        b[j >> 2] |= ((w[pb >> 2] >> (8 * (3 - (pb & 3)))) & 0xFFu) << (8 * (j & 3));
    }
    store_key(out, u32x4{a[0], a[1], a[2], a[3]}, u32x4{b[0], b[1], b[2], b[3]});
}

// the packed words' mask of a probe_len-byte prefix (seek.hip, delete.hip): key byte j is packed byte j + 1
struct SeekMask {
    uint32_t w[SORT_KEY_WORDS];
};

inline SeekMask seek_mask(uint32_t probe_len) {
    SeekMask M;
    for (int i = 0; i < SORT_KEY_WORDS; i++) {
        M.w[i] = 0;
        for (int b = 0; b < 4; b++)
            if ((uint32_t)(4 * i + b) < probe_len + 1) M.w[i] |= 0xFFu << (8 * (3 - b));
    }
    return M;
}

HONU_DEV void load_masked(const uint8_t *k, const SeekMask &M, uint32_t w[SORT_KEY_WORDS]) {
    pack_key(k, true, w);
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] &= M.w[i];
}

// bytes.Compare of two packed keys: -1, 0, 1 (word 0 is the most significant)
HONU_DEV int cmp_packed(const uint32_t a[SORT_KEY_WORDS], const uint32_t b[SORT_KEY_WORDS]) {
    int c = 0;
#pragma unroll
    for (int i = SORT_KEY_WORDS - 1; i >= 0; i--) c = a[i] != b[i] ? (a[i] < b[i] ? -1 : 1) : c;
    return c;
}

// a < b (or_equal: a <= b) by bytes.Compare
HONU_DEV bool packed_before(const uint32_t a[SORT_KEY_WORDS], const uint32_t b[SORT_KEY_WORDS], bool or_equal) {
    bool lt = or_equal;
#pragma unroll
    for (int i = SORT_KEY_WORDS - 1; i >= 0; i--) lt = a[i] != b[i] ? a[i] < b[i] : lt;
    return lt;
}

HONU_DEV bool packed_same(const uint32_t a[SORT_KEY_WORDS], const uint32_t b[SORT_KEY_WORDS]) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) eq = eq && a[i] == b[i];
    return eq;
}

// a count read on the device, clamped to the n rows it counts (N: n's width)
template <typename N> HONU_DEV N valid_rows(const uint64_t *valid, N n) { return (N)(*valid < n ? *valid : n); }

// an index is below n in an order honu_sort_keys wrote; whatever else it holds reads row n - 1 (n >= 1)
template <typename N> HONU_DEV N order_index(uint32_t i, N n) { return i < n ? i : n - 1; }

// a packed key staged in LDS with one word beside it: 9 words per row, an odd
// stride, so rows r and r + 1 lie in different banks
constexpr uint32_t KEY_ROW_WORDS = SORT_KEY_WORDS + 1;

HONU_DEV void lds_row_store(uint32_t *rows, uint32_t r, const uint32_t w[SORT_KEY_WORDS]) {
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) rows[r * KEY_ROW_WORDS + i] = w[i];
}

HONU_DEV void lds_row_load(const uint32_t *rows, uint32_t r, uint32_t w[SORT_KEY_WORDS]) {
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] = rows[r * KEY_ROW_WORDS + i];
}

// The first position of [lo, hi) that does not say yes, hi when all do: for a
// monotone predicate (yes up to a bound, no from it) the bound. Called by a
// whole wave with uniform lo and hi. A bisection whose every step is a round
// trip to memory would take 20 of them over 1M rows, so each step the lanes
// ask up to 64 evenly spaced mids at once (bracket.h) and the ballot's count t
// stands for "the first t said yes". yes(mid) is asked for lo <= mid < hi
// only; lanes past the bracket answer no.
// The invariant, for any answers whatsoever (garbage in device memory makes
// them so): a step takes [lo, hi) to [lo', hi') with lo <= lo' <= hi' <= hi
// and hi' - lo' < hi - lo, because t <= min(s, 64), mid(t - 1) + 1 <= mid(t)
// and mid(64) would be hi. So every mid asked lies in the caller's bracket and
// the loop ends: a bracket of s <= 64 rows in one step, one of s > 64 rows
// leaves at most ceil(s / 64) - 1, so no more than the least k >= 1 with
// 64^k >= s steps, 6 for any 32-bit bracket (four over 1M rows).
template <typename Yes> HONU_DEV uint32_t wave_bound(uint32_t lo, uint32_t hi, Yes yes) {
    const uint32_t lane = lane_id();
    while (lo < hi) {  // (wave-uniform)
        const uint32_t s = hi - lo;
        const bool y = lane < s && yes(bracket_mid(lo, s, lane));
        bracket_step(&lo, &hi, (uint32_t)__popcll(__ballot(y)));  // the first t lanes
    }
    return lo;
}

// The same by one thread, a bisection: lo <= the result <= hi and every mid
// asked lies in [lo, hi), whatever the answers
template <typename Yes> HONU_DEV uint32_t thread_bound(uint32_t lo, uint32_t hi, Yes yes) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (yes(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The rows of a sorted peer column that any row of a workgroup's tile can
// match (delete.hip: the delete list; compare.hip: the peer's column): the
// tile's rows ascend, so they are one range [lo, lo + dn), and it is staged in
// the caller's LDS rows (the 9-word row) when it has no more than `stage` of
// them. load gives row `at` of the range in pack's form, out of LDS when it
// is staged and through pack when it is not.
template <typename Pack> struct PeerRange {
    uint32_t lo, dn;
    bool staged;  // (block-uniform)
    const uint32_t *rows;
    Pack pack;
    HONU_DEV void load(uint32_t at, uint32_t d[SORT_KEY_WORDS]) const {
        if (staged) lds_row_load(rows, at, d);
        else pack(lo + at, d);
    }
};

// By the whole workgroup, with a barrier after each of its two steps when the
// step runs. The two ends are found once, a wave each (wave_bound over the
// masked keys of the peer's first n rows): end_key(last, k) gives the masked
// key of the tile's first row, or of its last, and n == 0 says there is none.
// pack(at, d) gives row `at` of the peer as it is staged, `rows` holds `stage`
// rows at least.
static_assert(HONU_WAVES_PER_BLOCK >= 2, "a wave for each end of the range");
template <typename EndKey, typename Pack>
HONU_DEV PeerRange<Pack> peer_range(EndKey end_key, const uint8_t *__restrict__ peer, uint32_t n, const SeekMask &M,
                                    Pack pack, uint32_t stage, uint32_t *rows) {
    __shared__ uint32_t range[2];
    const uint32_t wv = wave_in_block(), lane = lane_id();
    uint32_t lo = 0, hi = 0;
    if (n) {  // (block-uniform)
        if (threadIdx.x < 2 * HONU_WAVE) {
            uint32_t k[SORT_KEY_WORDS];
            end_key(wv != 0, k);
            const uint32_t b = wave_bound(0, n, [&](uint32_t mid) {  // wave 0 the lower bound, wave 1 the upper
                uint32_t d[SORT_KEY_WORDS];
                load_masked(peer + (uint64_t)HONU_KEY_LEN * mid, M, d);
                return packed_before(d, k, wv != 0);
            });
            if (lane == 0) range[wv] = b;
        }
        __syncthreads();
        lo = range[0];                       // <= n
        hi = range[1] < lo ? lo : range[1];  // <= n (lo <= hi over sorted columns)
    }
    const uint32_t dn = hi - lo;
    const bool staged = dn <= stage;
    if (dn && staged) {  // (block-uniform)
        for (uint32_t r = threadIdx.x; r < dn; r += HONU_BLOCK) {
            uint32_t d[SORT_KEY_WORDS];
            pack(lo + r, d);
            lds_row_store(rows, r, d);
        }
        __syncthreads();
    }
    return {lo, dn, staged, rows, pack};
}

// Both bounds of a probe by one thread (seek.hip, next.hip): the lower bound's
// loop notes what each key it loads says about the upper bound, so the upper
// bound's own loop starts from what is left (nothing, for a probe that is not
// stored). pos: the first position in [lo, hi] whose key is >= p; end: the
// first in [ulo, uhi] whose key is > p. The caller knows both brackets to hold
// their answer; a position equal to a bracket's upper end is never loaded.
// load(i, k) gives the masked packed key at position i.
template <typename Load>
HONU_DEV void seek_bounds(Load load, const uint32_t p[SORT_KEY_WORDS], uint32_t lo, uint32_t hi, uint32_t ulo,
                          uint32_t uhi, uint32_t &pos, uint32_t &end) {
    uint32_t k[SORT_KEY_WORDS];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        load(mid, k);
        const int c = cmp_packed(k, p);
        if (c < 0) lo = mid + 1;
        else hi = mid;
        // what the same key says about the upper bound
        if (c > 0) uhi = uhi < mid ? uhi : mid;
        else ulo = ulo > mid + 1 ? ulo : mid + 1;
    }
    pos = lo;
    ulo = ulo > pos ? ulo : pos;
    while (ulo < uhi) {
        const uint32_t mid = ulo + ((uhi - ulo) >> 1);
        load(mid, k);
        if (cmp_packed(k, p) <= 0) ulo = mid + 1;
        else uhi = mid;
    }
    end = ulo;
}

// one honu_seek row (seek.hip, compare.hip) as five plain 4-byte stores
HONU_DEV void seek_store(honu_seek *out, uint32_t pos, uint32_t end, uint32_t first, uint32_t latest,
                         uint32_t flags) {
    uint32_t *q = reinterpret_cast<uint32_t *>(out);
    q[0] = pos;
    q[1] = end;
    q[2] = first;
    q[3] = latest;
    q[4] = flags;
}

}  // namespace honu
