// keypack.h — the packed form of a 29-byte key, shared by the sort (sort.hip),
// the seek (seek.hip), the merge (merge.hip) and the delete (delete.hip): 32
// bytes read as eight big-endian words, byte 0 the validity (0 valid, 1 not),
// bytes 1-29 the key, bytes 30-31 zero. An unsigned compare of the words from
// word 0 down is bytes.Compare of the keys.
#pragma once

#include "common.h"

namespace honu {

constexpr int SORT_KEY_WORDS = 8;

// byte j (0..28) of a key loaded as its bytes [0,16) in a and [13,29) in b
HONU_DEV uint32_t key_byte(const u32x4 &a, const u32x4 &b, int j) {
    return j < 16 ? (a[j >> 2] >> (8 * (j & 3))) & 0xFFu : (b[(j - 13) >> 2] >> (8 * ((j - 13) & 3))) & 0xFFu;
}

// the packed form of the key at k (any byte address): two overlapping
// 16-byte loads cover the 29 bytes and not one more
HONU_DEV void pack_key(const uint8_t *k, bool valid, uint32_t w[SORT_KEY_WORDS]) {
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) w[i] = 0;
    if (!valid) {  // equal among themselves, so they keep their index order, and after every valid key
        w[0] = 1u << 24;
        return;
    }
    const u32x4 a = *reinterpret_cast<const u32x4u *>(k);
    const u32x4 b = *reinterpret_cast<const u32x4u *>(k + 13);
#pragma unroll
    for (int j = 0; j < HONU_KEY_LEN; j++) {
        const int pb = j + 1;  // packed byte
        w[pb >> 2] |= key_byte(a, b, j) << (8 * (3 - (pb & 3)));
    }
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

}  // namespace honu
