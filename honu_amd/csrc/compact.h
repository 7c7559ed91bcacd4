// compact.h — the stable stream compaction that delete.hip, filter.hip and
// reclaim.hip share: a workgroup per TILE rows, three steps.
//   mark   compact_mark: the tile's keep masks, one ballot per 64 rows, and
//          its kept count, from the caller's keep(j, t);
//   scan   launch_scan over the tiles' kept counts, in place: the caller's;
//   place  compact_ranks: the tile's masks and their popcount prefix in LDS.
//          A row's rank in its tile is a popcount of the masks below it, a
//          kept row goes to kept_before_tile + rank; what is written there,
//          and where a removed row goes, is the caller's loop.
// The workspace holds the keep masks (WORDS words per tile), then the kept
// counts (a word per tile). No atomics, no spin-wait and no state outside the
// launch. The arithmetic is compact_rank.h's.
#pragma once

#include "kernels.h"

#define HONU_COMPACT_FN HONU_DEV
#include "compact_rank.h"

namespace honu {

template <uint32_t TILE> struct CompactTile {
    static constexpr uint32_t WORDS = TILE / HONU_WAVE;               // ballots per tile
    static constexpr uint32_t ROUNDS = WORDS / HONU_WAVES_PER_BLOCK;  // ballots per wave
    static_assert(TILE % (HONU_WAVE * HONU_WAVES_PER_BLOCK) == 0, "a wave takes whole ballots");
    static_assert(WORDS <= HONU_BLOCK, "a thread per ballot in the place kernel");
};

struct CompactWork {
    uint64_t *mask;
    uint64_t *kept;
};

template <uint32_t TILE> uint64_t compact_tiles(uint64_t rows) { return (rows + TILE - 1) / TILE; }

template <uint32_t TILE> uint64_t compact_workspace_bytes(uint64_t rows) {
    const uint64_t tiles = compact_tiles<TILE>(rows);
    return up256(8 * CompactTile<TILE>::WORDS * tiles) + up256(8 * tiles);
}

template <uint32_t TILE> CompactWork compact_carve(void *work, uint64_t rows) {
    const uint64_t masks = up256(8 * CompactTile<TILE>::WORDS * compact_tiles<TILE>(rows));
    return {(uint64_t *)work, (uint64_t *)((uint8_t *)work + masks)};
}

// The mark of tile `tile` by its whole workgroup: W.mask gets the tile's
// ballots of keep(j, t), t = 64 j + lane the row in the tile, and W.kept its
// kept count. Every lane of every wave calls keep, ROUNDS times, in
// convergent control flow: keep may shuffle across the wave and may branch on
// j, which is wave-uniform. A row past the tile's rows answers false.
template <uint32_t TILE, typename Keep> HONU_DEV void compact_mark(const CompactWork &W, uint32_t tile, Keep keep) {
    using T = CompactTile<TILE>;
    __shared__ uint32_t cnt[HONU_WAVES_PER_BLOCK];
    const uint32_t wv = wave_in_block(), lane = lane_id();
    uint32_t kept = 0;
    for (uint32_t r = 0; r < T::ROUNDS; r++) {
        const uint32_t j = r * HONU_WAVES_PER_BLOCK + wv;  // the tile's ballot: rows [64 j, 64 j + 64)
        const uint64_t bits = __ballot(keep(j, j * HONU_WAVE + lane));
        if (lane == 0) W.mask[(uint64_t)tile * T::WORDS + j] = bits;
        kept += (uint32_t)__popcll(bits);
    }
    if (lane == 0) cnt[wv] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) sum += cnt[w];
        W.kept[tile] = sum;
    }
}

// A tile's masks as the place kernels read them. base: W.kept scanned, the
// rows kept before the tile
struct CompactRanks {
    const uint64_t *msk;
    const uint32_t *pre;  // rows kept in the tile's ballots before ballot j
    uint64_t base;
    HONU_DEV bool kept_bit(uint32_t j, uint32_t lane) const { return (msk[j] >> lane) & 1ull; }
    // the rows kept before row 64 j + lane, in all tiles
    HONU_DEV uint64_t kept_before(uint32_t j, uint32_t lane) const {
        return compact_rank_lane(base + pre[j], msk[j], lane);
    }
};

// by the whole workgroup (two barriers)
template <uint32_t TILE> HONU_DEV CompactRanks compact_ranks(const CompactWork &W, uint32_t tile) {
    using T = CompactTile<TILE>;
    __shared__ uint64_t msk[T::WORDS];
    __shared__ uint32_t pre[T::WORDS];
    if (threadIdx.x < T::WORDS) msk[threadIdx.x] = W.mask[(uint64_t)tile * T::WORDS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < T::WORDS) pre[threadIdx.x] = compact_words_before(msk, threadIdx.x);
    __syncthreads();
    return {msk, pre, W.kept[tile]};
}

}  // namespace honu
