// seek.hip — Cursor.Seek (iterator/cursor.go:44-55) for a batch of probes over
// the sorted key column honu_sort_keys writes: the step every read of the
// store starts from (Collection.Has / Exists, collection.go:47-65), and the two
// ends of an object's range [ObjectPrefix, ObjectLimit) (keys/keys.go:73-92).
//
// A probe is the first probe_len bytes of a 29-byte row. Keys and probes are
// compared in the sort's packed form (keycol.h) under a mask that clears the
// bytes past probe_len: big-endian words, unsigned, which is bytes.Compare of
// the probe_len-byte prefixes. A key that has the probe as a proper prefix is
// greater than the probe, so Seek's position is the lower bound over the
// prefixes, and the position past the probe's last key the upper bound.
//
// Two forms, one probe per lane in both:
//   direct  binary search straight over the column;
//   fenced  every workgroup first samples SEEK_FENCE evenly spaced keys into
//           LDS (packed and masked, 32 bytes each), resolves the top levels
//           of each search there and only the rest in global memory; the
//           workgroup takes its probes in a grid-stride loop.
// Both bounds come out of one routine: the lower bound's loop notes what each
// key it loads says about the upper bound, so the upper bound's own loop
// starts from what is left (nothing, for a probe that is not stored).
// No atomics, no spin-wait, no state outside the launch.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t SEEK_FENCE_LOG2 = 10;
constexpr uint32_t SEEK_FENCE = 1u << SEEK_FENCE_LOG2;  // 1024 keys x 32 bytes: 32 KiB, four workgroups per CU
// seek_variant 0: the direct form for fewer probes than this over more rows
// than that (the host knows n, not the valid count, which stays on the
// device), the fenced form otherwise. Measured: the fence's
// SEEK_FENCE scattered row reads cost a lone workgroup 0.5 us over a 1M-row
// column, which is beyond L2, and 64 probes do not earn that back, 1024 do;
// over a column that L2 holds (4 K and 64 K rows) the fence wins from 64 probes.
constexpr uint64_t SEEK_AUTO_PROBES = 1024;
constexpr uint64_t SEEK_AUTO_KEYS = 65536;

uint32_t seek_fence() { return SEEK_FENCE; }
uint64_t seek_auto_probes() { return SEEK_AUTO_PROBES; }
uint64_t seek_auto_keys() { return SEEK_AUTO_KEYS; }

HONU_DEV void seek_finish(honu_seek *out, uint32_t pos, uint32_t end, uint32_t valid, uint64_t n,
                          uint32_t probe_len, const uint32_t *__restrict__ order,
                          const honu_record_info *__restrict__ info) {
    uint32_t flags = pos == valid ? (uint32_t)HONU_SEEK_END : 0u;
    uint32_t first = HONU_SEEK_NONE, latest = HONU_SEEK_NONE;
    if (pos < end) {
        flags |= HONU_SEEK_FOUND;
        if (probe_len == HONU_KEY_LEN) flags |= HONU_SEEK_EXACT;
        if (order) {
            first = order[pos];
            latest = order[end - 1];
            if (info) {
                const uint64_t i = order_index(first, n), j = order_index(latest, n);  // (both rows' loads in flight)
                if (!info[i].tombstone) flags |= HONU_SEEK_FIRST_LIVE;
                if (!info[j].tombstone) flags |= HONU_SEEK_LATEST_LIVE;
            }
        }
    }
    seek_store(out, pos, end, first, latest, flags);
}

__global__ __launch_bounds__(HONU_BLOCK) void k_seek_direct(
    const uint8_t *__restrict__ sorted, const uint64_t *__restrict__ valid, uint64_t n,
    const uint8_t *__restrict__ probes, const int32_t *__restrict__ pstatus, uint32_t probe_len, SeekMask M,
    uint64_t m, const uint32_t *__restrict__ order, const honu_record_info *__restrict__ info,
    honu_seek *__restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (q >= m) return;
    if (pstatus && pstatus[q] != HONU_OK) {
        seek_store(out + q, 0, 0, HONU_SEEK_NONE, HONU_SEEK_NONE, HONU_SEEK_SKIPPED);
        return;
    }
    const uint32_t v = (uint32_t)valid_rows(valid, n);
    uint32_t p[SORT_KEY_WORDS];
    load_masked(probes + HONU_KEY_LEN * q, M, p);
    uint32_t pos, end;
    seek_bounds([&](uint32_t i, uint32_t k[SORT_KEY_WORDS]) { load_masked(sorted + (uint64_t)HONU_KEY_LEN * i, M, k); },
                p, 0, v, 0, v, pos, end);
    seek_finish(out + q, pos, end, v, n, probe_len, order, info);
}

// The fence holds the keys at positions s(i) = floor(i * valid / SEEK_FENCE),
// i < SEEK_FENCE (every key, s(i) = i, when there are no more than that);
// s(count) = valid stands for the end. c fence keys below the probe put the
// lower bound in [s(c - 1) + 1, s(c)], and likewise the upper bound.
__global__ __launch_bounds__(HONU_BLOCK) void k_seek_fenced(
    const uint8_t *__restrict__ sorted, const uint64_t *__restrict__ valid, uint64_t n,
    const uint8_t *__restrict__ probes, const int32_t *__restrict__ pstatus, uint32_t probe_len, SeekMask M,
    uint64_t m, const uint32_t *__restrict__ order, const honu_record_info *__restrict__ info,
    honu_seek *__restrict__ out) {
    __shared__ u32x4 fence[SEEK_FENCE][2];
    const uint32_t v = (uint32_t)valid_rows(valid, n);
    const bool sampled = v > SEEK_FENCE;
    const uint32_t fe = sampled ? SEEK_FENCE : v;
    auto at = [&](uint32_t i) -> uint32_t {
        return sampled ? (uint32_t)(((uint64_t)i * v) >> SEEK_FENCE_LOG2) : i;
    };
    for (uint32_t i = threadIdx.x; i < fe; i += HONU_BLOCK) {
        uint32_t w[SORT_KEY_WORDS];
        load_masked(sorted + (uint64_t)HONU_KEY_LEN * at(i), M, w);
        fence[i][0] = u32x4{w[0], w[1], w[2], w[3]};
        fence[i][1] = u32x4{w[4], w[5], w[6], w[7]};
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * HONU_BLOCK;
    for (uint64_t q = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x; q < m; q += stride) {
        if (pstatus && pstatus[q] != HONU_OK) {
            seek_store(out + q, 0, 0, HONU_SEEK_NONE, HONU_SEEK_NONE, HONU_SEEK_SKIPPED);
            continue;
        }
        uint32_t p[SORT_KEY_WORDS];
        load_masked(probes + HONU_KEY_LEN * q, M, p);
        uint32_t c, u;  // fence keys below the probe / not above it
        seek_bounds(
            [&](uint32_t i, uint32_t k[SORT_KEY_WORDS]) {
                const u32x4 a = fence[i][0], b = fence[i][1];
                k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w;
                k[4] = b.x, k[5] = b.y, k[6] = b.z, k[7] = b.w;
            },
            p, 0, fe, 0, fe, c, u);
        uint32_t pos, end;
        seek_bounds([&](uint32_t i, uint32_t k[SORT_KEY_WORDS]) { load_masked(sorted + (uint64_t)HONU_KEY_LEN * i, M, k); },
                    p, c ? at(c - 1) + 1 : 0, at(c), u ? at(u - 1) + 1 : 0, at(u), pos, end);
        seek_finish(out + q, pos, end, v, n, probe_len, order, info);
    }
}

hipError_t launch_key_seek(int variant, int num_cu, const uint8_t *sorted, const uint64_t *valid, uint64_t n,
                           const uint8_t *probes, const int32_t *pstatus, uint32_t probe_len, uint64_t m,
                           const uint32_t *order, const honu_record_info *info, honu_seek *out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const SeekMask M = seek_mask(probe_len);
    const uint64_t blocks = (m + HONU_BLOCK - 1) / HONU_BLOCK;
    const bool fenced = variant ? variant == 2 : m >= SEEK_AUTO_PROBES || n <= SEEK_AUTO_KEYS;
    if (fenced) {
        // four 32 KiB workgroups fit a CU's 160 KiB of LDS
        const uint64_t resident = 4ull * (uint64_t)(num_cu > 0 ? num_cu : 1);
        hipLaunchKernelGGL(k_seek_fenced, dim3((unsigned)(blocks < resident ? blocks : resident)), dim3(HONU_BLOCK),
                           0, s, sorted, valid, n, probes, pstatus, probe_len, M, m, order, info, out);
    } else {
        hipLaunchKernelGGL(k_seek_direct, dim3((unsigned)blocks), dim3(HONU_BLOCK), 0, s, sorted, valid, n, probes,
                           pstatus, probe_len, M, m, order, info, out);
    }
    return hipGetLastError();
}

}  // namespace honu
