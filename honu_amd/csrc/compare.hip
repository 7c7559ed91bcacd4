// compare.hip — the versions of two sorted key columns compared object by
// object: the step of a replication between "concatenated Objects + an offset
// table" and the walk that gathers them. A lamport.Scalar "uses a 'latest
// writer wins' policy to determine how to solve conflicts"
// (lamport/scalar.go:15-24), lamport.Compare is the happens-before test
// (scalar.go:47-78), and a key stores the version big endian "to maintain
// lexicographic sorting" (keys/keys.go:35-36): bytes.Compare of two keys of one
// object is lamport.Compare of their versions. A is the local column with its
// objects (honu_key_objects), B the peer's column or its digest.
//
// For object j of A with rows [a0, a1) and latest key K = A[a1 - 1], the rows
// [b0, b1) of B are those whose first 17 bytes are K's, and only B[b1 - 1], the
// peer's latest, decides: K against it gives LATER / EARLIER / EQUAL, the
// upper bound of it in [a0, a1) the rows [pos, end) the peer is behind by, and
// an equality at the older side's latest row says the histories have not
// forked. The row is a honu_seek row, so honu_key_list walks the result.
//
// Two launches:
//   compare  a workgroup per COMPARE_TILE consecutive objects, a thread per
//            object (the grid comes from na; a workgroup past `objects` leaves
//            at once). The rows of B that any of the tile's objects can match
//            are one range (keycol.h's peer_range over the 17-byte mask),
//            staged as whole keys in LDS when it has no more than `stage` rows
//            (COMPARE_STAGE) and masked on use; a longer one is searched in
//            global memory inside the range. A thread then takes both
//            bounds of its prefix in the range (seek_bounds), compares the full
//            packed keys, bisects [a0, a1 - 1) when it is ahead (thread_bound),
//            and tests the ancestor row. The tile's class counts, a ballot per
//            class and wave, go to the workspace;
//   sum      one workgroup adds the tiles' counts (d_counts given only).
// No atomics, no spin-wait and no state outside the launch, so the sums are
// the same every time. Every position derived from a count or offset read on
// the device is clamped to the va / vb rows: garbage in d_obj_off, d_objects or
// the valid counts may give wrong rows, never an access outside the na / nb
// rows or a search that does not end.
#include "kernels.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t COMPARE_TILE = HONU_BLOCK;  // objects per workgroup: a thread each
constexpr uint32_t COMPARE_STAGE = 1024;       // rows of B a workgroup stages
// 1024 x 36 bytes: 36 KiB, four workgroups (16 waves) per CU of 160 KiB, as delete.hip's mark kernel; a tile
// of 256 objects whose peer holds up to four versions of each stays on the staged path
constexpr uint32_t COMPARE_CLASSES = 5;      // only mine, later and the peer has it, earlier, equal, forks
constexpr uint32_t COMPARE_PART_WORDS = 8;   // a tile's counts in the workspace: the classes, then zeros
static_assert(COMPARE_PART_WORDS >= COMPARE_CLASSES && COMPARE_PART_WORDS <= HONU_WAVE, "a lane per word");

uint32_t compare_tile() { return COMPARE_TILE; }
uint32_t compare_stage() { return COMPARE_STAGE; }
static uint64_t compare_tiles(uint64_t na) { return (na + COMPARE_TILE - 1) / COMPARE_TILE; }

// the tiles' counts
uint64_t compare_workspace_bytes(uint64_t na) { return up256(4 * COMPARE_PART_WORDS * compare_tiles(na)); }

struct CompareArgs {
    const uint8_t *a;  // the local column
    const uint32_t *order_a;
    const uint64_t *valid_a;
    uint32_t na;
    const uint64_t *obj_off;
    const uint64_t *objects;
    const uint8_t *b;  // the peer's
    const uint64_t *valid_b;
    uint32_t nb;
    uint32_t stage;  // <= COMPARE_STAGE
};

// the rows [a0, a1) of object j (j < objects <= na: d_obj_off has na + 1 values), inside [0, va]
HONU_DEV void compare_object(const CompareArgs &C, uint32_t j, uint32_t va, uint32_t &a0, uint32_t &a1) {
    const uint64_t o0 = C.obj_off[j], o1 = C.obj_off[(uint64_t)j + 1];
    a1 = o1 < va ? (uint32_t)o1 : va;
    a0 = o0 < a1 ? (uint32_t)o0 : a1;
}

__global__ __launch_bounds__(HONU_BLOCK) void k_compare(CompareArgs C, SeekMask M, honu_seek *__restrict__ out,
                                                         uint32_t *__restrict__ peer, uint32_t *__restrict__ part) {
    __shared__ uint32_t rows[COMPARE_STAGE * KEY_ROW_WORDS];
    __shared__ uint32_t cnt[HONU_WAVES_PER_BLOCK][COMPARE_PART_WORDS];
    const uint32_t objects = valid_rows(C.objects, C.na);
    const uint32_t j0 = blockIdx.x * COMPARE_TILE;  // below na
    if (j0 >= objects) return;                      // (block-uniform)
    const uint32_t len = objects - j0 < COMPARE_TILE ? objects - j0 : COMPARE_TILE;
    const uint32_t va = valid_rows(C.valid_a, C.na), vb = C.nb ? valid_rows(C.valid_b, C.nb) : 0;
    const uint32_t wv = wave_in_block(), lane = lane_id();

    // the rows of B that an object of the tile can match, staged as their whole keys
    const auto R = peer_range(
        [&](bool last, uint32_t k[SORT_KEY_WORDS]) {  // the latest key of the tile's first or last object
            uint32_t a0, a1;
            compare_object(C, last ? j0 + len - 1 : j0, va, a0, a1);
            load_masked(C.a + (uint64_t)HONU_KEY_LEN * (a1 ? a1 - 1 : 0), M, k);
        },
        C.b, va ? vb : 0, M,
        [&](uint32_t at, uint32_t d[SORT_KEY_WORDS]) { pack_key(C.b + (uint64_t)HONU_KEY_LEN * at, true, d); }, C.stage,
        rows);
    const uint32_t lo = R.lo, dn = R.dn;

    const uint32_t t = threadIdx.x;
    uint32_t cls = COMPARE_CLASSES;  // none: a thread past the tile
    bool fork = false;
    if (t < len) {
        const uint32_t j = j0 + t;
        uint32_t a0, a1;
        compare_object(C, j, va, a0, a1);
        uint32_t pos = a0, flags = 0, at_peer = HONU_SEEK_NONE;
        if (a1) {  // (an object has a row: a1 == 0 comes of garbage alone and gets an empty row)
            uint32_t K[SORT_KEY_WORDS], k[SORT_KEY_WORDS], pb[SORT_KEY_WORDS], d[SORT_KEY_WORDS];
            pack_key(C.a + (uint64_t)HONU_KEY_LEN * (a1 - 1), true, K);
#pragma unroll
            for (int i = 0; i < SORT_KEY_WORDS; i++) k[i] = K[i] & M.w[i];
            uint32_t b0 = 0, b1 = 0;
            if (dn)
                seek_bounds(
                    [&](uint32_t at, uint32_t x[SORT_KEY_WORDS]) {
                        R.load(at, x);
#pragma unroll
                        for (int i = 0; i < SORT_KEY_WORDS; i++) x[i] &= M.w[i];
                    },
                    k, 0, dn, 0, dn, b0, b1);
            if (b0 < b1) {
                flags |= HONU_CMP_PEER_HAS;
                at_peer = lo + b1 - 1;
                R.load(b1 - 1, pb);
                const int c = cmp_packed(K, pb);
                bool ancestor = true;
                if (c > 0) {  // the first row above the peer's latest: K is above it, so at most a1 - 1
                    pos = thread_bound(a0, a1 - 1, [&](uint32_t mid) {
                        pack_key(C.a + (uint64_t)HONU_KEY_LEN * mid, true, d);
                        return packed_before(d, pb, true);
                    });
                    ancestor = false;
                    if (pos > a0) {
                        pack_key(C.a + (uint64_t)HONU_KEY_LEN * (pos - 1), true, d);
                        ancestor = packed_same(d, pb);
                    }
                    flags |= HONU_CMP_LATER;
                    cls = 1;
                } else if (c < 0) {  // K among the peer's rows: its lower bound in [b0, b1 - 1), then equality
                    pos = a1;
                    const uint32_t at = thread_bound(b0, b1 - 1, [&](uint32_t mid) {
                        R.load(mid, d);
                        return packed_before(d, K, false);
                    });
                    R.load(at, d);  // (at <= b1 - 1)
                    ancestor = packed_same(d, K);
                    flags |= HONU_CMP_EARLIER;
                    cls = 2;
                } else {
                    pos = a1;
                    flags |= HONU_CMP_EQUAL;
                    cls = 3;
                }
                if (ancestor) flags |= HONU_CMP_ANCESTOR;
                fork = !ancestor;
            } else {
                flags |= HONU_CMP_LATER;
                cls = 0;
            }
        }
        uint32_t first = HONU_SEEK_NONE, latest = HONU_SEEK_NONE;
        if (pos < a1) {
            flags |= HONU_SEEK_FOUND;
            if (C.order_a) {
                first = C.order_a[pos];
                latest = C.order_a[a1 - 1];
            }
        }
        seek_store(out + j, pos, a1, first, latest, flags);
        if (peer) peer[j] = at_peer;
    }

    // the tile's counts: a ballot per class, the waves' counts added by one lane per word
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t c = 0; c < COMPARE_CLASSES; c++) {
        const uint32_t got = (uint32_t)__popcll(__ballot(c + 1 < COMPARE_CLASSES ? cls == c : fork));
        mine = lane == c ? got : mine;
    }
    if (lane < COMPARE_PART_WORDS) cnt[wv][lane] = mine;
    __syncthreads();
    if (t < COMPARE_PART_WORDS) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) sum += cnt[w][t];
        part[(uint64_t)blockIdx.x * COMPARE_PART_WORDS + t] = sum;
    }
}

// d_counts: the objects compared, the classes in the workspace's order, then zeros
__global__ __launch_bounds__(HONU_BLOCK) void k_compare_sum(const uint64_t *__restrict__ objects_p, uint32_t na,
                                                             const uint32_t *__restrict__ part,
                                                             uint64_t *__restrict__ counts) {
    __shared__ uint64_t acc[HONU_WAVES_PER_BLOCK][COMPARE_CLASSES];
    const uint32_t objects = valid_rows(objects_p, na);
    const uint32_t tiles = (uint32_t)(((uint64_t)objects + COMPARE_TILE - 1) / COMPARE_TILE);  // the ones that ran
    uint64_t s[COMPARE_CLASSES];
#pragma unroll
    for (uint32_t c = 0; c < COMPARE_CLASSES; c++) s[c] = 0;
    for (uint32_t tile = threadIdx.x; tile < tiles; tile += HONU_BLOCK)
#pragma unroll
        for (uint32_t c = 0; c < COMPARE_CLASSES; c++) s[c] += part[(uint64_t)tile * COMPARE_PART_WORDS + c];
    const uint32_t wv = wave_in_block(), lane = lane_id();
#pragma unroll
    for (uint32_t c = 0; c < COMPARE_CLASSES; c++) {
        const uint64_t w = wave_sum(s[c]);
        if (lane == 0) acc[wv][c] = w;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        uint64_t v = 0;
        if (threadIdx.x == 0) v = objects;
        else if (threadIdx.x <= COMPARE_CLASSES)
            for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) v += acc[w][threadIdx.x - 1];
        counts[threadIdx.x] = v;
    }
}

hipError_t launch_key_compare(const uint8_t *sa, const uint32_t *order_a, const uint64_t *valid_a, uint64_t na,
                              const uint64_t *obj_off, const uint64_t *objects, const uint8_t *sb,
                              const uint64_t *valid_b, uint64_t nb, uint32_t stage, honu_seek *out, uint32_t *peer,
                              uint64_t *counts, void *work, hipStream_t s) {
    if (na == 0) return counts ? hipMemsetAsync(counts, 0, 8 * sizeof(uint64_t), s) : hipSuccess;
    const CompareArgs C = {sa,      order_a, valid_a,     (uint32_t)na,
                           obj_off, objects, sb,          valid_b,
                           (uint32_t)nb,     stage < COMPARE_STAGE ? stage : COMPARE_STAGE};
    hipLaunchKernelGGL(k_compare, dim3((unsigned)compare_tiles(na)), dim3(HONU_BLOCK), 0, s, C, seek_mask(17), out, peer,
                       (uint32_t *)work);
    if (counts)
        hipLaunchKernelGGL(k_compare_sum, dim3(1), dim3(HONU_BLOCK), 0, s, objects, (uint32_t)na,
                           (const uint32_t *)work, counts);
    return hipGetLastError();
}

}  // namespace honu
