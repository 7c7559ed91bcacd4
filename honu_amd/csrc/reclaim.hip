// reclaim.hip — the space a Drop frees (store.go:314-322: "to free up space
// in the database"; the DeleteBucket of store.go:399-404, after which bbolt
// "marks the pages as free"): a compaction of the records arena and of every
// per-record array beside it. A record stays when a valid row of the column
// names it, d_order[p] == r for some p < v; the records that stay are
// renumbered 0 .. kept - 1 in ascending old index, so arrival order survives,
// and the column's order is rewritten to the new indices.
//
// compact.h's mark / scan / place over records, a workgroup per RECLAIM_TILE
// of them, then fetch.hip's lengths / scan / copy over the records that stay:
//   clear    hipMemsetAsync over the marks, a byte per record;
//   mark     a thread per column position p < v: marks[d_order[p]] = 1 when the
//            index is below nrec. Plain stores: the stores that race to one
//            mark all store the same byte;
//   count    the compaction's mark: a record stays when its mark is set;
//   scan     launch_scan over the tiles' counts, the total to d_kept;
//   place    a kept record's new index j is its rank: d_remap[r] = j,
//            d_source[j] = r, the record's key (copy_key), key status and info
//            row to row j, its checked length to d_rec_off_out[j] and its
//            status to d_status[j]. A freed record r writes HONU_SEEK_NONE to
//            d_remap[r] and the zero length of slot kept + (r - kept_before_r),
//            so the slots [kept, nrec) are all written; slot nrec is the first
//            thread's;
//   scan     launch_scan in place over the nrec + 1 lengths, the total to
//            d_val_total;
//   renumber a thread per column position: d_order_out[p] = remap[d_order[p]]
//            for p < v and an index below nrec, else HONU_SEEK_NONE;
//   copy     k_copy_segments<ReclaimSegments> (copy.hip) over nrec segments,
//            the new arena its logical byte space.
// The remap goes to d_remap or, without one, to the workspace. The kernels
// here have no atomics, no spin-wait and no state outside the launch either;
// launch_scan is the only step in which workgroups depend on each other. The
// grids come from n and nrec, never from a count on the device. An index read
// from d_order is checked against nrec before anything is read with it, and
// every offset pair against rec_bytes before its length counts.
#include "compact.h"
#include "keycol.h"

namespace honu {

constexpr uint32_t RECLAIM_TILE = 1024;  // records per workgroup

uint32_t reclaim_tile() { return RECLAIM_TILE; }

// the marks (a byte per record), the compaction's masks and counts, then the remap of a call without
// d_remap (a word per record)
uint64_t reclaim_workspace_bytes(uint64_t nrec) {
    return up256(nrec) + compact_workspace_bytes<RECLAIM_TILE>(nrec) + up256(4 * nrec);
}

struct ReclaimWork {
    uint8_t *marks;
    CompactWork c;
    uint32_t *remap;
};

static ReclaimWork reclaim_carve(void *work, uint64_t nrec) {
    uint8_t *at = (uint8_t *)work + up256(nrec);
    return {(uint8_t *)work, compact_carve<RECLAIM_TILE>(at, nrec),
            (uint32_t *)(at + compact_workspace_bytes<RECLAIM_TILE>(nrec))};
}

__global__ __launch_bounds__(HONU_BLOCK) void k_reclaim_mark(const uint32_t *__restrict__ order,
                                                              const uint64_t *__restrict__ valid, uint32_t n,
                                                              uint32_t nrec, uint8_t *__restrict__ marks) {
    const uint64_t p = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= valid_rows(valid, n)) return;
    const uint32_t r = order[p];
    if (r < nrec) marks[r] = 1;
}

__global__ __launch_bounds__(HONU_BLOCK) void k_reclaim_count(uint32_t nrec, ReclaimWork W) {
    const uint32_t r0 = blockIdx.x * RECLAIM_TILE;  // below nrec
    const uint32_t len = nrec - r0 < RECLAIM_TILE ? nrec - r0 : RECLAIM_TILE;
    compact_mark<RECLAIM_TILE>(W.c, blockIdx.x,
                               [&](uint32_t, uint32_t t) { return t < len && W.marks[(uint64_t)r0 + t] != 0; });
}

struct ReclaimArrays {
    const uint8_t *keys;
    const int32_t *key_status;
    const honu_record_info *info;
    uint8_t *keys_out;
    int32_t *key_status_out;
    honu_record_info *info_out;
};

// W.kept scanned (the records kept before the tile), *kept_total the total
__global__ __launch_bounds__(HONU_BLOCK) void k_reclaim_place(
    const uint64_t *__restrict__ rec_off, uint32_t nrec, uint64_t rec_bytes, ReclaimArrays A,
    const uint64_t *__restrict__ kept_total, uint32_t *__restrict__ remap, uint32_t *__restrict__ source,
    uint64_t *__restrict__ len_out, int32_t *__restrict__ status, ReclaimWork W) {
    const uint64_t kept = *kept_total < nrec ? *kept_total : nrec;
    if (blockIdx.x == 0 && threadIdx.x == 0) len_out[nrec] = 0;
    const uint32_t r0 = blockIdx.x * RECLAIM_TILE;  // below nrec
    const uint32_t len = nrec - r0 < RECLAIM_TILE ? nrec - r0 : RECLAIM_TILE;
    const CompactRanks K = compact_ranks<RECLAIM_TILE>(W.c, blockIdx.x);
    const uint32_t wv = wave_in_block(), lane = lane_id();
    for (uint32_t q = 0; q < CompactTile<RECLAIM_TILE>::ROUNDS; q++) {
        const uint32_t j = q * HONU_WAVES_PER_BLOCK + wv;
        const uint32_t t = j * HONU_WAVE + lane;
        if (t >= len) continue;
        const uint64_t r = (uint64_t)r0 + t;
        const uint64_t kept_before = K.kept_before(j, lane);
        if (!K.kept_bit(j, lane)) {
            remap[r] = HONU_SEEK_NONE;
            const uint64_t slot = compact_removed_dst(kept, r, kept_before);  // in [kept, nrec) with the count's masks
            if (compact_inside(slot, nrec)) len_out[slot] = 0;
            continue;
        }
        if (!compact_inside(kept_before, kept)) {  // (masks or a count that are not the count's)
            remap[r] = HONU_SEEK_NONE;
            continue;
        }
        const uint64_t d = kept_before;
        remap[r] = (uint32_t)d;
        source[d] = (uint32_t)r;
        const uint64_t a = rec_off[r], b = rec_off[r + 1];
        const bool ok = a <= b && b <= rec_bytes;
        len_out[d] = ok ? b - a : 0;
        if (status) status[d] = ok ? HONU_OK : HONU_ERR_INPUT;
        if (A.keys) copy_key(A.keys_out + (uint64_t)HONU_KEY_LEN * d, A.keys + (uint64_t)HONU_KEY_LEN * r);
        if (A.key_status) A.key_status_out[d] = A.key_status[r];
        if (A.info) {  // 32 bytes, verbatim; the rows are 8-byte aligned
            const uint64_t *src = reinterpret_cast<const uint64_t *>(A.info + r);
            uint64_t *dst = reinterpret_cast<uint64_t *>(A.info_out + d);
            const uint64_t w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3];
            dst[0] = w0;
            dst[1] = w1;
            dst[2] = w2;
            dst[3] = w3;
        }
    }
}
static_assert(sizeof(honu_record_info) == 32, "the info row moves as four words");

__global__ __launch_bounds__(HONU_BLOCK) void k_reclaim_renumber(const uint32_t *__restrict__ order,
                                                                  const uint64_t *__restrict__ valid, uint32_t n,
                                                                  uint32_t nrec, const uint32_t *__restrict__ remap,
                                                                  uint32_t *__restrict__ order_out) {
    const uint64_t p = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= n) return;
    uint32_t o = HONU_SEEK_NONE;
    if (p < valid_rows(valid, n)) {
        const uint32_t r = order[p];
        if (r < nrec) o = remap[r];
    }
    order_out[p] = o;
}

hipError_t launch_key_reclaim(const LaunchGeom &g, const uint32_t *order, const uint64_t *valid, uint64_t n,
                              const uint8_t *keys, const int32_t *key_status, const honu_record_info *info,
                              const uint8_t *rec, const uint64_t *rec_off, uint64_t nrec, uint64_t rec_bytes,
                              uint32_t *order_out, uint32_t *remap, uint32_t *source, uint8_t *keys_out,
                              int32_t *key_status_out, honu_record_info *info_out, uint64_t *rec_off_out,
                              int32_t *status, uint8_t *values, uint64_t val_cap, uint64_t *kept,
                              uint64_t *val_total, void *work, const ScanState &S, hipStream_t s) {
    const uint64_t pb = (n + HONU_BLOCK - 1) / HONU_BLOCK;  // a thread per column position
    hipError_t e;
    if (nrec == 0) {
        if ((e = hipMemsetAsync(kept, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(val_total, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(rec_off_out, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
        if (n && (e = hipMemsetAsync(order_out, 0xFF, 4 * n, s)) != hipSuccess) return e;  // HONU_SEEK_NONE
        return hipSuccess;
    }
    const ReclaimWork W = reclaim_carve(work, nrec);
    const uint64_t tiles = compact_tiles<RECLAIM_TILE>(nrec);
    if (!remap) remap = W.remap;
    if ((e = hipMemsetAsync(W.marks, 0, nrec, s)) != hipSuccess) return e;
    if (n)
        hipLaunchKernelGGL(k_reclaim_mark, dim3((unsigned)pb), dim3(HONU_BLOCK), 0, s, order, valid, (uint32_t)n,
                           (uint32_t)nrec, W.marks);
    hipLaunchKernelGGL(k_reclaim_count, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, (uint32_t)nrec, W);
    // (tiles <= nrec + 1 <= the state's rows: the caller)
    if ((e = launch_scan(W.c.kept, tiles, 1, W.c.kept, kept, S, s)) != hipSuccess) return e;
    const ReclaimArrays A{keys, key_status, info, keys_out, key_status_out, info_out};
    hipLaunchKernelGGL(k_reclaim_place, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, rec_off, (uint32_t)nrec,
                       rec_bytes, A, kept, remap, source, rec_off_out, status, W);
    if ((e = launch_scan(rec_off_out, nrec + 1, 1, rec_off_out, val_total, S, s)) != hipSuccess) return e;
    if (n)
        hipLaunchKernelGGL(k_reclaim_renumber, dim3((unsigned)pb), dim3(HONU_BLOCK), 0, s, order, valid, (uint32_t)n,
                           (uint32_t)nrec, remap, order_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // from nrec alone, never from the kept count: from kept on the offsets are flat and every segment empty
    return launch_reclaim_copy(g, source, nrec, rec, rec_off, rec_off_out, values, val_cap, s);
}

}  // namespace honu
