// fetch.hip — Cursor.Object() (iterator/cursor.go:31-38: make + copy of the
// value under the cursor) for a batch of listed rows: the step every
// reference read path ends in, once per row that List, Versions or Retrieve
// visits (collection.go:32-35, 97-110). The rows are honu_key_list's, the
// values the records of a CSR arena; they come out as a CSR arena of their
// own (d_values, d_val_off), the input form of the decode calls, and every
// count stays on the device.
//
// Three launches, no workspace:
//   lengths  a thread per row g in [0, cap]: the row's record length, or 0
//            for a row at or past w = min(d_total[0], cap), a tombstone under
//            HONU_FETCH_LIVE, a record index not below nrec or offsets that
//            do not lie in order inside the arena; the value to d_val_off[g]
//            (0 to d_val_off[cap]), the row's status to d_status[g], g < w;
//   scan     launch_scan in place over the cap + 1 values, the total to
//            d_val_total (the context's scan state covers max_records rows:
//            honu_key_fetch refuses cap + 1 above that);
//   copy     k_copy_segments<FetchSegments> (copy.hip) over cap segments, the
//            destination arena its logical byte space.
// The kernel here has no atomics and no state outside the launch. Every index
// read from a row is checked against nrec before d_rec_off is read, and every
// offset pair against rec_bytes before its length counts: garbage in d_rows or
// d_rec_off gives statuses, never an access out of bounds.
#include "kernels.h"

namespace honu {

__global__ __launch_bounds__(HONU_BLOCK) void k_fetch_lengths(
    const honu_list_row *__restrict__ rows, const uint64_t *__restrict__ total_p, uint32_t cap,
    const uint64_t *__restrict__ rec_off, uint32_t nrec, uint64_t rec_bytes, uint32_t flags,
    uint64_t *__restrict__ val_off, int32_t *__restrict__ status) {
    const uint64_t g = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (g > cap) return;
    const uint64_t total = *total_p;
    const uint64_t w = total < cap ? total : cap;  // rows that take part
    uint64_t len = 0;
    if (g < w) {
        const u32x4 row = *reinterpret_cast<const u32x4 *>(rows + g);  // range, pos, record, flags
        const uint32_t r = row[2];
        int32_t st = HONU_OK;
        if ((flags & HONU_FETCH_LIVE) && (row[3] & HONU_LIST_ROW_TOMBSTONE)) {
            // Object() of a row a listing does not return: nothing, and d_rec_off is not read
        } else if (r >= nrec) {
            st = HONU_ERR_INPUT;
        } else {
            const uint64_t a = rec_off[r], b = rec_off[(uint64_t)r + 1];
            if (a <= b && b <= rec_bytes) len = b - a;
            else st = HONU_ERR_INPUT;
        }
        if (status) status[g] = st;
    }
    val_off[g] = len;
}

hipError_t launch_key_fetch(const LaunchGeom &g, const honu_list_row *rows, const uint64_t *total, uint64_t cap,
                            const uint8_t *rec, const uint64_t *rec_off, uint64_t nrec, uint64_t rec_bytes,
                            uint32_t flags, uint64_t *val_off, int32_t *status, uint8_t *values, uint64_t val_cap,
                            uint64_t *val_total, const ScanState &S, hipStream_t s) {
    const uint64_t cb = (cap + 1 + HONU_BLOCK - 1) / HONU_BLOCK;
    hipLaunchKernelGGL(k_fetch_lengths, dim3((unsigned)cb), dim3(HONU_BLOCK), 0, s, rows, total, (uint32_t)cap,
                       rec_off, (uint32_t)nrec, rec_bytes, flags, val_off, status);
    // (cap + 1 <= the state's rows: the caller)
    const hipError_t e = launch_scan(val_off, cap + 1, 1, val_off, val_total, S, s);
    if (e != hipSuccess) return e;
    // from cap alone, never from a count on the device: past w the offsets are flat and every segment empty
    return launch_fetch_copy(g, rows, cap, rec, rec_off, val_off, values, val_cap, s);
}

}  // namespace honu
