// sort.hip — sort.Sort(keys.Keys) over a key column (keys/keys.go:126-130:
// bytes.Compare order), and the cut of the sorted column into objects with
// their versions (keys.go:73-92: [ObjectPrefix, ObjectLimit)).
//
// A stable least-significant-digit radix sort with 8-bit digits over
// (packed key, index) pairs. A key is packed once into 32 bytes, read as eight
// big-endian words: byte 0 the validity (0 valid, 1 not), bytes 1-29 the key,
// bytes 30-31 zero. Digit d (0 the least significant) is packed byte 29 - d,
// so a digit is a shift and a mask of one word, validity is the thirtieth and
// most significant digit, and a key moves as two 16-byte stores.
//
// The pack also ORs (packed key XOR packed key 0) over the column: a digit
// whose byte of that mask is zero is shared by every key, and its pass would
// move nothing. k_sort_plan turns the mask into one word per pass (runs or
// not, which ping-pong side it reads); a pass's kernels read their word and
// an empty pass returns at once. The decision is on the device, so the whole
// call records into a graph. (The mask decides exactly what 30 histograms
// would — "one bin holds every key" — for eight atomics per workgroup.)
//
// A pass that runs: per-tile digit counts into a digit-major table, an
// exclusive scan of the table (launch_scan, or one workgroup when the table
// has more rows than the context's scan state is sized for), then a stable
// scatter. No spin-wait of its own.
#include "compact.h"  // compact_lanes_below
#include "keycol.h"

namespace honu {

constexpr int SORT_ITEMS = 8;                               // keys per thread
constexpr uint32_t SORT_TILE = HONU_BLOCK * SORT_ITEMS;     // keys per workgroup per pass
constexpr uint32_t SORT_WAVE_KEYS = HONU_WAVE * SORT_ITEMS; // consecutive keys of one wave
constexpr int SORT_DIGITS = 30;
// plan words (SortWork::plan): [d] pass d: bit 0 runs, bit 1 the side it reads;
// [30] the side the sorted pairs end on; [32..39] the OR mask
constexpr int PLAN_FINAL = 30, PLAN_MASK = 32, PLAN_WORDS = 64;

uint32_t sort_tile() { return SORT_TILE; }

static uint64_t sort_tiles(uint64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }

uint64_t sort_workspace_bytes(uint64_t n) {
    return up256(4 * PLAN_WORDS) + 2 * up256(32 * n) + 2 * up256(4 * n) + up256(8 * (n + 1)) +
           up256(8 * 256 * sort_tiles(n));
}

SortWork sort_carve(void *work, uint64_t n) {
    SortWork w;
    uint8_t *p = (uint8_t *)work;
    w.plan = (uint32_t *)p;
    p += up256(4 * PLAN_WORDS);
    for (int s = 0; s < 2; s++) {
        w.key[s] = (u32x4 *)p;
        p += up256(32 * n);
    }
    for (int s = 0; s < 2; s++) {
        w.idx[s] = (uint32_t *)p;
        p += up256(4 * n);
    }
    w.col = (uint64_t *)p;
    p += up256(8 * (n + 1));
    w.table = (uint64_t *)p;
    return w;
}

// which word of the packed key holds digit d, and the shift that brings it down
HONU_HD uint32_t digit_word(int d) { return (uint32_t)(29 - d) >> 2; }
HONU_HD uint32_t digit_shift(int d) { return (3u - ((uint32_t)(29 - d) & 3u)) * 8u; }

__global__ __launch_bounds__(HONU_BLOCK) void k_sort_pack(const uint8_t *__restrict__ keys,
                                                          const int32_t *__restrict__ status, uint64_t n,
                                                          SortWork W) {
    __shared__ uint32_t sh[SORT_KEY_WORDS];
    if (threadIdx.x < SORT_KEY_WORDS) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t first[SORT_KEY_WORDS], acc[SORT_KEY_WORDS];
    pack_key(keys, !status || status[0] == HONU_OK, first);
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++) acc[i] = 0;
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + threadIdx.x;
#pragma unroll 2
    for (int it = 0; it < SORT_ITEMS; it++) {
        const uint64_t p = base + (uint64_t)it * HONU_BLOCK;
        if (p >= n) break;
        uint32_t w[SORT_KEY_WORDS];
        pack_key(keys + HONU_KEY_LEN * p, !status || status[p] == HONU_OK, w);
#pragma unroll
        for (int i = 0; i < SORT_KEY_WORDS; i++) acc[i] |= w[i] ^ first[i];
        W.key[0][2 * p] = u32x4{w[0], w[1], w[2], w[3]};
        W.key[0][2 * p + 1] = u32x4{w[4], w[5], w[6], w[7]};
        W.idx[0][p] = (uint32_t)p;
    }
#pragma unroll
    for (int i = 0; i < SORT_KEY_WORDS; i++)
        if (acc[i]) atomicOr(&sh[i], acc[i]);
    __syncthreads();
    if (threadIdx.x < SORT_KEY_WORDS && sh[threadIdx.x])
        atomicOr(&W.plan[PLAN_MASK + threadIdx.x], sh[threadIdx.x]);
}

__global__ void k_sort_plan(SortWork W) {
    if (threadIdx.x || blockIdx.x) return;
    uint32_t side = 0;
    for (int d = 0; d < SORT_DIGITS; d++) {
        const uint32_t run = ((W.plan[PLAN_MASK + digit_word(d)] >> digit_shift(d)) & 0xFFu) != 0;
        W.plan[d] = run | (side << 1);
        side ^= run;
    }
    W.plan[PLAN_FINAL] = side;
}

// table[digit * tiles + tile] = keys of the tile with that digit
__global__ __launch_bounds__(HONU_BLOCK) void k_sort_count(int d, uint64_t n, uint64_t tiles, SortWork W) {
    const uint32_t plan = W.plan[d];
    if (!(plan & 1u)) return;
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t *src = reinterpret_cast<const uint32_t *>(W.key[plan >> 1]) + digit_word(d);
    const uint32_t sh = digit_shift(d);
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + threadIdx.x;
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; it++) {
        const uint64_t p = base + (uint64_t)it * HONU_BLOCK;
        if (p < n) atomicAdd(&cnt[(src[SORT_KEY_WORDS * p] >> sh) & 0xFFu], 1u);
    }
    __syncthreads();
    W.table[(uint64_t)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// the table's exclusive scan in one workgroup, in place: for a table with
// more rows than the context's scan state covers (a batch under 256 keys has
// a 256-row table)
__global__ __launch_bounds__(HONU_BLOCK) void k_sort_scan_one(int d, uint64_t rows, SortWork W) {
    if (!(W.plan[d] & 1u)) return;
    __shared__ uint64_t sh[HONU_WAVES_PER_BLOCK];
    uint64_t carry = 0;
    for (uint64_t r0 = 0; r0 < rows; r0 += HONU_BLOCK) {
        const uint64_t r = r0 + threadIdx.x;
        const uint64_t v = r < rows ? W.table[r] : 0;
        const uint64_t incl = wave_inclusive_scan(v);
        if (lane_id() == HONU_WAVE - 1) sh[threadIdx.x / HONU_WAVE] = incl;
        __syncthreads();
        uint64_t add = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < HONU_WAVES_PER_BLOCK; j++) {
            if (j < (int)(threadIdx.x / HONU_WAVE)) add += sh[j];
            tot += sh[j];
        }
        __syncthreads();
        if (r < rows) W.table[r] = carry + add + incl - v;
        carry += tot;
    }
}

// The stable scatter of one tile. A wave owns SORT_WAVE_KEYS consecutive keys
// and takes them 64 at a time in order; the lanes that hold the same digit
// find each other with eight ballots, a key's rank among them is the popcount
// below its lane, and the wave's running count of the digit (LDS, the wave's
// own row) is the rank of the first. Waves, rounds and lanes all go in key
// order, so equal digits keep their order.
__global__ __launch_bounds__(HONU_BLOCK) void k_sort_scatter(int d, uint64_t n, uint64_t tiles, SortWork W) {
    const uint32_t plan = W.plan[d];
    if (!(plan & 1u)) return;
    __shared__ uint32_t cnt[HONU_WAVES_PER_BLOCK][256];
    const uint32_t side = plan >> 1, wv = threadIdx.x / HONU_WAVE, lane = lane_id();
#pragma unroll
    for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const u32x4 *skey = W.key[side];
    const uint32_t *sword = reinterpret_cast<const uint32_t *>(skey) + digit_word(d);
    const uint32_t sh = digit_shift(d);
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wv * SORT_WAVE_KEYS + lane;
    const uint64_t below = compact_lanes_below(lane);
    uint32_t dg[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; it++) {
        const uint64_t p = base + (uint64_t)it * HONU_WAVE;
        const bool in = p < n;
        dg[it] = in ? (sword[SORT_KEY_WORDS * p] >> sh) & 0xFFu : 0;
        uint64_t peers = __ballot(in);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (dg[it] >> b) & 1u;
            const uint64_t m = __ballot(in && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t before = cnt[wv][dg[it]];
        wave_sync();
        rank[it] = before + (uint32_t)__popcll(peers & below);
        if (in && !(peers & below)) cnt[wv][dg[it]] = before + (uint32_t)__popcll(peers);
        wave_sync();
    }
    __syncthreads();
    {  // thread t: digit t's first position per wave = the scanned table's + the waves before
        uint64_t run = W.table[(uint64_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < HONU_WAVES_PER_BLOCK; w++) {
            const uint32_t c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = (uint32_t)run;  // positions are below n <= 2^32 - 1
            run += c;
        }
    }
    __syncthreads();
    u32x4 *dkey = W.key[side ^ 1];
    const uint32_t *sidx = W.idx[side];
    uint32_t *didx = W.idx[side ^ 1];
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; it++) {
        const uint64_t p = base + (uint64_t)it * HONU_WAVE;
        if (p >= n) break;
        const uint64_t q = (uint64_t)cnt[wv][dg[it]] + rank[it];
        const u32x4 k0 = skey[2 * p], k1 = skey[2 * p + 1];
        const uint32_t ix = sidx[p];
        dkey[2 * q] = k0;
        dkey[2 * q + 1] = k1;
        didx[q] = ix;
    }
}

// the sorted pairs -> d_order, d_sorted (optional) and the valid count
__global__ __launch_bounds__(HONU_BLOCK) void k_sort_emit(const uint8_t *__restrict__ keys, uint64_t n,
                                                          uint32_t *__restrict__ order,
                                                          uint8_t *__restrict__ sorted, uint64_t *valid,
                                                          SortWork W) {
    const uint64_t p = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t side = W.plan[PLAN_FINAL];
    const u32x4 *key = W.key[side];
    const uint32_t ix = W.idx[side][p];
    order[p] = ix;
    const u32x4 k0 = key[2 * p];
    const bool ok = (k0.x >> 24) == 0;
    // the valid keys come first: the last of them, or an invalid key 0, knows the count
    if (!ok && p == 0) *valid = 0;
    if (ok && (p + 1 == n || (key[2 * p + 2].x >> 24) != 0)) *valid = p + 1;
    if (!sorted) return;
    uint8_t *out = sorted + HONU_KEY_LEN * p;
    if (!ok) {  // packed as zeros: the row's own bytes
        copy_key(out, keys + (uint64_t)HONU_KEY_LEN * ix);
        return;
    }
    const u32x4 k1 = key[2 * p + 1];
    const uint32_t w[SORT_KEY_WORDS] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    unpack_key(out, w);
}

hipError_t launch_sort_keys(const uint8_t *keys, const int32_t *status, uint64_t n, uint32_t *order,
                            uint8_t *sorted, uint64_t *valid, void *work, const ScanState &S,
                            uint64_t scan_rows, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(valid, 0, sizeof(uint64_t), s);
    const SortWork W = sort_carve(work, n);
    const uint64_t tiles = sort_tiles(n), rows = 256 * tiles;
    hipError_t e = hipMemsetAsync(W.plan, 0, 4 * PLAN_WORDS, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sort_pack, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, keys, status, n, W);
    hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(HONU_WAVE), 0, s, W);
    for (int d = 0; d < SORT_DIGITS; d++) {
        hipLaunchKernelGGL(k_sort_count, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, d, n, tiles, W);
        if (rows <= scan_rows) {
            // (an empty pass's table is scanned all the same: launch_scan knows no plan, and the
            // table is the workspace's own)
            e = launch_scan(W.table, rows, 1, W.table, W.col, S, s);
            if (e != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_sort_scan_one, dim3(1), dim3(HONU_BLOCK), 0, s, d, rows, W);
        }
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)tiles), dim3(HONU_BLOCK), 0, s, d, n, tiles, W);
    }
    hipLaunchKernelGGL(k_sort_emit, dim3((unsigned)((n + HONU_BLOCK - 1) / HONU_BLOCK)), dim3(HONU_BLOCK), 0, s,
                       keys, n, order, sorted, valid, W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------
// objects: the sorted positions cut where key[0:17] (ObjectPrefix,
// keys.go:74-79) changes
// ------------------------------------------------------------------------
HONU_DEV bool same_prefix(const uint8_t *x, const uint8_t *y) {
    const u32x4 a = *reinterpret_cast<const u32x4u *>(x), b = *reinterpret_cast<const u32x4u *>(y);
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w && x[16] == y[16];
}

// col[p] = 1 where position p starts an object (p < valid), else 0
__global__ __launch_bounds__(HONU_BLOCK) void k_obj_heads(const uint8_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ order,
                                                          const uint64_t *__restrict__ valid, uint64_t n,
                                                          uint64_t *__restrict__ col) {
    const uint64_t p = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    if (p >= n) return;
    uint64_t head = 0;
    if (p < valid_rows(valid, n)) {
        const uint64_t i = order_index(order[p], n), j = p ? order_index(order[p - 1], n) : 0;
        head = p == 0 || !same_prefix(keys + HONU_KEY_LEN * i, keys + HONU_KEY_LEN * j);
    }
    col[p] = head;
}

// col scanned in place (col[p] = objects that start before p), *objects the total
__global__ __launch_bounds__(HONU_BLOCK) void k_obj_place(const uint32_t *__restrict__ order,
                                                          const uint64_t *__restrict__ valid, uint64_t n,
                                                          const uint64_t *__restrict__ col,
                                                          const uint64_t *__restrict__ objects,
                                                          uint64_t *__restrict__ obj_off,
                                                          uint32_t *__restrict__ latest) {
    const uint64_t p = (uint64_t)blockIdx.x * HONU_BLOCK + threadIdx.x;
    const uint64_t v = valid_rows(valid, n), total = *objects;
    if (p > v) return;
    if (p == v) {
        obj_off[total] = v;
        return;
    }
    const uint64_t before = col[p], upto = p + 1 < n ? col[p + 1] : total;
    if (upto != before) obj_off[before] = p;                // p starts object `before`
    const uint64_t next = p + 1 < v ? (p + 2 < n ? col[p + 2] : total) : upto + 1;
    if (latest && next != upto) latest[upto - 1] = order[p];  // p + 1 starts an object, or ends the valid keys
}

hipError_t launch_key_objects(const uint8_t *keys, const uint32_t *order, const uint64_t *valid, uint64_t n,
                              uint64_t *obj_off, uint32_t *latest, uint64_t *objects, void *work,
                              const ScanState &S, hipStream_t s) {
    const SortWork W = sort_carve(work, n);
    const unsigned blocks = (unsigned)((n + 1 + HONU_BLOCK - 1) / HONU_BLOCK);
    if (n) hipLaunchKernelGGL(k_obj_heads, dim3(blocks), dim3(HONU_BLOCK), 0, s, keys, order, valid, n, W.col);
    hipError_t e = launch_scan(W.col, n, 1, W.col, objects, S, s);  // (n == 0: *objects = 0)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_obj_place, dim3(blocks), dim3(HONU_BLOCK), 0, s, order, valid, n, W.col, objects,
                       obj_off, latest);
    return hipGetLastError();
}

}  // namespace honu
