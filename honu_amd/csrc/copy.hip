// copy.hip — the HBM-bound half of the codec: moving payload bytes.
//
// Encode copies each record's `data` (object.go:35, lani Encode's copy,
// encode.go:74) behind its header; materialising decode copies each
// Data() subslice (object.go:97) into a packed, 16-byte aligned arena.
//
// Work is split by BYTES, not by records: the segments lie back to back in a
// "logical" byte space (the source arena for encode, the destination arena
// for decode), and wave w of W owns the logical range [w*B/W, (w+1)*B/W)
// rounded to 16 bytes. A wave binary-searches its first segment once, then
// streams forward across segment boundaries, so every wave moves the same
// number of bytes whatever the record-size mix (XLarge records no longer
// make stragglers) and there is no tail of half-idle CUs at the end of a
// launch. Within a range the copy is 16 bytes per lane, UNROLL chunks in
// flight per lane, realigned with v_alignbyte when source and destination
// phases differ (encode: always, the header length varies).
#include "kernels.h"

namespace honu {

// Segment i of an encode: src = payload[payload_off[i] ...], logical start =
// payload_off[i], dst = out + out_off[i] + 1 + uvarint_len(len).
struct EncodeSegments {
    const uint8_t *payload;
    const uint64_t *payload_off;
    uint8_t *out;
    uint64_t out_cap;
    const uint64_t *out_off;
    const int32_t *status;

    HONU_DEV uint64_t start(uint64_t i) const { return payload_off[i]; }
    HONU_DEV uint64_t lo() const { return payload_off[0]; }
    bool units;  // honu_encode_payloads_units: the encoder wrote the payload's partial end 64-byte units
    HONU_DEV bool get(uint64_t i, uint64_t &len, const uint8_t *&src, uint8_t *&dst, uint64_t &skip) const {
        // the header/tail encoder may still be running on another stream:
        // its HONU_ERR_CAPACITY is not visible here, so the capacity check
        // is repeated (nothing is written past out_cap)
        // every field loaded unconditionally (all in one round trip)
        const int32_t st = status[i];
        const uint64_t o0 = out_off[i], o1 = out_off[i + 1];
        const uint64_t s = payload_off[i];
        len = payload_off[i + 1] - s;
        src = payload + s;
        dst = out + o0 + 1 + uvarint_len(len);
        skip = 0;
        if (units) {  // the same units as lane.h encode_record_lane (absolute addresses)
            const uint64_t a0 = (uint64_t)dst, a1 = a0 + len;
            const uint64_t h_end = ((a0 + PAYLOAD_UNIT - 1) & ~(PAYLOAD_UNIT - 1)) < a1
                                       ? ((a0 + PAYLOAD_UNIT - 1) & ~(PAYLOAD_UNIT - 1)) : a1;
            const uint64_t t_beg = (a1 & ~(PAYLOAD_UNIT - 1)) > h_end ? (a1 & ~(PAYLOAD_UNIT - 1)) : h_end;
            skip = h_end - a0;
            len = t_beg - h_end;
            src += skip;
            dst += skip;
        }
        return st == HONU_OK && o1 <= out_cap && len != 0;
    }
};

// Segment i of a materialising decode: logical start = offs[3i+2] (the
// destination offset), src = rec + scratch[i].data_src.
struct DecodeSegments {
    const uint8_t *rec;
    const honu_record_info *info;
    const DecodeScratch *scratch;
    const uint64_t *offs;
    uint8_t *data;

    HONU_DEV uint64_t start(uint64_t i) const { return offs[3 * i + 2]; }
    HONU_DEV uint64_t lo() const { return 0; }
    uint64_t n_;  // (read by the retired sweep form only; stays until the kernel's arguments may move)
    HONU_DEV bool get(uint64_t i, uint64_t &len, const uint8_t *&src, uint8_t *&dst, uint64_t &skip) const {
        skip = 0;
        const int32_t st = info[i].data_status;  // every field in one round trip
        len = info[i].data_len;
        src = rec + scratch[i].data_src;
        dst = data + offs[3 * i + 2];
        return st == HONU_OK && len != 0;
    }
};

// Segment i of honu_decode_data: logical start = offs[i] (one column, the
// destination offset), src = rec + scratch[i].data_src.
struct SpanSegments {
    const uint8_t *rec;
    const honu_record_info *info;
    const DecodeScratch *scratch;
    const uint64_t *offs;
    uint8_t *data;

    HONU_DEV uint64_t start(uint64_t i) const { return offs[i]; }
    HONU_DEV uint64_t lo() const { return 0; }
    HONU_DEV bool get(uint64_t i, uint64_t &len, const uint8_t *&src, uint8_t *&dst, uint64_t &skip) const {
        skip = 0;
        const int32_t st = info[i].data_status;  // every field in one round trip
        len = info[i].data_len;
        src = rec + scratch[i].data_src;
        dst = data + offs[i];
        return st == HONU_OK && len != 0;
    }
};

// Segment g of honu_key_fetch (fetch.hip): row g of a list, logical start =
// val_off[g] (the destination offset, the scanned lengths: n + 1 values, flat
// from the list's last row on), src = rec + rec_off[rows[g].record].
// The length is the difference of the scanned offsets, and it is the validity
// too: the length pass gave a row a length other than 0 only after it found
// the record index below nrec and the offsets in order inside the arena, so a
// row with a length needs no second check, and a row without one (past the
// list's end, a tombstone left out, a refused index or offset pair) is not
// looked up in rec_off at all.
struct FetchSegments {
    const honu_list_row *rows;
    const uint8_t *rec;
    const uint64_t *rec_off;
    const uint64_t *val_off;
    uint8_t *values;
    uint64_t val_cap;

    HONU_DEV uint64_t start(uint64_t g) const { return val_off[g]; }
    HONU_DEV uint64_t lo() const { return 0; }
    HONU_DEV bool get(uint64_t g, uint64_t &len, const uint8_t *&src, uint8_t *&dst, uint64_t &skip) const {
        skip = 0;
        const uint64_t o0 = val_off[g], o1 = val_off[g + 1];  // with the row's index in one round trip
        const uint32_t r = rows[g].record;
        len = o1 - o0;
        // the rows that fit are a prefix (the offsets are monotone); nothing is written at or past val_cap
        const bool ok = len != 0 && o1 <= val_cap;
        src = rec + (ok ? rec_off[r] : 0);
        dst = values + o0;
        return ok;
    }
};

// Segment j of honu_key_reclaim (reclaim.hip): new record j, logical start =
// val_off[j] (the destination offset, the scanned lengths: n + 1 values, flat
// from the kept count on), src = rec + rec_off[source[j]]. FetchSegments with
// the record index from d_source: the place pass gave a slot a length other
// than 0 only below the kept count, where source[j] is a checked index with
// offsets in order inside the arena; a slot without a length (at or past the
// kept count, where source holds nothing written, or a refused offset pair) is
// not looked up in rec_off at all.
struct ReclaimSegments {
    const uint32_t *source;
    const uint8_t *rec;
    const uint64_t *rec_off;
    const uint64_t *val_off;
    uint8_t *values;
    uint64_t val_cap;

    HONU_DEV uint64_t start(uint64_t j) const { return val_off[j]; }
    HONU_DEV uint64_t lo() const { return 0; }
    HONU_DEV bool get(uint64_t j, uint64_t &len, const uint8_t *&src, uint8_t *&dst, uint64_t &skip) const {
        skip = 0;
        const uint64_t o0 = val_off[j], o1 = val_off[j + 1];  // with the record's index in one round trip
        const uint32_t r = source[j];
        len = o1 - o0;
        // the records that fit are a prefix (the offsets are monotone); nothing is written at or past val_cap
        const bool ok = len != 0 && o1 <= val_cap;
        src = rec + (ok ? rec_off[r] : 0);
        dst = values + o0;
        return ok;
    }
};

#define SMALL_SEG_WAVES_FACTOR 4
// average segment bytes from which a launch uses 1 / SMALL_SEG_WAVES_FACTOR of
// its waves
#ifndef COPY_FEW_WAVES_MIN
#define COPY_FEW_WAVES_MIN (64u << 10)
#endif
constexpr int COPY_UNROLL = 4;  // 16-byte chunks in flight per lane

// Two segment classes: a launch of long segments on average (>=
// COPY_FEW_WAVES_MIN) gives its first 1 / SMALL_SEG_WAVES_FACTOR of waves the
// long segments (byte ranges as below, short segments skipped) and the other
// waves, which used to return at once, the short ones (each wave a range of
// segment indices, short segments whole): the short records of a mixed batch
// no longer hold up the few streaming waves. 1M Mixed encode + decode
// 1238-1248 -> 1266-1268 GiB/s on one box, 1152-1176 -> 1189-1230 on another
// (interleaved; every Large and XLarge payload is >= 64 KB, so those batches
// have no short class, and they measured equal within the runs' order effect;
// profiles/r05/copy_classes/). (Every wave on every segment instead: Mixed 7 %
// slower, the long segments' streams too many.)
template <class Seg>
HONU_DEV void copy_short_run(const Seg &seg, uint64_t i0, uint64_t i1, uint64_t short_max) {
    uint64_t len_nx = 0, skip = 0;
    const uint8_t *src_nx = nullptr;
    uint8_t *dst_nx = nullptr;
    bool ok_nx = i0 < i1 && seg.get(i0, len_nx, src_nx, dst_nx, skip);
    for (uint64_t i = i0; i < i1; i++) {
        const uint64_t len = len_nx;
        const uint8_t *src = src_nx;
        uint8_t *dst = dst_nx;
        const bool ok = ok_nx;
        if (i + 1 < i1) ok_nx = seg.get(i + 1, len_nx, src_nx, dst_nx, skip);
        if (ok && len < short_max) wave_copy<COPY_UNROLL>(dst, src, len);
    }
}

// The logical range [lo, hi) of a streaming wave: its first segment by binary
// search, then forward across segment boundaries (skip_short: segments under
// short_max are the short class's).
template <class Seg>
HONU_DEV void copy_range(const Seg &seg, uint64_t n, uint64_t lo, uint64_t hi, bool skip_short,
                         uint64_t short_max) {
    if (lo >= hi) return;
    // largest i with start(i) <= lo
    uint64_t a = 0, b = n;  // invariant: start(a) <= lo, answer in [a, b)
    while (b - a > 1) {
        const uint64_t mid = (a + b) >> 1;
        if (seg.start(mid) <= lo) a = mid;
        else b = mid;
    }
    // A segment's descriptors (start, then status / lengths / pointers) are
    // loaded one segment ahead: issued before the current segment's copy, they
    // arrive with its loads, so a short segment costs one round trip instead
    // of three (start -> descriptors -> bytes).
    // (skip: the segment's copy starts that many bytes into it, EncodeSegments
    // with units; its logical range is then [start + skip, + len))
    uint64_t s_nx = seg.start(a), len_nx = 0, skip_nx = 0;
    const uint8_t *src_nx = nullptr;
    uint8_t *dst_nx = nullptr;
    bool ok_nx = seg.get(a, len_nx, src_nx, dst_nx, skip_nx);
    for (uint64_t i = a; i < n; i++) {
        const uint64_t s0 = s_nx, len = len_nx, s = s0 + skip_nx;
        const uint8_t *src = src_nx;
        uint8_t *dst = dst_nx;
        const bool ok = ok_nx;
        if (s0 >= hi) break;
        if (i + 1 < n) {
            s_nx = seg.start(i + 1);
            ok_nx = seg.get(i + 1, len_nx, src_nx, dst_nx, skip_nx);
        }
        if (!ok) continue;
        if (skip_short && len < short_max) continue;  // the short class's
        const uint64_t x = s > lo ? s : lo;
        const uint64_t e = s + len;
        const uint64_t y = e < hi ? e : hi;
        if (x < y)
            wave_copy<COPY_UNROLL>(dst + (x - s), src + (x - s), y - x);
    }
}

// Range tails from a counter (tickets: this launch's counter pair, one line of
// a ring of COPY_TICKET_LINES lines in the context that successive copy calls
// take in turn, so copies running at once on different streams never share
// one: ADVICE r05; nullptr: off). In a launch whose segments average at least
// COPY_STEAL_MIN bytes, a streaming wave copies the first 1 - COPY_STEAL / 64
// of its range, then takes the other streaming waves' range tails, in order,
// from tickets[0]: the waves whose ranges hold fewer bytes to copy (a mixed
// batch's short segments are skipped inside them) or that share their CU with
// a metadata kernel take more tails instead of leaving the launch's end to
// the slowest. tickets[1] counts the waves done, and the last one resets both,
// so every launch finds them zero (as the look-back state; a replayed hipGraph
// too). Measured (4 interleaved rounds each, profiles/r05/copy_steal/): 1M
// Mixed encode -1.4 % per step (every copy launch -2 % in the kernel trace),
// Mixed encode + decode -2.9 %, Medium -1.2 % (-3.5 % on another box), Large
// equal; with it on 1M Small too, +1.9 % (2.6 KB payloads: hence the bound).
#define COPY_STEAL_MIN (16u << 10)
#define COPY_STEAL 8u
template <class Seg>
__global__ __launch_bounds__(HONU_BLOCK) void k_copy_segments(Seg seg, uint64_t n,
                                                               const uint64_t *__restrict__ total_p,
                                                               uint64_t short_max, uint32_t *tickets,
                                                               uint32_t steal) {
    uint64_t W = (uint64_t)gridDim.x * HONU_WAVES_PER_BLOCK;
    const uint64_t w = (uint64_t)blockIdx.x * HONU_WAVES_PER_BLOCK + wave_in_block();
    const uint64_t base = seg.lo();
    const uint64_t total = *total_p - base;
    // Large segments stream best from few waves (DRAM rows stay open: 2 WG per
    // CU measured best); short segments are latency bound and want every wave
    // the launch has (SMALL_SEG_WAVES_FACTOR x more).
    const bool few = n && total / n >= COPY_FEW_WAVES_MIN;
    if (few) {
        const uint64_t Wall = W;
        W /= SMALL_SEG_WAVES_FACTOR;
        if (w >= W) {  // the short class: run w - W of Wall - W index runs
            const uint64_t v = w - W, V = Wall - W;
            copy_short_run(seg, n * v / V, n * (v + 1) / V, short_max);
            return;
        }
    }
    if (w >= W) return;
    auto range = [&](uint64_t v, uint64_t &lo, uint64_t &hi) {
        lo = base + ((total * v / W) & ~15ull);
        hi = (v + 1 == W) ? base + total : base + ((total * (v + 1) / W) & ~15ull);
    };
    uint64_t lo, hi;
    range(w, lo, hi);
    if (tickets && n && total / n >= COPY_STEAL_MIN) {  // uniform over the launch
        auto cut = [&](uint64_t l, uint64_t h) {  // where a range's tail starts (steal / 64 of it)
            return h - ((((h - l) * steal) >> 6) & ~15ull);
        };
        copy_range(seg, n, lo, cut(lo, hi), few, short_max);
        for (;;) {
            uint32_t t = 0;
            if (__lane_id() == 0) t = atomicAdd(&tickets[0], 1u);
            t = __shfl(t, 0);
            if (t >= W) break;  // each wave's last take: W of them past the tails
            uint64_t l, h;
            range(t, l, h);
            copy_range(seg, n, cut(l, h), h, few, short_max);
        }
        if (__lane_id() == 0 && atomicAdd(&tickets[1], 1u) == (uint32_t)W - 1) {
            atomicExch(&tickets[0], 0u);  // every wave has taken its last ticket
            atomicExch(&tickets[1], 0u);
        }
        return;
    }
    copy_range(seg, n, lo, hi, few, short_max);
}

// One form: unroll 4, default cache policy, two segment classes, range tails
// (context param "copy_steal"). Measured and not kept (sources in git history,
// commit 426ce70, there as copy variants of the A/B build; numbers in
// DESIGN_HISTORY.md, "two segment classes" / "range tails from a counter" and
// the paragraphs after them unless another place is named):
// non-temporal loads and stores, both / loads only / stores only (variants
// 2-3, 11, 12): 1M Large 1270 / 1197-1230 / 1223 against 1345 GiB/s in round
// 1, 1166-1210 against 1252-1332 in round 5 (profiles/r05/copy_nt/); the sweep
// form, a tile -> segment map and waves striding tiles inside one window
// (6-7): not better (round 1, "a tile-interleaved sweep variant"); one
// unaligned 16-byte load per chunk instead of two aligned loads and a funnel
// (13-15): Large encode copy 5.18 -> 4.85 TB/s, decode 5.89 -> 5.50; unroll
// 8 / 2 / 16 (1, 4, 5): 8 is -2.4 % on Medium and slower on Small, 2 is
// -0.6 % on Small, and the size class is known on the device only
// (profiles/r05/copy_unroll/); one segment class (40): the numbers above
// copy_short_run; the short class's bound from the environment (42): 32 KB
// within the noise, 128 and 256 KB slower on Mixed; the tails' share from the
// environment (45): 4 / 16 / 24 of 64 slower than 8 (share_sweep/); run tails
// for the short class from a second counter pair (46): Mixed encode 30.64
// against 30.26 ms, within the run-order effect (short_tails/).
template <class Seg>
static hipError_t launch_copy(const LaunchGeom &g, const Seg &seg, uint64_t n,
                              const uint64_t *total, uint32_t *tickets, hipStream_t s) {
    const dim3 grid(g.copy_blocks * SMALL_SEG_WAVES_FACTOR), block(HONU_BLOCK);
    hipLaunchKernelGGL((k_copy_segments<Seg>), grid, block, 0, s, seg, n, total,
                       (uint64_t)COPY_FEW_WAVES_MIN, g.copy_steal ? tickets : nullptr, COPY_STEAL);
    return hipGetLastError();
}

hipError_t launch_encode_copy(const LaunchGeom &g, const uint8_t *payload,
                              const uint64_t *payload_off, uint64_t n, uint8_t *out,
                              uint64_t out_cap, const uint64_t *out_off, const int32_t *status,
                              bool units, hipStream_t s) {
    if (n == 0) return hipSuccess;
    EncodeSegments seg{payload, payload_off, out, out_cap, out_off, status, units};
    return launch_copy(g, seg, n, payload_off + n, g.copy_tickets, s);
}
// (g.copy_tickets: the launch's own counter line, api.hip copy_geom)

hipError_t launch_span_copy(const LaunchGeom &g, const uint8_t *rec, uint64_t n,
                            const honu_record_info *info, const DecodeScratch *scratch,
                            const uint64_t *offs, uint8_t *data, hipStream_t s) {
    if (n == 0) return hipSuccess;
    SpanSegments seg{rec, info, scratch, offs, data};
    return launch_copy(g, seg, n, offs + n, g.copy_tickets, s);
}

hipError_t launch_decode_copy(const LaunchGeom &g, const uint8_t *rec, uint64_t n,
                              const honu_record_info *info, const DecodeScratch *scratch,
                              const uint64_t *offs, const uint64_t *totals, uint8_t *data,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    DecodeSegments seg{rec, info, scratch, offs, data, n};  // (n: the unread n_)
    return launch_copy(g, seg, n, totals + 2, g.copy_tickets, s);
}

// n = the list's cap: segments [0, n), the total at val_off + n. The full grid
// however few rows the list holds, and the classes by total / n, not by the
// rows listed: both counts are on the device only
hipError_t launch_fetch_copy(const LaunchGeom &g, const honu_list_row *rows, uint64_t n, const uint8_t *rec,
                             const uint64_t *rec_off, const uint64_t *val_off, uint8_t *values,
                             uint64_t val_cap, hipStream_t s) {
    if (n == 0) return hipSuccess;
    FetchSegments seg{rows, rec, rec_off, val_off, values, val_cap};
    return launch_copy(g, seg, n, val_off + n, g.copy_tickets, s);
}

// n = nrec: segments [0, n), the total at val_off + n. As launch_fetch_copy:
// the full grid however few records stay, the classes by total / n
hipError_t launch_reclaim_copy(const LaunchGeom &g, const uint32_t *source, uint64_t n, const uint8_t *rec,
                               const uint64_t *rec_off, const uint64_t *val_off, uint8_t *values,
                               uint64_t val_cap, hipStream_t s) {
    if (n == 0) return hipSuccess;
    ReclaimSegments seg{source, rec, rec_off, val_off, values, val_cap};
    return launch_copy(g, seg, n, val_off + n, g.copy_tickets, s);
}

}  // namespace honu
