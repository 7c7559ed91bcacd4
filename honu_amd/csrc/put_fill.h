// put_fill.h — the host side of the write feed (put_feed.cpp): checking and
// sizing a record (put_plan), reserving its place in a slot (put_place) and
// copying the bytes it references there (put_fill), one record at a time or a
// batch's records over a few threads (put_fill_batch).
//
// HIP-free: the slot is a plain struct of host pointers and fill counters
// (put_feed.cpp's Slot extends it with the pinned allocations, the device
// side and the stream), so tests/test_feed_host.py builds this header into a
// stand-alone program under the sanitizers.
#pragma once

#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/honu_codec.h"
#include "host_copy.h"

namespace honu {

// Upper bound of the Metadata tail + object header beyond the bytes that
// append() counts separately (span bytes, payload, 18 per ACL entry, 5 per
// region): 1+10 header, 1 nil flag, 32 ObjectID/CollectionID, Version 48
// (flag, PID 5, VID 10, Region 5, Parent flag+15, Tombstone 1, time 10),
// Schema 26 (flag, frame length 10, 3 x 5), MIME length 10, Owner/Group/
// Permissions 33, ACL count 10, Regions count 10, Publisher 53 (flag, 2
// ULIDs, 2 frame lengths), Encryption 44 (flag, 4 frame lengths, 3 enums),
// Compression 12, Flags 1, Created/Modified 20 (metadata.go:108-200).
constexpr uint64_t kFixedBound = 12 + 32 + 48 + 26 + 10 + 33 + 10 + 10 + 53 + 44 + 12 + 1 + 20;

// A slot's host inputs and its fill point. With batch_records = n and
// batch_bytes = b the arrays hold: h_meta n rows, h_var and h_pay b + 16
// bytes, h_acl b / 20 + 1 entries + 16 bytes, h_reg b / 4 + 1 entries + 16
// bytes, h_poff n + 1 offsets (put_slot_alloc).
struct PutSlotHost {
    honu_meta *h_meta = nullptr;
    uint8_t *h_var = nullptr;
    honu_acl *h_acl = nullptr;
    uint32_t *h_reg = nullptr;
    uint8_t *h_pay = nullptr;
    uint64_t *h_poff = nullptr;
    // fill
    uint64_t n = 0, var = 0, acl = 0, reg = 0, pay = 0, budget = 0, bound = 0;
};

// The spans a row's present sub-structs reference (absent ones are ignored by
// the encoder, metadata.go:120-179, and zeroed here).
inline void live_spans(const honu_meta &r, honu_span *out[8], bool live[8], honu_meta &w) {
    out[0] = &w.schema_name;
    out[1] = &w.mime;
    out[2] = &w.ip_address;
    out[3] = &w.user_agent;
    out[4] = &w.public_key_id;
    out[5] = &w.encryption_key;
    out[6] = &w.hmac_secret;
    out[7] = &w.signature;
    const uint32_t p = r.present;
    live[0] = p & HONU_HAS_SCHEMA;
    live[1] = true;
    live[2] = live[3] = p & HONU_HAS_PUBLISHER;
    live[4] = live[5] = live[6] = live[7] = p & HONU_HAS_ENCRYPTION;
}

// A record's placement: what append() checks and counts before any byte
// moves (phase 1), then where its bytes go in the slot (phase 2).
struct PutPlan {
    honu_meta w;  // the row, absent sub-structs' spans zeroed
    uint64_t span_bytes = 0, nacl = 0, nreg = 0, need = 0, bound = 0;
    uint64_t var_at = 0, acl_at = 0, reg_at = 0, pay_at = 0;  // slot positions
};

// Phase 1: validate the row's spans and lists against the caller's arrays
// and size the record (HONU_ERR_INPUT: nothing may be appended). cap_bytes
// is the feed's batch_bytes.
inline int32_t put_plan(uint64_t cap_bytes, const honu_meta *row, const uint8_t *var,
                        uint64_t var_len, const honu_acl *acl, uint64_t acl_len,
                        const uint32_t *regions, uint64_t regions_len, uint64_t data_len,
                        PutPlan &p) {
    p.w = *row;
    honu_span *spans[8];
    bool live[8];
    live_spans(*row, spans, live, p.w);
    p.span_bytes = p.nacl = p.nreg = 0;
    if (row->present & HONU_HAS_META) {
        for (int k = 0; k < 8; k++) {
            if (!live[k]) {
                *spans[k] = honu_span{0, 0};
                continue;
            }
            const honu_span sv = *spans[k];
            if (sv.len && (!var || sv.off > var_len || sv.len > var_len - sv.off)) return HONU_ERR_INPUT;
            p.span_bytes += sv.len;
        }
        if (row->present & (HONU_ACL_INPLACE | HONU_REGIONS_INPLACE))
            return HONU_ERR_INPUT;  // a decode output row (table forms only)
        p.nacl = row->acl_count;
        p.nreg = row->regions_count;
        if (p.nacl && (!acl || row->acl_off > acl_len || p.nacl > acl_len - row->acl_off))
            return HONU_ERR_INPUT;
        if (p.nreg && (!regions || row->regions_off > regions_len || p.nreg > regions_len - row->regions_off))
            return HONU_ERR_INPUT;
    } else {  // Marshal(nil, data): the encoder reports HONU_ERR_PANIC
        for (int k = 0; k < 8; k++) *spans[k] = honu_span{0, 0};
        p.w.acl_count = p.w.regions_count = 0;
    }
    if (p.nacl > cap_bytes / sizeof(honu_acl) || p.nreg > cap_bytes / 4) return HONU_ERR_CAPACITY;
    p.need = p.span_bytes + data_len + sizeof(honu_acl) * p.nacl + 4 * p.nreg;
    p.bound = kFixedBound + p.span_bytes + data_len + 18 * p.nacl + 5 * p.nreg;
    return HONU_OK;
}

// Phase 2: copy the referenced bytes to the plan's slot positions, compacted,
// and store the rebased row as record `idx` of the slot.
inline void put_fill(PutSlotHost &s, uint64_t idx, const PutPlan &p, const honu_meta *row,
                     const uint8_t *var, const honu_acl *acl, const uint32_t *regions,
                     const uint8_t *data, uint64_t data_len) {
    honu_meta w = p.w;
    honu_span *spans[8];
    bool live[8];
    live_spans(w, spans, live, w);
    uint64_t at = p.var_at;
    for (int k = 0; k < 8; k++) {
        honu_span &sv = *spans[k];
        if (!sv.len) {
            sv.off = 0;
            continue;
        }
        std::memcpy(s.h_var + at, var + sv.off, sv.len);
        sv.off = at;
        at += sv.len;
    }
    if (p.nacl) std::memcpy(s.h_acl + p.acl_at, acl + row->acl_off, sizeof(honu_acl) * p.nacl);
    if (p.nreg) std::memcpy(s.h_reg + p.reg_at, regions + row->regions_off, 4 * p.nreg);
    if (p.nacl && !(w.present & HONU_ACL_SIZED)) {
        // the list's encoded length, from the entries just copied (HONU_ACL_SIZED:
        // the size pass then reads no ACL entry; a row that carries one keeps it)
        uint64_t nb = 0;
        for (uint64_t j = 0; j < p.nacl; j++) nb += acl[row->acl_off + j].present ? 18 : 1;
        w.acl_bytes = nb;
        w.present |= HONU_ACL_SIZED;
    }
    w.acl_off = p.nacl ? p.acl_at : 0;
    w.regions_off = p.nreg ? p.reg_at : 0;
    if (data_len) std::memcpy(s.h_pay + p.pay_at, data, data_len);
    s.h_meta[idx] = w;
    s.h_poff[idx + 1] = p.pay_at + data_len;
}

// Reserve the plan's positions at the slot's fill point.
inline void put_place(PutSlotHost &s, PutPlan &p, uint64_t data_len) {
    p.var_at = s.var;
    p.acl_at = s.acl;
    p.reg_at = s.reg;
    p.pay_at = s.pay;
    s.var += p.span_bytes;
    s.acl += p.nacl;
    s.reg += p.nreg;
    s.pay += data_len;
    s.budget += p.need;
    s.bound += p.bound;
    s.n += 1;
}

// Phase 2 of append_batch: the copies of the placed records plans[0, k)
// (slot records first.., rows[i] with payload[payload_off[i], payload_off[i +
// 1])), record ranges over a few threads for big batches. bytes = the sum of
// the plans' need. threads 0: host_copy_threads() from kParallelCopyMin
// bytes on, else the calling thread; threads > 0: that many, whatever the size.
inline void put_fill_batch(PutSlotHost &s, uint64_t first, const std::vector<PutPlan> &plans,
                           uint64_t bytes, const honu_meta *rows, const uint8_t *var,
                           const honu_acl *acl, const uint32_t *regions, const uint8_t *payload,
                           const uint64_t *payload_off, unsigned threads = 0) {
    const uint64_t k = plans.size();
    auto fill = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t a = payload_off[i], b = payload_off[i + 1];
            put_fill(s, first + i, plans[i], rows + i, var, acl, regions,
                     payload ? payload + a : nullptr, b - a);
        }
    };
    const unsigned T = threads ? threads
                       : bytes >= kParallelCopyMin && k > 1 ? host_copy_threads() : 1;
    if (T == 1) {
        fill(0, k);
    } else {  // equal-byte record ranges
        std::vector<uint64_t> need(k);
        for (uint64_t i = 0; i < k; i++) need[i] = plans[i].need;
        const std::vector<uint64_t> cuts = record_cuts(need, bytes, T);
        std::vector<std::thread> pool;
        for (size_t c = 1; c + 1 < cuts.size(); c++) pool.emplace_back(fill, cuts[c], cuts[c + 1]);
        fill(cuts[0], cuts[1]);
        for (std::thread &th : pool) th.join();
    }
}

}  // namespace honu
