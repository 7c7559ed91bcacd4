// put_feed.cpp — the write feed (include/honu_codec.h, "Write feed"): the
// batching a store's Put path needs in front of the GPU encoder. In the
// reference every Put marshals one record on the calling goroutine
// (object.Marshal, object.go:24-45, called from store.go:226,530 and the
// tests); here records are appended into pinned memory (row + the bytes its
// spans and lists reference, compacted, + payload) and each submitted batch
// is copied to the device, marshalled (sizes, scan, header + Metadata tails,
// payload copy) and copied back on its own stream while the next batch fills.
//
// Two slots, as the read feed (feed.cpp). The encoded records come back by a
// D2H copy sized by an upper bound of the batch's encoded bytes that append()
// keeps (kFixedBound, put_fill.h), so submit() never has to wait for the size
// pass. Everything that touches HIP is here; checking, placing and copying a
// record into a slot's host arrays is put_fill.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/honu_codec.h"
#include "host_copy.h"
#include "put_fill.h"

using honu::kFixedBound;
using honu::put_fill;
using honu::put_place;
using honu::put_plan;
using honu::PutPlan;

namespace {

enum SlotState { FREE = 0, INFLIGHT = 1, DONE = 2 };

// The pinned host inputs and the fill counters are put_fill.h's PutSlotHost.
struct Slot : honu::PutSlotHost {
    honu_ctx *ctx = nullptr;
    hipStream_t stream = nullptr;
    // pinned host outputs
    uint8_t *h_out = nullptr;
    uint64_t *h_ooff = nullptr;
    int32_t *h_st = nullptr;
    // device
    honu_meta *d_meta = nullptr;
    uint8_t *d_var = nullptr;
    honu_acl *d_acl = nullptr;
    uint32_t *d_reg = nullptr;
    uint8_t *d_pay = nullptr;
    uint64_t *d_poff = nullptr;
    uint8_t *d_out = nullptr;
    uint64_t *d_ooff = nullptr;
    int32_t *d_st = nullptr;
    uint64_t ticket = 0;
    SlotState state = FREE;
};

}  // namespace

struct honu_put_feed {
    int device = 0;
    uint64_t cap_n = 0, cap_bytes = 0, acl_cap = 0, reg_cap = 0, out_cap = 0;
    Slot slot[2];
    int cur = 0;
    uint64_t next_ticket = 1;
};

#define PCHK(x)                                   \
    do {                                          \
        if ((x) != hipSuccess) return HONU_E_HIP; \
    } while (0)

static void put_slot_free(Slot &s) {
    if (s.ctx) honu_ctx_destroy(s.ctx);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    void *host[] = {s.h_meta, s.h_var, s.h_acl, s.h_reg, s.h_pay, s.h_poff, s.h_out, s.h_ooff, s.h_st};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    void *dev[] = {s.d_meta, s.d_var, s.d_acl, s.d_reg, s.d_pay, s.d_poff, s.d_out, s.d_ooff, s.d_st};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    s = Slot();
}

static int32_t put_slot_alloc(honu_put_feed *f, Slot &s) {
    int32_t err = HONU_OK;
    s.ctx = honu_ctx_create(f->device, f->cap_n, &err);
    if (!s.ctx) return err ? err : HONU_E_HIP;
    PCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    const uint64_t n = f->cap_n, b = f->cap_bytes + 16;
    const uint64_t sz_meta = sizeof(honu_meta) * n, sz_acl = sizeof(honu_acl) * f->acl_cap + 16;
    const uint64_t sz_reg = 4 * f->reg_cap + 16, sz_off = 8 * (n + 1), sz_out = f->out_cap + 16;
    PCHK(hipHostMalloc((void **)&s.h_meta, sz_meta, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_var, b, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_acl, sz_acl, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_reg, sz_reg, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_pay, b, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_poff, sz_off, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_out, sz_out, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_ooff, sz_off, hipHostMallocDefault));
    PCHK(hipHostMalloc((void **)&s.h_st, 4 * n + 16, hipHostMallocDefault));
    PCHK(hipMalloc((void **)&s.d_meta, sz_meta));
    PCHK(hipMalloc((void **)&s.d_var, b));
    PCHK(hipMalloc((void **)&s.d_acl, sz_acl));
    PCHK(hipMalloc((void **)&s.d_reg, sz_reg));
    PCHK(hipMalloc((void **)&s.d_pay, b));
    PCHK(hipMalloc((void **)&s.d_poff, sz_off));
    PCHK(hipMalloc((void **)&s.d_out, sz_out));
    PCHK(hipMalloc((void **)&s.d_ooff, sz_off));
    PCHK(hipMalloc((void **)&s.d_st, 4 * n + 16));
    s.h_poff[0] = 0;
    return HONU_OK;
}

honu_put_feed *honu_put_feed_create(int device, uint64_t batch_records, uint64_t batch_bytes,
                                    int32_t *err) {
    int32_t dummy;
    if (!err) err = &dummy;
    *err = HONU_OK;
    if (!batch_records || !batch_bytes) {
        *err = HONU_E_ARG;
        return nullptr;
    }
    honu_put_feed *f = new honu_put_feed();
    f->device = device;
    f->cap_n = batch_records;
    f->cap_bytes = batch_bytes;
    // every input byte (span bytes, payload, 20 per ACL entry, 4 per region)
    // counts against batch_bytes, so these tables can never overflow
    f->acl_cap = batch_bytes / sizeof(honu_acl) + 1;
    f->reg_cap = batch_bytes / 4 + 1;
    // Σ put_bound: input bytes + 1 per region (5-byte varints for 4 counted
    // bytes) + kFixedBound per record
    f->out_cap = batch_bytes + batch_bytes / 4 + kFixedBound * batch_records;
    if (hipSetDevice(device) != hipSuccess) {
        *err = HONU_E_NO_DEVICE;
        delete f;
        return nullptr;
    }
    for (Slot &s : f->slot) {
        const int32_t st = put_slot_alloc(f, s);
        if (st != HONU_OK) {
            *err = st;
            honu_put_feed_destroy(f);
            return nullptr;
        }
    }
    return f;
}

void honu_put_feed_destroy(honu_put_feed *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    for (Slot &s : f->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        put_slot_free(s);
    }
    delete f;
}

static Slot *put_filling(honu_put_feed *f, int32_t *err) {
    Slot &s = f->slot[f->cur];
    if (s.state == INFLIGHT) {
        *err = HONU_E_ARG;  // its batch was submitted and not waited for
        return nullptr;
    }
    if (s.state == DONE) {
        s.state = FREE;
        s.n = s.var = s.acl = s.reg = s.pay = s.budget = s.bound = 0;
        s.h_poff[0] = 0;
    }
    return &s;
}

int32_t honu_put_feed_append(honu_put_feed *f, const honu_meta *row, const uint8_t *var,
                             uint64_t var_len, const honu_acl *acl, uint64_t acl_len,
                             const uint32_t *regions, uint64_t regions_len, const uint8_t *data,
                             uint64_t data_len) {
    if (!f || !row || (data_len && !data)) return HONU_E_ARG;
    int32_t err = HONU_OK;
    Slot *sp = put_filling(f, &err);
    if (!sp) return err;
    Slot &s = *sp;
    PutPlan p;
    err = put_plan(f->cap_bytes, row, var, var_len, acl, acl_len, regions, regions_len, data_len, p);
    if (err) return err;
    if (s.n == f->cap_n || p.need > f->cap_bytes - s.budget) return HONU_ERR_CAPACITY;
    const uint64_t idx = s.n;
    put_place(s, p, data_len);
    put_fill(s, idx, p, row, var, acl, regions, data, data_len);
    return HONU_OK;
}

int32_t honu_put_feed_append_batch(honu_put_feed *f, const honu_meta *rows, uint64_t n,
                                   const uint8_t *var, uint64_t var_len, const honu_acl *acl,
                                   uint64_t acl_len, const uint32_t *regions, uint64_t regions_len,
                                   const uint8_t *payload, const uint64_t *payload_off,
                                   uint64_t *appended) {
    if (!f || (n && (!rows || !payload_off)) || !appended) return HONU_E_ARG;
    *appended = 0;
    int32_t st = HONU_OK;
    Slot *sp = put_filling(f, &st);
    if (!sp) return st;
    Slot &s = *sp;
    // phase 1, serial: check and place every record that goes in
    std::vector<PutPlan> plans;
    plans.reserve(n < f->cap_n - s.n ? n : f->cap_n - s.n);
    const uint64_t first = s.n;
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t a = payload_off[i], b = payload_off[i + 1];
        if (b < a || (b > a && !payload)) {
            st = b < a ? HONU_ERR_INPUT : HONU_E_ARG;
            break;
        }
        PutPlan p;
        st = put_plan(f->cap_bytes, rows + i, var, var_len, acl, acl_len, regions, regions_len,
                      b - a, p);
        if (st) break;
        if (s.n == f->cap_n || p.need > f->cap_bytes - s.budget) {
            st = HONU_ERR_CAPACITY;
            break;
        }
        put_place(s, p, b - a);
        plans.push_back(p);
        bytes += p.need;
    }
    // phase 2: the copies, record ranges over a few threads for big batches
    const uint64_t k = plans.size();
    honu::put_fill_batch(s, first, plans, bytes, rows, var, acl, regions, payload, payload_off);
    *appended = k;
    return st;
}

uint64_t honu_put_feed_pending(const honu_put_feed *f) {
    if (!f) return 0;
    const Slot &s = f->slot[f->cur];
    return s.state == FREE ? s.n : 0;
}

int32_t honu_put_feed_submit(honu_put_feed *f, uint64_t *ticket) {
    if (!f) return HONU_E_ARG;
    int32_t err = HONU_OK;
    Slot *sp = put_filling(f, &err);
    if (!sp) return err;
    Slot &s = *sp;
    PCHK(hipSetDevice(f->device));
    const uint64_t n = s.n;
    hipStream_t q = s.stream;
    PCHK(hipMemcpyAsync(s.d_poff, s.h_poff, 8 * (n + 1), hipMemcpyHostToDevice, q));
    if (n) PCHK(hipMemcpyAsync(s.d_meta, s.h_meta, sizeof(honu_meta) * n, hipMemcpyHostToDevice, q));
    if (s.var) PCHK(hipMemcpyAsync(s.d_var, s.h_var, s.var, hipMemcpyHostToDevice, q));
    if (s.acl) PCHK(hipMemcpyAsync(s.d_acl, s.h_acl, sizeof(honu_acl) * s.acl, hipMemcpyHostToDevice, q));
    if (s.reg) PCHK(hipMemcpyAsync(s.d_reg, s.h_reg, 4 * s.reg, hipMemcpyHostToDevice, q));
    if (s.pay) PCHK(hipMemcpyAsync(s.d_pay, s.h_pay, s.pay, hipMemcpyHostToDevice, q));
    err = honu_marshal_batch(s.ctx, s.d_meta, s.d_var, s.var, s.d_acl, s.acl, s.d_reg, s.reg,
                             s.d_pay, s.d_poff, n, s.d_out, f->out_cap, s.d_ooff, s.d_st, q);
    if (err) return err;
    PCHK(hipMemcpyAsync(s.h_ooff, s.d_ooff, 8 * (n + 1), hipMemcpyDeviceToHost, q));
    if (n) PCHK(hipMemcpyAsync(s.h_st, s.d_st, 4 * n, hipMemcpyDeviceToHost, q));
    // the bound, not the exact total: known now, so nothing waits here
    if (s.bound) PCHK(hipMemcpyAsync(s.h_out, s.d_out, s.bound, hipMemcpyDeviceToHost, q));
    s.state = INFLIGHT;
    s.ticket = f->next_ticket++;
    if (ticket) *ticket = s.ticket;
    f->cur ^= 1;
    return HONU_OK;
}

int32_t honu_put_feed_wait(honu_put_feed *f, uint64_t ticket, honu_put_result *out) {
    if (!f || !out) return HONU_E_ARG;
    Slot *sp = nullptr;
    for (Slot &s : f->slot)
        if (s.state != FREE && s.ticket == ticket) sp = &s;
    if (!sp) return HONU_E_ARG;
    Slot &s = *sp;
    PCHK(hipSetDevice(f->device));
    if (s.state == INFLIGHT) {
        PCHK(hipStreamSynchronize(s.stream));
        s.state = DONE;
    }
    out->n = s.n;
    out->records = s.h_out;
    out->rec_off = s.h_ooff;
    out->status = s.h_st;
    return HONU_OK;
}
