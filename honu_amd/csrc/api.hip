// api.hip — the C ABI (include/honu_codec.h) over the gfx950 kernels.
//
// One context per device: it owns the only allocations the library makes
// (per-record decode scratch, count/offset columns and scan partials), sized
// once for a maximum batch so that every codec call is allocation- and
// sync-free and can be captured into a hipGraph.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kernels.h"

using namespace honu;

struct honu_ctx {
    int device;
    uint64_t max_n;
    LaunchGeom geom;
    void *ws;
    uint64_t *counts;        // 3 * max_n
    uint64_t *offs;          // 3 * max_n
    uint64_t *totals;        // 4 (3: decode totals; word 3: the HBM probe's sink)
    DecodeScratch *scratch;  // max_n
    uint32_t *reg_inline;    // 8 * max_n: region ids handed from the group parse to fill
    EncAclPos *enc_acl;      // max_n: ACL list hand-over, lane encoder -> group ACL encoder
    FusedState dec;          // look-back state of the fused decode (fused.hip)
    uint64_t lb_bytes;       // the look-back blocks + status words + copy counters, from dec.lb
    ScanState scan;          // look-back state of the one-launch scans (scan.hip)
    // speculation back-off (fused.hip): a guarded recovery launch that ran sets
    // *dec.spec_seen (pinned host words, written by the device); the next call
    // sees it and decodes SPEC_BACKOFF_CALLS calls without speculation, so a stream
    // of batches with malformed records pays ~1.1x instead of ~2x per batch
    uint32_t spec_off;       // calls left without speculation
    int speculate;           // honu_ctx_set_param("speculate"): 0 off, 1 on, 2 where it hides a wait
    // honu_encode_records: the ACL lists' kernel on a stream of the context's
    // own, beside the header/tail encoder (forked from and joined back into
    // the caller's stream by events)
    hipStream_t aux;
    hipEvent_t ev_fork, ev_join;
    int enc_fork;            // honu_ctx_set_param("encode_fork", 0 off / 1 on / 2 auto: when lane_blocks caps the grid)
    bool acl_inplace;        // honu_ctx_set_param("acl_inplace"): decode returns all-present ACL lists in place
    bool reg_inplace;        // honu_ctx_set_param("regions_inplace"): decode returns region lists in place
    int guard_blocks;        // honu_ctx_set_param("guard_blocks"): one-wave workgroups of the guarded launch
                             // (0: as many as the speculative launch has waves)
    uint32_t copy_seq;       // copy calls issued: call k takes counter line k % COPY_TICKET_LINES
    int enc_form;            // the last honu_encode_records* call: 0 none, 1 plain, 2 units
};

// The launch geometry of one payload-copy call: the context's, with the
// range-tail counters of the next line of the ring (kernels.h), so copy calls
// in flight at once on different streams each count on a line of their own
// (one shared line let a launch skip tails another one took).
static LaunchGeom copy_geom(honu_ctx *ctx) {
    LaunchGeom g = ctx->geom;
    const uint32_t k = __atomic_fetch_add(&ctx->copy_seq, 1u, __ATOMIC_RELAXED) % COPY_TICKET_LINES;
    g.copy_tickets = ctx->geom.copy_tickets + (uint64_t)k * COPY_TICKET_STRIDE;
    return g;
}
static constexpr uint32_t SPEC_BACKOFF_CALLS = 16;
// Speculation only where it hides a look-back wait (materialising decodes,
// table forms): a zero-copy in-place launch skips those waits already, and
// there the flag gather and guard cost more than the walk's own flag check
// (round 6: 0.392 vs 0.427 ms for 1M Large records, profiles/r06).
#ifndef SPECULATE_DEFAULT
#define SPECULATE_DEFAULT 2
#endif

static thread_local char g_last_error[256];

static int32_t hip_fail(hipError_t e, const char *what) {
    snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
    return HONU_E_HIP;
}
#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t e_ = (x);                       \
        if (e_ != hipSuccess) return hip_fail(e_, #x); \
    } while (0)

static int32_t arg_fail(const char *what) {
    snprintf(g_last_error, sizeof g_last_error, "invalid argument: %s", what);
    return HONU_E_ARG;
}

static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the caller's workspace against the `need` bytes that fn_of_arg ("honu_x_workspace(n)") returns: no
// smaller, and non-null and 256-byte aligned when any are needed; 0 or the refusal
static int32_t work_args(uint64_t need, const void *d_work, uint64_t work_bytes, const char *fn_of_arg) {
    if (work_bytes < need) {
        char what[128];
        snprintf(what, sizeof what, "workspace smaller than %s", fn_of_arg);
        return arg_fail(what);
    }
    if (need && (!d_work || !aligned(d_work, 256))) return arg_fail("workspace must be non-null and 256-byte aligned");
    return HONU_OK;
}

// record_variant 5 runs the batch entries through the split kernels of
// variant 0, 6 through the fused decode at every size; variant 0 picks by size
#define FUSED_DECODE_MIN_RECORDS (48ull << 10)

// Fused kernels: persistent waves (2 workgroups of 4 waves per CU fit the LDS
// and registers), fewer under a lane_blocks cap.
static int fused_blocks(const LaunchGeom &g) {
    const int resident = 2 * g.num_cu;
    return g.lane_blocks > 0 && g.lane_blocks < resident ? g.lane_blocks : resident;
}

// p: count elements at byte offset `at` of base; returns the offset after them
template <class T>
static uint64_t carve(T *&p, void *base, uint64_t at, uint64_t count) {
    p = (T *)((uintptr_t)base + at);
    return at + count * sizeof(T);
}

// The context's workspace laid out in order from base; returns the end offset.
// A null base gives the bytes to allocate (the pointers are then not for use).
// From dec.lb to the end: what a clean look-back state zeroes (lb_bytes).
static uint64_t ctx_carve(honu_ctx *c, void *base) {
    const uint64_t n = c->max_n;
    const uint64_t tiles = (n + HONU_WAVE - 1) / HONU_WAVE;
    // 3 status words per tile, then 3 per 64-tile group (lookback.h
    // lb_resolve_grouped*)
    const uint64_t groups = (tiles / HONU_WAVE + 1) > LB_GROUPS ? tiles / HONU_WAVE + 1 : LB_GROUPS;
    uint64_t at = 0;
    at = carve(c->counts, base, at, 3 * n);
    at = carve(c->offs, base, at, 3 * n);
    at = carve(c->totals, base, at, 4);
    at = carve(c->scratch, base, at, n);
    at = carve(c->reg_inline, base, at, 8 * n);
    at = carve(c->enc_acl, base, at, n);
    at = carve(c->dec.lb, base, at, 1);
    at = carve(c->scan.lb, base, at, 1);
    at = carve(c->dec.status, base, at, 3 * tiles);
    at = carve(c->dec.gstatus, base, at, 3 * groups);  // (the same epoch scheme as the tile words)
    c->dec.words = 3 * tiles + 3 * groups;
    c->scan.words = scan_status_words(n);
    at = carve(c->scan.status, base, at, c->scan.words);
    // the copies' range-tail counters: a ring of 128-byte lines
    return carve(c->geom.copy_tickets, base, at, (uint64_t)COPY_TICKET_LINES * COPY_TICKET_STRIDE);
}

// A stream with a CU mask or a non-default priority: honu_encode_records then
// does not fork the ACL lists onto the context's own (unmasked, default
// priority) stream, so the work stays where the caller put it.
static bool stream_is_restricted(hipStream_t s, int num_cu) {
    int prio = 0;
    if (hipStreamGetPriority(s, &prio) == hipSuccess && prio != 0) return true;
    uint32_t mask[32] = {0};
    const uint32_t words = (uint32_t)((num_cu + 31) / 32);
    if (words > 32 || hipExtStreamGetCUMask(s, words, mask) != hipSuccess) return false;
    bool any = false, all = true;  // (an all-zero answer: no mask)
    for (int i = 0; i < num_cu; i++) {
        const bool on = mask[i / 32] >> (i % 32) & 1u;
        any |= on;
        all &= on;
    }
    return any && !all;
}

// The product library takes its configuration from honu_ctx_set_param only:
// it behaves the same whatever the caller's process environment holds. The
// A/B build (make ab) also reads HONU_* variables at context creation, for
// tools/*.sh sweeps that cannot set params.
static int env_int(const char *name, int dflt) {
#ifdef HONU_AB
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

extern "C" {

uint32_t honu_abi_version(void) { return HONU_ABI_VERSION; }
uint64_t honu_sizeof_meta(void) { return sizeof(honu_meta); }
uint64_t honu_sizeof_acl(void) { return sizeof(honu_acl); }
uint64_t honu_sizeof_collection(void) { return sizeof(honu_collection); }
uint64_t honu_sizeof_index(void) { return sizeof(honu_index); }
uint64_t honu_sizeof_record_info(void) { return sizeof(honu_record_info); }
uint64_t honu_sizeof_seek(void) { return sizeof(honu_seek); }
uint64_t honu_sizeof_list_row(void) { return sizeof(honu_list_row); }
uint64_t honu_sizeof_next(void) { return sizeof(honu_next); }
const char *honu_last_error(void) { return g_last_error; }

const char *honu_status_string(int32_t st) {
    switch (st) {
    case HONU_OK: return "ok";
    case HONU_ERR_BAD_VERSION: return "object is malformed: cannot decode specified version";
    case HONU_ERR_MALFORMED: return "object is malformed: cannot parse data or metadata";
    case HONU_ERR_EOF: return "EOF";
    case HONU_ERR_UNEXPECTED_EOF: return "unexpected EOF";
    case HONU_ERR_NO_LENGTH: return "field not written with length value";
    case HONU_ERR_PARSE_BOOLEAN: return "could not parse boolean value";
    case HONU_ERR_PARSE_VARINT: return "could not parse varint";
    case HONU_ERR_PANIC: return "input on which the Go reference panics";
    case HONU_ERR_CAPACITY: return "output capacity exceeded";
    case HONU_ERR_INPUT: return "input span or list outside its arena";
    case HONU_UNPARSED: return "metadata not decoded (headers only)";
    case HONU_E_ARG: return "invalid argument";
    case HONU_E_WORKSPACE: return "batch larger than the context's reserved records";
    case HONU_E_HIP: return "HIP runtime error";
    case HONU_E_NO_DEVICE: return "no gfx950 device";
    default: return "unknown status";
    }
}

honu_ctx *honu_ctx_create(int device, uint64_t max_records, int32_t *err) {
    int32_t dummy;
    if (!err) err = &dummy;
    *err = HONU_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        snprintf(g_last_error, sizeof g_last_error, "no HIP device %d (count %d)", device, count);
        *err = HONU_E_NO_DEVICE;
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess ||
        strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_last_error, sizeof g_last_error, "device %d is %s, this build targets gfx950",
                 device, prop.gcnArchName);
        *err = HONU_E_NO_DEVICE;
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        *err = HONU_E_HIP;
        return nullptr;
    }
    honu_ctx *c = (honu_ctx *)calloc(1, sizeof(honu_ctx));
    if (!c) {
        *err = HONU_E_HIP;
        return nullptr;
    }
    // every failure below ends here: whatever was created is destroyed
    auto fail = [&](int32_t e, const char *what) -> honu_ctx * {
        if (what) snprintf(g_last_error, sizeof g_last_error, "%s", what);
        if (c->ev_join) (void)hipEventDestroy(c->ev_join);
        if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
        if (c->aux) (void)hipStreamDestroy(c->aux);
        if (c->dec.spec_seen) (void)hipHostFree(c->dec.spec_seen);
        if (c->ws) (void)hipFree(c->ws);
        free(c);
        *err = e;
        return nullptr;
    };
    c->device = device;
    c->max_n = max_records ? max_records : 1;
    c->geom.num_cu = prop.multiProcessorCount;
    c->geom.per_record_blocks = env_int("HONU_RECORD_BLOCKS", prop.multiProcessorCount * 8);
    c->geom.lane_blocks = env_int("HONU_LANE_BLOCKS", 0);
    c->geom.copy_blocks = env_int("HONU_COPY_BLOCKS", prop.multiProcessorCount * 2);
    c->geom.record_variant = env_int("HONU_RECORD_VARIANT", 0);
    if (c->geom.record_variant != 5 && c->geom.record_variant != 6)
        c->geom.record_variant = 0;
    c->acl_inplace = env_int("HONU_ACL_INPLACE", 1) != 0;
    c->reg_inplace = env_int("HONU_REGIONS_INPLACE", 1) != 0;
    c->guard_blocks = env_int("HONU_GUARD_BLOCKS", 0);
    if (c->guard_blocks < 0) c->guard_blocks = 0;
    const uint64_t end = ctx_carve(c, nullptr), bytes = end + 256;
    if (hipMalloc(&c->ws, bytes) != hipSuccess) {
        c->ws = nullptr;
        char msg[96];
        snprintf(msg, sizeof msg, "hipMalloc(%llu) failed", (unsigned long long)bytes);
        return fail(HONU_E_HIP, msg);
    }
    if (hipHostMalloc((void **)&c->dec.spec_seen, 2 * sizeof(uint32_t),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        c->dec.spec_seen = nullptr;
        return fail(HONU_E_HIP, "hipHostMalloc(spec_seen) failed");
    }
    c->dec.spec_seen[0] = 0;
    c->dec.spec_seen[1] = 0;
    c->speculate = SPECULATE_DEFAULT;
    c->enc_fork = env_int("HONU_ENCODE_FORK", 2);
    if (c->enc_fork < 0 || c->enc_fork > 2) c->enc_fork = 2;
    if (hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess) {
        c->aux = nullptr;
        return fail(HONU_E_HIP, "stream creation failed");
    }
    if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess) {
        c->ev_fork = nullptr;
        return fail(HONU_E_HIP, "event creation failed");
    }
    if (hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        c->ev_join = nullptr;
        return fail(HONU_E_HIP, "event creation failed");
    }
    ctx_carve(c, c->ws);
    c->lb_bytes = (uint64_t)((uint8_t *)c->ws + end - (uint8_t *)c->dec.lb);
    c->geom.copy_steal = 1;
    c->scan.max_blocks = 4 * prop.multiProcessorCount;
    // clean look-back state: epoch 0 with no published tile. On a stream of
    // the call's own, so work other contexts have in flight keeps running.
    hipStream_t s = nullptr;
    bool ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipMemsetAsync(c->dec.lb, 0, c->lb_bytes, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (s) (void)hipStreamDestroy(s);
    if (!ok) return fail(HONU_E_HIP, "look-back state initialisation failed");
    return c;
}

int32_t honu_ctx_reset(honu_ctx *ctx, void *stream) {
    if (!ctx) return arg_fail("ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(ctx->dec.lb, 0, ctx->lb_bytes, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return HONU_OK;
}

void honu_ctx_destroy(honu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->aux);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    (void)hipStreamDestroy(ctx->aux);
    (void)hipFree(ctx->ws);
    (void)hipHostFree(ctx->dec.spec_seen);
    free(ctx);
}

uint64_t honu_ctx_max_records(const honu_ctx *ctx) { return ctx ? ctx->max_n : 0; }

int32_t honu_ctx_set_param(honu_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return arg_fail("ctx/name");
    if (!strcmp(name, "copy_blocks") && value > 0) ctx->geom.copy_blocks = (int)value;
    else if (!strcmp(name, "record_blocks") && value > 0) ctx->geom.per_record_blocks = (int)value;
    else if (!strcmp(name, "lane_blocks") && value >= 0) ctx->geom.lane_blocks = (int)value;
    else if (!strcmp(name, "speculate") && value >= 0 && value <= 2) ctx->speculate = (int)value;
    else if (!strcmp(name, "encode_fork") && value >= 0 && value <= 2) ctx->enc_fork = (int)value;
    else if (!strcmp(name, "acl_inplace") && (value == 0 || value == 1)) ctx->acl_inplace = value != 0;
    else if (!strcmp(name, "regions_inplace") && (value == 0 || value == 1)) ctx->reg_inplace = value != 0;
    else if (!strcmp(name, "guard_blocks") && value >= 0 && value <= 65536) ctx->guard_blocks = (int)value;
    else if (!strcmp(name, "speculate_backoff") && value >= 0 && value <= (int64_t)SPEC_BACKOFF_CALLS) {
        __atomic_store_n(ctx->dec.spec_seen, 0u, __ATOMIC_RELAXED);
        ctx->spec_off = (uint32_t)value;
    }
    else if (!strcmp(name, "copy_steal") && (value == 0 || value == 1)) ctx->geom.copy_steal = (int)value;
    else if (!strcmp(name, "copy_variant") || !strcmp(name, "encode_variant") || !strcmp(name, "inline_recovery")) {
        // kept for compatibility: there is one copy engine, one header/tail encoder and one
        // recovery form (the guarded launch), each form 0
        if (value != 0) return arg_fail(name);
    }
    else if (!strcmp(name, "record_variant") &&
             (value == 0 || value == 5 || value == 6))
        ctx->geom.record_variant = (int)value;
    else if (!strcmp(name, "seek_variant") && value >= 0 && value <= 2) ctx->geom.seek_variant = (int)value;
    else return arg_fail(name);
    return HONU_OK;
}

int32_t honu_ctx_get_param(const honu_ctx *ctx, const char *name, int64_t *value) {
    if (!ctx || !name || !value) return arg_fail("ctx/name/value");
    if (!strcmp(name, "copy_blocks")) *value = ctx->geom.copy_blocks;
    else if (!strcmp(name, "record_blocks")) *value = ctx->geom.per_record_blocks;
    else if (!strcmp(name, "lane_blocks")) *value = ctx->geom.lane_blocks;
    else if (!strcmp(name, "speculate")) *value = ctx->speculate;
    else if (!strcmp(name, "encode_fork")) *value = ctx->enc_fork;
    else if (!strcmp(name, "acl_inplace")) *value = ctx->acl_inplace ? 1 : 0;
    else if (!strcmp(name, "regions_inplace")) *value = ctx->reg_inplace ? 1 : 0;
    else if (!strcmp(name, "guard_blocks")) *value = ctx->guard_blocks;
    else if (!strcmp(name, "recoveries"))  // recovery launches that ran, since the context was created
        *value = __atomic_load_n(ctx->dec.spec_seen + 1, __ATOMIC_RELAXED);
    else if (!strcmp(name, "speculate_backoff"))  // calls the next call starts without speculation
        *value = __atomic_load_n(ctx->dec.spec_seen, __ATOMIC_RELAXED) ? SPEC_BACKOFF_CALLS : ctx->spec_off;
    else if (!strcmp(name, "copy_steal")) *value = ctx->geom.copy_steal;
    else if (!strcmp(name, "copy_variant") || !strcmp(name, "encode_variant") || !strcmp(name, "inline_recovery"))
        *value = 0;  // (see set_param)
    else if (!strcmp(name, "record_variant")) *value = ctx->geom.record_variant;
    else if (!strcmp(name, "walk_flag_checks")) *value = decode_walk_flag_checks();  // read only: the build's
    else if (!strcmp(name, "sort_tile")) *value = sort_tile();  // read only: keys per workgroup per sort pass
    else if (!strcmp(name, "seek_variant")) *value = ctx->geom.seek_variant;
    else if (!strcmp(name, "seek_fence")) *value = seek_fence();  // read only: keys of the fenced seek's LDS stage
    else if (!strcmp(name, "seek_auto_probes")) *value = (int64_t)seek_auto_probes();  // read only: what
    else if (!strcmp(name, "seek_auto_keys")) *value = (int64_t)seek_auto_keys();      // "seek_variant" 0 picks by
    else if (!strcmp(name, "merge_tile")) *value = merge_tile();  // read only: output positions per workgroup of the merge
    else if (!strcmp(name, "delete_tile")) *value = delete_tile();  // read only: column positions per workgroup of the delete
    else if (!strcmp(name, "list_tile")) *value = list_tile();    // read only: output rows per workgroup of the list
    else if (!strcmp(name, "list_stage")) *value = list_stage();  // read only: range offsets a workgroup of the list stages in LDS
    else if (!strcmp(name, "filter_tile")) *value = filter_tile();  // read only: list rows per workgroup of the filter
    else if (!strcmp(name, "compare_tile")) *value = compare_tile();    // read only: objects per workgroup of the compare
    else if (!strcmp(name, "compare_stage")) *value = compare_stage();  // read only: peer rows a workgroup of the compare stages in LDS
    else if (!strcmp(name, "reclaim_tile")) *value = reclaim_tile();  // read only: records per workgroup of the reclaim
    else if (!strcmp(name, "route_stage")) *value = route_stage();  // read only: table rows a workgroup of the route stages in LDS
    else if (!strcmp(name, "merge_buckets_stage")) *value = merge_buckets_stage();  // read only: buckets of a tile whose offsets the bucketed merge stages in LDS
    else return arg_fail(name);
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
int32_t honu_encode_sizes(honu_ctx *ctx, const honu_meta *d_meta, uint64_t var_len,
                          const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                          uint64_t regions_len, const uint64_t *d_payload_off, uint64_t n,
                          uint64_t *d_sizes, int32_t *d_status, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_meta || !d_payload_off || !d_sizes)) return arg_fail("null pointer");
    if (!aligned(d_meta, 16)) return arg_fail("rows must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4)) return arg_fail("tables must be 4-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_encode_sizes_grp(d_meta, var_len, d_acl, acl_len, d_regions, regions_len,
                                   d_payload_off, n, d_sizes, d_status, ctx->geom.lane_blocks,
                                   (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_exclusive_scan(honu_ctx *ctx, const uint64_t *d_in, uint64_t n, uint64_t *d_out,
                            void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_scan(d_in, n, 1, d_out, d_out + n, ctx->scan, (hipStream_t)stream));
    return HONU_OK;
}

// units: the payload arena (honu_encode_records_units), or null
static int32_t encode_records(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                              const honu_acl *d_acl, const uint32_t *d_regions, const uint8_t *units,
                              const uint64_t *d_payload_off, uint64_t n, uint8_t *d_out,
                              uint64_t out_cap, const uint64_t *d_out_off, int32_t *d_status,
                              void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_meta || !d_payload_off || !d_out || !d_out_off || !d_status))
        return arg_fail("null pointer");
    if (!aligned(d_out, 16) || !aligned(d_meta, 16))
        return arg_fail("records arena and rows must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4)) return arg_fail("tables must be 4-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    ctx->enc_form = units ? 2 : 1;  // (the payload call checks it: never mix the two forms)
    // header + tail with the ACL lists' partial end chunks (one record per
    // lane), then the lists' whole chunks (16 lanes per record). (Measured and
    // not kept, source in commit 426ce70 enc.hip: the whole record by a
    // 16-lane group in one launch, DESIGN_HISTORY "Round 3: a header/tail
    // encoder without a serial writer".)
    hipStream_t s = (hipStream_t)stream;
    // (auto: not on a CU-masked or prioritised caller stream, whose placement
    // the fork would escape)
    const bool fork = ctx->enc_fork == 1 ||
                      (ctx->enc_fork == 2 && ctx->geom.lane_blocks > 0 && n &&
                       !stream_is_restricted(s, ctx->geom.num_cu));
    if (fork && n) {
        // the lists' whole chunks on the context's own stream, beside the
        // header/tail encoder (disjoint bytes: the lane encoder writes the
        // lists' partial end chunks, or skips a list with nil entries whole)
        HIPCHK(hipEventRecord(ctx->ev_fork, s));
        HIPCHK(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
        HIPCHK(launch_encode_acl_grp_self(d_meta, d_acl, d_payload_off, n, d_out, out_cap, d_out_off, d_status,
                                          ctx->geom.lane_blocks, ctx->aux));
        HIPCHK(hipEventRecord(ctx->ev_join, ctx->aux));
        HIPCHK(launch_encode_meta_lane(d_meta, d_var, d_acl, d_regions, d_payload_off, n, d_out,
                                       out_cap, d_out_off, d_status, ctx->enc_acl,
                                       ctx->geom.lane_blocks, ctx->geom.num_cu, units, s));
        HIPCHK(hipStreamWaitEvent(s, ctx->ev_join, 0));
        return HONU_OK;
    }
    HIPCHK(launch_encode_meta_lane(d_meta, d_var, d_acl, d_regions, d_payload_off, n, d_out,
                                   out_cap, d_out_off, d_status, ctx->enc_acl,
                                   ctx->geom.lane_blocks, ctx->geom.num_cu, units, s));
    HIPCHK(launch_encode_acl_grp(d_meta, d_acl, n, d_out, d_status, ctx->enc_acl,
                                 ctx->geom.lane_blocks, s));
    return HONU_OK;
}

int32_t honu_encode_records(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                            const honu_acl *d_acl, const uint32_t *d_regions,
                            const uint64_t *d_payload_off, uint64_t n, uint8_t *d_out,
                            uint64_t out_cap, const uint64_t *d_out_off, int32_t *d_status,
                            void *stream) {
    return encode_records(ctx, d_meta, d_var, d_acl, d_regions, nullptr, d_payload_off, n, d_out, out_cap,
                          d_out_off, d_status, stream);
}

int32_t honu_encode_records_units(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                                  const honu_acl *d_acl, const uint32_t *d_regions,
                                  const uint8_t *d_payload, const uint64_t *d_payload_off, uint64_t n,
                                  uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                                  int32_t *d_status, void *stream) {
    if (n && !d_payload) return arg_fail("null pointer");
    return encode_records(ctx, d_meta, d_var, d_acl, d_regions, d_payload, d_payload_off, n, d_out, out_cap,
                          d_out_off, d_status, stream);
}

static int32_t encode_payloads(honu_ctx *ctx, const uint8_t *d_payload, const uint64_t *d_payload_off,
                               uint64_t n, uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                               const int32_t *d_status, bool units, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_payload_off || !d_out || !d_out_off || !d_status)) return arg_fail("null pointer");
    if (!aligned(d_out, 16)) return arg_fail("records arena must be 16-byte aligned");
    // the units pair completes only what its own records call left out: a
    // payload call of the other form than the context's last records call
    // would leave bytes unwritten (or write them twice) with every status OK
    if (ctx->enc_form && ctx->enc_form != (units ? 2 : 1))
        return arg_fail(units ? "honu_encode_payloads_units after honu_encode_records (mixed forms)"
                              : "honu_encode_payloads after honu_encode_records_units (mixed forms)");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_encode_copy(copy_geom(ctx), d_payload, d_payload_off, n, d_out, out_cap, d_out_off,
                              d_status, units, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_encode_payloads(honu_ctx *ctx, const uint8_t *d_payload, const uint64_t *d_payload_off,
                             uint64_t n, uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                             const int32_t *d_status, void *stream) {
    return encode_payloads(ctx, d_payload, d_payload_off, n, d_out, out_cap, d_out_off, d_status, false, stream);
}

int32_t honu_encode_payloads_units(honu_ctx *ctx, const uint8_t *d_payload, const uint64_t *d_payload_off,
                                   uint64_t n, uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                                   const int32_t *d_status, void *stream) {
    return encode_payloads(ctx, d_payload, d_payload_off, n, d_out, out_cap, d_out_off, d_status, true, stream);
}

int32_t honu_encode(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var, uint64_t var_len,
                    const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                    uint64_t regions_len, const uint8_t *d_payload, const uint64_t *d_payload_off,
                    uint64_t n, uint8_t *d_out, uint64_t out_cap, const uint64_t *d_out_off,
                    int32_t *d_status, void *stream) {
    (void)var_len;
    (void)acl_len;
    (void)regions_len;
    if (!d_payload) {  // a batch of empty payloads only (nothing to copy): the plain pair,
                       // which reads the arena only for a non-empty payload
        int32_t st = honu_encode_records(ctx, d_meta, d_var, d_acl, d_regions, d_payload_off, n, d_out,
                                         out_cap, d_out_off, d_status, stream);
        if (st) return st;
        return honu_encode_payloads(ctx, d_payload, d_payload_off, n, d_out, out_cap, d_out_off, d_status,
                                    stream);
    }
    // the payload-unit pair (one kernel per 64-byte unit of the output)
    int32_t st = honu_encode_records_units(ctx, d_meta, d_var, d_acl, d_regions, d_payload, d_payload_off, n,
                                           d_out, out_cap, d_out_off, d_status, stream);
    if (st) return st;
    return honu_encode_payloads_units(ctx, d_payload, d_payload_off, n, d_out, out_cap, d_out_off,
                                      d_status, stream);
}

int32_t honu_marshal_batch(honu_ctx *ctx, const honu_meta *d_meta, const uint8_t *d_var,
                           uint64_t var_len, const honu_acl *d_acl, uint64_t acl_len,
                           const uint32_t *d_regions, uint64_t regions_len,
                           const uint8_t *d_payload, const uint64_t *d_payload_off, uint64_t n,
                           uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off,
                           int32_t *d_status, void *stream) {
    // the checks of the phases below, before the first of them launches: a
    // refused call has stored nothing
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_meta || !d_payload_off || !d_out || !d_out_off || !d_status)) return arg_fail("null pointer");
    if (!aligned(d_out, 16) || !aligned(d_meta, 16))
        return arg_fail("records arena and rows must be 16-byte aligned");
    int32_t st = honu_encode_sizes(ctx, d_meta, var_len, d_acl, acl_len, d_regions, regions_len,
                                   d_payload_off, n, d_out_off, d_status, stream);
    if (st) return st;
    st = honu_exclusive_scan(ctx, d_out_off, n, d_out_off, stream);
    if (st) return st;
    return honu_encode(ctx, d_meta, d_var, var_len, d_acl, acl_len, d_regions, regions_len,
                       d_payload, d_payload_off, n, d_out, out_cap, d_out_off, d_status, stream);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
int32_t honu_decode_parse(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                          uint64_t n, honu_meta *d_meta, honu_record_info *d_info, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rec || !d_rec_off || !d_meta || !d_info)) return arg_fail("null pointer");
    if (!aligned(d_rec, 16) || !aligned(d_meta, 16) || !aligned(d_info, 8))
        return arg_fail("records arena and rows must be 16-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_decode_parse_win(d_rec, d_rec_off, n, d_meta, d_info, ctx->scratch,
                                   ctx->reg_inline, ctx->counts, ctx->geom.lane_blocks,
                                   ctx->acl_inplace, ctx->reg_inplace, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_decode_tables(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n, honu_meta *d_meta,
                           honu_record_info *d_info, honu_acl *d_acl, uint64_t acl_cap,
                           uint32_t *d_regions, uint64_t regions_cap, uint8_t *d_data,
                           uint64_t data_cap, uint64_t *d_totals, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4) || !aligned(d_data, 16))
        return arg_fail("tables 4-byte / data arena 16-byte aligned");
    if (acl_cap && !d_acl) return arg_fail("acl table");
    if (regions_cap && !d_regions) return arg_fail("region table");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    uint64_t *tot = d_totals ? d_totals : ctx->totals;
    HIPCHK(launch_scan(ctx->counts, n, 3, ctx->offs, tot, ctx->scan, s));
    HIPCHK(launch_decode_fill_grp(d_rec, n, d_meta, d_info, ctx->scratch, ctx->reg_inline,
                                  ctx->counts, ctx->offs, d_acl, acl_cap, d_regions, regions_cap,
                                  d_data, data_cap, ctx->geom.lane_blocks, s));
    return HONU_OK;
}

int32_t honu_decode_payloads(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n,
                             const honu_record_info *d_info, uint8_t *d_data,
                             const uint64_t *d_totals, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (!d_data || !aligned(d_data, 16)) return arg_fail("data arena");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t *tot = d_totals ? d_totals : ctx->totals;
    HIPCHK(launch_decode_copy(copy_geom(ctx), d_rec, n, d_info, ctx->scratch, ctx->offs, tot, d_data,
                              (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_decode_fill(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                         uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                         honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                         uint64_t regions_cap, uint8_t *d_data, uint64_t data_cap,
                         uint64_t *d_totals, void *stream) {
    (void)d_rec_off;
    int32_t st = honu_decode_tables(ctx, d_rec, n, d_meta, d_info, d_acl, acl_cap, d_regions,
                                    regions_cap, d_data, data_cap, d_totals, stream);
    if (st || !d_data) return st;
    return honu_decode_payloads(ctx, d_rec, n, d_info, d_data, d_totals, stream);
}

int32_t honu_decode_records(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                            uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                            honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                            uint64_t regions_cap, int32_t materialize, uint64_t data_cap,
                            uint64_t *d_totals, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rec || !d_rec_off || !d_meta || !d_info)) return arg_fail("null pointer");
    if (!aligned(d_rec, 16) || !aligned(d_meta, 16) || !aligned(d_info, 8))
        return arg_fail("records arena and rows must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4)) return arg_fail("tables must be 4-byte aligned");
    if (acl_cap && !d_acl) return arg_fail("acl table");
    if (regions_cap && !d_regions) return arg_fail("region table");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    uint64_t *tot = d_totals ? d_totals : ctx->totals;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(tot, 0, 3 * sizeof(uint64_t), s));
        return HONU_OK;
    }
    // speculation back-off: a recovery of an earlier call has finished (the
    // word is read without waiting: a recovery still in flight is seen later)
    if (__atomic_load_n(ctx->dec.spec_seen, __ATOMIC_RELAXED)) {
        __atomic_store_n(ctx->dec.spec_seen, 0u, __ATOMIC_RELAXED);
        ctx->spec_off = SPEC_BACKOFF_CALLS;
    }
    // speculation hides the look-back wait; a zero-copy call with both list
    // forms in place has none to hide (fused.hip: tiles without table entries
    // do not wait), so "speculate" 2 (auto) decodes it without speculation:
    // no ACL flag burst after the walk re-reading the list's lines, no guarded
    // second launch
    const bool hides = materialize || !ctx->acl_inplace || !ctx->reg_inplace;
    const bool spec = (ctx->speculate == 1 || (ctx->speculate == 2 && hides)) && ctx->spec_off == 0;
    if (ctx->spec_off) ctx->spec_off--;
    const DecodeOut O{d_meta,   d_info,           d_acl,        acl_cap,   d_regions, regions_cap,
                      data_cap, materialize != 0, ctx->scratch, ctx->offs, tot,       ctx->reg_inplace};
    const FusedOpts opt{fused_blocks(ctx->geom), ctx->guard_blocks, spec, ctx->acl_inplace};
    HIPCHK(launch_decode_fused(d_rec, d_rec_off, n, O, ctx->dec, opt, s));
    return HONU_OK;
}

int32_t honu_decode_batch(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                          uint64_t n, honu_meta *d_meta, honu_record_info *d_info,
                          honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                          uint64_t regions_cap, uint8_t *d_data, uint64_t data_cap,
                          uint64_t *d_totals, void *stream) {
    // fused from 48 K records (measured: even with split at ~48 K, 3-5 % ahead
    // at 62-65 K, and the 1M Large bench's 62 K-record chunks 4 % faster with
    // one metadata launch per chunk beside the copies; below, the split
    // kernels' extra waves hide the walk's latency better), always with
    // record_variant 6
    const int rv = ctx ? ctx->geom.record_variant : 0;
    // every argument check of the phases below, before the first of them
    // launches: a refused call has stored nothing
    if (ctx && n > ctx->max_n) return HONU_E_WORKSPACE;
    if (!aligned(d_rec, 16) || !aligned(d_meta, 16) || !aligned(d_info, 8))
        return arg_fail("records arena and rows must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4) || !aligned(d_data, 16))
        return arg_fail("tables 4-byte / data arena 16-byte aligned");
    if ((acl_cap && !d_acl) || (regions_cap && !d_regions)) return arg_fail("table");
    if (rv == 6 || (rv == 0 && n >= FUSED_DECODE_MIN_RECORDS)) {
        int32_t st = honu_decode_records(ctx, d_rec, d_rec_off, n, d_meta, d_info, d_acl, acl_cap,
                                         d_regions, regions_cap, d_data != nullptr, data_cap,
                                         d_totals, stream);
        if (st || !d_data) return st;
        return honu_decode_payloads(ctx, d_rec, n, d_info, d_data, d_totals, stream);
    }
    int32_t st = honu_decode_parse(ctx, d_rec, d_rec_off, n, d_meta, d_info, stream);
    if (st) return st;
    return honu_decode_fill(ctx, d_rec, d_rec_off, n, d_meta, d_info, d_acl, acl_cap, d_regions,
                            regions_cap, d_data, data_cap, d_totals, stream);
}

int32_t honu_decode_headers(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                            uint64_t n, honu_record_info *d_info, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_rec || !d_rec_off || !d_info)) return arg_fail("null pointer");
    if (!aligned(d_info, 8)) return arg_fail("record info must be 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_decode_headers(d_rec, d_rec_off, n, d_info, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_decode_data_place(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                               uint64_t n, honu_record_info *d_info, uint64_t data_cap,
                               uint64_t *d_totals, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rec || !d_rec_off || !d_info)) return arg_fail("null pointer");
    if (!aligned(d_info, 8)) return arg_fail("record info must be 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (d_totals) HIPCHK(hipMemsetAsync(d_totals, 0, 8, s));
        return HONU_OK;
    }
    // spans -> exclusive scan of the aligned sizes (offs[n] = total) -> place
    HIPCHK(launch_decode_spans(d_rec, d_rec_off, n, d_info, ctx->scratch, ctx->counts, s));
    HIPCHK(launch_scan(ctx->counts, n, 1, ctx->offs, ctx->offs + n, ctx->scan, s));
    HIPCHK(launch_decode_data_place(n, d_info, ctx->offs, data_cap, s));
    if (d_totals)
        HIPCHK(hipMemcpyAsync(d_totals, ctx->offs + n, 8, hipMemcpyDeviceToDevice, s));
    return HONU_OK;
}

int32_t honu_decode_data_copy(honu_ctx *ctx, const uint8_t *d_rec, uint64_t n,
                              const honu_record_info *d_info, uint8_t *d_data, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rec || !d_info || !d_data)) return arg_fail("null pointer");
    if (!aligned(d_data, 16)) return arg_fail("data arena must be 16-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_span_copy(copy_geom(ctx), d_rec, n, d_info, ctx->scratch, ctx->offs, d_data,
                            (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_decode_data(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                         uint64_t n, honu_record_info *d_info, uint8_t *d_data, uint64_t data_cap,
                         uint64_t *d_totals, void *stream) {
    if (n && !d_data) return arg_fail("data arena");
    int32_t st = honu_decode_data_place(ctx, d_rec, d_rec_off, n, d_info, data_cap, d_totals, stream);
    if (st) return st;
    return honu_decode_data_copy(ctx, d_rec, n, d_info, d_data, stream);
}

int32_t honu_decode_keys(honu_ctx *ctx, const honu_meta *d_meta, const honu_record_info *d_info,
                         uint64_t n, uint8_t *d_keys, int32_t *d_key_status, void *stream) {
    if (!ctx) return arg_fail("ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_decode_keys(ctx->geom, d_meta, d_info, n, d_keys, d_key_status,
                              (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// key order (keys/keys.go:126-130) and version ranges (keys.go:73-92)
// ---------------------------------------------------------------------------
uint64_t honu_sort_keys_workspace(uint64_t n) { return sort_workspace_bytes(n); }

// the checks the two calls share; 0 or the refusal. (Not work_args: these calls look at the pointer first,
// whatever n, and which error a doubly wrong call reports is behaviour.)
static int32_t sort_args(honu_ctx *ctx, uint64_t n, const void *d_work, uint64_t work_bytes) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n || n > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    if (!d_work || !aligned(d_work, 256)) return arg_fail("workspace must be non-null and 256-byte aligned");
    if (work_bytes < sort_workspace_bytes(n)) return arg_fail("workspace smaller than honu_sort_keys_workspace(n)");
    return HONU_OK;
}

int32_t honu_sort_keys(honu_ctx *ctx, const uint8_t *d_keys, const int32_t *d_key_status, uint64_t n,
                       uint32_t *d_order, uint8_t *d_sorted, uint64_t *d_valid, void *d_work,
                       uint64_t work_bytes, void *stream) {
    const int32_t st = sort_args(ctx, n, d_work, work_bytes);
    if (st) return st;
    if (!d_valid || (n && (!d_keys || !d_order))) return arg_fail("null pointer");
    if (!aligned(d_key_status, 4) || !aligned(d_order, 4) || !aligned(d_valid, 8))
        return arg_fail("status and order 4-byte / valid count 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_sort_keys(d_keys, d_key_status, n, d_order, d_sorted, d_valid, d_work, ctx->scan,
                            ctx->max_n, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_key_objects(honu_ctx *ctx, const uint8_t *d_keys, const uint32_t *d_order,
                         const uint64_t *d_valid, uint64_t n, uint64_t *d_obj_off, uint32_t *d_latest,
                         uint64_t *d_objects, void *d_work, uint64_t work_bytes, void *stream) {
    const int32_t st = sort_args(ctx, n, d_work, work_bytes);
    if (st) return st;
    if (!d_valid || !d_obj_off || !d_objects || (n && (!d_keys || !d_order))) return arg_fail("null pointer");
    if (!aligned(d_order, 4) || !aligned(d_latest, 4) || !aligned(d_valid, 8) || !aligned(d_obj_off, 8) ||
        !aligned(d_objects, 8))
        return arg_fail("order and latest 4-byte / counts and offsets 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_objects(d_keys, d_order, d_valid, n, d_obj_off, d_latest, d_objects, d_work, ctx->scan,
                              (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// Cursor.Seek over the sorted column (iterator/cursor.go:44-55)
// ---------------------------------------------------------------------------
int32_t honu_key_seek(honu_ctx *ctx, const uint8_t *d_sorted, const uint64_t *d_valid, uint64_t n,
                      const uint8_t *d_probes, const int32_t *d_probe_status, uint32_t probe_len, uint64_t m,
                      const uint32_t *d_order, const honu_record_info *d_info, honu_seek *d_out,
                      void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    if (probe_len > HONU_KEY_LEN) return arg_fail("probe_len above 29");
    if (!d_valid || (n && !d_sorted) || (m && (!d_probes || !d_out))) return arg_fail("null pointer");
    if (d_info && !d_order) return arg_fail("d_info needs d_order");
    if (!aligned(d_out, 4) || !aligned(d_order, 4) || !aligned(d_probe_status, 4) || !aligned(d_valid, 8) ||
        !aligned(d_info, 8))
        return arg_fail("rows, order and status 4-byte / valid count and record info 8-byte aligned");
    if (m == 0) return HONU_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_seek(ctx->geom.seek_variant, ctx->geom.num_cu, d_sorted, d_valid, n, d_probes,
                           d_probe_status, probe_len, m, d_order, d_info, d_out, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// a batch of Puts into the sorted column (store.go:232, 395, 530)
// ---------------------------------------------------------------------------
int32_t honu_key_merge(honu_ctx *ctx, const uint8_t *d_sorted_a, const uint32_t *d_order_a,
                       const uint64_t *d_valid_a, uint64_t na, const uint8_t *d_sorted_b,
                       const uint32_t *d_order_b, const uint64_t *d_valid_b, uint64_t nb, uint32_t b_base,
                       uint8_t *d_sorted_out, uint32_t *d_order_out, uint64_t *d_valid_out, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (na > 0xFFFFFFFFull || nb > 0xFFFFFFFFull || na + nb > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    if ((uint64_t)b_base + nb > 0xFFFFFFFFull) return arg_fail("b_base + nb above 2^32 - 1");
    if (!d_valid_a || !d_valid_b || !d_valid_out) return arg_fail("null valid count");
    if ((na && !d_sorted_a) || (nb && !d_sorted_b) || (na + nb && !d_sorted_out)) return arg_fail("null column");
    if (d_order_out && (!d_order_a || !d_order_b)) return arg_fail("d_order_out needs both input orders");
    if (!aligned(d_order_a, 4) || !aligned(d_order_b, 4) || !aligned(d_order_out, 4) || !aligned(d_valid_a, 8) ||
        !aligned(d_valid_b, 8) || !aligned(d_valid_out, 8))
        return arg_fail("orders 4-byte / valid counts 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_merge(d_sorted_a, d_order_a, d_valid_a, na, d_sorted_b, d_order_b, d_valid_b, nb, b_base,
                            d_sorted_out, d_order_out, d_valid_out, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// a batch of Deletes from the sorted column (store.go:378-383, 399-404) and
// the rows a Put superseded
// ---------------------------------------------------------------------------
uint64_t honu_key_delete_workspace(uint64_t n) { return delete_workspace_bytes(n); }

int32_t honu_key_delete(honu_ctx *ctx, const uint8_t *d_sorted, const uint32_t *d_order, const uint64_t *d_valid,
                        uint64_t n, const uint8_t *d_del, const uint64_t *d_valid_del, uint64_t m,
                        uint32_t probe_len, uint32_t flags, uint8_t *d_sorted_out, uint32_t *d_order_out,
                        uint64_t *d_valid_out, uint64_t *d_removed, void *d_work, uint64_t work_bytes,
                        void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    // the tiles' kept counts are scanned with the context's scan state, which covers max_records rows
    if (delete_tiles(n) > ctx->max_n) return HONU_E_WORKSPACE;
    if (probe_len > HONU_KEY_LEN) return arg_fail("probe_len above 29");
    if (flags & ~(uint32_t)HONU_DELETE_SUPERSEDED) return arg_fail("unknown flag bits");
    if (!d_valid || !d_valid_out || (m && !d_valid_del)) return arg_fail("null valid count");
    if ((n && (!d_sorted || !d_sorted_out)) || (m && !d_del)) return arg_fail("null column");
    if (n && d_order_out && !d_order) return arg_fail("d_order_out needs d_order");
    if (!aligned(d_order, 4) || !aligned(d_order_out, 4) || !aligned(d_valid, 8) || !aligned(d_valid_del, 8) ||
        !aligned(d_valid_out, 8) || !aligned(d_removed, 8))
        return arg_fail("orders 4-byte / counts 8-byte aligned");
    const int32_t st = work_args(delete_workspace_bytes(n), d_work, work_bytes, "honu_key_delete_workspace(n)");
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_delete(d_sorted, d_order, d_valid, n, d_del, d_valid_del, m, probe_len, flags, d_sorted_out,
                             d_order_out, d_valid_out, d_removed, d_work, ctx->scan, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// a batch of cursor walks over seek ranges (iterator/cursor.go:57-89;
// collection.go:32-35, 97-110; store.go:379)
// ---------------------------------------------------------------------------
int32_t honu_key_list(honu_ctx *ctx, const uint8_t *d_sorted, const uint32_t *d_order, const uint64_t *d_valid,
                      uint64_t n, const honu_seek *d_ranges, uint64_t m, uint32_t limit, uint32_t flags,
                      const uint64_t *d_obj_off, const uint64_t *d_objects, const honu_record_info *d_info,
                      uint64_t *d_range_off, honu_list_row *d_rows, uint8_t *d_keys_out, uint64_t cap,
                      uint64_t *d_total, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || cap > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    // the m + 1 counts are scanned in place with the context's scan state, which covers max_records rows
    if (m + 1 > ctx->max_n) return HONU_E_WORKSPACE;
    if (flags & ~(uint32_t)(HONU_LIST_REVERSE | HONU_LIST_LATEST)) return arg_fail("unknown flag bits");
    if (!d_valid || !d_range_off || !d_total) return arg_fail("null d_valid, d_range_off or d_total");
    if ((m && !d_ranges) || (n && !d_sorted) || (cap && !d_rows)) return arg_fail("null ranges, column or rows");
    if ((flags & HONU_LIST_LATEST) && (!d_obj_off || !d_objects)) return arg_fail("LATEST needs d_obj_off and d_objects");
    if (d_info && !d_order) return arg_fail("d_info needs d_order");
    if (!aligned(d_ranges, 4) || !aligned(d_order, 4) || !aligned(d_valid, 8) || !aligned(d_objects, 8) ||
        !aligned(d_obj_off, 8) || !aligned(d_range_off, 8) || !aligned(d_total, 8) || !aligned(d_info, 8) ||
        !aligned(d_rows, 16))
        return arg_fail("ranges and order 4-byte / counts, offsets and info 8-byte / rows 16-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_list(ctx->geom.num_cu, d_sorted, d_order, d_valid, n, d_ranges, m, limit, flags, d_obj_off,
                           d_objects, d_info, d_range_off, d_rows, d_keys_out, cap, d_total, ctx->scan,
                           (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// Cursor.Object() over listed rows (iterator/cursor.go:31-38;
// collection.go:32-35, 97-110)
// ---------------------------------------------------------------------------
int32_t honu_key_fetch(honu_ctx *ctx, const honu_list_row *d_rows, const uint64_t *d_total, uint64_t cap,
                       const uint8_t *d_rec, const uint64_t *d_rec_off, uint64_t nrec, uint64_t rec_bytes,
                       uint32_t flags, uint64_t *d_val_off, int32_t *d_status, uint8_t *d_values, uint64_t val_cap,
                       uint64_t *d_val_total, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (cap > 0xFFFFFFFFull || nrec > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    // the cap + 1 lengths are scanned in place with the context's scan state, which covers max_records rows
    if (cap + 1 > ctx->max_n) return HONU_E_WORKSPACE;
    if (flags & ~(uint32_t)HONU_FETCH_LIVE) return arg_fail("unknown flag bits");
    if (!d_total || !d_val_off || !d_val_total) return arg_fail("null d_total, d_val_off or d_val_total");
    if ((cap && !d_rows) || !d_rec_off) return arg_fail("null rows or record offsets");
    if ((rec_bytes && !d_rec) || (val_cap && !d_values)) return arg_fail("null arena of a size other than 0");
    if (!aligned(d_status, 4) || !aligned(d_total, 8) || !aligned(d_rec_off, 8) || !aligned(d_val_off, 8) ||
        !aligned(d_val_total, 8) || !aligned(d_rows, 16))
        return arg_fail("status 4-byte / counts and offsets 8-byte / rows 16-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_fetch(copy_geom(ctx), d_rows, d_total, cap, d_rec, d_rec_off, nrec, rec_bytes, flags,
                            d_val_off, d_status, d_values, val_cap, d_val_total, ctx->scan, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// the live-object filter over listed rows (collection.go:132-134, 97-101,
// 53-54)
// ---------------------------------------------------------------------------
uint64_t honu_key_filter_workspace(uint64_t cap) { return filter_workspace_bytes(cap); }

int32_t honu_key_filter(honu_ctx *ctx, const honu_list_row *d_rows, const uint8_t *d_keys,
                        const uint64_t *d_range_off, uint64_t m, const uint64_t *d_total, uint64_t cap,
                        uint32_t flags, const uint64_t *d_valid, uint64_t n, const uint64_t *d_obj_off,
                        const uint32_t *d_latest, const uint64_t *d_objects, const honu_record_info *d_info,
                        honu_list_row *d_rows_out, uint8_t *d_keys_out, uint64_t *d_range_off_out,
                        uint64_t *d_total_out, void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (cap > 0xFFFFFFFFull || m > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    // the tiles' kept counts are scanned with the context's scan state, which covers max_records rows
    if (filter_tiles(cap) > ctx->max_n) return HONU_E_WORKSPACE;
    if (flags & ~(uint32_t)(HONU_FILTER_TOMBSTONE | HONU_FILTER_DELETED)) return arg_fail("unknown flag bits");
    if (!d_range_off || !d_total || !d_range_off_out || !d_total_out)
        return arg_fail("null d_range_off, d_total, d_range_off_out or d_total_out");
    if (cap && (!d_rows || !d_rows_out)) return arg_fail("null rows");
    if ((flags & HONU_FILTER_DELETED) && (!d_valid || !d_obj_off || !d_latest || !d_objects || !d_info))
        return arg_fail("DELETED needs d_valid, d_obj_off, d_latest, d_objects and d_info");
    if (!d_keys != !d_keys_out) return arg_fail("d_keys and d_keys_out go together");
    if ((d_rows && d_rows_out == d_rows) || d_range_off_out == d_range_off || d_total_out == d_total ||
        (d_keys && d_keys_out == d_keys))
        return arg_fail("an output is an input");
    if (!aligned(d_latest, 4) || !aligned(d_range_off, 8) || !aligned(d_total, 8) || !aligned(d_valid, 8) ||
        !aligned(d_obj_off, 8) || !aligned(d_objects, 8) || !aligned(d_info, 8) || !aligned(d_range_off_out, 8) ||
        !aligned(d_total_out, 8) || !aligned(d_rows, 16) || !aligned(d_rows_out, 16))
        return arg_fail("latest 4-byte / counts, offsets and info 8-byte / rows 16-byte aligned");
    const int32_t st = work_args(filter_workspace_bytes(cap), d_work, work_bytes, "honu_key_filter_workspace(cap)");
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_filter(d_rows, d_keys, d_range_off, m, d_total, cap, flags, d_valid, n, d_obj_off, d_latest,
                             d_objects, d_info, d_rows_out, d_keys_out, d_range_off_out, d_total_out, d_work,
                             ctx->scan, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// the version each of a batch of writes writes (lamport/pid.go:10-15;
// collection.go:75-137; store.go:361-395)
// ---------------------------------------------------------------------------
uint64_t honu_key_next_workspace(uint64_t m) { return next_workspace_bytes(m); }

int32_t honu_key_next(honu_ctx *ctx, const uint8_t *d_sorted, const uint64_t *d_valid, uint64_t n,
                      const uint32_t *d_order, const honu_record_info *d_info, const uint8_t *d_requests,
                      const int32_t *d_req_status, uint64_t m, uint32_t op, uint32_t pid, uint32_t region,
                      int64_t now, honu_next *d_out, uint8_t *d_keys_out, int32_t *d_key_status, honu_meta *d_meta,
                      void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx) return arg_fail("ctx");
    // the requests are sorted with the context's scan state, which covers max_records rows
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || m > ctx->max_n) return HONU_E_WORKSPACE;
    if (op > (uint32_t)HONU_NEXT_DELETE) return arg_fail("unknown op");
    if (!d_valid || (n && !d_sorted)) return arg_fail("null d_valid or column");
    if (m && (!d_requests || !d_out || !d_keys_out || !d_key_status))
        return arg_fail("null requests, d_out, d_keys_out or d_key_status");
    if (d_info && !d_order) return arg_fail("d_info needs d_order");
    if (d_requests && d_keys_out == d_requests) return arg_fail("an output is an input");
    if (!aligned(d_order, 4) || !aligned(d_req_status, 4) || !aligned(d_key_status, 4) || !aligned(d_out, 8) ||
        !aligned(d_valid, 8) || !aligned(d_info, 8) || !aligned(d_meta, 8))
        return arg_fail("order and statuses 4-byte / d_out, valid count, record info and rows 8-byte aligned");
    const int32_t st = work_args(next_workspace_bytes(m), d_work, work_bytes, "honu_key_next_workspace(m)");
    if (st) return st;
    if (m == 0) return HONU_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_next(d_sorted, d_valid, n, d_order, d_info, d_requests, d_req_status, m, op, pid, region, now,
                           d_out, d_keys_out, d_key_status, d_meta, d_work, ctx->scan, ctx->max_n,
                           (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// the versions of two columns compared object by object (lamport/scalar.go:15-78;
// keys/keys.go:35-36)
// ---------------------------------------------------------------------------
uint64_t honu_key_compare_workspace(uint64_t na) { return compare_workspace_bytes(na); }

int32_t honu_key_compare(honu_ctx *ctx, const uint8_t *d_sorted_a, const uint32_t *d_order_a,
                         const uint64_t *d_valid_a, uint64_t na, const uint64_t *d_obj_off_a,
                         const uint64_t *d_objects_a, const uint8_t *d_sorted_b, const uint64_t *d_valid_b,
                         uint64_t nb, honu_seek *d_out, uint32_t *d_peer, uint64_t *d_counts, void *d_work,
                         uint64_t work_bytes, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (na > 0xFFFFFFFFull || nb > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    if (!d_valid_a || !d_valid_b || !d_obj_off_a || !d_objects_a)
        return arg_fail("null valid count, d_obj_off_a or d_objects_a");
    if ((na && (!d_sorted_a || !d_out)) || (nb && !d_sorted_b)) return arg_fail("null column or d_out");
    if (!aligned(d_out, 4) || !aligned(d_peer, 4) || !aligned(d_order_a, 4) || !aligned(d_counts, 8) ||
        !aligned(d_valid_a, 8) || !aligned(d_valid_b, 8) || !aligned(d_obj_off_a, 8) || !aligned(d_objects_a, 8))
        return arg_fail("rows, peer and order 4-byte / counts and offsets 8-byte aligned");
    const int32_t st = work_args(compare_workspace_bytes(na), d_work, work_bytes, "honu_key_compare_workspace(na)");
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    // (make ab: HONU_COMPARE_STAGE below compare_stage sends more tiles down the unstaged path, 0 all of them)
    const uint32_t stage = (uint32_t)env_int("HONU_COMPARE_STAGE", (int)compare_stage());
    HIPCHK(launch_key_compare(d_sorted_a, d_order_a, d_valid_a, na, d_obj_off_a, d_objects_a, d_sorted_b, d_valid_b,
                              nb, stage, d_out, d_peer, d_counts, d_work, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// the space a Drop frees: the records arena and the per-record arrays
// compacted to the records the column still names (store.go:314-322, 399-404)
// ---------------------------------------------------------------------------
uint64_t honu_key_reclaim_workspace(uint64_t nrec) { return reclaim_workspace_bytes(nrec); }

int32_t honu_key_reclaim(honu_ctx *ctx, const uint32_t *d_order, const uint64_t *d_valid, uint64_t n,
                         const uint8_t *d_keys, const int32_t *d_key_status, const honu_record_info *d_info,
                         const uint8_t *d_rec, const uint64_t *d_rec_off, uint64_t nrec, uint64_t rec_bytes,
                         uint32_t flags, uint32_t *d_order_out, uint32_t *d_remap, uint32_t *d_source,
                         uint8_t *d_keys_out, int32_t *d_key_status_out, honu_record_info *d_info_out,
                         uint64_t *d_rec_off_out, int32_t *d_status, uint8_t *d_values, uint64_t val_cap,
                         uint64_t *d_kept, uint64_t *d_val_total, void *d_work, uint64_t work_bytes,
                         void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > 0xFFFFFFFFull || nrec > 0xFFFFFFFFull) return HONU_E_WORKSPACE;
    // the nrec + 1 lengths are scanned in place with the context's scan state, which covers max_records rows
    if (nrec + 1 > ctx->max_n) return HONU_E_WORKSPACE;
    if (flags) return arg_fail("unknown flag bits");
    if (!d_valid || !d_kept || !d_val_total) return arg_fail("null d_valid, d_kept or d_val_total");
    if (!d_rec_off || !d_rec_off_out || !d_source) return arg_fail("null record offsets or d_source");
    if (n && (!d_order || !d_order_out)) return arg_fail("null order");
    if ((rec_bytes && !d_rec) || (val_cap && !d_values)) return arg_fail("null arena of a size other than 0");
    if (!d_keys != !d_keys_out || !d_key_status != !d_key_status_out || !d_info != !d_info_out)
        return arg_fail("a per-record array and its output go together");
    if (!aligned(d_order, 4) || !aligned(d_order_out, 4) || !aligned(d_remap, 4) || !aligned(d_source, 4) ||
        !aligned(d_key_status, 4) || !aligned(d_key_status_out, 4) || !aligned(d_status, 4) ||
        !aligned(d_valid, 8) || !aligned(d_kept, 8) || !aligned(d_val_total, 8) || !aligned(d_rec_off, 8) ||
        !aligned(d_rec_off_out, 8) || !aligned(d_info, 8) || !aligned(d_info_out, 8))
        return arg_fail("orders, remap, source and statuses 4-byte / counts, offsets and info 8-byte aligned");
    const int32_t st =
        work_args(reclaim_workspace_bytes(nrec), d_work, work_bytes, "honu_key_reclaim_workspace(nrec)");
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_reclaim(copy_geom(ctx), d_order, d_valid, n, d_keys, d_key_status, d_info, d_rec, d_rec_off,
                              nrec, rec_bytes, d_order_out, d_remap, d_source, d_keys_out, d_key_status_out,
                              d_info_out, d_rec_off_out, d_status, d_values, val_cap, d_kept, d_val_total, d_work,
                              ctx->scan, (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// a batch taken apart by collection: one bucket per collection ID
// (store.go:236-240; tx.go:112-120, 141-158; collection.go:86)
// ---------------------------------------------------------------------------
uint64_t honu_key_route_workspace(uint64_t m) { return route_workspace_bytes(m); }

int32_t honu_key_route(honu_ctx *ctx, const uint8_t *d_ids, uint64_t id_stride, const int32_t *d_status, uint64_t m,
                       const uint32_t *d_seq, const uint8_t *d_table, uint64_t k, const uint8_t *d_keys,
                       uint32_t *d_bucket, honu_list_row *d_rows, uint32_t *d_local, uint8_t *d_keys_out,
                       uint64_t *d_bucket_off, uint64_t *d_bucket_count, void *d_work, uint64_t work_bytes,
                       void *stream) {
    if (!ctx) return arg_fail("ctx");
    // the classes are sorted with the context's scan state, which covers max_records rows
    if (m > 0xFFFFFFFFull || m > ctx->max_n || k > 0xFFFFFFFCull) return HONU_E_WORKSPACE;
    if (!d_bucket_off || !d_bucket_count) return arg_fail("null d_bucket_off or d_bucket_count");
    if (m && !d_ids) return arg_fail("null d_ids");
    if (id_stride < 16) return arg_fail("id_stride below 16");
    if (k && !d_table) return arg_fail("null d_table");
    if (!d_keys != !d_keys_out) return arg_fail("d_keys and d_keys_out go together");
    if (!aligned(d_status, 4) || !aligned(d_seq, 4) || !aligned(d_bucket, 4) || !aligned(d_local, 4) ||
        !aligned(d_bucket_off, 8) || !aligned(d_bucket_count, 8) || !aligned(d_rows, 16))
        return arg_fail("status, seq, bucket and local 4-byte / offsets and counts 8-byte / rows 16-byte aligned");
    const int32_t st = work_args(route_workspace_bytes(m), d_work, work_bytes, "honu_key_route_workspace(m)");
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_key_route(d_ids, id_stride, d_status, m, d_seq, d_table, k, d_keys, d_bucket, d_rows, d_local,
                            d_keys_out, d_bucket_off, d_bucket_count, d_work, ctx->scan, ctx->max_n,
                            (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// a routed batch of Puts into every collection's bucket at once
// (store.go:232-240, 395, 530; tx.go:112-120)
// ---------------------------------------------------------------------------
int32_t honu_key_merge_buckets(honu_ctx *ctx, uint64_t k, const uint8_t *d_sorted_a, const uint32_t *d_order_a,
                               const uint64_t *d_off_a, const uint64_t *d_count_a, uint64_t na,
                               const uint8_t *d_sorted_b, const uint32_t *d_order_b, const uint64_t *d_off_b,
                               uint64_t nb, const uint32_t *d_base, uint32_t b_base, uint8_t *d_sorted_out,
                               uint32_t *d_order_out, uint64_t *d_off_out, uint64_t *d_count_out, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (na > 0xFFFFFFFFull || nb > 0xFFFFFFFFull || na + nb > 0xFFFFFFFFull || k > 0xFFFFFFFCull)
        return HONU_E_WORKSPACE;
    // with counts the buckets' rows are scanned with the context's scan state, which covers max_records rows
    if (d_count_a && k + 1 > ctx->max_n) return HONU_E_WORKSPACE;
    if (!d_off_a || !d_off_b || !d_off_out) return arg_fail("null offsets");
    if ((na && !d_sorted_a) || (nb && !d_sorted_b) || (na + nb && !d_sorted_out)) return arg_fail("null column");
    if (d_order_out && na && !d_order_a) return arg_fail("d_order_out needs d_order_a");
    if (!d_base && (uint64_t)b_base + nb > 0xFFFFFFFFull) return arg_fail("b_base + nb above 2^32 - 1");
    if (!aligned(d_order_a, 4) || !aligned(d_order_b, 4) || !aligned(d_order_out, 4) || !aligned(d_base, 4) ||
        !aligned(d_off_a, 8) || !aligned(d_count_a, 8) || !aligned(d_off_b, 8) || !aligned(d_off_out, 8) ||
        !aligned(d_count_out, 8))
        return arg_fail("orders and bases 4-byte / offsets and counts 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_merge_buckets(k, d_sorted_a, d_order_a, d_off_a, d_count_a, na, d_sorted_b, d_order_b, d_off_b, nb,
                                d_base, b_base, d_sorted_out, d_order_out, d_off_out, d_count_out, ctx->scan,
                                (hipStream_t)stream));
    return HONU_OK;
}

// ---------------------------------------------------------------------------
// system objects (object/system.go)
// ---------------------------------------------------------------------------
int32_t honu_system_sizes(honu_ctx *ctx, const honu_collection *d_rows, uint64_t var_len,
                          const honu_acl *d_acl, uint64_t acl_len, const uint32_t *d_regions,
                          uint64_t regions_len, const honu_index *d_index, uint64_t index_len,
                          uint64_t n, uint64_t *d_sizes, int32_t *d_status, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_rows || !d_sizes)) return arg_fail("null pointer");
    if (!aligned(d_rows, 16)) return arg_fail("rows must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4) || !aligned(d_index, 8))
        return arg_fail("tables must be aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_system_sizes(d_rows, var_len, d_acl, acl_len, d_regions, regions_len, d_index,
                               index_len, n, d_sizes, d_status, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_system_encode(honu_ctx *ctx, const honu_collection *d_rows, const uint8_t *d_var,
                           const honu_acl *d_acl, const uint32_t *d_regions,
                           const honu_index *d_index, uint64_t n, uint8_t *d_out,
                           uint64_t out_cap, const uint64_t *d_out_off, int32_t *d_status,
                           void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_rows || !d_out || !d_out_off || !d_status)) return arg_fail("null pointer");
    if (!aligned(d_rows, 16) || !aligned(d_out, 16))
        return arg_fail("rows and output arena must be 16-byte aligned");
    if (!aligned(d_acl, 4) || !aligned(d_regions, 4) || !aligned(d_index, 8))
        return arg_fail("tables must be aligned");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_system_encode(d_rows, d_var, d_acl, d_regions, d_index, n, d_out, out_cap,
                                d_out_off, d_status, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_system_marshal_batch(honu_ctx *ctx, const honu_collection *d_rows,
                                  const uint8_t *d_var, uint64_t var_len, const honu_acl *d_acl,
                                  uint64_t acl_len, const uint32_t *d_regions,
                                  uint64_t regions_len, const honu_index *d_index,
                                  uint64_t index_len, uint64_t n, uint8_t *d_out,
                                  uint64_t out_cap, uint64_t *d_out_off, int32_t *d_status,
                                  void *stream) {
    // the checks of the phases below, before the first of them launches: a
    // refused call has stored nothing
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rows || !d_out || !d_out_off || !d_status)) return arg_fail("null pointer");
    if (!aligned(d_rows, 16) || !aligned(d_out, 16))
        return arg_fail("rows and output arena must be 16-byte aligned");
    int32_t st = honu_system_sizes(ctx, d_rows, var_len, d_acl, acl_len, d_regions, regions_len,
                                   d_index, index_len, n, d_out_off, d_status, stream);
    if (st) return st;
    st = honu_exclusive_scan(ctx, d_out_off, n, d_out_off, stream);
    if (st) return st;
    return honu_system_encode(ctx, d_rows, d_var, d_acl, d_regions, d_index, n, d_out, out_cap,
                              d_out_off, d_status, stream);
}

static int32_t collection_decode(honu_ctx *ctx, bool headless, const uint8_t *d_rec,
                                 const uint64_t *d_rec_off, uint64_t n, honu_collection *d_rows,
                                 int32_t *d_status, honu_acl *d_acl, uint64_t acl_cap,
                                 uint32_t *d_regions, uint64_t regions_cap, honu_index *d_index,
                                 uint64_t index_cap, uint64_t *d_totals, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n > ctx->max_n) return HONU_E_WORKSPACE;
    if (n && (!d_rec || !d_rec_off || !d_rows || !d_status)) return arg_fail("null pointer");
    if (!aligned(d_rec, 16)) return arg_fail("records arena must be 16-byte aligned");
    if (!aligned(d_rows, 16) || !aligned(d_acl, 4) || !aligned(d_regions, 4) ||
        !aligned(d_index, 8))
        return arg_fail("rows 16-byte / tables 4- and 8-byte aligned");
    if ((acl_cap && !d_acl) || (regions_cap && !d_regions) || (index_cap && !d_index))
        return arg_fail("table");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    uint64_t *tot = d_totals ? d_totals : ctx->totals;
    HIPCHK(launch_system_parse(d_rec, d_rec_off, n, headless, d_rows, d_status, ctx->scratch,
                               ctx->counts, s));
    HIPCHK(launch_scan(ctx->counts, n, 3, ctx->offs, tot, ctx->scan, s));
    HIPCHK(launch_system_fill(d_rec, n, d_rows, d_status, ctx->scratch, ctx->counts, ctx->offs,
                              d_acl, acl_cap, d_regions, regions_cap, d_index, index_cap, s));
    return HONU_OK;
}

int32_t honu_system_decode_batch(honu_ctx *ctx, const uint8_t *d_rec, const uint64_t *d_rec_off,
                                 uint64_t n, honu_collection *d_rows, int32_t *d_status,
                                 honu_acl *d_acl, uint64_t acl_cap, uint32_t *d_regions,
                                 uint64_t regions_cap, honu_index *d_index, uint64_t index_cap,
                                 uint64_t *d_totals, void *stream) {
    return collection_decode(ctx, false, d_rec, d_rec_off, n, d_rows, d_status, d_acl, acl_cap,
                             d_regions, regions_cap, d_index, index_cap, d_totals, stream);
}

int32_t honu_collection_decode_batch(honu_ctx *ctx, const uint8_t *d_rec,
                                     const uint64_t *d_rec_off, uint64_t n,
                                     honu_collection *d_rows, int32_t *d_status, honu_acl *d_acl,
                                     uint64_t acl_cap, uint32_t *d_regions, uint64_t regions_cap,
                                     honu_index *d_index, uint64_t index_cap, uint64_t *d_totals,
                                     void *stream) {
    return collection_decode(ctx, true, d_rec, d_rec_off, n, d_rows, d_status, d_acl, acl_cap,
                             d_regions, regions_cap, d_index, index_cap, d_totals, stream);
}

// ---------------------------------------------------------------------------
// synthetic payload, digests, memory helpers
// ---------------------------------------------------------------------------
int32_t honu_gen_payload(honu_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n,
                         const uint64_t *d_payload_off, uint8_t *d_payload, void *stream) {
    if (!ctx) return arg_fail("ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_gen_payload(ctx->geom, seed, first, n, d_payload_off, d_payload,
                              (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_hbm_probe(honu_ctx *ctx, int32_t mode, const void *d_src, void *d_dst, uint64_t bytes,
                       uint32_t blocks_per_cu, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (mode < 0 || mode > 4) return arg_fail("mode");
    if (!aligned(d_src, 16) || !aligned(d_dst, 16) || (mode != 1 && !d_src) || (mode != 0 && !d_dst))
        return arg_fail("buffers must be non-null and 16-byte aligned");
    if (!blocks_per_cu) blocks_per_cu = 2;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_hbm_probe(mode, d_src, d_dst, bytes, blocks_per_cu * (uint32_t)ctx->geom.num_cu,
                            reinterpret_cast<uint32_t *>(ctx->totals + 3), (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_digest_records(honu_ctx *ctx, const uint8_t *d_arena, const uint64_t *d_off,
                            const uint64_t *d_len, uint64_t n, uint64_t *d_digest, void *stream) {
    if (!ctx) return arg_fail("ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_digest(ctx->geom, d_arena, d_off, d_len, n, d_digest, (hipStream_t)stream));
    return HONU_OK;
}

int32_t honu_verify_decoded(honu_ctx *ctx, const honu_meta *d_src, const uint8_t *d_var,
                            const honu_acl *d_src_acl, const uint32_t *d_src_regions,
                            const uint64_t *d_payload_off, const uint8_t *d_rec,
                            const honu_meta *d_dec, const honu_record_info *d_info,
                            const honu_acl *d_dec_acl, const uint32_t *d_dec_regions, uint64_t n,
                            uint32_t *d_mismatch, void *stream) {
    if (!ctx) return arg_fail("ctx");
    if (n && (!d_src || !d_payload_off || !d_rec || !d_dec || !d_info || !d_mismatch))
        return arg_fail("null pointer");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_verify_decoded(ctx->geom, d_src, d_var, d_src_acl, d_src_regions, d_payload_off,
                                 d_rec, d_dec, d_info, d_dec_acl, d_dec_regions, n, d_mismatch,
                                 (hipStream_t)stream));
    return HONU_OK;
}

void *honu_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void honu_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
void *honu_device_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
void honu_device_free(void *p) {
    if (p) (void)hipFree(p);
}
int32_t honu_memcpy_h2d(void *d_dst, const void *h_src, uint64_t bytes, void *stream) {
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return HONU_OK;
}
int32_t honu_memcpy_d2h(void *h_dst, const void *d_src, uint64_t bytes, void *stream) {
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return HONU_OK;
}
int32_t honu_stream_sync(void *stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return HONU_OK;
}

}  // extern "C"
