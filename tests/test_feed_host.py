"""The host side of the feeds (honu_amd/csrc/host_copy.h, put_fill.h) as a
stand-alone C++ program, built and run twice: under ASan + UBSan and under
TSan. Nothing is loaded into Python. Plain loops in the program are the
reference.

host_copy / host_copy_ranges, T = 1, 2, 3, 8: totals 0, 1, T - 1, T, T + 1,
kParallelCopyMin - 1, kParallelCopyMin, kParallelCopyMin + 1 and 20 MiB + 11
(no multiple of 2, 3 or 8); one job (it spans every thread), jobs with
zero-length jobs at the start, in the middle and at the end, jobs that end
exactly on the threads' cuts, a long job between two 3-byte ones. Every
destination is an allocation of its own and equals its source byte for byte;
the 64 bytes before and after it keep their fill.

record_cuts, T = 1, 2, 3, 8: k = 2, k < T, k = 5000; needs uniform, one giant
record first / in the middle / last, all zero but one, all zero, random. The
cuts start at 0, end at k, never decrease, number at most T + 1, their ranges
cover every record once, and (equal bytes: cut t falls at the first record
where the running sum reaches bytes t / T) no range holds more than
bytes / T + 1 + the largest need.

put_plan / put_place / put_fill / put_fill_batch on seeded random batches
(every `present` combination, span lengths from 0, overlapping and unordered
spans, absent sub-structs with out-of-range spans, ACL lists with nil
entries, region lists, payloads of 0 to 300 KiB, rows with and without
HONU_ACL_SIZED and HONU_HAS_META): filled record by record as append() does,
then as two append_batch calls with T forced to 2, 3 and 8, into slot arrays
allocated as put_slot_alloc sizes them for a batch that fits exactly. Every
array and counter of every run equals a per-record reference, and what lies
past the fill point keeps its fill.

put_plan's refusals: every span x {off > var_len, off + len > var_len, off =
2^64 - 1, a sum that wraps from a huge len, var NULL}, refused with its
sub-struct present, accepted and zeroed with it absent; lists outside their
arrays (a wrapping sum among them) or with a NULL array; the in-place flags;
list lengths above what a batch holds; a row without HONU_HAS_META.

The two-line program prints honu::kParallelCopyMin, which must be the
threshold tests/test_gpu_feeds.py sizes its batches from.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "honu_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "@CSRC@/put_fill.h"

using namespace honu;

static uint64_t g_state = 1;
static uint64_t rnd() {
    uint64_t x = (g_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(c, ...)             \
    do {                          \
        if (!(c)) {               \
            printf("FAILED ");    \
            printf(__VA_ARGS__);  \
            printf("\n");         \
            exit(1);              \
        }                         \
    } while (0)

static unsigned long long n_copy = 0, n_cuts = 0, n_fill = 0, n_plan = 0;

/* ---------------------------------------------------------------- host_copy */
static const uint64_t GUARD = 64;
static std::vector<uint8_t> g_src;

static void copy_case(const std::vector<uint64_t> &lens, unsigned T, bool ranges, const char *what) {
    uint64_t total = 0;
    std::vector<HostCopy> jobs;
    std::vector<uint8_t *> bufs;
    for (uint64_t len : lens) {
        uint8_t *b = (uint8_t *)malloc(len + 2 * GUARD);
        memset(b, 0xA5, GUARD);
        memset(b + GUARD, 0x5A, len);
        memset(b + GUARD + len, 0xA5, GUARD);
        bufs.push_back(b);
        jobs.push_back(HostCopy{b + GUARD, g_src.data() + total, len});
        total += len;
    }
    CHECK(total <= g_src.size(), "%s: the case is larger than the source", what);
    if (ranges)
        host_copy_ranges(jobs, total, T);
    else
        host_copy(jobs, total, T);
    uint64_t at = 0;
    for (size_t j = 0; j < lens.size(); j++) {
        const uint8_t *b = bufs[j];
        CHECK(!lens[j] || !memcmp(b + GUARD, g_src.data() + at, lens[j]),
              "%s: job %zu of %zu differs (T %u, total %llu, ranges %d)", what, j, lens.size(), T,
              (unsigned long long)total, (int)ranges);
        for (uint64_t g = 0; g < GUARD; g++)
            CHECK(b[g] == 0xA5 && b[GUARD + lens[j] + g] == 0xA5,
                  "%s: a guard band of job %zu changed (T %u, total %llu, ranges %d)", what, j, T,
                  (unsigned long long)total, (int)ranges);
        at += lens[j];
        free(bufs[j]);
    }
    n_copy++;
}

static void copy_tests() {
    const uint64_t big = (20ull << 20) + 11;
    g_src.resize(big);
    for (uint64_t i = 0; i + 8 <= big; i += 8) {
        const uint64_t x = rnd();
        memcpy(&g_src[i], &x, 8);
    }
    for (uint64_t i = big & ~7ull; i < big; i++) g_src[i] = (uint8_t)rnd();
    const unsigned Ts[] = {1, 2, 3, 8};
    for (unsigned T : Ts) {
        const uint64_t totals[] = {0, 1, T - 1, T, T + 1, kParallelCopyMin - 1, kParallelCopyMin,
                                   kParallelCopyMin + 1, big};
        for (uint64_t total : totals)
            /* from the threshold on host_copy is host_copy_ranges: once is enough */
            for (int ranges = 0; ranges < (total < kParallelCopyMin ? 2 : 1); ranges++) {
                copy_case({total}, T, ranges, "one job");
                /* zero-length jobs at the start, in the middle and at the end */
                const uint64_t a = below(total + 1), b = below(total - a + 1), c = total - a - b;
                copy_case({0, a, 0, 0, b, c, 0}, T, ranges, "zero-length jobs");
                /* the totals beside the threshold ask which path runs: two shapes do */
                if (total >= kParallelCopyMin - 1 && total != big) continue;
                copy_case({0, 0, total, 0}, T, ranges, "zero-length jobs around one");
                /* jobs that end exactly on the threads' cuts */
                std::vector<uint64_t> on;
                for (unsigned t = 0; t < T; t++) on.push_back(total * (t + 1) / T - total * t / T);
                copy_case(on, T, ranges, "jobs on the cuts");
                if (total >= 6) copy_case({3, total - 6, 3}, T, ranges, "a long job between short ones");
                /* many small jobs (the small totals: one byte each) */
                std::vector<uint64_t> many;
                const uint64_t parts = total < 64 ? total : 64;
                for (uint64_t p = 0; p < parts; p++) many.push_back(total * (p + 1) / parts - total * p / parts);
                copy_case(many, T, ranges, "many jobs");
            }
    }
}

/* -------------------------------------------------------------- record_cuts */
static void cuts_case(const std::vector<uint64_t> &need, unsigned T, const char *what) {
    const uint64_t k = need.size();
    uint64_t bytes = 0, top = 0;
    for (uint64_t x : need) bytes += x, top = x > top ? x : top;
    const std::vector<uint64_t> c = record_cuts(need, bytes, T);
    CHECK(c.size() >= 2 && c.size() <= (size_t)T + 1, "%s: %zu cuts for T %u", what, c.size(), T);
    CHECK(c.front() == 0 && c.back() == k, "%s: the cuts span [%llu, %llu), k %llu", what,
          (unsigned long long)c.front(), (unsigned long long)c.back(), (unsigned long long)k);
    std::vector<uint8_t> seen(k, 0);
    for (size_t j = 0; j + 1 < c.size(); j++) {
        CHECK(c[j] <= c[j + 1], "%s: cut %zu decreases (T %u, k %llu)", what, j + 1, T, (unsigned long long)k);
        uint64_t sum = 0;
        for (uint64_t i = c[j]; i < c[j + 1]; i++) seen[i]++, sum += need[i];
        CHECK(sum <= bytes / T + 1 + top, "%s: range %zu holds %llu of %llu bytes (T %u)", what, j,
              (unsigned long long)sum, (unsigned long long)bytes, T);
    }
    for (uint64_t i = 0; i < k; i++) CHECK(seen[i] == 1, "%s: record %llu filled %d times", what, (unsigned long long)i, seen[i]);
    n_cuts++;
}

static void cuts_tests() {
    const unsigned Ts[] = {1, 2, 3, 8};
    for (unsigned T : Ts) {
        std::vector<uint64_t> ks = {2, 5000};
        if (T > 2) ks.push_back(T - 1);
        if (T > 3) ks.push_back(3);
        for (uint64_t k : ks) {
            const uint64_t at[] = {0, k / 2, k - 1};
            cuts_case(std::vector<uint64_t>(k, 100), T, "uniform");
            cuts_case(std::vector<uint64_t>(k, 0), T, "all zero");
            for (uint64_t g : at) {
                std::vector<uint64_t> giant(k, 10), lone(k, 0);
                giant[g] = 1ull << 24;
                lone[g] = 12345;
                cuts_case(giant, T, "one giant record");
                cuts_case(lone, T, "all zero but one");
            }
            for (int r = 0; r < 20; r++) {
                std::vector<uint64_t> v(k);
                for (uint64_t &x : v) x = below(4) ? below(3000) : below(300 << 10);
                cuts_case(v, T, "random");
            }
        }
    }
}

/* ---------------------------------------------------------------- the fill */
static const uint32_t PRESENT_BITS = HONU_HAS_META | HONU_HAS_VERSION | HONU_HAS_PARENT | HONU_HAS_SCHEMA |
                                     HONU_HAS_PUBLISHER | HONU_HAS_ENCRYPTION | HONU_HAS_COMPRESSION |
                                     HONU_REGIONS_NONNIL | HONU_ACL_SIZED;

static honu_span *span_of(honu_meta &r, int k) {
    honu_span *s[8] = {&r.schema_name, &r.mime, &r.ip_address, &r.user_agent,
                       &r.public_key_id, &r.encryption_key, &r.hmac_secret, &r.signature};
    return s[k];
}
static bool span_live(uint32_t present, int k) {
    if (!(present & HONU_HAS_META)) return false;
    if (k == 0) return present & HONU_HAS_SCHEMA;
    if (k == 1) return true;
    if (k <= 3) return present & HONU_HAS_PUBLISHER;
    return present & HONU_HAS_ENCRYPTION;
}

struct Batch {
    std::vector<honu_meta> rows;
    std::vector<uint8_t> var, payload;
    std::vector<honu_acl> acl;
    std::vector<uint32_t> regions;
    std::vector<uint64_t> poff;
};

struct SlotMem {  /* the arrays as put_slot_alloc sizes them */
    PutSlotHost s;
    uint64_t cap_n, cap_bytes, sz[6];
    uint8_t *raw[6];
    SlotMem(uint64_t n, uint64_t b) : cap_n(n), cap_bytes(b) {
        sz[0] = sizeof(honu_meta) * n;
        sz[1] = b + 16;
        sz[2] = sizeof(honu_acl) * (b / sizeof(honu_acl) + 1) + 16;
        sz[3] = 4 * (b / 4 + 1) + 16;
        sz[4] = b + 16;
        sz[5] = 8 * (n + 1);
        for (int i = 0; i < 6; i++) {
            raw[i] = (uint8_t *)malloc(sz[i] ? sz[i] : 1);
            memset(raw[i], 0xCD, sz[i]);
        }
        s.h_meta = (honu_meta *)raw[0];
        s.h_var = raw[1];
        s.h_acl = (honu_acl *)raw[2];
        s.h_reg = (uint32_t *)raw[3];
        s.h_pay = raw[4];
        s.h_poff = (uint64_t *)raw[5];
        s.h_poff[0] = 0;
    }
    ~SlotMem() {
        for (uint8_t *p : raw) free(p);
    }
};

static Batch make_batch(uint64_t seed) {
    g_state = seed * 0x1234567ull + 99;
    Batch b;
    const uint64_t n = 1 + below(seed % 5 == 0 ? 3 : 48);
    b.var.resize(below(3) ? 600 + below(2000) : below(8));
    for (uint8_t &x : b.var) x = (uint8_t)rnd();
    b.acl.resize(below(4) ? 1 + below(60) : 0);
    for (honu_acl &a : b.acl) {
        for (uint8_t &x : a.client_id) x = (uint8_t)rnd();
        a.permissions = (uint8_t)rnd();
        a.present = below(4) ? 1 : 0;
        a._pad[0] = a._pad[1] = (uint8_t)rnd();
    }
    b.regions.resize(below(4) ? 1 + below(40) : 0);
    for (uint32_t &x : b.regions) x = (uint32_t)rnd();
    b.poff.push_back(0);
    static const uint64_t lens[] = {0, 0, 1, 5, 127, 128, 129, 400};
    for (uint64_t i = 0; i < n; i++) {
        honu_meta r;
        uint8_t *raw = (uint8_t *)&r;
        for (size_t j = 0; j < sizeof r; j++) raw[j] = (uint8_t)rnd();
        /* every combination of the presence bits shows up over the seeds */
        r.present = (uint32_t)rnd() & PRESENT_BITS;
        if (below(8)) r.present |= HONU_HAS_META;
        for (int k = 0; k < 8; k++) {
            honu_span *sp = span_of(r, k);
            if (span_live(r.present, k)) {
                sp->len = lens[below(8)];
                if (sp->len > b.var.size()) sp->len = below(b.var.size() + 1);
                sp->off = below(b.var.size() - sp->len + 1);
                if (!sp->len && below(2)) sp->off = rnd(); /* an empty span may point anywhere */
            } else if (below(2)) { /* an absent sub-struct's span is not validated */
                sp->off = rnd();
                sp->len = rnd();
            }
        }
        if (r.present & HONU_HAS_META) {
            r.acl_count = b.acl.size() && below(3) ? below(b.acl.size() + 1) : 0;
            r.acl_off = r.acl_count ? below(b.acl.size() - r.acl_count + 1) : rnd();
            r.regions_count = b.regions.size() && below(3) ? below(b.regions.size() + 1) : 0;
            r.regions_off = r.regions_count ? below(b.regions.size() - r.regions_count + 1) : rnd();
        }
        b.rows.push_back(r);
        const uint64_t dl = below(10) == 0 ? below(300 << 10) + 1 : below(4) ? below(3000) : 0;
        const uint64_t p0 = b.payload.size();
        b.payload.resize(p0 + dl);
        for (uint64_t j = 0; j < dl; j += 8) {
            const uint64_t x = rnd();
            memcpy(&b.payload[p0 + j], &x, dl - j < 8 ? dl - j : 8);
        }
        b.poff.push_back(b.payload.size());
    }
    return b;
}

/* the straightforward statement of what a slot holds after the batch */
struct Expect {
    std::vector<honu_meta> rows;
    std::vector<uint8_t> var, pay;
    std::vector<honu_acl> acl;
    std::vector<uint32_t> reg;
    std::vector<uint64_t> poff;
    uint64_t budget = 0, bound = 0;
};

static Expect expect_of(const Batch &b) {
    Expect e;
    e.poff.push_back(0);
    for (size_t i = 0; i < b.rows.size(); i++) {
        honu_meta w = b.rows[i];
        const bool has = w.present & HONU_HAS_META;
        uint64_t span_bytes = 0;
        for (int k = 0; k < 8; k++) { /* compacted in field order, rebased; dead or empty: {0, 0} */
            honu_span *sp = span_of(w, k);
            if (span_live(w.present, k) && sp->len) {
                const uint64_t at = e.var.size();
                e.var.insert(e.var.end(), b.var.begin() + sp->off, b.var.begin() + sp->off + sp->len);
                sp->off = at;
                span_bytes += sp->len;
            } else {
                *sp = honu_span{0, 0};
            }
        }
        if (!has) w.acl_count = w.regions_count = 0;
        const uint64_t na = w.acl_count, nr = w.regions_count;
        if (na && !(w.present & HONU_ACL_SIZED)) {
            uint64_t nb = 0;
            for (uint64_t j = 0; j < na; j++) nb += b.acl[w.acl_off + j].present ? 18 : 1;
            w.acl_bytes = nb;
            w.present |= HONU_ACL_SIZED;
        } /* a row that carries HONU_ACL_SIZED keeps its acl_bytes, whatever it says */
        const uint64_t a0 = w.acl_off, r0 = w.regions_off;
        w.acl_off = na ? e.acl.size() : 0;
        w.regions_off = nr ? e.reg.size() : 0;
        for (uint64_t j = 0; j < na; j++) e.acl.push_back(b.acl[a0 + j]);
        for (uint64_t j = 0; j < nr; j++) e.reg.push_back(b.regions[r0 + j]);
        const uint64_t dl = b.poff[i + 1] - b.poff[i];
        e.pay.insert(e.pay.end(), b.payload.begin() + b.poff[i], b.payload.begin() + b.poff[i + 1]);
        e.poff.push_back(e.pay.size());
        e.rows.push_back(w);
        e.budget += span_bytes + dl + 20 * na + 4 * nr;
        e.bound += 311 + span_bytes + dl + 18 * na + 5 * nr;
    }
    return e;
}

static void check_slot(const SlotMem &m, const Expect &e, const char *what, uint64_t seed) {
    const PutSlotHost &s = m.s;
    const uint64_t n = e.rows.size();
    CHECK(s.n == n && s.var == e.var.size() && s.acl == e.acl.size() && s.reg == e.reg.size() &&
              s.pay == e.pay.size(), "%s, seed %llu: the fill counters", what, (unsigned long long)seed);
    CHECK(s.budget == e.budget && s.bound == e.bound, "%s, seed %llu: budget %llu (expected %llu), bound %llu (%llu)",
          what, (unsigned long long)seed, (unsigned long long)s.budget, (unsigned long long)e.budget,
          (unsigned long long)s.bound, (unsigned long long)e.bound);
    for (uint64_t i = 0; i < n; i++)
        CHECK(!memcmp(&s.h_meta[i], &e.rows[i], sizeof(honu_meta)), "%s, seed %llu: row %llu", what,
              (unsigned long long)seed, (unsigned long long)i);
    CHECK(!memcmp(s.h_poff, e.poff.data(), 8 * (n + 1)), "%s, seed %llu: h_poff", what, (unsigned long long)seed);
    const void *got[6] = {s.h_meta, s.h_var, s.h_acl, s.h_reg, s.h_pay, s.h_poff};
    const void *exp[6] = {e.rows.data(), e.var.data(), e.acl.data(), e.reg.data(), e.pay.data(), e.poff.data()};
    const uint64_t used[6] = {sizeof(honu_meta) * n, e.var.size(), sizeof(honu_acl) * e.acl.size(),
                              4 * e.reg.size(), e.pay.size(), 8 * (n + 1)};
    for (int a = 0; a < 6; a++) {
        CHECK(used[a] <= m.sz[a], "%s, seed %llu: array %d over its allocation", what, (unsigned long long)seed, a);
        CHECK(!used[a] || !memcmp(got[a], exp[a], used[a]), "%s, seed %llu: array %d differs", what,
              (unsigned long long)seed, a);
        static const std::vector<uint8_t> fill(4096, 0xCD);
        for (uint64_t j = used[a]; j < m.sz[a]; j += 4096)
            CHECK(!memcmp(m.raw[a] + j, fill.data(), m.sz[a] - j < 4096 ? m.sz[a] - j : 4096),
                  "%s, seed %llu: array %d written past its fill point, from byte %llu on", what,
                  (unsigned long long)seed, a, (unsigned long long)j);
    }
}

/* phase 1 of append_batch over rows [lo, hi) of the batch */
static void place(SlotMem &m, const Batch &b, uint64_t lo, uint64_t hi, std::vector<PutPlan> &plans, uint64_t &bytes) {
    for (uint64_t i = lo; i < hi; i++) {
        PutPlan p;
        const uint64_t dl = b.poff[i + 1] - b.poff[i];
        const int32_t st = put_plan(m.cap_bytes, &b.rows[i], b.var.data(), b.var.size(), b.acl.data(),
                                    b.acl.size(), b.regions.data(), b.regions.size(), dl, p);
        CHECK(st == HONU_OK, "put_plan refuses row %llu: %d", (unsigned long long)i, st);
        CHECK(!(m.s.n == m.cap_n || p.need > m.cap_bytes - m.s.budget), "row %llu does not fit an exact batch",
              (unsigned long long)i);
        put_place(m.s, p, dl);
        plans.push_back(p);
        bytes += p.need;
    }
}

static void fill_tests() {
    CHECK(kFixedBound == 311, "kFixedBound is %llu", (unsigned long long)kFixedBound);
    CHECK(sizeof(honu_meta) == 352 && sizeof(honu_acl) == 20, "the row sizes");
    uint32_t seen_present = 0, seen_absent = 0, combos = 0; /* of the five bits the fill reads */
    for (uint64_t seed = 1; seed <= 80; seed++) {
        const Batch b = make_batch(seed);
        const Expect e = expect_of(b);
        const uint64_t n = b.rows.size();
        for (const honu_meta &r : b.rows) {
            seen_present |= r.present, seen_absent |= ~r.present;
            const uint32_t p = r.present;
            combos |= 1u << ((p & HONU_HAS_META ? 1 : 0) | (p & HONU_HAS_SCHEMA ? 2 : 0) | (p & HONU_HAS_PUBLISHER ? 4 : 0) |
                             (p & HONU_HAS_ENCRYPTION ? 8 : 0) | (p & HONU_ACL_SIZED ? 16 : 0));
        }
        { /* record by record, as append() */
            SlotMem m(n, e.budget);
            for (uint64_t i = 0; i < n; i++) {
                std::vector<PutPlan> one;
                uint64_t bytes = 0;
                place(m, b, i, i + 1, one, bytes);
                put_fill(m.s, i, one[0], &b.rows[i], b.var.data(), b.acl.data(), b.regions.data(),
                         b.payload.data() + b.poff[i], b.poff[i + 1] - b.poff[i]);
            }
            check_slot(m, e, "serial", seed);
            /* one byte more is what append() refuses */
            CHECK(1 > m.cap_bytes - m.s.budget, "an exact batch has room left");
            n_fill++;
        }
        const unsigned Ts[] = {2, 3, 8};
        for (unsigned T : Ts) { /* two append_batch calls, the second at first > 0 */
            SlotMem m(n, e.budget);
            const uint64_t half = seed % 3 ? n / 2 : n;
            const uint64_t parts[3] = {0, half, n};
            for (int h = 0; h < 2; h++) {
                std::vector<PutPlan> plans;
                uint64_t bytes = 0;
                const uint64_t first = m.s.n, lo = parts[h];
                place(m, b, lo, parts[h + 1], plans, bytes);
                put_fill_batch(m.s, first, plans, bytes, b.rows.data() + lo, b.var.data(), b.acl.data(),
                               b.regions.data(), b.payload.data(), b.poff.data() + lo, T);
            }
            check_slot(m, e, "threaded", seed);
            n_fill++;
        }
        { /* the default thread count: below kParallelCopyMin, the calling thread */
            SlotMem m(n, e.budget);
            std::vector<PutPlan> plans;
            uint64_t bytes = 0;
            place(m, b, 0, n, plans, bytes);
            put_fill_batch(m.s, 0, plans, bytes, b.rows.data(), b.var.data(), b.acl.data(),
                           b.regions.data(), b.payload.data(), b.poff.data());
            check_slot(m, e, "default", seed);
            n_fill++;
        }
    }
    CHECK((seen_present & PRESENT_BITS) == PRESENT_BITS && (seen_absent & PRESENT_BITS) == PRESENT_BITS,
          "the batches do not vary every presence bit");
    CHECK(combos == 0xFFFFFFFFu, "the batches miss a combination of the presence bits: %08x", combos);
}

/* ------------------------------------------------------- put_plan refusals */
static const uint64_t VAR_LEN = 64, CAP = 1 << 16;
static uint8_t g_var[VAR_LEN];
static honu_acl g_acl[8];
static uint32_t g_reg[8];

static uint32_t owner_bit(int k) {
    return k == 0 ? HONU_HAS_SCHEMA : k == 1 ? HONU_HAS_META : k <= 3 ? HONU_HAS_PUBLISHER : HONU_HAS_ENCRYPTION;
}

static int32_t plan(const honu_meta &r, const uint8_t *var, const honu_acl *acl, uint64_t acl_len,
                    const uint32_t *reg, uint64_t reg_len, uint64_t dl, PutPlan &p) {
    n_plan++;
    return put_plan(CAP, &r, var, VAR_LEN, acl, acl_len, reg, reg_len, dl, p);
}

static void plan_tests() {
    honu_meta base;
    memset(&base, 0, sizeof base);
    base.present = HONU_HAS_META | HONU_HAS_SCHEMA | HONU_HAS_PUBLISHER | HONU_HAS_ENCRYPTION;
    /* the last two: sums that wrap, from a huge off and from a huge len */
    const honu_span bad[4] = {{VAR_LEN + 1, 1}, {VAR_LEN - 2, 3}, {~0ull, 2}, {8, ~0ull - 3}};
    PutPlan p;
    for (int k = 0; k < 8; k++) {
        for (int kind = 0; kind < 5; kind++) {
            honu_meta r = base;
            /* kind 4: a span in range and no var arena */
            *span_of(r, k) = kind < 4 ? bad[kind] : honu_span{3, 5};
            const uint8_t *var = kind < 4 ? g_var : nullptr;
            CHECK(plan(r, var, g_acl, 8, g_reg, 8, 7, p) == HONU_ERR_INPUT, "span %d, kind %d: not refused", k, kind);
            r.present &= ~owner_bit(k); /* absent: not validated, zeroed, costs nothing */
            CHECK(plan(r, var, g_acl, 8, g_reg, 8, 7, p) == HONU_OK, "span %d, kind %d: refused though absent", k, kind);
            for (int j = 0; j < 8; j++)
                CHECK(span_of(p.w, j)->off == 0 && span_of(p.w, j)->len == 0, "span %d, kind %d: span %d not zeroed", k, kind, j);
            CHECK(p.span_bytes == 0 && p.need == 7 && p.bound == kFixedBound + 7, "span %d, kind %d: an absent span costs", k, kind);
        }
        /* the edges that are in range */
        const honu_span good[3] = {{VAR_LEN - 3, 3}, {0, VAR_LEN}, {VAR_LEN + 9, 0}};
        for (int g = 0; g < 3; g++) {
            honu_meta r = base;
            *span_of(r, k) = good[g];
            CHECK(plan(r, g_var, g_acl, 8, g_reg, 8, 0, p) == HONU_OK, "span %d, edge %d: refused", k, g);
            CHECK(p.span_bytes == good[g].len && p.need == good[g].len, "span %d, edge %d: its size", k, g);
        }
    }
    /* lists outside their arrays, or with a NULL array */
    const uint64_t lists[5][2] = {{9, 1}, {6, 3}, {~0ull, 2}, {2, 3}, {2, ~0ull}};
    for (int which = 0; which < 2; which++)
        for (int kind = 0; kind < 5; kind++) {
            honu_meta r = base;
            (which ? r.regions_off : r.acl_off) = lists[kind][0];
            (which ? r.regions_count : r.acl_count) = lists[kind][1];
            const bool null = kind == 3;
            const int32_t st = plan(r, g_var, null && !which ? nullptr : g_acl, 8, null && which ? nullptr : g_reg, 8, 0, p);
            CHECK(st == HONU_ERR_INPUT, "list %d, kind %d: not refused (%d)", which, kind, st);
        }
    {
        honu_meta r = base; /* lists that end with their arrays */
        r.acl_off = 5, r.acl_count = 3, r.regions_off = 0, r.regions_count = 8;
        CHECK(plan(r, g_var, g_acl, 8, g_reg, 8, 2, p) == HONU_OK, "lists at the ends of their arrays");
        CHECK(p.nacl == 3 && p.nreg == 8 && p.need == 2 + 60 + 32 && p.bound == kFixedBound + 2 + 54 + 40, "their size");
        r.acl_count = r.regions_count = 0; /* empty lists need no array */
        r.acl_off = r.regions_off = ~0ull;
        CHECK(plan(r, nullptr, nullptr, 0, nullptr, 0, 0, p) == HONU_OK, "empty lists without arrays");
    }
    for (uint32_t flag : {(uint32_t)HONU_ACL_INPLACE, (uint32_t)HONU_REGIONS_INPLACE}) {
        honu_meta r = base;
        r.present |= flag;
        CHECK(plan(r, g_var, g_acl, 8, g_reg, 8, 0, p) == HONU_ERR_INPUT, "an in-place flag is accepted");
    }
    { /* more entries than a batch can hold; the arrays are not read by the plan */
        honu_meta r = base;
        r.acl_count = CAP / sizeof(honu_acl) + 1;
        CHECK(plan(r, g_var, g_acl, 1ull << 40, g_reg, 8, 0, p) == HONU_ERR_CAPACITY, "nacl above a batch");
        r.acl_count = CAP / sizeof(honu_acl);
        CHECK(plan(r, g_var, g_acl, 1ull << 40, g_reg, 8, 0, p) == HONU_OK, "nacl a batch holds");
        r.acl_count = 0, r.regions_count = CAP / 4 + 1;
        CHECK(plan(r, g_var, g_acl, 8, g_reg, 1ull << 40, 0, p) == HONU_ERR_CAPACITY, "nreg above a batch");
        r.regions_count = CAP / 4;
        CHECK(plan(r, g_var, g_acl, 8, g_reg, 1ull << 40, 0, p) == HONU_OK && p.need == CAP, "nreg a batch holds");
    }
    { /* Marshal(nil, data): no spans, no lists, whatever the row says */
        honu_meta r;
        memset(&r, 0xFF, sizeof r);
        r.present &= ~(uint32_t)HONU_HAS_META;
        CHECK(plan(r, nullptr, nullptr, 0, nullptr, 0, 11, p) == HONU_OK, "a row without HONU_HAS_META is refused");
        for (int j = 0; j < 8; j++) CHECK(span_of(p.w, j)->off == 0 && span_of(p.w, j)->len == 0, "nil row: span %d", j);
        CHECK(p.nacl == 0 && p.nreg == 0 && p.w.acl_count == 0 && p.w.regions_count == 0, "nil row: its lists");
        CHECK(p.span_bytes == 0 && p.need == 11 && p.bound == kFixedBound + 11, "nil row: its size");
    }
}

int main() {
    copy_tests();
    cuts_tests();
    fill_tests();
    plan_tests();
    printf("ok copy %llu cuts %llu fill %llu plan %llu\n", n_copy, n_cuts, n_fill, n_plan);
    return 0;
}
"""

THRESHOLD = r"""
#include <cstdio>
#include "@CSRC@/host_copy.h"
int main() { return printf("%llu\n", (unsigned long long)honu::kParallelCopyMin) < 0; }
"""

SANITIZERS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}


def _build(tmp_path, name, text, flags):
    src = tmp_path / (name + ".cpp")
    src.write_text(text.replace("@CSRC@", CSRC))
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-Wall", "-Werror", *flags,
                    "-o", str(exe), str(src)], check=True)
    return exe


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_feed_host_code_under_sanitizers(tmp_path, sanitizer):
    exe = _build(tmp_path, "feed_host_" + sanitizer, PROGRAM, SANITIZERS[sanitizer])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    w = r.stdout.split()
    counts = dict(zip(w[1::2], map(int, w[2::2])))
    assert counts["copy"] >= 250 and counts["cuts"] >= 300 and counts["fill"] == 400
    assert counts["plan"] >= 100
    # the threshold the GPU tests size their batches from, read in the same run
    from test_gpu_feeds import PARALLEL_COPY_MIN
    t = subprocess.run([str(_build(tmp_path, "threshold", THRESHOLD, []))], capture_output=True, text=True)
    assert t.returncode == 0 and int(t.stdout) == PARALLEL_COPY_MIN
