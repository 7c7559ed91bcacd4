"""The arithmetic of the route (honu_amd/csrc/route_find.h, the plain
functions route.hip's find and emit are written on) on the host: a C program
that runs the ID compare, the lower bound over the table in both of its forms
(the table's bytes at an odd address; the staged big-endian words), the class
of a position, the sort row of a class and an offset as a bound over the
sorted classes.

Tables of 0, 1, 2, 3, 2047, 2048 and 2049 rows, ascending and distinct, that
hold the all-0x00 and the all-0xff ID, rows that differ from another row only
in byte 15 and rows that differ only in byte 0. Probes: every row, every row
with byte 0 or byte 15 one up and one down, the all-0x00 and all-0xff IDs and
seeded IDs, so below, between and above the rows. Everything is checked against
a plain linear scan with memcmp. Seeded unsorted tables with repeats, and
sorted-class rows of arbitrary bytes: every class lies in [0, k + 1] and every
bound inside its bracket (the program runs under the sanitizers where the
compiler links them, so a row asked outside the table would be seen).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "honu_amd", "csrc", "route_find.h")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "%s"

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static unsigned long long checked = 0;

static void fail(const char *what, uint32_t k, uint64_t x) {
    printf("FAILED %%s: %%u rows, with %%llu\n", what, k, (unsigned long long)x);
    exit(1);
}

static void seeded(uint8_t id[16], uint64_t seed) {
    const uint64_t a = mix(seed), b = mix(seed ^ 0x55);
    memcpy(id, &a, 8);
    memcpy(id + 8, &b, 8);
}

static int by_bytes(const void *a, const void *b) { return memcmp(a, b, 16); }

static int holds(const uint8_t *rows, uint32_t n, const uint8_t id[16]) {
    uint32_t r;
    for (r = 0; r < n; r++)
        if (!memcmp(rows + 16 * r, id, 16)) return 1;
    return 0;
}

/* k distinct rows, ascending: the two extreme IDs, seeded rows, and rows that differ from an
   earlier one in byte 15 alone or in byte 0 alone */
static void make_table(uint8_t *rows, uint32_t k, uint64_t seed) {
    uint32_t n = 0;
    uint64_t j = 0;
    uint8_t id[16];
    if (k >= 2) {
        memset(rows, 0x00, 16);
        memset(rows + 16, 0xFF, 16);
        n = 2;
    }
    while (n < k) {
        j++;
        if (n >= 3 && j %% 4 == 0) {
            memcpy(id, rows + 16 * (mix(seed ^ j) %% n), 16);
            id[15] ^= (uint8_t)(1u << (mix(j) %% 8));
        } else if (n >= 3 && j %% 4 == 1) {
            memcpy(id, rows + 16 * (mix(seed ^ j) %% n), 16);
            id[0] ^= (uint8_t)(1u << (mix(j) %% 8));
        } else {
            seeded(id, seed ^ (j << 20));
        }
        if (holds(rows, n, id)) continue;
        memcpy(rows + 16 * n++, id, 16);
    }
    qsort(rows, k, 16, by_bytes);
}

/* one probe against the linear scan */
static void probe(const uint8_t *table, const uint32_t *words, uint32_t k, const uint8_t id[16]) {
    uint32_t below = 0, first = k, r, w[4], lb;
    int same;
    for (r = 0; r < k; r++) {
        const int c = memcmp(table + 16 * r, id, 16);
        if (c < 0) below++;
        if (c == 0 && first == k) first = r;
    }
    route_bytes_id(id, w);
    lb = route_lower_bound_bytes(table, k, w);
    if (lb != below) fail("the lower bound over the table's bytes", k, lb);
    if (route_lower_bound_words(words, k, w) != lb) fail("the two forms differ", k, lb);
    same = lb < k && route_id_same(words + 4 * lb, w);
    if (route_class(1, lb, same, k) != first) fail("the class", k, first);
    if (route_class(0, lb, same, k) != k + 1) fail("the class of a position that does not take part", k, lb);
    checked++;
}

static void sorted_table(uint32_t k, uint64_t seed) {
    uint8_t *rows = malloc(16 * (size_t)k + 1), *store = malloc(16 * (size_t)k + 1), *table = store + 1; /* odd address */
    uint32_t *words = malloc(16 * (size_t)k + 4);
    uint32_t r, j, a[4], b[4];
    uint8_t id[16];
    make_table(rows, k, seed);
    memcpy(table, rows, 16 * (size_t)k);
    for (r = 0; r < k; r++) route_bytes_id(table + 16 * r, words + 4 * r);
    for (r = 0; r + 1 < k; r++) { /* the compare against memcmp, neighbours and a far row */
        const uint32_t far = (uint32_t)(mix(seed ^ r) %% k);
        if (memcmp(table + 16 * r, table + 16 * (r + 1), 16) >= 0) fail("the table is not ascending", k, r);
        route_bytes_id(table + 16 * r, a);
        route_bytes_id(table + 16 * far, b);
        if (route_id_before(a, b) != (memcmp(table + 16 * r, table + 16 * far, 16) < 0)) fail("before", k, r);
        if (route_id_same(a, b) != (r == far)) fail("same", k, r);
        if (!route_id_before(words + 4 * r, words + 4 * (r + 1)) || route_id_before(words + 4 * (r + 1), words + 4 * r))
            fail("neighbours", k, r);
    }
    for (r = 0; r < k; r++) {
        memcpy(id, table + 16 * r, 16);
        probe(table, words, k, id);
        for (j = 0; j < 4; j++) { /* byte 0 or byte 15, one up or one down (wrapping) */
            memcpy(id, table + 16 * r, 16);
            id[j & 1 ? 15 : 0] += (uint8_t)(j & 2 ? 1 : 255);
            probe(table, words, k, id);
        }
    }
    memset(id, 0x00, 16);
    probe(table, words, k, id);
    memset(id, 0xFF, 16);
    probe(table, words, k, id);
    for (j = 0; j < 2000; j++) {
        seeded(id, seed ^ 0xABCDEF ^ ((uint64_t)j << 24));
        probe(table, words, k, id);
    }
    free(rows), free(store), free(words);
}

/* rows out of order and repeated: wrong classes perhaps, never one outside [0, k + 1] */
static void unsorted_table(uint32_t k, uint64_t seed) {
    uint8_t *table = malloc(16 * (size_t)k + 1);
    uint32_t *words = malloc(16 * (size_t)k + 4);
    uint32_t r, j, w[4];
    uint8_t id[16];
    for (r = 0; r < k; r++) {
        if (r && mix(seed ^ r) %% 3 == 0) memcpy(table + 16 * r, table + 16 * (mix(seed + r) %% r), 16);
        else seeded(table + 16 * r, seed ^ ((uint64_t)r << 16));
        route_bytes_id(table + 16 * r, words + 4 * r);
    }
    for (j = 0; j < 3000; j++) {
        uint32_t lb, lw, c;
        if (k && j %% 2) memcpy(id, table + 16 * (mix(seed ^ j) %% k), 16);
        else seeded(id, seed ^ 0x777 ^ ((uint64_t)j << 28));
        route_bytes_id(id, w);
        lb = route_lower_bound_bytes(table, k, w);
        lw = route_lower_bound_words(words, k, w);
        if (lb > k || lw != lb) fail("a bound outside an unsorted table, or the forms differ", k, lb);
        c = route_class((int)(j %% 5 != 0), lb, lb < k && route_id_same(words + 4 * lb, w), k);
        if (c > k + 1) fail("a class above k + 1", k, c);
        if (c < k && memcmp(table + 16 * c, id, 16)) fail("a class whose row is not the ID", k, c);
        checked++;
    }
    free(table), free(words);
}

/* the sort row of a class */
static void rows_of_classes(void) {
    static const uint32_t cs[] = {0, 1, 2, 255, 256, 257, 65535, 65536, 0xFFFFFF, 0x1000000, 0x12345678, 0xFFFFFFFDu};
    unsigned i, j;
    for (i = 0; i < sizeof cs / sizeof *cs; i++) {
        const uint32_t c = cs[i], w0 = route_row_word0(c), w1 = route_row_word1(c);
        uint8_t row[29];
        memset(row, 0, sizeof row);
        for (j = 0; j < 4; j++) row[j] = (uint8_t)(w0 >> (8 * j)), row[4 + j] = (uint8_t)(w1 >> (8 * j)); /* little-endian stores */
        if (row[0] != ROUTE_ROW_BYTE0 || route_bytes_be32(row + 1) != c || row[5] || row[6] || row[7]) fail("the sort row", 0, c);
        if (route_row_class(row, 0xFFFFFFFCu) != c) fail("the row's class", 0, c);
        if (route_row_class(row, 3) != (c < 4 ? c : 4)) fail("the row's class is clamped to k + 1", 3, c);
        checked++;
    }
}

/* offsets over sorted classes: counts[c] rows of class c, c <= k + 1 */
static void offsets(uint32_t k, uint64_t seed, uint32_t most) {
    uint32_t *counts = calloc(k + 2, sizeof *counts), *start = calloc(k + 3, sizeof *start);
    uint32_t c, g, m = 0;
    uint8_t *sorted;
    for (c = 0; c < k + 2; c++) {
        counts[c] = mix(seed ^ c) %% 3 == 0 ? 0 : (uint32_t)(mix(seed + c) %% (most + 1)); /* empty classes between full ones */
        start[c] = m;
        m += counts[c];
    }
    start[k + 2] = m;
    sorted = calloc(29 * (size_t)m + 1, 1);
    for (c = 0; c < k + 2; c++)
        for (g = start[c]; g < start[c + 1]; g++) {
            const uint32_t w0 = route_row_word0(c), w1 = route_row_word1(c);
            memcpy(sorted + 29 * (size_t)g, &w0, 4), memcpy(sorted + 29 * (size_t)g + 4, &w1, 4);
        }
    for (c = 0; c <= k + 2; c++) {
        const uint32_t lo = route_offset(sorted, 0, m, c, k);
        if (lo != start[c]) fail("an offset", k, c);
        if (c < k + 2 && route_offset(sorted, lo, m, c + 1, k) - lo != counts[c]) fail("a count", k, c);
        checked++;
    }
    for (g = 0; g < m; g++) { /* the emit's row: its class, head, and index inside the class */
        const uint32_t cg = route_row_class(sorted + 29 * (size_t)g, k);
        const int head = g == 0 || route_row_class(sorted + 29 * (size_t)(g - 1), k) != cg;
        const uint32_t local = head ? 0 : g - route_offset(sorted, 0, g - 1, cg, k);
        if (g < start[cg] || g >= start[cg + 1]) fail("a row's class", k, g);
        if (head != (g == start[cg]) || local != g - start[cg]) fail("a row's head or local index", k, g);
        checked++;
    }
    for (g = 0; g < 29 * m; g++) sorted[g] = (uint8_t)mix(seed ^ g); /* arbitrary bytes: inside the bracket */
    for (c = 0; c <= k + 2 && m; c++) {
        const uint32_t lo = (uint32_t)(mix(seed ^ c ^ 9) %% m), r = route_offset(sorted, lo, m, c, k);
        if (r < lo || r > m) fail("an offset outside its bracket", k, r);
        checked++;
    }
    free(counts), free(start), free(sorted);
}

int main(void) {
    static const uint32_t ks[] = {0, 1, 2, 3, 2047, 2048, 2049};
    unsigned i;
    for (i = 0; i < sizeof ks / sizeof *ks; i++) {
        sorted_table(ks[i], mix(ks[i] + 1));
        unsorted_table(ks[i], mix(ks[i] + 101));
        offsets(ks[i], mix(ks[i] + 201), ks[i] > 100 ? 3 : 700);
    }
    rows_of_classes();
    printf("ok %%llu\n", checked);
    return 0;
}
"""


def test_compare_bounds_classes_and_offsets(tmp_path):
    c = tmp_path / "route_find.c"
    c.write_text(PROGRAM % HEADER)
    exe = tmp_path / "route_find"
    cc = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-o", str(exe), str(c)]
    # with the sanitizers where the compiler links them for a plain C program, without them elsewhere
    if subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                      capture_output=True).returncode != 0:
        subprocess.run(cc, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 50000
