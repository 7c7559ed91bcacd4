"""The arithmetic of the bucketed column (honu_amd/csrc/bucket_off.h, the plain
functions merge_buckets.hip is written on) on the host: a C program with its
own main reads cases from a file, runs the clamp, a bucket's rows, the output
offsets, an output position's bucket, the local diagonal and its bracket, a
row's bucket in both forms (the arrays; the staged words), a bucket's span in
a staged run and the B row's index, and prints what it got. numpy says what it
should have been.

Every load of an offset or count goes through the header's load macro, which
the program defines as a function that checks the address against the case's
arrays and counts the loads: an entry outside [0, k] (or a count outside
[0, k)) fails the program whatever the sanitizers see, and the arrays are
exact-size allocations so that they see it too where the compiler links them.

Ascending offsets with runs of equal entries (empty buckets), offsets above n
(clamped), k = 0 and 1, with and without counts: exact against numpy.
Descending offsets and random garbage, counts and scanned offsets included:
only that every index asked was in range, every result inside its bounds and
every loop ended (the program returns, under a time limit).
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "honu_amd", "csrc", "bucket_off.h")
M32 = (1 << 32) - 1

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

static const uint64_t *arr[4];
static uint64_t arr_len[4];
static unsigned long long loads = 0;

static uint64_t checked_load(const uint64_t *p) {
    int i;
    loads++;
    for (i = 0; i < 4; i++)
        if (arr[i] && p >= arr[i] && p < arr[i] + arr_len[i]) return *p;
    printf("FAILED a load outside the arrays\n");
    exit(1);
}
#define HONU_BUCKET_LOAD(p) checked_load(p)
#include "%s"

static uint64_t *read_u64(FILE *f, uint64_t n) {
    uint64_t *a = malloc(n ? 8 * n : 1), i; /* exact size: the sanitizer sees entry n */
    for (i = 0; i < n; i++) {
        unsigned long long v;
        if (fscanf(f, "%%llu", &v) != 1) exit(2);
        a[i] = v;
    }
    return a;
}

static unsigned long long num(FILE *f) {
    unsigned long long v;
    if (fscanf(f, "%%llu", &v) != 1) exit(2);
    return v;
}

int main(int argc, char **argv) {
    FILE *f = fopen(argv[argc - 1], "r");
    unsigned long long cases, t, i, n;
    if (!f) return 2;
    cases = num(f);
    for (t = 0; t < cases; t++) {
        bucket_cols B;
        uint64_t *oa, *ob, *ca = NULL, *oo = NULL;
        int counted;
        B.k = (uint32_t)num(f), B.na = (uint32_t)num(f), B.nb = (uint32_t)num(f), counted = (int)num(f);
        oa = read_u64(f, (uint64_t)B.k + 1), ob = read_u64(f, (uint64_t)B.k + 1);
        if (counted) ca = read_u64(f, B.k), oo = read_u64(f, (uint64_t)B.k + 1);
        B.off_a = oa, B.off_b = ob, B.count_a = ca, B.off_out = oo;
        arr[0] = oa, arr[1] = ob, arr[2] = ca, arr[3] = oo;
        arr_len[0] = arr_len[1] = arr_len[3] = (uint64_t)B.k + 1, arr_len[2] = B.k;
        for (i = 0; i <= B.k; i++)
            printf("C %%u %%u %%u %%u %%u %%u\n", bucket_ea(&B, (uint32_t)i), bucket_eb(&B, (uint32_t)i),
                   bucket_out(&B, (uint32_t)i), bucket_pa(&B, (uint32_t)i), i < B.k ? bucket_va(&B, (uint32_t)i) : 0,
                   i < B.k ? bucket_vb(&B, (uint32_t)i) : 0);
        n = num(f); /* output positions */
        for (i = 0; i < n; i++) {
            const uint32_t d = (uint32_t)num(f), c = bucket_of_pos(&B, d);
            uint32_t l;
            if (c >= B.k) { printf("FAILED a bucket not below k\n"); return 1; }
            l = bucket_diag(&B, c, d);
            printf("D %%u %%u %%u %%u\n", c, l, bucket_split_lo(l, bucket_vb(&B, c)), bucket_split_hi(l, bucket_va(&B, c)));
        }
        n = num(f); /* rows of a slice of nbk buckets from c0 */
        for (i = 0; i < n; i++) {
            const uint32_t c0 = (uint32_t)num(f), nbk = (uint32_t)num(f), x = (uint32_t)num(f);
            uint32_t *pa = malloc(4 * (size_t)nbk), *eb = malloc(4 * (size_t)nbk), j;
            for (j = 0; j < nbk; j++) pa[j] = bucket_pa(&B, c0 + j), eb[j] = bucket_eb(&B, c0 + j);
            printf("S %%u %%u %%u %%u\n", bucket_of_row(&B, 0, c0, nbk, x), bucket_of_row(&B, 1, c0, nbk, x),
                   bucket_of_row_words(pa, nbk, x), bucket_of_row_words(eb, nbk, x));
            free(pa), free(eb);
        }
        free(oa), free(ob), free(ca), free(oo);
    }
    n = num(f); /* spans */
    for (i = 0; i < n; i++) {
        const uint32_t first = (uint32_t)num(f), next = (uint32_t)num(f), start = (uint32_t)num(f), len = (uint32_t)num(f);
        uint32_t lo, hi;
        bucket_span(first, next, start, len, &lo, &hi);
        printf("P %%u %%u\n", lo, hi);
    }
    n = num(f); /* B rows' indices */
    for (i = 0; i < n; i++) {
        const uint32_t order = (uint32_t)num(f), base = (uint32_t)num(f);
        printf("I %%u\n", bucket_b_index(order, base));
    }
    printf("ok %%llu\n", loads);
    return 0;
}
"""


class Case:
    def __init__(self, na, nb, off_a, off_b, count_a=None, off_out=None, exact=True):
        self.na, self.nb, self.k = int(na), int(nb), len(off_a) - 1
        self.off_a, self.off_b = [int(x) for x in off_a], [int(x) for x in off_b]
        self.count_a = None if count_a is None else [int(x) for x in count_a]
        self.exact = exact
        self.off_out = None
        if count_a is not None:
            if off_out is None:  # what the scan writes
                _, _, _, _, va, vb = self.columns(np.zeros(self.k + 1, np.uint64))
                off_out = np.concatenate([[0], np.cumsum(va + vb)])
            self.off_out = [int(x) for x in off_out]
        self.pos, self.slices = [], []

    def columns(self, off_out=None):
        """numpy's ea, eb, out, pa (k + 1 each), va, vb (k each), as Python ints in object arrays."""
        k = self.k
        ea = np.array([min(x, self.na) for x in self.off_a], dtype=object)
        eb = np.array([min(x, self.nb) for x in self.off_b], dtype=object)
        va = np.array([max(ea[c + 1] - ea[c], 0) for c in range(k)], dtype=object)
        vb = np.array([max(eb[c + 1] - eb[c], 0) for c in range(k)], dtype=object)
        if self.count_a is not None:
            va = np.array([min(self.count_a[c], va[c]) for c in range(k)], dtype=object)
            oo = self.off_out if off_out is None else off_out
            out = np.array([min(int(x), self.na + self.nb) for x in oo], dtype=object)
            pa = np.array([max(out[c] - eb[c], 0) for c in range(k + 1)], dtype=object)
        else:
            out = ea + eb
            out[0] = 0
            pa = ea.copy()
        return ea, eb, out, pa, va, vb

    def text(self):
        w = [f"{self.k} {self.na} {self.nb} {int(self.count_a is not None)}", " ".join(map(str, self.off_a)),
             " ".join(map(str, self.off_b))]
        if self.count_a is not None:
            w += [" ".join(map(str, self.count_a)), " ".join(map(str, self.off_out))]
        w += [str(len(self.pos)), " ".join(map(str, self.pos))]
        w += [str(len(self.slices)), " ".join(f"{a} {b} {c}" for a, b, c in self.slices)]
        return "\n".join(w)


def ascending(rng, k, n, empties, over=0):
    """k + 1 ascending offsets over n rows from 0, about `empties` of the buckets empty; the last
    `over` entries pushed above n."""
    sizes = rng.integers(1, 9, k) * (rng.random(k) >= empties)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if off[-1] > 0:
        off = off * n // max(int(off[-1]), 1) if n < off[-1] else off
    off = [int(x) for x in off]
    for j in range(over):
        off[k - j] = n + 1 + 7 * (over - j)
    return off


def add_queries(case, rng):
    k, n = case.k, case.na + case.nb
    if k == 0:
        return
    _, _, out, _, _, _ = case.columns()
    total = int(out[k])
    ds = set(int(x) for x in out.tolist()) | {0, n, max(total - 1, 0)}
    ds |= {min(max(d + e, 0), n) for d in list(ds) for e in (-1, 1)}
    ds |= set(int(x) for x in rng.integers(0, n + 1, 40))
    case.pos = sorted(ds)
    for _ in range(60):
        c0 = int(rng.integers(0, k))
        nbk = int(rng.integers(1, k - c0 + 1))
        case.slices.append((c0, nbk, int(rng.integers(0, n + 2))))
    case.slices.append((0, k, 0))
    case.slices.append((0, k, M32))


def build_cases():
    rng = np.random.default_rng(612)
    cases = []
    # ascending, with runs of equal entries, with and without counts
    for k, na, nb, empties in ((1, 40, 9, 0.0), (1, 0, 5, 0.0), (1, 7, 0, 0.0), (3, 60, 30, 0.4), (17, 500, 300, 0.5),
                               (200, 3000, 900, 0.7), (161, 1000, 1000, 0.0), (50, 0, 0, 1.0)):
        oa, ob = ascending(rng, k, na, empties), ascending(rng, k, nb, empties)
        na2, nb2 = max(na, oa[-1]), max(nb, ob[-1])
        cases.append(Case(na2, nb2, oa, ob))
        va = np.diff(np.array(oa))
        for counts in (va - (va > 0) * rng.integers(0, 2, k), va + rng.integers(0, 3, k), np.zeros(k, np.int64)):
            cases.append(Case(na2, nb2, oa, ob, count_a=counts))
    # offsets above n are clamped: the last entries of either side
    for over_a, over_b in ((1, 0), (0, 2), (3, 3)):
        oa, ob = ascending(rng, 12, 100, 0.3), ascending(rng, 12, 80, 0.3)
        na, nb = oa[-1], ob[-1]
        for j in range(over_a):
            oa[12 - j] = na + 5 + (over_a - j)
        for j in range(over_b):
            ob[12 - j] = nb + (1 << 40) + (over_b - j)
        cases.append(Case(na, nb, oa, ob))
        cases.append(Case(na, nb, oa, ob, count_a=[1 << 63] * 12))
    # k = 0
    cases.append(Case(5, 6, [0], [0]))
    cases.append(Case(0, 0, [0], [0], count_a=[], off_out=[0]))
    for c in cases:
        add_queries(c, rng)
    # descending and garbage: ranges and termination alone
    wild = []
    for k in (1, 2, 5, 64, 300):
        na, nb = int(rng.integers(0, 2000)), int(rng.integers(0, 2000))
        desc_a = sorted((int(x) for x in rng.integers(0, na + 50, k + 1)), reverse=True)
        desc_b = sorted((int(x) for x in rng.integers(0, nb + 50, k + 1)), reverse=True)
        wild.append(Case(na, nb, desc_a, desc_b, exact=False))
        wild.append(Case(na, nb, desc_a, desc_b, count_a=rng.integers(0, 20, k),
                         off_out=sorted((int(x) for x in rng.integers(0, na + nb + 9, k + 1)), reverse=True),
                         exact=False))
        for top in (50, 1 << 20, 1 << 64):
            g = lambda m: [int(x) for x in rng.integers(0, top, m, dtype=np.uint64)]  # noqa: E731
            wild.append(Case(na, nb, g(k + 1), g(k + 1), exact=False))
            wild.append(Case(na, nb, g(k + 1), g(k + 1), count_a=g(k), off_out=g(k + 1), exact=False))
    for c in wild:
        n = c.na + c.nb
        c.pos = sorted(set(int(x) for x in rng.integers(0, n + 1, 50)) | {0, n})
        for _ in range(50):
            c0 = int(rng.integers(0, c.k))
            c.slices.append((c0, int(rng.integers(1, c.k - c0 + 1)), int(rng.integers(0, M32 + 1))))
    return cases + wild


SPANS = [(0, 0, 0, 0), (5, 9, 3, 100), (5, 9, 7, 100), (5, 9, 10, 100), (5, 9, 0, 6), (5, 9, 0, 4), (9, 5, 3, 100),
         (M32, M32, 0, 1024), (0, M32, M32, 1024), (100, 50, 70, 10)]
INDICES = [(0, 0), (5, 7), (M32, 1), (M32, M32), (123456, 1 << 31)]


def run_program(tmp_path, cases):
    c = tmp_path / "bucket_off.c"
    c.write_text(PROGRAM % HEADER)
    exe = tmp_path / "bucket_off"
    cc = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-o", str(exe), str(c)]
    # with the sanitizers where the compiler links them for a plain C program, without them elsewhere
    if subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                      capture_output=True).returncode != 0:
        subprocess.run(cc, check=True)
    text = [str(len(cases))] + [x.text() for x in cases]
    text += [str(len(SPANS))] + [" ".join(map(str, s)) for s in SPANS]
    text += [str(len(INDICES))] + [" ".join(map(str, s)) for s in INDICES]
    inp = tmp_path / "cases.txt"
    inp.write_text("\n".join(text) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, env=env, timeout=120)  # every loop ends
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    return lines


def test_bucket_arithmetic_against_numpy(tmp_path):
    cases = build_cases()
    lines = iter(run_program(tmp_path, cases))

    def take(tag):
        w = next(lines).split()
        assert w[0] == tag, (tag, w)
        return [int(x) for x in w[1:]]

    exact = wild = 0
    for case in cases:
        k, n = case.k, case.na + case.nb
        ea, eb, out, pa, va, vb = case.columns()
        got_va, got_vb = [], []
        for c in range(k + 1):
            g = take("C")
            want = [ea[c], eb[c], out[c], pa[c], va[c] if c < k else 0, vb[c] if c < k else 0]
            assert g == [int(x) for x in want], (k, c, g, want)  # the columns are exact whatever the offsets hold
            got_va.append(g[4]), got_vb.append(g[5])
            assert g[0] <= case.na and g[1] <= case.nb and g[2] <= n
            if c < k:  # the views lie inside the arenas
                assert g[0] + g[4] <= case.na and g[1] + g[5] <= case.nb
        for d in case.pos:
            c, l, lo, hi = take("D")
            assert 0 <= c < k and l <= got_va[c] + got_vb[c] and lo <= hi <= got_va[c]
            assert hi == lo or (l - 1 - (hi - 1) >= 0 and l - 1 - lo < got_vb[c])  # B's row of every mid asked
            if case.exact and d < int(out[k]):
                want_c = int(np.searchsorted(np.array(out[1:], np.int64), d, side="right"))
                assert c == want_c and out[c] <= d < out[c + 1], (k, d, c, want_c)
                assert l == d - out[c] and lo == max(l - vb[c], 0) and hi == min(l, va[c])
                exact += 1
        for c0, nbk, x in case.slices:
            ja, jb, jaw, jbw = take("S")
            assert ja == jaw and jb == jbw and 0 <= ja < nbk and 0 <= jb < nbk
            if case.exact:
                for j, col in ((ja, pa), (jb, eb)):
                    sl = np.array(col[c0:c0 + nbk], np.int64)
                    want = min(max(int(np.searchsorted(sl, x, side="right")) - 1, 0), nbk - 1)
                    assert j == want, (k, c0, nbk, x, j, want)
                exact += 1
            else:
                wild += 1
    for first, nxt, start, ln in SPANS:
        lo, hi = take("P")
        want_lo = min(max(first - start, 0), ln)
        assert (lo, hi) == (want_lo, max(min(max(nxt - start, 0), ln), want_lo)) and lo <= hi <= ln
    for order, base in INDICES:
        assert take("I") == [(order + base) & M32]
    assert exact > 3000 and wild > 1500, (exact, wild)
    assert int(next(lines).split()[1]) > 100000
