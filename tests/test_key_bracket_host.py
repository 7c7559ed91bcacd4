"""The bracket arithmetic of wave_bound (honu_amd/csrc/bracket.h, the plain
functions keycol.h's wave search is written on) on the host: a C program that
plays the 64 lanes of a wave as wave_bound does, a lane asking its mid when it
lies in the bracket, the ballot's count going to bracket_step.

For every bracket size and start below, (a) a monotone predicate with bound b
(yes below b) returns exactly b, for b at both ends and a sample in between
(every b for the small sizes), and (b) seeded answers that depend on nothing
but a hash of (seed, step, mid) keep the invariant. After every step of both:
lo <= lo' <= hi' <= hi, hi' - lo' < hi - lo, every mid asked in [lo, hi), and
the step count within the least k >= 1 with 64^k >= size, 6 at the most.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "honu_amd", "csrc", "bracket.h")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "%s"

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static void fail(const char *what, uint32_t lo, uint32_t hi, uint64_t x) {
    printf("FAILED %%s: bracket [%%u, %%u) with %%llu\n", what, lo, hi, (unsigned long long)x);
    exit(1);
}

static int max_steps(uint32_t s) {
    int k = 1;
    uint64_t p = 64;
    if (s == 0) return 0;
    while (p < s) p *= 64, k++;
    return k;
}

/* the wave: monotone (yes below b) when seed == 0, else hashed answers */
static uint32_t run(uint32_t lo0, uint32_t hi0, uint32_t b, uint64_t seed) {
    uint32_t lo = lo0, hi = hi0;
    int steps = 0;
    while (lo < hi) {
        const uint32_t s = hi - lo;
        uint32_t t = 0, l, before_lo = lo, before_hi = hi;
        for (l = 0; l < 64; l++) {
            uint32_t mid;
            if (!(l < s)) continue; /* past the bracket: no */
            mid = bracket_mid(lo, s, l);
            if (mid < lo || mid >= hi) fail("a mid outside the bracket", lo, hi, mid);
            t += seed ? (uint32_t)(mix(seed ^ mix(((uint64_t)steps << 32) | mid)) & 1) : mid < b;
        }
        bracket_step(&lo, &hi, t);
        if (!(before_lo <= lo && lo <= hi && hi <= before_hi)) fail("the bracket left its bounds", before_lo, before_hi, t);
        if (!(hi - lo < s)) fail("the bracket did not shrink", before_lo, before_hi, t);
        if (++steps > max_steps(hi0 - lo0) || steps > 6) fail("too many steps", lo0, hi0, (uint64_t)steps);
    }
    if (lo < lo0 || lo > hi0) fail("the result outside the bracket", lo0, hi0, lo);
    return lo;
}

static unsigned long long runs = 0;

static void bracket(uint32_t lo, uint32_t size) {
    const uint32_t hi = lo + size;
    uint64_t i;
    const uint64_t dense = size <= 129 ? size : 0;
    for (i = 0; i <= dense; i++) /* every bound of a small bracket */
        if (run(lo, hi, lo + (uint32_t)i, 0) != lo + (uint32_t)i) fail("a small bracket's bound", lo, hi, lo + i);
    for (i = 0; i < 300; i++) { /* both ends, the rows beside them, a sample in between */
        uint32_t b = i == 0 ? lo : i == 1 ? hi : i == 2 ? lo + (size > 0) : i == 3 ? hi - (size > 0)
                   : lo + (uint32_t)(mix(((uint64_t)lo << 32) ^ size ^ (i << 48)) %% ((uint64_t)size + 1));
        if (run(lo, hi, b, 0) != b) fail("a monotone predicate's bound", lo, hi, b);
        runs++;
    }
    for (i = 1; i <= 300; i++) run(lo, hi, 0, mix(i ^ ((uint64_t)size << 20) ^ lo) | 1), runs++;
}

int main(void) {
    static const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 4095, 4096, 4097, 4160, 4161, 1u << 20};
    static const uint32_t los[] = {0, 1, 63, 64, 1000003, 1u << 31, 0xFFFFFFFFu - (1u << 20)};
    unsigned i, j;
    for (j = 0; j < sizeof los / sizeof *los; j++) {
        for (i = 0; i < sizeof sizes / sizeof *sizes; i++) {
            bracket(los[j], sizes[i]);
            bracket(0xFFFFFFFFu - sizes[i], sizes[i]); /* the bracket that ends at 2^32 - 1 */
        }
        bracket(los[j], 0xFFFFFFFFu - los[j]); /* 2^32 - 1 - lo */
    }
    if (max_steps(0xFFFFFFFFu) != 6 || max_steps(64) != 1 || max_steps(65) != 2 || max_steps(4097) != 3) return 2;
    printf("ok %%llu\n", runs);
    return 0;
}
"""


def test_bracket_invariant_and_exact_bounds(tmp_path):
    c = tmp_path / "bracket.c"
    c.write_text(PROGRAM % HEADER)
    exe = tmp_path / "bracket"
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 100000
