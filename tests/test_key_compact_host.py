"""The rank arithmetic of the stable stream compaction
(honu_amd/csrc/compact_rank.h, the plain functions compact.h's mark and place
are written on) on the host: a C program that plays the lanes as the kernels
of delete.hip, filter.hip and reclaim.hip do. A column is whole tiles of 1024
rows and a last tile of 1, 63, 64, 65, 128 or 1024 rows; the mark gives each
tile its 16 ballots and its kept count, a plain loop scans the counts, and the
place takes every row's rank out of the tile's masks and their prefix.

For the masks all kept, none kept, alternating, one bit per word and seeded
random, against a plain loop over the rows: the kept rows' ranks are
0 .. kept - 1 in row order, the removed rows' destinations kept .. rows - 1 in
row order, the two sets are disjoint and cover the rows, the rank of row x out
of the masks alone (filter's offsets) is the lane's, and no clamp changes
anything. With seeded masks, counts and a total that do not belong together,
every destination the clamps let through lies inside the rows.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "honu_amd", "csrc", "compact_rank.h")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "%s"

#define TILE 1024u
#define WORDS (TILE / 64)
#define MAX_TILES 3
#define MAX_ROWS (MAX_TILES * TILE)

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static void fail(const char *what, uint32_t n, int pattern, uint64_t x) {
    printf("FAILED %%s: %%u rows, pattern %%d, with %%llu\n", what, n, pattern, (unsigned long long)x);
    exit(1);
}

/* does row p stay? 0 all, 1 none, 2 alternating, 3 one bit per word, else seeded */
static int stays(int pattern, uint64_t seed, uint32_t p) {
    switch (pattern) {
    case 0: return 1;
    case 1: return 0;
    case 2: return p & 1;
    case 3: return p %% 64 == (p / 64 * 7 + 5) %% 64;
    default: return (int)(mix(seed ^ mix(p)) & 1);
    }
}

static uint64_t msk[MAX_TILES][WORDS], cnt[MAX_TILES], base[MAX_TILES];
static uint8_t seen[MAX_ROWS];
static unsigned long long checked = 0;

/* the mark: a ballot per 64 rows, a row past the column answers no */
static void mark(uint32_t n, uint32_t tiles, int pattern, uint64_t seed) {
    uint32_t tile, j, lane;
    for (tile = 0; tile < tiles; tile++) {
        cnt[tile] = 0;
        for (j = 0; j < WORDS; j++) {
            uint64_t bits = 0;
            for (lane = 0; lane < 64; lane++) {
                const uint32_t p = tile * TILE + j * 64 + lane;
                if (p < n && stays(pattern, seed, p)) bits |= 1ull << lane;
            }
            msk[tile][j] = bits;
            cnt[tile] += (uint64_t)__builtin_popcountll(bits);
        }
    }
}

/* the mark's own masks and counts: the place against a plain loop over the rows */
static void own(uint32_t n, int pattern, uint64_t seed) {
    const uint32_t tiles = (n + TILE - 1) / TILE;
    uint32_t tile, j, lane, p;
    uint64_t kept = 0, k = 0, r = 0;
    mark(n, tiles, pattern, seed);
    for (tile = 0; tile < tiles; tile++) base[tile] = kept, kept += cnt[tile]; /* the scan */
    memset(seen, 0, sizeof seen);
    for (p = 0; p < n; p++) { /* rows in order: k kept and r removed before row p */
        uint64_t before, dst;
        int bit;
        tile = p / TILE, j = p %% TILE / 64, lane = p %% 64;
        before = compact_rank_lane(base[tile] + compact_words_before(msk[tile], j), msk[tile][j], lane); /* pre[j] */
        bit = (int)((msk[tile][j] >> lane) & 1);
        if (bit != stays(pattern, seed, p)) fail("a mask bit is not the row's answer", n, pattern, p);
        if (before != k) fail("kept_before is not the kept rows before the row", n, pattern, p);
        if (compact_rank_row(base[tile], msk[tile], p %% TILE) != before) fail("the rank of row x", n, pattern, p);
        dst = bit ? before : compact_removed_dst(kept, p, before);
        if (dst != (bit ? k : kept + r)) fail("a destination out of row order", n, pattern, p);
        if (compact_dst_or_stay(dst, n, p) != dst) fail("delete's clamp moved a row", n, pattern, p);
        if (bit && compact_at_most(before, p) != before) fail("filter's clamp moved a row", n, pattern, p);
        if (!compact_inside(bit ? before : dst, bit ? kept : n)) fail("reclaim's clamp dropped a slot", n, pattern, p);
        if (dst >= n || seen[dst]++) fail("two rows at one destination", n, pattern, dst);
        if (bit) k++;
        else r++;
        checked++;
    }
    if (k != kept || k + r != n) fail("the sets do not cover the rows", n, pattern, k);
    if (compact_at_most(kept, n) != kept) fail("the total above the rows", n, pattern, kept);
}

/* masks, scanned counts and a total that are not one mark's: the clamps */
static void foreign(uint32_t n, uint64_t seed) {
    const uint32_t tiles = (n + TILE - 1) / TILE;
    const uint64_t total = mix(seed) %% 4 ? mix(seed ^ 1) %% (2ull * n + 2) : mix(seed ^ 1);
    const uint64_t kept = total < n ? total : n; /* as every place kernel reads it */
    uint32_t tile, j, lane;
    for (tile = 0; tile < tiles; tile++) {
        base[tile] = mix(seed ^ tile) %% 3 ? mix(seed ^ tile ^ 2) %% (2ull * n + 2) : mix(seed ^ tile ^ 2);
        for (j = 0; j < WORDS; j++) msk[tile][j] = mix(seed ^ mix(((uint64_t)tile << 8) | j)); /* bits past n too */
    }
    for (tile = 0; tile < tiles; tile++)
        for (j = 0; j < WORDS; j++)
            for (lane = 0; lane < 64; lane++) {
                const uint64_t p = (uint64_t)tile * TILE + j * 64 + lane;
                const uint64_t before = compact_rank_lane(base[tile] + compact_words_before(msk[tile], j), msk[tile][j], lane);
                const int bit = (int)((msk[tile][j] >> lane) & 1);
                uint64_t dst;
                if (p >= n) continue;
                if (compact_rank_row(base[tile], msk[tile], (uint32_t)(p %% TILE)) != before) fail("the rank of row x", n, -1, p);
                /* delete.hip */
                dst = compact_dst_or_stay(bit ? before : compact_removed_dst(kept, p, before), n, p);
                if (dst >= n) fail("delete writes outside the rows", n, -1, dst);
                /* filter.hip: the place and the offsets */
                if (bit && compact_at_most(before, p) >= n) fail("filter writes outside the rows", n, -1, p);
                if (compact_at_most(before, kept) > n) fail("an offset above the rows", n, -1, p);
                /* reclaim.hip: a freed record's slot, a kept record's row */
                dst = compact_removed_dst(kept, p, before);
                if (!bit && compact_inside(dst, n) && dst >= n) fail("reclaim writes a slot outside", n, -1, dst);
                if (bit && compact_inside(before, kept) && before >= n) fail("reclaim writes a row outside", n, -1, p);
                checked++;
            }
}

int main(void) {
    static const uint32_t last[] = {1, 63, 64, 65, 128, 1024};
    uint32_t lane, whole;
    unsigned i;
    int pattern;
    for (lane = 0; lane < 64; lane++) { /* the lanes below, bit by bit */
        uint64_t m = 0;
        uint32_t l;
        for (l = 0; l < lane; l++) m |= 1ull << l;
        if (compact_lanes_below(lane) != m) fail("the lanes below", 0, 0, lane);
    }
    for (whole = 0; whole < MAX_TILES; whole++)
        for (i = 0; i < sizeof last / sizeof *last; i++) {
            const uint32_t n = whole * TILE + last[i];
            for (pattern = 0; pattern < 4; pattern++) own(n, pattern, 0);
            for (pattern = 4; pattern < 12; pattern++) own(n, pattern, mix(((uint64_t)n << 8) | (unsigned)pattern));
            for (pattern = 0; pattern < 32; pattern++) foreign(n, mix(((uint64_t)n << 16) | (unsigned)pattern | 1u << 15));
        }
    printf("ok %%llu\n", checked);
    return 0;
}
"""


def test_ranks_destinations_and_clamps(tmp_path):
    c = tmp_path / "compact.c"
    c.write_text(PROGRAM % HEADER)
    exe = tmp_path / "compact"
    cc = ["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-o", str(exe), str(c)]
    # with the sanitizers where the compiler links them for a plain C program, without them elsewhere
    if subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                      capture_output=True).returncode != 0:
        subprocess.run(cc, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 500000
