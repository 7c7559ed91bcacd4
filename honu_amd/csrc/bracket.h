// bracket.h — the arithmetic of the 64-mids-per-step search (wave_bound,
// keycol.h) as plain functions: no HIP, <stdint.h> alone, the qualifier from a
// macro, so the host program of tests/test_key_bracket_host.py runs what the
// kernels run.
#pragma once

#include <stdint.h>

#ifndef HONU_BRACKET_FN
#define HONU_BRACKET_FN static inline
#endif

// lane l's mid in the bracket [lo, lo + s), l < min(s, 64): lo + floor(l s / 64)
// over more than 64 rows (distinct, lo the first), else lo + l. (l = 64 gives
// the bracket's end or less: bracket_step asks for it.)
HONU_BRACKET_FN uint32_t bracket_mid(uint32_t lo, uint32_t s, uint32_t l) {
    return s > 64 ? lo + (uint32_t)(((uint64_t)l * s) >> 6) : lo + l;
}

// the bracket after t of its lanes said yes, t <= min(hi - lo, 64): taken as
// the first t, so the answer lies past mid(t - 1) and at or before mid(t)
HONU_BRACKET_FN void bracket_step(uint32_t *lo, uint32_t *hi, uint32_t t) {
    const uint32_t l0 = *lo, h0 = *hi, s = h0 - l0;
    const uint32_t above = t < 64 ? bracket_mid(l0, s, t) : h0;
    const uint32_t l = t ? bracket_mid(l0, s, t - 1) + 1 : l0;
    const uint32_t h = above < h0 ? above : h0;
    *lo = l < h ? l : h;
    *hi = h;
}
