"""CPU self-test of tests/guards.py: numpy "writers" that are deliberately
wrong in the ways a byte-layout kernel goes wrong, each of which the helper
must catch. This is the evidence that the GPU write-set tests
(test_gpu_bounds.py, test_gpu_placement.py) would fail on a subtly wrong
kernel; no GPU run with a broken kernel is needed for it."""
import numpy as np
import pytest

import guards

# a records arena of four ranges; range 2 is a skipped (failed) record's
RANGES = [(0, 37), (37, 101), (101, 150), (150, 203)]
SKIPPED = 2
TOTAL = RANGES[-1][1]
EXPECT = (np.arange(TOTAL) * 7 + 3).astype(np.uint8)


def allowed():
    return [r for k, r in enumerate(RANGES) if k != SKIPPED]


def write_right(view):
    for a, b in allowed():
        view[a:b] = EXPECT[a:b]


def check(view):
    """What every GPU test does after a call: the exact compare inside the
    allowed ranges, then the pattern everywhere else."""
    got = guards.block_of(view).bytes()
    for a, b in allowed():
        assert got[a:b].tobytes() == EXPECT[a:b].tobytes(), (a, b)
    guards.assert_untouched(view, allowed())


def run(writer, phase=0):
    def body(fill):
        view = guards.guarded(TOTAL, phase=phase, fill=fill)
        writer(view)
        check(view)
    return guards.twice(body)


@pytest.mark.parametrize("phase", [0, 1, 16, 63, 129])
def test_right_writer_passes(phase):
    run(write_right, phase)


def test_block_layout_and_pattern():
    v = guards.guarded(100, phase=24, fill=0x00)
    b = guards.block_of(v)
    assert v.ctypes.data % 256 == 24 and len(v) == 100  # front = 256: the phase is the address's
    assert b.raw.ctypes.data % 256 == 0 and len(b.raw) == 256 + 24 + 100 + 256
    w = guards.block_of(guards.guarded(100, phase=24, fill=0xFF)).raw
    assert ((b.raw ^ w) == 0xFF).all()  # the fills differ in every bit of every byte
    assert (b.raw[:-1] != b.raw[1:]).all()  # position dependent
    guards.assert_untouched(v, [])
    z = guards.guarded(0, fill=0xFF)  # an empty view is still a valid address to pass
    assert len(z) == 0 and z.ctypes.data % 256 == 0
    guards.assert_untouched(z, [])
    with pytest.raises(ValueError):
        guards.assert_untouched(v, [(90, 101)])  # a range outside the view is a test bug


def test_overshoot_by_one_byte_is_caught():
    """A tail one byte past its range: into the skipped record (inside the
    arena) and past the arena's end (the back guard band)."""
    def into_neighbour(view):
        write_right(view)
        view[101] = EXPECT[101]  # range 1 ends at 101; 101 starts the skipped range
    with pytest.raises(AssertionError, match=r"first at offset 101 .*1 byte\(s\) past the end of allowed range \[0, 101\)"):
        run(into_neighbour)

    def past_end(view):
        write_right(view)
        guards.block_of(view).raw[256 + TOTAL] = 0x5A
    with pytest.raises(AssertionError, match=r"offset 203 \(in the back guard band, 1 byte"):
        run(past_end)


def test_tail_rounded_up_to_16_is_caught():
    def rounded(view):
        write_right(view)
        raw = guards.block_of(view).raw
        end = 256 + TOTAL
        raw[end:(end + 15) // 16 * 16] = 0  # a whole-chunk store at a partial end chunk
    with pytest.raises(AssertionError, match=r"first at offset 203 .*last at offset 207 "):
        run(rounded)


def test_write_into_skipped_range_is_caught():
    def all_ranges(view):
        view[:] = EXPECT  # the skipped record's bytes too, right as they are
    with pytest.raises(AssertionError, match=r"49 byte\(s\) written outside .*first at offset 101 .*last at offset 149 "):
        run(all_ranges)


def test_write_before_the_view_is_caught():
    def before(view):
        write_right(view)
        b = guards.block_of(view)
        b.raw[b.start - 1] ^= 0x01
    with pytest.raises(AssertionError, match=r"first at offset -1 \(in the front guard band, 1 byte\(s\) before the start"):
        run(before, phase=16)


def test_unwritten_interior_byte_is_caught():
    """A writer that leaves one byte of its range unwritten: the byte holds
    the pattern, which differs between the two fills, so the exact compare
    fails under at least one of them (and it is the compare, not
    assert_untouched, that sees it)."""
    seen = []

    def skips_one(view):
        write_right(view)
        b = guards.block_of(view)
        view[60] = guards.pattern(len(b.raw), b.fill)[b.start + 60]  # as if never stored

    def body(fill):
        view = guards.guarded(TOTAL, fill=fill)
        skips_one(view)
        guards.assert_untouched(view, allowed())  # nothing outside: passes
        try:
            check(view)
        except AssertionError:
            seen.append(fill)
    guards.twice(body)
    assert seen, "an unwritten byte passed the exact compare under both fills"
    # and with one fill alone it can pass by luck: a value that equals the pattern
    lucky = guards.guarded(TOTAL, fill=0x00)
    write_right(lucky)
    lucky[60] = EXPECT[60]
    check(lucky)


def test_torch_cpu_tensors_work_alike():
    torch = pytest.importorskip("torch")
    v = guards.guarded(77, phase=3, fill=0xFF, device="cpu")
    assert v.data_ptr() % 256 == 3 and v.numel() == 77
    guards.assert_untouched(v, [])
    v[10:20] = 1
    guards.assert_untouched(v, [(10, 20)])
    with pytest.raises(AssertionError, match="first at offset 10 .*last at offset 19 "):
        guards.assert_untouched(v, [(0, 10), (20, 77)])
    guards.block_of(v).raw[0] ^= 0xFF
    with pytest.raises(AssertionError, match=r"offset -259 \(in the front guard band"):
        guards.assert_untouched(v, [(10, 20)])
