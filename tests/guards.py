"""Guard bands, poisoned outputs and displaced arenas for the write-set tests.

A kernel that stores one byte too many, rounds a tail up to its 16-byte chunk
or reaches into a neighbour's range normally goes unseen: the neighbour's own
writer overwrites the byte later, or nobody looks past the arena's end. Here
every output buffer is a view into a larger block that holds a
position-dependent pattern everywhere, guard bands in front and behind
included, and after the call every byte outside the ranges the call owns must
still hold it (assert_untouched). Run under two complementary fills (twice),
a byte the call never wrote differs from its expected value under at least
one of them, so an output can no longer be right by what it held before.

Works on numpy arrays (device=None: the CPU self-test, tests/test_guards.py)
and on torch tensors alike. A plain helper module, not a conftest.
"""
import numpy as np

ALIGN = 256
FILLS = (0x00, 0xFF)  # complementary: the two patterns differ in every bit of every byte


def _tile(fill: int) -> np.ndarray:
    """One period of the pattern: byte i of a block holds
    ((131 i + 17) & 0xFF) ^ fill; 131 is odd, so the period is 256 bytes and
    every 16-byte chunk differs from its neighbours."""
    i = np.arange(256, dtype=np.int64)
    return (((131 * i + 17) & 0xFF) ^ (fill & 0xFF)).astype(np.uint8)


def pattern(nbytes: int, fill: int) -> np.ndarray:
    """The pattern of a whole block of nbytes bytes (host copy)."""
    return np.resize(_tile(fill), nbytes)


class Block:
    """A guarded allocation: `raw` is the whole patterned block (its byte 0 on
    a 256-byte boundary), `view` the nbytes bytes from front + phase on."""

    def __init__(self, raw, view, nbytes, phase, fill, front, back):
        self.raw, self.view = raw, view
        self.nbytes, self.phase, self.fill, self.front, self.back = nbytes, phase, fill, front, back
        self.start = front + phase  # of the view, in raw
        # the view's address, also of an empty one (torch reports 0 for it): an
        # empty output is still passed as a pointer into guarded memory, never NULL
        self.address = _address(raw) + self.start

    def host(self) -> np.ndarray:
        """The whole block's bytes now."""
        return self.raw if isinstance(self.raw, np.ndarray) else self.raw.cpu().numpy()

    def bytes(self) -> np.ndarray:
        """The view's bytes now (host copy)."""
        return self.host()[self.start:self.start + self.nbytes].copy()


class _View(np.ndarray):
    """numpy view that can carry its Block (plain ndarrays take no attribute)."""
    _guard = None


def _address(a) -> int:
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def guarded(nbytes, phase=0, fill=FILLS[0], front=256, back=256, device=None):
    """A view of `nbytes` bytes that starts front + phase bytes into a block
    of front + phase + nbytes + back bytes on a 256-byte boundary. The whole
    block holds the pattern seeded by `fill`. device=None: numpy; else the
    torch device. block_of(view) returns the Block; assert_untouched takes
    either."""
    nbytes, phase = int(nbytes), int(phase)
    if nbytes < 0 or phase < 0 or front < 0 or back < 0:
        raise ValueError("negative size")
    size = front + phase + nbytes + back
    padded = (size + 255) // 256 * 256  # whole pattern periods
    if device is None:
        store = np.empty(padded + ALIGN, np.uint8)
        skew = -_address(store) % ALIGN
        raw = store[skew:skew + padded]
        raw.reshape(-1, 256)[:] = _tile(fill)
        raw = raw[:size]
        view = raw[front + phase:front + phase + nbytes].view(_View)
    else:
        import torch
        store = torch.empty(padded + ALIGN, dtype=torch.uint8, device=device)
        skew = -_address(store) % ALIGN
        raw = store[skew:skew + padded]
        raw.view(-1, 256).copy_(torch.from_numpy(_tile(fill)).to(device))
        raw = raw[:size]
        view = raw[front + phase:front + phase + nbytes]
    assert _address(raw) % ALIGN == 0
    view._guard = Block(raw, view, nbytes, phase, fill, front, back)
    return view


def address(view) -> int:
    """The address to pass for a guarded view (0 for None)."""
    return 0 if view is None else block_of(view).address


def block_of(view) -> Block:
    b = view if isinstance(view, Block) else getattr(view, "_guard", None)
    if b is None:
        raise TypeError("not a guarded view (slices of one do not carry the block)")
    return b


def _merge(allowed, nbytes):
    """Sorted, merged half-open ranges; every one must lie inside the view."""
    rs = []
    for a, b in allowed:
        a, b = int(a), int(b)
        if a < 0 or b > nbytes or a > b:
            raise ValueError(f"allowed range [{a}, {b}) is not inside the view [0, {nbytes})")
        if a < b:
            rs.append((a, b))
    rs.sort()
    out = []
    for a, b in rs:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def _adjoins(off, ranges, nbytes):
    """Which allowed range an offending offset (relative to the view) adjoins."""
    where = "in the front guard band" if off < 0 else ("in the back guard band" if off >= nbytes else "in the view")
    if not ranges:
        return f"{where}; no range is allowed"
    best = min(ranges, key=lambda r: 0 if r[0] <= off < r[1] else min(abs(off - r[0]), abs(off - (r[1] - 1))))
    a, b = best
    if off >= b:
        return f"{where}, {off - b + 1} byte(s) past the end of allowed range [{a}, {b})"
    return f"{where}, {a - off} byte(s) before the start of allowed range [{a}, {b})"


def assert_untouched(block, allowed):
    """Every byte of the whole block outside the union of `allowed` (half-open
    byte ranges relative to the view) still holds its pattern; both guard
    bands count as outside. On failure: the first and last offending offsets
    (relative to the view) and the allowed range each adjoins."""
    b = block_of(block)
    now = b.host()
    ranges = _merge(allowed, b.nbytes)
    bad = now != pattern(len(now), b.fill)
    if ranges:
        edge = np.zeros(len(now) + 1, np.int32)
        r = np.asarray(ranges, np.int64) + b.start
        np.add.at(edge, r[:, 0], 1)
        np.add.at(edge, r[:, 1], -1)
        bad &= np.cumsum(edge[:-1]) == 0
    idx = np.flatnonzero(bad)
    if len(idx):
        first, last = int(idx[0]) - b.start, int(idx[-1]) - b.start
        raise AssertionError(
            f"{len(idx)} byte(s) written outside the allowed ranges of a {b.nbytes}-byte view "
            f"(phase {b.phase}, fill {b.fill:#04x}): first at offset {first} "
            f"({_adjoins(first, ranges, b.nbytes)}), last at offset {last} "
            f"({_adjoins(last, ranges, b.nbytes)})")


def twice(fn):
    """Run the test body fn(fill) under the two complementary fills. A byte
    the code under test never writes holds a different value in the two runs,
    so it cannot equal the expected one in both."""
    return [fn(fill) for fill in FILLS]
