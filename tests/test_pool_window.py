"""The 32-bit window arithmetic of pool_begin against the 64-bit form it replaced.

Every workgroup of every search kernel deals its iteration's parent window over chunks
before its first bound (csrc/hip/pool_device.hpp pool_begin): parents per chunk of an even
spread, clamped to the chunk size, and the number of chunks. The kernels do this in 32-bit
arithmetic (csrc/core/pool_window.hpp pool_deal32); `pool_deal(..., wide=True)` is the
64-bit form. The two must agree on every window the engines can form: B up to
max_parents (2^19 for the PFSP engines), spread over the grid, over the fixed 1024 chunks
of an armed split, or over max_chunks, in chunks of at most BPF / BPF_CP / BP parents.
"""
import itertools
import random

import pytest

from dist_gpu_accelerated_tree_search_amd import ops

BP = 256  # FrontGeom::BP
# grids: GRID_WGS x 256 CUs for the kernels' 4 / 5 / 6 workgroups per CU, the probes' small
# ones, and an engine whose window is narrower than the device
GRIDS = [1, 2, 3, 7, 255, 256, 1024, 1280, 1536, 2048]
# spreads pool_begin uses besides the grid: min(1024, max_chunks) while a split is armed
SPREADS = sorted(set(GRIDS) | {1, 4, 64, 1024, 2048})
CAPS = [1, 12, 32, 256, 448]  # BPF, BPF_CP, BP (a one-parent cap and the N-Queens chunk too)


def windows():
    b = {0, 1, 2, 11, 12, 13, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1 << 19, (1 << 19) - 1, (1 << 19) + 1}
    for g in GRIDS:
        for k in (1, 12, 32, BP):
            b |= {g * k - 1, g * k, g * k + 1}
    return sorted(x for x in b if x >= 0)


def test_32_bit_form_matches_64_bit_form_on_the_kernel_windows():
    C = ops.cpu()
    n = 0
    for B, spread, cap in itertools.product(windows(), SPREADS, CAPS):
        narrow = C.pool_deal(B, spread, cap)
        wide = C.pool_deal(B, spread, cap, wide=True)
        assert narrow == wide, (B, spread, cap, narrow, wide)
        per, bp, nchunks = narrow
        # what pool_begin relies on: chunks of 1..cap parents that cover the window exactly once
        assert 1 <= bp <= cap
        assert (nchunks - 1) * bp < B <= nchunks * bp if B else nchunks == 0
        assert per == -(-B // spread)
        n += 1
    assert n > 5000


def test_random_windows():
    C = ops.cpu()
    rng = random.Random(20)
    for _ in range(20000):
        B = rng.randrange(0, 1 << rng.choice([4, 9, 13, 19, 20, 24, 31]))
        spread = rng.randrange(1, 1 << rng.choice([1, 8, 11, 12]))
        cap = rng.choice(CAPS + [rng.randrange(1, 4096)])
        assert C.pool_deal(B, spread, cap) == C.pool_deal(B, spread, cap, wide=True), (B, spread, cap)


def test_largest_window_does_not_wrap():
    # the rounding-up must not go through B + spread - 1 (it would wrap past 2^32 here)
    C = ops.cpu()
    top = (1 << 31) - 1
    for B in (top, top - 1, top - 255, 1 << 30):
        for spread in (1, 2, 1280, 2048, 1 << 20, top):
            for cap in (1, BP, 1 << 20, top):
                assert C.pool_deal(B, spread, cap) == C.pool_deal(B, spread, cap, wide=True), (B, spread, cap)


def test_window_above_31_bits_is_refused():
    C = ops.cpu()
    with pytest.raises(ValueError):
        C.pool_deal(1 << 31, 1280, BP)
    assert C.pool_deal(1 << 31, 1280, BP, wide=True)[2] == (1 << 31) // BP
