"""The remain table of the 20-job front bucket (core/pfsp_front.hpp pfsp_front_remain_table).

A node's remain — the sum of its unscheduled jobs' p rows, per machine — depends on its job
set and the instance only. The front kernels look it up: the 20-bit set is cut into groups
of bits, the table holds one row of packed u16 pairs per group pattern, and the remain is
the 32-bit sum of one row per group. Here the table from the CPU binding is summed exactly
like that (uint32 words, so a carry from a low half into a high one would show) and
compared with a direct row sum in numpy.
"""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

SEED = 7

# 20 x 5 / 10 / 20: the three machine buckets; 17 x 7: jobs and machines below the bucket
# (zero rows and zero halves). The top of the value range: up to 50 jobs the front layout
# takes an instance only if all its processing times sum below 65536, which no near_limit
# instance of two or more machines does (its times are 65535 // (jobs + machines - 1) each),
# so the shapes whose remain halves pass 32,768 are the bottleneck generator's, the front
# layout's own value-range instances (sum exactly 65535): 20 x 10 with machine 4 (a low half
# next to a non-zero high half) and 20 x 5 with machine 2 (the same in the 5-machine bucket)
SHAPES = ["20x5", "20x10", "20x20", "17x7", "bottleneck10", "bottleneck5"]
HIGH = {"bottleneck10": 4, "bottleneck5": 2}  # the machine whose full remain is 32,768 or more


@functools.lru_cache(maxsize=None)
def model_of(shape):
    if shape == "bottleneck10":
        return PfspModel(None, 1, p=tl.bottleneck(20, 10, 4, SEED))
    if shape == "bottleneck5":
        return PfspModel(None, 1, p=tl.bottleneck(20, 5, 2, SEED))
    jobs, machines = (int(x) for x in shape.split("x"))
    return PfspModel.synthetic(jobs, machines, seed=SEED, lb=1)


def bucket_of(machines):
    return 5 if machines <= 5 else 10 if machines <= 10 else 20


def table_of(model):
    t = np.asarray(ops.cpu().pfsp_front_remain_table(model.native))
    assert t.dtype == np.uint32 and t.ndim == 3
    return t


def group_sets(model, groups, bits):
    """Every set reachable as one group's pattern with the other groups empty or full, cut
    to the instance's jobs."""
    every = (1 << model.jobs) - 1
    out = []
    for g in range(groups):
        gm = ((1 << bits) - 1) << (bits * g)
        for pat in range(1 << bits):
            for others in (0, every & ~gm):
                out.append(((pat << (bits * g)) | others) & every)
    return np.asarray(out, dtype=np.uint32)


def lookup(table, sets):
    """The kernels' look-up: one row per group, added as uint32 words, then the halves."""
    groups, pats, hw = table.shape
    bits = pats.bit_length() - 1
    acc = np.zeros((len(sets), hw), dtype=np.uint32)
    for g in range(groups):
        acc += table[g, (sets >> np.uint32(bits * g)) & np.uint32(pats - 1)]
    return np.stack([acc & np.uint32(0xFFFF), acc >> np.uint32(16)], axis=2).reshape(len(sets), 2 * hw).astype(np.int64)


def direct(model, sets, width):
    p = np.zeros((model.jobs, width), dtype=np.int64)
    p[:, :model.machines] = np.asarray(model.native.p, dtype=np.int64).reshape(model.machines, model.jobs).T
    member = ((sets[:, None] >> np.arange(model.jobs, dtype=np.uint32)[None, :]) & 1).astype(np.int64)
    return member @ p


@pytest.mark.parametrize("shape", SHAPES)
def test_shape_and_padding(shape):
    m = model_of(shape)
    assert m.front_layout and m.jobs <= 20
    t = table_of(m)
    groups, pats, hw = t.shape
    bits = pats.bit_length() - 1
    assert pats == 1 << bits and groups * bits == 20
    assert hw == (bucket_of(m.machines) + 1) // 2
    assert not t[:, 0, :].any()  # the empty pattern of every group
    # jobs beyond the instance's add nothing: a pattern and the pattern cut to the jobs agree
    every = (1 << m.jobs) - 1
    for g in range(groups):
        for pat in range(pats):
            cut = ((pat << (bits * g)) & every) >> (bits * g)
            assert np.array_equal(t[g, pat], t[g, cut]), (g, pat)
    # machines beyond the instance's stay zero halves
    halves = np.stack([t & 0xFFFF, t >> 16], axis=3).reshape(groups, pats, 2 * hw)
    assert not halves[:, :, m.machines:].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_group_patterns_against_row_sums(shape):
    m = model_of(shape)
    t = table_of(m)
    sets = group_sets(m, t.shape[0], t.shape[1].bit_length() - 1)
    assert len(sets) == 2 * t.shape[0] * t.shape[1]
    assert np.array_equal(lookup(t, sets), direct(m, sets, 2 * t.shape[2]))


@pytest.mark.parametrize("shape", SHAPES)
def test_random_sets_against_row_sums(shape):
    m = model_of(shape)
    t = table_of(m)
    rng = np.random.default_rng(11)
    sets = rng.integers(0, 1 << m.jobs, size=2000, dtype=np.uint32)
    sets[:2] = (0, (1 << m.jobs) - 1)
    assert np.array_equal(lookup(t, sets), direct(m, sets, 2 * t.shape[2]))


def test_the_value_range_shapes_reach_the_high_bit():
    # what the two value-range shapes are here for: a low remain half of 32,768 or more next
    # to a high half that is not empty
    for shape, machine in HIGH.items():
        m = model_of(shape)
        assert machine % 2 == 0
        full = np.asarray([(1 << m.jobs) - 1], dtype=np.uint32)
        r = lookup(table_of(m), full)[0]
        assert r[machine] >= 32768 and r[machine + 1] > 0, (shape, r.tolist())


def test_layouts_without_a_table_are_refused():
    for model in (PfspModel(31, 1), PfspModel(None, 1, p=tl.near_limit(20, 10, SEED))):
        with pytest.raises(Exception):
            ops.cpu().pfsp_front_remain_table(model.native)
