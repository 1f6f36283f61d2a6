"""The front kernel's remain look-up, packed bound chain and leaf handling on the GPU.

In the 20-job bucket a parent's remain comes from a table staged in LDS (one row per group
of set bits, FrontRemTab), the pair chain reads the parent's fronts and remain + tail as
packed halves, and leaf parents are handled after the bound loop. The chunks here hold, for
every bit group and each of its non-empty patterns, one node with the other groups empty
and one with them full, so every table row is read next to empty and to full neighbours;
single-bit sets are leaf parents, so every chunk mixes them with shallower nodes in the
same wave. One iteration through `pfsp_front_expand_probe`, production and instrumented
instantiation, against the host (tests/test_gpu_front_prod.py, test_gpu_front_emit.py).
"""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from test_front_remain_table import SHAPES, model_of, table_of
from test_gpu_front_emit import child_bounds, children_of, layout, leaf_parents, pack, ptable
from test_gpu_front_prod import check_against_host, same_bytes

pytestmark = pytest.mark.gpu

# The incumbent of a shape is this quantile of the host's child bounds: the median where it
# lets 20 % to 80 % of the children survive (asserted below), else the quantile that does.
QUANTILE = {}


def node_of(model, rest):
    """The node whose unscheduled set is `rest`: depth = jobs - popcount, the front of the
    scheduled jobs in ascending order."""
    p = ptable(model)
    _, _, _, bucket = layout(model)
    fr = np.zeros(bucket, dtype=np.int64)
    for j in range(model.jobs):
        if (rest >> j) & 1:
            continue
        t = 0
        for m in range(bucket):
            t = max(t, fr[m]) + p[j, m]
            fr[m] = t
    return model.jobs - bin(rest).count("1"), rest, fr


@functools.lru_cache(maxsize=None)
def chunk(shape):
    """(model, nodes of the group patterns, incumbent, the half with the other groups empty)."""
    m = model_of(shape)
    groups, pats, _ = table_of(m).shape
    bits = pats.bit_length() - 1
    every = (1 << m.jobs) - 1
    d, r, f, deep = [], [], [], []
    for g in range(groups):
        gm = ((1 << bits) - 1) << (bits * g)
        for pat in range(1, pats):
            for others in (0, every & ~gm):
                rest = ((pat << (bits * g)) | others) & every
                if rest == 0:
                    continue
                dd, rr, ff = node_of(m, rest)
                d.append(dd)
                r.append(rr)
                f.append(ff)
                deep.append(others == 0)
    nodes = pack(m, np.asarray(d), np.asarray(r, dtype=np.uint64), np.asarray(f))
    assert 64 < len(nodes) <= 256
    depth = np.asarray(d)
    assert (depth == m.jobs - 1).any() and (depth < m.jobs - 1).any()  # leaf parents among the others
    # the incumbent: a quantile of the bounds of the children that can survive (not leaves)
    lbs = np.concatenate([b for (_, b), dd in zip(child_bounds(m, nodes), d) if dd + 1 < m.jobs])
    q = QUANTILE.get(shape, 0.5)
    best = int(np.quantile(lbs, q, method="lower"))
    frac = float((lbs < best).mean())
    print(f"{shape}: {len(nodes)} nodes, {len(lbs)} children, incumbent {best} (quantile {q}): {frac:.2f} survive")
    assert 0.2 <= frac <= 0.8, (shape, q, frac)
    return m, nodes, best, np.asarray(deep)


@pytest.mark.parametrize("steps", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_group_pattern_chunk(shape, steps):
    # steps 0: one level per kernel; 1: local step 0, every remain from the table; 3: staged
    # nodes (carried remains) mixed with pops from the slot region
    m, nodes, best, _ = chunk(shape)
    r = same_bytes(m, nodes, best, steps)
    assert sum(r["counts"]) > 0 and r["leaves"] > 0
    check_against_host(m, nodes, best, steps, r)


@pytest.mark.parametrize("shape", SHAPES)
def test_bound_records(shape):
    # every bound the instrumented kernel evaluates, with the parent's remain as the kernel
    # holds it, against the host. The probe that records them runs whole solves, so it gets
    # the half of the chunk whose other groups are empty: subtrees of at most 4 jobs
    m, nodes, best, deep = chunk(shape)
    start = nodes[deep]
    # (the incumbent no leaf of these subtrees improves: the explored tree then does not
    # depend on the order in which the leaves are met)
    best = m.drain(best, start)[2]
    H = ops.require_gpu(0)
    r = H.pfsp_front_probe(m.jobs, m.machines, list(m.native.p), m.lb, np.ascontiguousarray(start, dtype=np.uint8),
                           best, cap=1 << 16)
    assert r["records"] > 0 and r["checked"] == r["records"]
    assert r["bad_job"] == 0 and r["bad_remain"] == 0 and r["bad_lb"] == 0, r
    tree, sol, low = m.drain(best, start)
    assert (r["tree"], r["sol"], r["best"]) == (tree, sol, low)


@pytest.mark.parametrize("steps", [0, 1, 3])
@pytest.mark.parametrize("shape", ["20x10", "20x20"])
def test_leaf_parents_among_shallower(shape, steps):
    # leaf parents (depth jobs - 1, random prefixes) interleaved lane by lane with the
    # chunk's shallower nodes, under an incumbent above some leaf makespans and below others
    m, nodes, _, _ = chunk(shape)
    leaves = leaf_parents(m, 60)
    spans = np.concatenate([b for _, b in child_bounds(m, leaves)])
    best = int(np.median(spans))
    assert (spans < best).any() and (spans >= best).any()
    mixed = np.zeros((120, m.node_bytes), dtype=np.uint8)
    mixed[0::2] = leaves
    mixed[1::2] = nodes[:60]
    r = same_bytes(m, mixed, best, steps)
    _, host_leaves, low, _ = children_of(m, mixed, best)
    assert r["leaves"] >= host_leaves >= 60
    if steps <= 1:
        assert r["leaves"] == host_leaves and r["best"] == min(best, low) == int(spans.min())
    check_against_host(m, mixed, best, steps, r)
