"""The production instantiation of the front kernel against the instrumented one.

`pfsp_front_kernel` is compiled twice: the instrumented instantiation holds the probe
hooks (stamps, bound records) and the dynamic local DFS, the production one — what every
engine launch without a probe runs — holds none of them. `pfsp_front_expand_probe` sets no
probe pointer, so one iteration must write the same bytes through either: the children of
every chunk, the per-chunk counts, the inner-node counts, the leaves and the incumbent.
Both are also checked against the host's expansion (tests/test_gpu_front_emit.py).
"""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from test_gpu_front_emit import BP, check_one_step, child_bounds, children_of, level, model_of, replay_local

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1


def expand(model, parents, best, steps, production):
    H = ops.require_gpu(0)
    return H.pfsp_front_expand_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                                     np.ascontiguousarray(parents, dtype=np.uint8), int(best), steps=steps,
                                     production=production)


def same_bytes(model, parents, best, steps):
    """One iteration through both instantiations: identical in every field."""
    inst = expand(model, parents, best, steps, False)
    prod = expand(model, parents, best, steps, True)
    print(f"{len(parents)} parents, steps {steps}: counts {prod['counts']} leaves {prod['leaves']} best {prod['best']}")
    assert prod["bp"] == inst["bp"]
    assert prod["counts"] == inst["counts"]
    assert prod["inner"] == inst["inner"]
    assert prod["leaves"] == inst["leaves"]
    assert prod["best"] == inst["best"]
    assert prod["children"].shape == inst["children"].shape
    assert np.array_equal(prod["children"], inst["children"])
    return prod


def check_against_host(model, parents, best, steps, r):
    """The production result against the host: in order for one step, as the stack each
    chunk leaves (a multiset) for several."""
    bp = r["bp"]
    slot = 2 * BP * (20 if model.jobs <= 20 else 50)
    at = leaves = 0
    low = None
    assert len(r["counts"]) == -(-len(parents) // bp)
    for c, cnt in enumerate(r["counts"]):
        mine = parents[c * bp:(c + 1) * bp]
        got = r["children"][at:at + cnt]
        if steps <= 1:
            kids, lf, lo, _ = children_of(model, mine, best)
            assert cnt == len(kids), (c, cnt, len(kids))
            assert np.array_equal(got, kids), c
            assert r["inner"][c] == 0
            if lo is not None:
                low = lo if low is None else min(low, lo)
        else:
            stack, pushed, lf = replay_local(model, mine, best, steps, slot)
            assert cnt == len(stack), (c, cnt, len(stack))
            assert r["inner"][c] == pushed - len(stack)
            assert sorted(map(bytes, got)) == sorted(map(bytes, stack)), c
        at += cnt
        leaves += lf
    assert at == len(r["children"])
    assert r["leaves"] == leaves
    if steps <= 1:
        assert r["best"] == (min(best, low) if low is not None else best)


# ---- one level per kernel: one lane, two waves, two chunks ------------------------------

@pytest.mark.parametrize("n", [1, 65, 257])
def test_one_level(n):
    m = model_of(14)
    best = m.best_known
    parents = m.root() if n == 1 else level(14, 10, best)[3000:3000 + n]
    best = INT_MAX if n == 1 else best
    r = same_bytes(m, parents, best, 0)
    assert len(r["counts"]) == -(-n // BP) and sum(r["counts"]) > 0
    check_against_host(m, parents, best, 0, r)


# ---- local DFS, one step and three -------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("n", [65, 257])
def test_local_dfs(n, steps):
    m = model_of(14)
    best = m.best_known
    parents = level(14, 10, best)[2000:2000 + n]
    r = same_bytes(m, parents, best, steps)
    assert sum(r["counts"]) > 0
    if steps > 1:
        assert sum(r["inner"]) > 0  # (a later step did run)
    check_against_host(m, parents, best, steps, r)


def test_local_dfs_reaches_the_leaves():
    # from depth 17 the steps count leaves (and must not move the optimum)
    m = model_of(14)
    best = m.best_known
    parents = level(14, 17, best)[2000:2257]  # (a slice whose subtrees survive down to depth 19)
    r = same_bytes(m, parents, best, 3)
    assert r["leaves"] > 0 and r["best"] == best
    check_against_host(m, parents, best, 3, r)


# ---- every machine and job bucket, on small generated instances -------------------------

@functools.lru_cache(maxsize=None)
def generated(jobs, machines):
    """A generated instance, ~300 parents of one of its levels and an incumbent that prunes
    about half of their children (the median child bound)."""
    m = PfspModel.synthetic(jobs, machines, seed=11, lb=1)
    lv = ops.cpu().pfsp_bfs_level(m.native, m.lb, INT_MAX, 3 if jobs <= 20 else 2)
    parents = lv[:300]
    best = int(np.median(np.concatenate([lbs for _, lbs in child_bounds(m, parents)])))
    return m, parents, best


@pytest.mark.parametrize("steps", [0, 1, 3])
@pytest.mark.parametrize("jobs", [12, 24])
@pytest.mark.parametrize("machines", [4, 8, 15])
def test_buckets(machines, jobs, steps):
    # machine buckets 5 / 10 / 20 (padded machines in each), job buckets 20 / 50
    m, parents, best = generated(jobs, machines)
    assert 256 < len(parents) <= 300
    r = same_bytes(m, parents, best, steps)
    assert sum(r["counts"]) > 0
    check_against_host(m, parents, best, steps, r)


def test_host_check_is_the_emit_tests():
    # the instrumented default of the probe still passes the emit tests' own check
    m = model_of(14)
    check_one_step(m, level(14, 10, m.best_known)[3000:3257], m.best_known, 0)
