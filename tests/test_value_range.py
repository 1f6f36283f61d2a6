"""The top of the PFSP kernels' 16-bit value range, on the host (no GPU).

The GPU kernels pack schedule times into 16 bits (front nodes, `front | remain << 16` LDS
words, u16 child fronts, packed u16x2 walks); the Taillard instances stay below 27,000.
The generators of utils/taillard.py build instances whose values reach [32768, 65536) and
instances just beyond what fits. Here: the generators keep their promises, the two guards
(front layout, `pfsp_fronts_fit_u16`) switch exactly where they should, and the host
oracle the GPU tests (test_gpu_value_range.py) compare against is itself consistent at
these values (front layout == permutation layout, solves invariant under scaling).

This module also holds the cases both files use.
"""
import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops, solve_cpu
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

INT_MAX = 2**31 - 1
SEED = 7

# (jobs, machines, parents): one shape per node bucket (20 / 50 / 100 / 200 / 500 jobs) and
# machine bucket (5 / 10 / 20)
SHAPES = [(12, 5, 200), (12, 10, 200), (24, 20, 100), (60, 20, 30), (100, 10, 12), (200, 10, 6), (500, 20, 3)]
OVER_SHAPES = [(12, 5), (24, 20), (60, 20), (100, 20)]
# (jobs, machines, bottleneck machine, q of the other rows); 20 x 2: padding machines
BOTTLENECKS = [(20, 5, 1, None), (20, 10, 4, None), (20, 20, 9, None), (50, 5, 2, None), (50, 10, 5, None),
               (50, 20, 10, 10), (20, 2, 0, None)]
SMALL_BOTTLENECKS = [(12, 5, 1), (13, 10, 4), (12, 20, 9)]
# whole solves by scaling: synthetic(12, machines, seed)
SOLVES = [(5, 105), (10, 110), (20, 120)]


def scale_to_limit(jobs, machines):
    """The largest k at which k * synthetic() still has (jobs + machines - 1) * max p < 65536."""
    return tl.U16_MAX // ((jobs + machines - 1) * 99)


def model_of(p, lb, best_known=None):
    return PfspModel(None, lb, p=p, best_known=best_known)


def staircase_max(p):
    """Completion time of the last job on the last machine in the identity order."""
    f = np.zeros(p.shape[0], dtype=np.int64)
    for j in range(p.shape[1]):
        t = 0
        for m in range(p.shape[0]):
            t = max(t, f[m]) + int(p[m, j])
            f[m] = t
    return int(f[-1])


# ---- the generators --------------------------------------------------------------------

@pytest.mark.parametrize("jobs,machines,_n", SHAPES)
def test_near_limit_promises(jobs, machines, _n):
    p = tl.near_limit(jobs, machines, SEED)
    c = tl.U16_MAX // (jobs + machines - 1)
    assert p.shape == (machines, jobs) and p.max() == c and p.min() >= c - 98
    assert np.array_equal(p.ravel()[1:], ((c - 99) + tl.synthetic(jobs, machines, SEED)).ravel()[1:])
    assert (jobs + machines - 1) * int(p.max()) < 65536 <= (jobs + machines - 1) * (int(p.max()) + 1)
    assert p.sum(axis=1).max() < 65536


@pytest.mark.parametrize("jobs,machines", OVER_SHAPES)
def test_over_limit_promises(jobs, machines):
    p = tl.over_limit(jobs, machines, SEED)
    inst = model_of(p, 2).native
    assert p.max() == tl.U16_MAX // jobs
    # what the table checks of the GPU engines look at fits 16 bits ...
    assert p.sum(axis=1).max() < 65536 and max(inst.lags) < 65536 and max(inst.min_tails) < 65536
    # ... a prefix completion time does not
    assert staircase_max(p) > 65535


def test_scaled_promises():
    base = tl.synthetic(12, 10, 110)
    for k in (1, 31, 55):
        assert np.array_equal(tl.scaled(12, 10, 110, k), k * base)
    assert scale_to_limit(12, 10) == 31 and (12 + 10 - 1) * 99 * 31 < 65536 <= (12 + 10 - 1) * 99 * 32
    with pytest.raises(ValueError):
        tl.scaled(12, 10, 110, 0)


@pytest.mark.parametrize("jobs,machines,b,q", BOTTLENECKS + [(j, m, b, None) for j, m, b in SMALL_BOTTLENECKS])
@pytest.mark.parametrize("total", [65535, 65536])
def test_bottleneck_promises(jobs, machines, b, q, total):
    p = tl.bottleneck(jobs, machines, b, SEED, total=total, q=q)
    syn = tl.synthetic(jobs, machines, SEED)
    assert p.shape == (machines, jobs) and int(p.sum()) == total
    others = np.delete(np.arange(machines), b)
    assert np.array_equal(p[others], syn[others] if q is None else 1 + (syn[others] - 1) % q)
    k = int(p[b, 1]) // int(syn[b, 1])
    assert np.array_equal(p[b, 1:], k * syn[b, 1:]) and p[b, 0] >= k * syn[b, 0]
    # the largest multiplier: one more would pass the total
    assert int(p[others].sum()) + (k + 1) * int(syn[b].sum()) > total


# ---- the guards ------------------------------------------------------------------------

@pytest.mark.parametrize("jobs,machines,b,q", BOTTLENECKS + [(j, m, b, None) for j, m, b in SMALL_BOTTLENECKS])
def test_front_layout_switches_at_a_total_of_65536(jobs, machines, b, q):
    for lb in (0, 1):
        assert model_of(tl.bottleneck(jobs, machines, b, SEED, total=65535, q=q), lb).front_layout
        assert not model_of(tl.bottleneck(jobs, machines, b, SEED, total=65536, q=q), lb).front_layout


def test_fronts_fit_u16_on_every_taillard_instance():
    C = ops.cpu()
    assert all(C.pfsp_fronts_fit_u16(C.PfspInstance.taillard(i)) for i in range(1, 121))


def test_fronts_fit_u16_switches_between_near_and_over_limit():
    C = ops.cpu()
    for jobs, machines, _ in SHAPES:
        assert C.pfsp_fronts_fit_u16(model_of(tl.near_limit(jobs, machines, SEED), 2).native), (jobs, machines)
        if jobs <= 200:
            k = scale_to_limit(jobs, machines)
            assert C.pfsp_fronts_fit_u16(model_of(tl.scaled(jobs, machines, SEED, k), 2).native)
    for jobs, machines in OVER_SHAPES:
        assert not C.pfsp_fronts_fit_u16(model_of(tl.over_limit(jobs, machines, SEED), 2).native), (jobs, machines)
    assert not C.pfsp_fronts_fit_u16(model_of(tl.scaled(12, 20, 120, 55), 2).native)
    # one step past near_limit: (jobs + machines - 1) * max p reaches 65536 and so does the total
    p = tl.near_limit(12, 5, SEED)
    p[0, 0] += 1
    assert not C.pfsp_fronts_fit_u16(model_of(p, 2).native)
    # a total below 65536 is enough whatever the largest time
    assert C.pfsp_fronts_fit_u16(model_of(tl.bottleneck(20, 10, 4, SEED), 2).native)
    assert not C.pfsp_fronts_fit_u16(model_of(tl.bottleneck(20, 10, 4, SEED, total=65536), 2).native)


# ---- the host oracle at these values ---------------------------------------------------

@pytest.mark.parametrize("jobs,machines,b,q", BOTTLENECKS)
def test_front_bounds_equal_permutation_bounds_at_65535(jobs, machines, b, q):
    model = model_of(tl.bottleneck(jobs, machines, b, SEED, q=q), 0)
    assert model.front_layout
    C = ops.cpu()
    rng = np.random.default_rng(11)
    depths = rng.integers(0, jobs, size=120)
    perms = np.stack([rng.permutation(jobs) for _ in range(120)])
    perm_nodes = nd.pfsp_pack(depths, perms, jobs)
    ref = model.child_bounds_cpu(perm_nodes)  # child order k = depth..N-1
    assert ref.max() > 32767
    got = np.asarray(C.pfsp_children_bounds(model.native, 0, model.to_engine_layout(perm_nodes)))  # ascending jobs
    off = 0
    for d, q_ in zip(depths, perms):
        kids = list(q_[d:])
        by_job = dict(zip(kids, ref[off:off + len(kids)]))
        assert list(got[off:off + len(kids)]) == [by_job[j] for j in sorted(kids)]
        off += len(kids)
    assert off == len(got)


@pytest.mark.parametrize("jobs,machines,b", SMALL_BOTTLENECKS)
@pytest.mark.parametrize("lb", [0, 1])
def test_front_trees_equal_permutation_trees_at_65535(jobs, machines, b, lb, monkeypatch):
    C = ops.cpu()
    native = model_of(tl.bottleneck(jobs, machines, b, SEED), lb).native
    opt = C.run_pfsp(native, lb, INT_MAX, threads=0)["best"]
    assert opt > 32767
    all_jobs = (1 << jobs) - 1
    got = {}
    for front in ("1", "0"):
        monkeypatch.setenv("TTS_FRONT", front)
        assert C.pfsp_front_layout(native, lb) == (front == "1")
        # a bottleneck machine makes LB1 tight: the root's bound is the optimum and the tree
        # from it is empty, so also the levels of the tree from 100 above it, as the sets of
        # unscheduled jobs of their nodes
        r = C.run_pfsp(native, lb, opt, threads=0)
        levels = []
        for depth in (1, 2, 3, 4):
            lv = C.pfsp_bfs_level(native, lb, opt + 100, depth)
            if front == "1":
                rest = [int(x) for x in nd.pfsp_front_unpack(lv, {5: 5, 10: 10, 20: 20}[machines])[1]]
            else:
                d, perms = nd.pfsp_unpack(lv, jobs)
                rest = [all_jobs & ~sum(1 << int(j) for j in q[:depth]) for q in perms]
            levels.append(sorted(rest))
        got[front] = (r["tree"], r["sol"], r["best"], levels)
    assert got["1"] == got["0"] and got["1"][2] == opt
    assert len(got["1"][3][3]) > 1000


@pytest.mark.parametrize("machines,seed", SOLVES)
@pytest.mark.parametrize("lb", [1, 2])
def test_solve_cpu_is_invariant_under_scaling(machines, seed, lb):
    base = model_of(tl.synthetic(12, machines, seed), lb)
    opt = solve_cpu(base, ub=0).best
    base.best_known = opt
    ref = solve_cpu(base, ub=1)
    assert ref.best == opt and ref.tree > 300
    for k in (scale_to_limit(12, machines), 55):
        r = solve_cpu(model_of(tl.scaled(12, machines, seed, k), lb, best_known=k * opt), ub=1)
        assert (r.tree, r.sol, r.best) == (ref.tree, ref.sol, k * opt), k
