"""The front kernel on 101-500-job nodes (256- and 512-bit job sets, a u16 depth,
TTS_FRONT_WIDE=2) against the host: the bounds kernel, one iteration byte for byte through
both instantiations, the element-wise probe of whole solves, the rank split, leaves and the
incumbent, the top of the u16 range, and the engine API. The host side of every comparison
is the permutation-layout code or PfspFrontProblem::decompose (pfsp_front_expand), never the
device. Every engine here is built with max_parents <= 1 << 13 for 200 jobs and <= 1 << 12
for 500 jobs (a chunk's slot region is 102,400 nodes of up to 96 B / 256,000 of up to 128 B)."""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import EngineOptions, PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl
from test_front_wide import SEED, deep_nodes, random_perm_nodes, root_lb1
from test_front_xwide import XSOLVES, around_256, xsolve_model

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
BP = 256  # parents per chunk (FrontGeom::BP)


def window(jobs):
    return 1 << 13 if jobs <= 200 else 1 << 12


def slot(jobs):
    """Chunk slot region of the job bucket (FrontGeom::SLOT)."""
    return 2 * BP * (200 if jobs <= 200 else 500)


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")


# ---- host expansion ------------------------------------------------------------------------

def children_of(model, nodes, best):
    """One expansion of `nodes` in order on the host: (surviving children, parents in order
    and jobs ascending; leaves evaluated; the lowest leaf bound or None)."""
    return ops.cpu().pfsp_front_expand(model.native, model.lb, np.ascontiguousarray(nodes, dtype=np.uint8), int(best))


def replay_local(model, parents, best, steps):
    """Host replay of one chunk's local DFS (front_local): its stack left, the nodes it
    pushed, the leaves it evaluated."""
    nj = 200 if model.jobs <= 200 else 500
    stack = np.zeros((0, model.node_bytes), dtype=np.uint8)
    pushed = leaves = 0
    cur = parents
    for s in range(steps):
        if s > 0:
            if len(stack) == 0:
                break
            npop = min(len(stack), BP)
            cur, stack = stack[len(stack) - npop:], stack[:len(stack) - npop]
        kids, lf, _ = children_of(model, cur, best)
        stack = np.concatenate([stack, kids])
        pushed += len(kids)
        leaves += lf
        if not (s + 1 < steps and len(stack) > 0 and len(stack) + BP * nj <= slot(model.jobs)):
            break
    return stack, pushed, leaves


# ---- the bounds kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("jobs", [101, 129, 193, 200, 201, 257, 449, 500])
@pytest.mark.parametrize("machines", [4, 9, 17])
def test_bounds_kernel(machines, jobs):
    m = PfspModel.synthetic(jobs, machines, 20 + machines, lb=0)
    assert m.front_layout
    perm_nodes, _, _ = random_perm_nodes(jobs, 200, 11)
    ref = m.child_bounds_cpu(perm_nodes)
    got = np.asarray(m.child_bounds_gpu(perm_nodes))
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("inst", [91, 101, 111])
def test_bounds_kernel_taillard(inst):
    m = PfspModel(inst, 0)
    assert m.front_layout
    perm_nodes, _, _ = random_perm_nodes(m.jobs, 200, 11)
    assert np.array_equal(np.asarray(m.child_bounds_gpu(perm_nodes)), m.child_bounds_cpu(perm_nodes))


# ---- one iteration, byte for byte ------------------------------------------------------------

def expand(model, parents, best, steps, production):
    H = ops.require_gpu(0)
    assert parents.shape[1] == model.node_bytes
    return H.pfsp_front_expand_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                                     np.ascontiguousarray(parents, dtype=np.uint8), int(best), steps=steps,
                                     production=production)


def median_bound(m, parents):
    return int(np.median(np.asarray(ops.cpu().pfsp_children_bounds(m.native, m.lb, parents))))


@functools.lru_cache(maxsize=None)
def generated(jobs, machines):
    """A generated instance, 300 random parents (every depth) and an incumbent that prunes
    about half of their children (the median child bound)."""
    m = PfspModel.synthetic(jobs, machines, seed=11, lb=1)
    perm_nodes, _, _ = random_perm_nodes(jobs, 300, 17, dmax=jobs - 2)
    parents = m.to_engine_layout(perm_nodes)
    return m, parents, median_bound(m, parents)


@functools.lru_cache(maxsize=None)
def generated_deep(jobs, machines):
    """As generated(), the parents 2 to 12 levels above the leaves."""
    m = PfspModel.synthetic(jobs, machines, seed=11, lb=1)
    rng = np.random.default_rng(23)
    depths = rng.integers(jobs - 12, jobs - 1, size=300)
    perms = np.stack([rng.permutation(jobs) for _ in range(300)])
    parents = m.to_engine_layout(nd.pfsp_pack(depths, perms, jobs))
    return m, parents, median_bound(m, parents)


def one_iteration(model, parents, best, steps):
    inst = expand(model, parents, best, steps, False)
    prod = expand(model, parents, best, steps, True)
    for k in ("bp", "counts", "inner", "leaves", "best"):
        assert prod[k] == inst[k], k
    assert np.array_equal(prod["children"], inst["children"])
    r, bp = prod, prod["bp"]
    at = leaves = 0
    low = None
    assert len(r["counts"]) == -(-len(parents) // bp)
    for c, cnt in enumerate(r["counts"]):
        mine = parents[c * bp:(c + 1) * bp]
        got = r["children"][at:at + cnt]
        if steps <= 1:
            kids, lf, lo = children_of(model, mine, best)
            assert cnt == len(kids), (c, cnt, len(kids))
            assert np.array_equal(got, kids), c
            assert r["inner"][c] == 0
            if lo is not None:
                low = lo if low is None else min(low, lo)
        else:
            stack, pushed, lf = replay_local(model, mine, best, steps)
            assert cnt == len(stack), (c, cnt, len(stack))
            assert r["inner"][c] == pushed - len(stack)
            assert sorted(map(bytes, got)) == sorted(map(bytes, stack)), c
        at += cnt
        leaves += lf
    assert at == len(r["children"]) and r["leaves"] == leaves
    if steps <= 1:
        assert r["best"] == (min(best, low) if low is not None else best)
    return r


SHAPES = [(200, 5), (193, 9), (200, 20), (500, 5), (449, 9), (500, 20)]


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_level(shape, n):
    m, parents, best = generated(*shape)
    if n == 1:  # the root, no incumbent: every job survives from one lane
        r = one_iteration(m, m.root(), INT_MAX, 0)
        assert r["counts"] == [m.jobs]
    else:
        r = one_iteration(m, parents[:n], best, 0)
        assert len(r["counts"]) == -(-n // BP) and sum(r["counts"]) > 0


def test_one_level_widest_chunk():
    # one chunk whose survivor count passes 2^16: 256 depth-1 parents of a 500-job instance
    # with no incumbent write 256 x 499 = 127,744 children (17 bits of the combined scan)
    m = PfspModel.synthetic(500, 9, 4, lb=1)
    kids, _, _ = children_of(m, m.root(), INT_MAX)
    parents = kids[:256]
    exp, _, _ = children_of(m, parents, INT_MAX)
    assert len(exp) == 127744
    for production in (True, False):
        r = expand(m, parents, INT_MAX, 0, production)
        assert r["counts"] == [127744]
        assert np.array_equal(r["children"], exp)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_local_dfs(shape, steps):
    m, parents, best = generated_deep(*shape)
    r = one_iteration(m, parents[:257], best, steps)
    assert sum(r["counts"]) > 0
    if steps > 1:
        assert sum(r["inner"]) > 0  # (a later step did run)


@pytest.mark.parametrize("steps", [0, 2])
@pytest.mark.parametrize("jobs,machines", [(300, 9), (500, 20)])
def test_depths_and_jobs_around_256(jobs, machines, steps):
    # parents at depths 254 to 258 whose unscheduled jobs include 255 and 256: a depth or a
    # job id cut to 8 bits changes a child's bytes here
    m = PfspModel.synthetic(jobs, machines, 3, lb=1)
    perm_nodes, depths, _ = around_256(jobs, 5, (254, 255, 256, 257, 258))
    parents = m.to_engine_layout(perm_nodes)
    r = one_iteration(m, parents, median_bound(m, parents), steps)
    assert sum(r["counts"]) > 0
    if steps == 0:
        # without an incumbent every child is written: those of the depth-258 parents, and
        # those appending jobs 255 and 256 (the other of the two is then still unscheduled)
        r = one_iteration(m, parents, INT_MAX, 0)
        d, rest, _ = nd.pfsp_front_unpack(r["children"], 10 if machines <= 10 else 20, jobs=jobs)
        assert r["counts"] == [sum(jobs - int(x) for x in depths)] and d.max() == 259
        assert {1, 2} <= {(int(x) >> 255) & 3 for x in rest}


@pytest.mark.parametrize("jobs,machines", [(200, 9), (500, 17)])
def test_leaves_in_the_window(jobs, machines):
    # parents at depth jobs - 1 mixed into the window: their single child is a leaf, counted
    # and offered to the incumbent, never written
    m = PfspModel.synthetic(jobs, machines, 6, lb=1)
    rng = np.random.default_rng(31)
    depths = rng.integers(jobs - 6, jobs, size=300)
    depths[::7] = jobs - 1
    perms = np.stack([rng.permutation(jobs) for _ in range(300)])
    parents = m.to_engine_layout(nd.pfsp_pack(depths, perms, jobs))
    _, lf, low = children_of(m, parents, INT_MAX)
    assert lf >= 43 and low is not None
    r = one_iteration(m, parents, INT_MAX, 0)  # every leaf improves on +inf
    assert r["leaves"] == lf and r["best"] == low
    r = one_iteration(m, parents, low + 1, 0)
    assert r["leaves"] == lf and r["best"] == low
    r = one_iteration(m, parents, low - 5, 0)  # no leaf improves: the incumbent stays
    assert r["leaves"] == lf and r["best"] == low - 5


# ---- element-wise probe of whole solves --------------------------------------------------------

def probe(model, nodes, best, **kw):
    H = ops.require_gpu(0)
    kw.setdefault("max_parents", window(model.jobs))
    kw.setdefault("cap", 1 << 20)
    assert kw["max_parents"] <= window(model.jobs)
    return H.pfsp_front_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                              np.ascontiguousarray(nodes, dtype=np.uint8), int(best), **kw)


def check(r, kinds=()):
    assert r["records"] > 0
    assert r["checked"] == r["records"], "probe buffer too small"
    assert r["bad_job"] == 0 and r["bad_remain"] == 0 and r["bad_lb"] == 0, r
    for k in kinds:
        assert r["by_kind"][k] > 0, (k, r["by_kind"])


@functools.lru_cache(maxsize=None)
def solve_case(name):
    """(model, start nodes, incumbent, the tree and sol the host computed with the
    permutation layout: tests/test_front_xwide.py XSOLVES)."""
    model, nodes, best = xsolve_model(name)
    assert model.front_layout
    tree, sol = XSOLVES[name][3]
    return model, nodes, best, tree, sol


PROBED = ["ta101+150", "ta111+24", "syn193x20+24", "ta111k9", "ta101k7"]


# (every solve here starts from the root or from 64 nodes, a narrow window: fused
# child-parallel chunks, or one level per kernel without them)
@pytest.mark.parametrize("cfg,kinds", [
    ({}, ["child_parallel"]),
    ({"local_min": 0}, ["child_parallel"]),
    ({"deep_levels": 4, "local_min": 0}, ["child_parallel"]),
    ({"fuse_max": 0}, ["one_level"]),
])
@pytest.mark.parametrize("name", PROBED)
def test_front_probe_whole_solves(name, cfg, kinds):
    model, nodes, best, tree, sol = solve_case(name)
    r = probe(model, nodes, best, **cfg)
    print(name, cfg, r["by_kind"], r["tree"], r["sol"])
    check(r, kinds)
    assert (r["tree"], r["sol"], r["best"]) == (tree, sol, best)


def test_front_probe_local_dfs_records(monkeypatch):
    # a backlog from one parent on: the solve runs local DFS iterations
    model, nodes, best, tree, sol = solve_case("ta101+150")
    monkeypatch.setenv("TTS_LOCAL_MIN", "1")
    r = probe(model, nodes, best, max_parents=1 << 12, fuse_max=0)
    check(r, ["local_dfs"])
    assert (r["tree"], r["sol"]) == (tree, sol)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["ta101+150", "ta101k7"])
def test_front_probe_split_iteration(name, world):
    # the ranks of an in-graph split: the shares together are the whole tree, the leaves and
    # nodes of the replicated iterations counted on rank 0 only
    model, nodes, best, tree, sol = solve_case(name)
    # (from the root: the split once the replicated pool holds two nodes; the 64 deep nodes
    # are split in the first iteration)
    split_min = 2 if name == "ta101+150" else len(nodes)
    tot_t = tot_s = 0
    for rank in range(world):
        r = probe(model, nodes, best, split_rank=rank, split_world=world, split_min=split_min)
        check(r, ["split"])
        tot_t += r["tree"]
        tot_s += r["sol"]
    assert (tot_t, tot_s) == (tree, sol)


# ---- near the top of the u16 range -------------------------------------------------------------

def test_near_limit():
    p = tl.near_limit(500, 20, SEED)
    assert int(p.sum()) > 65535 and (500 + 20 - 1) * int(p.max()) < 65536
    m = PfspModel(None, 0, p=p)
    assert m.front_layout and m.node_bytes == 128
    perm_nodes, _, _ = random_perm_nodes(500, 200, 11)
    ref = m.child_bounds_cpu(perm_nodes)
    assert ref.max() > 32768  # (45,570: the bounds need the 16th bit; times of 28 to 126)
    assert np.array_equal(np.asarray(m.child_bounds_gpu(perm_nodes)), ref)
    # one whole probed solve from +inf (every bound it evaluates, the optimum it finds), and
    # its counts from that optimum (from +inf they depend on the order the leaves are met in)
    nodes = m.to_engine_layout(deep_nodes(500, 64, 22))
    _, hsol, opt = m.drain(INT_MAX, nodes)
    r = probe(m, nodes, INT_MAX)
    check(r)
    assert r["best"] == opt and opt > 32768 and r["sol"] > 0 and hsol > 0
    tree, sol, best = m.drain(opt, nodes)
    r = probe(m, nodes, opt)
    check(r)
    assert (r["tree"], r["sol"], r["best"]) == (tree, sol, best)


def test_optimum_from_infinity():
    # 257 x 13, 64 nodes 9 levels above the leaves, from +inf: counts depend on the order the
    # leaves are met in, the optimum does not (15,510 on the host, tests/test_front_xwide.py)
    m = PfspModel.synthetic(257, 13, 5, lb=0)
    nodes = m.to_engine_layout(deep_nodes(257, 64, 21, 9))
    r = probe(m, nodes, INT_MAX, cap=1 << 21)  # (1.2 M child bounds from +inf)
    check(r)
    assert r["best"] == 15510 and r["sol"] > 0


# ---- engine API ------------------------------------------------------------------------------------

def test_engine_api_200():
    from dist_gpu_accelerated_tree_search_amd.search import solve_engine

    _, make, delta, gold = XSOLVES["ta101+160"]
    model = make()
    assert model.describe()["layout"] == "front" and model.node_bytes == 96
    eng = model.make_engine("gpu", 0, EngineOptions(max_parents=1 << 13, ring_bytes=1 << 30))
    assert eng.node_bytes == 96
    r = solve_engine(model, eng, best=root_lb1(model.native) + delta)
    del eng
    assert (r.tree, r.sol) == gold


def test_engine_api_500():
    model, nodes, best = xsolve_model("ta111k10")
    assert model.describe()["layout"] == "front" and model.node_bytes == 128
    eng = model.make_engine("gpu", 0, EngineOptions(max_parents=1 << 12, ring_bytes=1 << 30))
    assert eng.node_bytes == 128
    eng.begin(nodes, best)
    eng.run()
    st = eng.stats()
    del eng
    assert (st["tree"], st["sol"]) == XSOLVES["ta111k10"][3]


def test_engines_outside_the_layout(monkeypatch):
    # an instance over the range rule builds a permutation engine, and so does a 200-job
    # instance under TTS_FRONT_WIDE=1 (engines built, not run)
    p = tl.over_limit(500, 20, SEED)
    m = PfspModel(None, 0, p=p)
    assert m.describe()["layout"] == "perm" and m.node_bytes == 1008
    eng = m.make_engine("gpu", 0, EngineOptions(max_parents=1 << 10, ring_bytes=1 << 28))
    assert eng.node_bytes == 1008
    del eng
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    m = PfspModel(101, 0)
    assert m.describe()["layout"] == "perm" and m.node_bytes == 208
    eng = m.make_engine("gpu", 0, EngineOptions(max_parents=1 << 10, ring_bytes=1 << 28))
    assert eng.node_bytes == 208
    del eng
