"""The front kernel on 51-100-job nodes (128-bit job sets, TTS_FRONT_WIDE=1) against the
host: the bounds kernel, one iteration byte for byte through both instantiations, the
element-wise probe of whole solves in every iteration shape, the rank split, leaves and the
incumbent, the top of the u16 range, and the engine API. Every engine here is built with
max_parents <= 1 << 14 (a chunk's slot region is 51,200 nodes of up to 80 B)."""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import EngineOptions, PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl
from test_front_wide import SEED, SOLVES, deep_nodes, random_perm_nodes, root_lb1, solve_model

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
BP = 256              # parents per chunk (FrontGeom::BP)
SLOT = 2 * BP * 100   # chunk slot region of the 100-job bucket (FrontGeom::SLOT)
WINDOW = 1 << 14


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")


def bucket_of(machines):
    return 5 if machines <= 5 else 10 if machines <= 10 else 20


# ---- host expansion of 100-job front nodes -----------------------------------------------

def children_of(model, nodes, best):
    """One expansion of `nodes` in order: (surviving children, parents in order and jobs
    ascending; leaves evaluated; the lowest leaf bound or None)."""
    mb = bucket_of(model.machines)
    depth, rest, front = nd.pfsp_front_unpack(nodes, mb, jobs=model.jobs)
    p = np.zeros((model.jobs, mb), dtype=np.int64)
    p[:, :model.machines] = np.asarray(model.native.p, dtype=np.int64).reshape(model.machines, model.jobs).T
    flat = np.asarray(ops.cpu().pfsp_children_bounds(model.native, model.lb, np.ascontiguousarray(nodes, dtype=np.uint8)))
    out, at, leaves, low = [], 0, 0, None
    for i in range(len(nodes)):
        r = int(rest[i])
        jobs = [j for j in range(model.jobs) if (r >> j) & 1]
        lbs = flat[at:at + len(jobs)]
        at += len(jobs)
        if depth[i] + 1 == model.jobs:
            leaves += len(jobs)
            if len(lbs):
                low = int(lbs.min()) if low is None else min(low, int(lbs.min()))
            continue
        for j, lb in zip(jobs, lbs):
            if lb >= best:
                continue
            node = np.zeros(model.node_bytes, dtype=np.uint8)
            node[0] = depth[i] + 1
            c = r & ~(1 << j)
            node[16:32] = np.array([c & (2**64 - 1), c >> 64], dtype="<u8").view(np.uint8)
            t, f = 0, np.zeros(mb, dtype="<u2")
            for m in range(mb):
                t = max(t, 0 if depth[i] == 0 else int(front[i][m])) + int(p[j, m])
                f[m] = t
            node[32:32 + 2 * mb] = f.view(np.uint8)
            out.append(node)
    assert at == len(flat)
    kids = np.stack(out) if out else np.zeros((0, model.node_bytes), dtype=np.uint8)
    return kids, leaves, low


def replay_local(model, parents, best, steps):
    """Host replay of one chunk's local DFS (front_local): its stack left, the nodes it
    pushed, the leaves it evaluated."""
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
        if not (s + 1 < steps and len(stack) > 0 and len(stack) + BP * 100 <= SLOT):
            break
    return stack, pushed, leaves


# ---- the bounds kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("jobs", [51, 64, 65, 100])
@pytest.mark.parametrize("machines", [4, 9, 17])
def test_bounds_kernel(machines, jobs):
    m = PfspModel.synthetic(jobs, machines, 20 + machines, lb=1)
    assert m.front_layout
    perm_nodes, _, _ = random_perm_nodes(jobs, 200, 11)
    ref = m.child_bounds_cpu(perm_nodes)
    got = np.asarray(m.child_bounds_gpu(perm_nodes))
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("inst", [61, 71, 81])
def test_bounds_kernel_taillard(inst):
    m = PfspModel(inst, 0)
    perm_nodes, _, _ = random_perm_nodes(100, 200, 11)
    assert np.array_equal(np.asarray(m.child_bounds_gpu(perm_nodes)), m.child_bounds_cpu(perm_nodes))


# ---- one iteration, byte for byte ------------------------------------------------------------

def expand(model, parents, best, steps, production):
    H = ops.require_gpu(0)
    return H.pfsp_front_expand_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                                     np.ascontiguousarray(parents, dtype=np.uint8), int(best), steps=steps,
                                     production=production)


@functools.lru_cache(maxsize=None)
def generated(jobs, machines):
    """A generated instance, 300 random parents (every depth) and an incumbent that prunes
    about half of their children (the median child bound)."""
    m = PfspModel.synthetic(jobs, machines, seed=11, lb=1)
    perm_nodes, _, _ = random_perm_nodes(jobs, 300, 17, dmax=jobs - 2)
    parents = m.to_engine_layout(perm_nodes)
    best = int(np.median(np.asarray(ops.cpu().pfsp_children_bounds(m.native, m.lb, parents))))
    return m, parents, best


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


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("shape", [(100, 5), (65, 13), (100, 20)])
def test_one_level(shape, n):
    m, parents, best = generated(*shape)
    if n == 1:  # the root, no incumbent: every job survives from one lane
        r = one_iteration(m, m.root(), INT_MAX, 0)
        assert r["counts"] == [m.jobs]
    else:
        r = one_iteration(m, parents[:n], best, 0)
        assert len(r["counts"]) == -(-n // BP) and sum(r["counts"]) > 0


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("shape", [(100, 5), (65, 13), (100, 20)])
def test_local_dfs(shape, steps):
    m, parents, best = generated(*shape)
    r = one_iteration(m, parents[:257], best, steps)
    assert sum(r["counts"]) > 0
    if steps > 1:
        assert sum(r["inner"]) > 0  # (a later step did run)


def test_one_level_widest_chunk():
    # the widest chunk: 256 depth-2 parents with no incumbent write 256 x 98 = 25,088 children,
    # more than 13 bits count and close to 2^15
    m = PfspModel.synthetic(100, 9, 4, lb=1)
    kids, _, _ = children_of(m, m.root(), INT_MAX)
    lvl2, _, _ = children_of(m, kids[:3], INT_MAX)
    parents = lvl2[np.arange(256) % len(lvl2)]
    r = expand(m, parents, INT_MAX, 0, True)
    assert r["counts"] == [256 * 98]
    exp, _, _ = children_of(m, parents, INT_MAX)
    assert np.array_equal(r["children"], exp)


# ---- element-wise probe of whole solves --------------------------------------------------------

def probe(model, nodes, best, **kw):
    H = ops.require_gpu(0)
    kw.setdefault("max_parents", WINDOW)
    assert kw["max_parents"] <= WINDOW
    return H.pfsp_front_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                              np.ascontiguousarray(nodes, dtype=np.uint8), int(best), cap=1 << 23, **kw)


def check(r, kinds=()):
    assert r["records"] > 0
    assert r["checked"] == r["records"], "probe buffer too small"
    assert r["bad_job"] == 0 and r["bad_remain"] == 0 and r["bad_lb"] == 0, r
    for k in kinds:
        assert r["by_kind"][k] > 0, (k, r["by_kind"])


@functools.lru_cache(maxsize=None)
def solve_case(name):
    """(model, start nodes, incumbent, host tree and sol of the start nodes)."""
    model, nodes, best = solve_model(name)
    tree, sol, _ = model.drain(best, nodes)
    return model, nodes, best, tree, sol


@pytest.mark.parametrize("cfg,kinds", [
    ({}, ["child_parallel"]),
    ({"local_min": 0}, ["child_parallel", "one_level"]),
    ({"deep_levels": 4, "local_min": 0}, ["child_parallel", "thread_per_node"]),
    ({"fuse_max": 0}, ["one_level"]),
])
@pytest.mark.parametrize("name", sorted(SOLVES))
def test_front_probe_whole_solves(name, cfg, kinds):
    model, nodes, best, tree, sol = solve_case(name)
    assert model.front_layout
    r = probe(model, nodes, best, **cfg)
    print(name, cfg, r["by_kind"], r["tree"], r["sol"])
    # the iteration shapes a configuration asks for only appear in a tree wide enough to leave
    # the fused child-parallel chunks: ta081's 29,182 nodes (the others have 0 to 3,623)
    check(r, kinds if name == "ta081" else [])
    assert (r["tree"], r["sol"]) == (tree, sol)


def test_front_probe_local_dfs_records(monkeypatch):
    # a backlog from one parent on: the solve runs local DFS iterations
    model, nodes, best, tree, sol = solve_case("ta081")
    monkeypatch.setenv("TTS_LOCAL_MIN", "1")
    r = probe(model, nodes, best, max_parents=1 << 12, fuse_max=0)
    check(r, ["local_dfs"])
    assert (r["tree"], r["sol"]) == (tree, sol)


def test_front_probe_split_iteration():
    # two ranks of an in-graph split: both shares together are the whole tree
    model, nodes, best, tree, sol = solve_case("ta071")
    tot_t = tot_s = 0
    for rank in (0, 1):
        r = probe(model, nodes, best, split_rank=rank, split_world=2, split_min=len(nodes) + 1)
        check(r, ["split"])
        tot_t += r["tree"]
        tot_s += r["sol"]
    assert (tot_t, tot_s) == (tree, sol)


# ---- leaves and the incumbent --------------------------------------------------------------------

@pytest.mark.parametrize("k", [7, 10])
def test_leaves_and_the_incumbent(k):
    # 64 nodes of depth jobs - 7 (and jobs - 10) from +inf: the optimum below them is the
    # host's. Tree and sol from +inf depend on the order leaves are met in, so they are compared
    # from that optimum (tests/test_front_wide.py: 5,918 nodes and 255 leaves from jobs - 10)
    m = PfspModel.synthetic(100, 10, 14, lb=0)
    nodes = m.to_engine_layout(deep_nodes(100, 64, 21, k))
    _, hsol, opt = m.drain(INT_MAX, nodes)
    r = probe(m, nodes, INT_MAX)
    check(r)
    assert r["best"] == opt and r["sol"] > 0 and hsol > 0
    tree, sol, best = m.drain(opt, nodes)
    r = probe(m, nodes, opt)
    check(r)
    assert (r["tree"], r["sol"], r["best"]) == (tree, sol, best)
    if k == 10:
        assert (tree, sol) == (5918, 255)


def test_leaves_ta061():
    # ta061 has no finite tree above its deep nodes' optimum (tests/test_front_wide.py): from
    # +inf every evaluated bound equals the host's and the optimum found is the host's
    m = PfspModel(61, 0)
    nodes = m.to_engine_layout(deep_nodes(100, 64, 21, 9))
    _, hsol, opt = m.drain(INT_MAX, nodes)
    r = probe(m, nodes, INT_MAX)
    check(r)
    assert r["best"] == opt and r["sol"] > 0 and hsol > 0


# ---- near the top of the u16 range -------------------------------------------------------------

def test_near_limit():
    p = tl.near_limit(100, 10, SEED)
    assert int(p.sum()) > 65535 and (100 + 10 - 1) * int(p.max()) < 65536
    m = PfspModel(None, 0, p=p)
    assert m.front_layout
    perm_nodes, _, _ = random_perm_nodes(100, 200, 11)
    ref = m.child_bounds_cpu(perm_nodes)
    assert ref.max() > 60000  # the bounds do sit at the top of the range
    assert np.array_equal(np.asarray(m.child_bounds_gpu(perm_nodes)), ref)
    # one whole probed solve from +inf (every bound it evaluates, the optimum it finds), and
    # its counts from that optimum (from +inf they depend on the order the leaves are met in)
    nodes = m.to_engine_layout(deep_nodes(100, 64, 22))
    _, hsol, opt = m.drain(INT_MAX, nodes)
    r = probe(m, nodes, INT_MAX)
    check(r)
    assert r["best"] == opt and opt > 60000 and r["sol"] > 0 and hsol > 0
    tree, sol, best = m.drain(opt, nodes)
    r = probe(m, nodes, opt)
    check(r)
    assert (r["tree"], r["sol"], r["best"]) == (tree, sol, best)


# ---- engine API ------------------------------------------------------------------------------------

def test_engine_api(monkeypatch):
    # ta081: the one Taillard instance with a finite tree from the root at a small delta
    # (tests/test_front_wide.py; ta061's does not finish)
    from dist_gpu_accelerated_tree_search_amd.search import solve_engine

    _, make, delta, gold = SOLVES["ta081"]
    model = make()
    opts = EngineOptions(max_parents=WINDOW, ring_bytes=1 << 30)
    assert model.describe()["layout"] == "front" and model.node_bytes == 80
    eng = model.make_engine("gpu", 0, opts)
    r = solve_engine(model, eng, best=root_lb1(model.native) + delta)
    del eng
    assert (r.tree, r.sol) == gold
    # ta061 through the same API: its 64 deep nodes
    m61, nodes, best, tree, sol = solve_case("ta061")
    assert m61.describe()["layout"] == "front" and m61.node_bytes == 48
    eng = m61.make_engine("gpu", 0, opts)
    eng.begin(nodes, best)
    eng.run()
    st = eng.stats()
    del eng
    assert (st["tree"], st["sol"]) == (tree, sol)
    # without the opt-in the same calls build the permutation engine
    monkeypatch.delenv("TTS_FRONT_WIDE")
    perm = make()
    assert perm.describe()["layout"] == "perm" and perm.node_bytes == 112
    eng = perm.make_engine("gpu", 0, opts)
    r = solve_engine(perm, eng, best=root_lb1(perm.native) + delta)
    del eng
    assert (r.tree, r.sol) == gold
