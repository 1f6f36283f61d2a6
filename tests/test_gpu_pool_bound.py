"""engine.pool_bound on the device engines (csrc/hip/pool_bound_kernels.hpp): every kernel
family — front nodes of 20 to 500 jobs, permutation nodes under LB1 and under LB2 — against
the host twin on the same bytes, and the time-limited solves on a GPU.

Reference of every case: the device pool read back with pop(size()) after the call (the node
layouts are identical), bounded by the CPU engine's pool_bound; pools of up to a few thousand
nodes also by the oracle of tests/test_pool_bound.py, written from the processing times
alone. lower, nodes and every bin are compared exactly. Windows are small (max_parents <=
2^12) and rings a few MB, except where a size is the point of the test."""
import json
import subprocess
import sys

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd.models.nqueens import QueensModel
from dist_gpu_accelerated_tree_search_amd.models.pfsp import EngineOptions, PfspModel
from dist_gpu_accelerated_tree_search_amd.search import solve_gpu
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl
from test_front_wide import random_perm_nodes
from test_gpu_perm_engines import geom
from test_perm_engines import CASES
from test_pool_bound import GOLDEN_TA014, cpu_engine, heuristic_best, mixed_frontier, oracle, own_bounds, same

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
ORACLE_MAX = 3000  # pools up to this size are also bounded by the numpy / lb1 / lb2 oracle
KBLOCK, MAX_BLOCKS = 256, 4096  # pool_bound_kernels.hpp: threads per workgroup, the grid's cap


def gpu_engine(model, max_parents=256, ring_bytes=1 << 20, **kw):
    """A small engine: a window of 256 parents (one chunk of the front kernels), one chunk of
    the LB1 and four of the LB2 kernel for the permutation nodes above 50 jobs — their rings are
    8 windows of children of 112 to 1008 B each."""
    kw.setdefault("iters_first", 6)
    if model.kind == "pfsp" and not model.front_layout and model.jobs > 50:
        max_parents = min(max_parents, geom(model)[0] * (4 if model.lb == 2 else 1))
    return model.make_engine("gpu", 0, EngineOptions(max_parents=max_parents, ring_bytes=ring_bytes, **kw))


def check(model, eng, bins=64):
    """pool_bound of the engine's pool as it is, against the host twin (and the oracle) on the
    nodes read back; the call leaves size, counters and incumbent alone. Returns (result, nodes)."""
    n, cap, st = eng.size(), eng.best, eng.stats()
    got = eng.pool_bound(bins)
    st2 = eng.stats()
    assert (eng.size(), eng.best) == (n, cap)
    assert all(st2[k] == st[k] for k in ("tree", "sol", "parents", "iters", "launches", "best"))
    assert st2["device_nodes"] + st2["host_nodes"] == n
    nodes = eng.pop(n)
    assert len(nodes) == n and eng.size() == 0
    ref = cpu_engine(model)
    ref.begin(nodes, cap)
    same(got, ref.pool_bound(bins))
    if n <= ORACLE_MAX:
        same(got, oracle(model, nodes, cap, bins))
    return got, nodes


def spread_cap(model, nodes):
    """An incumbent at the median own bound of `nodes`: half the pool stale, the rest below."""
    own = sorted(own_bounds(model, nodes))
    return own[len(own) // 2]


# ---- one case per kernel instantiation family ---------------------------------------------------
# (name, Taillard instance, lb, TTS_FRONT_WIDE or None, layout); LB2 above 50 jobs under the incumbents of
# tests/test_perm_engines.py, everything else under the best-known makespan
LB2_BEST = {81: CASES["ta081lb2+162"][5][2], 101: CASES["ta101lb2+154"][5][2], 111: CASES["ta111lb2+32"][5][2],
            71: CASES["ta071lb2+8"][5][2], 91: CASES["ta091lb2+20"][5][2]}
FAMILIES = [
    ("front20x5", 1, 1, None, "front"), ("front20x10", 14, 0, None, "front"), ("front20x20", 21, 0, None, "front"),
    ("front50x5", 31, 1, None, "front"), ("front50x10", 41, 0, None, "front"), ("front50x20", 51, 1, None, "front"),
    ("front100x5", 61, 0, "2", "front"), ("front200x10", 91, 1, "2", "front"), ("front500x20", 111, 0, "2", "front"),
    ("front100x20", 81, 1, "1", "front"),
    ("perm100x5", 61, 1, None, "perm"), ("perm200x10", 91, 0, None, "perm"), ("perm500x20", 111, 1, None, "perm"),
    ("lb2_20x5", 1, 2, None, "perm"), ("lb2_20x10", 14, 2, None, "perm"), ("lb2_20x20", 21, 2, None, "perm"),
    ("lb2_50x5", 31, 2, None, "perm"), ("lb2_50x10", 41, 2, None, "perm"), ("lb2_50x20", 56, 2, None, "perm"),
    ("lb2_100x10", 71, 2, None, "perm"), ("lb2_100x20", 81, 2, None, "perm"), ("lb2_200x10", 91, 2, None, "perm"),
    ("lb2_200x20", 101, 2, None, "perm"), ("lb2_500x20", 111, 2, None, "perm"),
]
FIDS = [f[0] for f in FAMILIES]


def family(spec, monkeypatch):
    _, inst, lb, wide, layout = spec
    if wide:
        monkeypatch.setenv("TTS_FRONT_WIDE", wide)
    else:
        monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
    m = PfspModel(inst, lb)
    assert m.describe()["layout"] == layout
    best = LB2_BEST.get(inst, m.best_known) if lb == 2 else m.best_known
    return m, int(best)


@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_family_begin_alone(spec, monkeypatch):
    """Host frontiers of mixed depths (the root among them), then random nodes of every depth
    under an incumbent at their median bound and enough bins to tell every bound apart."""
    m, best = family(spec, monkeypatch)
    eng = gpu_engine(m)
    nodes = mixed_frontier(m, best, (1, 30, 300))
    eng.begin(nodes, best)
    got, back = check(m, eng)
    assert got["nodes"] == len(nodes) and got["lower"] <= best
    deep = m.to_engine_layout(random_perm_nodes(m.jobs, 700, 17)[0])
    cap = spread_cap(m, deep)
    eng.begin(deep, cap)
    got, _ = check(m, eng, bins=4096)  # past the bins a workgroup keeps in LDS
    assert 0 < got["hist"][0] < len(deep) and got["hist"][1:4095].any()


@pytest.mark.parametrize("spec", FAMILIES, ids=FIDS)
def test_family_after_a_launch(spec, monkeypatch):
    """begin + run(max_launches=1): nodes the device wrote, of several depths."""
    m, best = family(spec, monkeypatch)
    eng = gpu_engine(m)
    nodes, _, _, best = m.warmup(best, 25)
    eng.begin(nodes, int(best))
    eng.run(max_launches=1)
    got, back = check(m, eng)
    print(spec[0], got["nodes"], got["lower"], got["cap"])
    assert got["lower"] <= got["cap"] <= best


# ---- pool sizes ------------------------------------------------------------------------------------

def small_models():
    """The 32-byte layouts of the three kernel families: front nodes, LB1 and LB2 permutation nodes."""
    front = PfspModel(14, 0)
    perm1 = PfspModel(None, 1, p=tl.near_limit(20, 10, 3))  # (too large for the front layout)
    lb2 = PfspModel(14, 2)
    assert front.front_layout and not perm1.front_layout and {front.node_bytes, perm1.node_bytes, lb2.node_bytes} == {32}
    return {"front": (front, front.best_known), "perm_lb1": (perm1, heuristic_best(perm1)), "lb2": (lb2, lb2.best_known)}


@pytest.mark.parametrize("kind", ["front", "perm_lb1", "lb2"])
def test_pool_sizes_around_a_workgroup(kind):
    m, best = small_models()[kind]
    frontier = mixed_frontier(m, best, (1, 30, 300))
    assert len(frontier) >= 257
    eng = gpu_engine(m)
    for n in (1, 255, 256, 257):
        eng.begin(frontier[len(frontier) - n:], best)
        got, _ = check(m, eng)
        assert got["nodes"] == n


@pytest.mark.parametrize("kind", ["front", "perm_lb1", "lb2"])
def test_pool_past_one_grid(kind):
    """One node more than the grid covers in one trip: 4096 workgroups of 256 nodes (a thread
    per node), of 4 nodes (LB2: a wave per node). 32-byte nodes: about 32 MB at most."""
    m, best = small_models()[kind]
    n = MAX_BLOCKS * (4 if kind == "lb2" else KBLOCK) + 1
    frontier = mixed_frontier(m, best, (1, 30, 300))
    nodes = np.ascontiguousarray(np.tile(frontier, (n // len(frontier) + 1, 1))[:n])
    eng = gpu_engine(m, ring_bytes=1 << 27)  # half the ring holds the pool
    eng.begin(nodes, best)
    assert eng.stats()["host_nodes"] == 0 and eng.stats()["device_nodes"] == n
    got = eng.pool_bound()
    ref = cpu_engine(m)
    ref.begin(nodes, best)
    same(got, ref.pool_bound())
    small = oracle(m, frontier, best, 64)
    assert got["lower"] == small["lower"] and got["nodes"] == n
    # the tiled pool holds every frontier node n // len or n // len + 1 times
    k = n // len(frontier)
    assert all(k * int(a) <= int(b) <= (k + 1) * int(a) for a, b in zip(small["hist"], got["hist"]))


# ---- where the pool lies ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["front", "lb2"])
def test_pool_across_the_ring_end(kind):
    m, best = small_models()[kind]
    eng = gpu_engine(m)
    cap = eng.stats()["capacity"]
    frontier = mixed_frontier(m, best, (1, 30, 300))
    fill = cap // 2 - 1000
    nodes = np.ascontiguousarray(np.tile(frontier, (fill // len(frontier) + 1, 1))[:fill])
    eng.begin(nodes, best)
    bot = 0
    for _ in range(2):  # the oldest nodes popped, new ones pushed, until the pool wraps
        assert len(eng.pop(fill - 500)) == fill - 500
        bot += fill - 500
        eng.push(nodes[:fill - 500])
        assert eng.stats()["host_nodes"] == 0
    n = eng.size()
    assert n == fill and bot < cap < bot + n  # the pool lies across the ring's end
    got, back = check(m, eng)
    assert got["nodes"] == n


@pytest.mark.parametrize("kind", ["front", "perm_lb1", "lb2"])
def test_pool_partly_in_pinned_spill(kind):
    """More than half a small ring: the rest waits in pinned host blocks and is bounded by the
    host twin. The result equals that of the same nodes all on the device."""
    m, best = small_models()[kind]
    small = gpu_engine(m)
    cap = small.stats()["capacity"]
    n = cap // 2 + 6000  # (from 4096 spilled nodes on the host part runs on several threads)
    frontier = mixed_frontier(m, best, (1, 30, 300))
    nodes = np.ascontiguousarray(np.tile(frontier, (n // len(frontier) + 1, 1))[:n])
    small.begin(nodes, best)
    st = small.stats()
    assert st["host_nodes"] > 0 and st["device_nodes"] > 0 and st["host_nodes"] + st["device_nodes"] == n
    big = gpu_engine(m, ring_bytes=n * 4 * 32)
    big.begin(nodes, best)
    assert big.stats()["host_nodes"] == 0
    got = small.pool_bound(32)
    same(got, big.pool_bound(32))
    assert small.stats()["host_nodes"] == st["host_nodes"]
    check(m, small, bins=32)


# ---- the edge cases of the host file -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["front", "perm_lb1", "lb2"])
def test_stale_nodes_after_a_lower_incumbent(kind):
    m, best = small_models()[kind]
    nodes = mixed_frontier(m, best, (1, 30, 300))
    own = sorted(own_bounds(m, nodes))
    eng = gpu_engine(m)
    eng.begin(nodes, best)
    eng.best = own[len(own) // 2]  # some nodes sit exactly at the new incumbent: stale is >=
    want = oracle(m, nodes, own[len(own) // 2], 16)
    assert 0 < want["hist"][0] < len(nodes) and want["hist"][0] == sum(b >= own[len(own) // 2] for b in own)
    assert sum(b == own[len(own) // 2] for b in own) >= 1
    same(eng.pool_bound(16), want)
    eng.best = own[0]
    got, _ = check(m, eng, bins=2)
    assert got["lower"] == got["cap"] == own[0] and got["hist"][0] == len(nodes)


@pytest.mark.parametrize("kind", ["front", "perm_lb1", "lb2"])
def test_no_incumbent(kind):
    m, _ = small_models()[kind]
    nodes = mixed_frontier(m, INT_MAX, (1, 30, 120))
    eng = gpu_engine(m)
    eng.begin(nodes, INT_MAX)  # a -u 0 begin
    got, _ = check(m, eng, bins=8)
    assert got["cap"] == INT_MAX and got["hist"][7] == len(nodes) and got["lower"] == min(own_bounds(m, nodes))
    eng.begin(nodes[:0], 1500)
    got = eng.pool_bound()
    assert (got["lower"], got["cap"], got["nodes"]) == (1500, 1500, 0) and not got["hist"].any()
    for bins in (1, 0):
        with pytest.raises(ValueError):
            eng.pool_bound(bins)


def test_near_limit_values(monkeypatch):
    """The top of the 16-bit value range: front nodes of a near_limit instance, permutation
    nodes under LB2 of one, and LB1 permutation nodes of an over_limit instance (bounds past 65535)."""
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    m = PfspModel(None, 1, p=tl.near_limit(60, 10, 3))
    assert m.front_layout
    best = heuristic_best(m)
    nodes = mixed_frontier(m, best, (1, 30, 300))
    assert max(own_bounds(m, nodes)) > 60000
    eng = gpu_engine(m)
    eng.begin(nodes, best)
    check(m, eng)
    monkeypatch.delenv("TTS_FRONT_WIDE")
    for p, lb, over in ((tl.near_limit(20, 10, 3), 2, False), (tl.over_limit(100, 10, 3), 1, True)):
        m = PfspModel(None, lb, p=p)
        assert not m.front_layout
        best = heuristic_best(m)
        nodes = mixed_frontier(m, best, (1, 30, 300))
        deep = m.to_engine_layout(random_perm_nodes(m.jobs, 300, 5)[0])
        assert (max(own_bounds(m, deep)) > 65535) == over
        eng = gpu_engine(m)
        eng.begin(nodes, best)
        check(m, eng)
        eng.begin(deep, spread_cap(m, deep))
        check(m, eng, bins=4096)


@pytest.mark.parametrize("machines", [7, 13])
@pytest.mark.parametrize("lb", [0, 2])
def test_padded_machine_buckets(machines, lb):
    m = PfspModel.synthetic(18, machines, 5, lb=lb)
    best = heuristic_best(m)
    eng = gpu_engine(m)
    eng.begin(mixed_frontier(m, best), best)
    check(m, eng)
    deep = m.to_engine_layout(random_perm_nodes(m.jobs, 500, 9)[0])
    eng.begin(deep, spread_cap(m, deep))
    check(m, eng, bins=2048)
    eng.begin(m.root(), INT_MAX)  # the root's fronts are the minimum heads, the padding machines' the cheapest route
    check(m, eng)


@pytest.mark.parametrize("machines", [7, 13])
def test_padded_machine_buckets_permutation_lb1(machines, monkeypatch):
    """The LB1 kernel of the permutation nodes with padding machines (above 50 jobs, no front
    layout): frontiers, random nodes of every depth, and the root, whose padding machines
    carry the cheapest job's whole route as their head."""
    monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
    m = PfspModel.synthetic(60, machines, 5, lb=1)
    assert not m.front_layout and m.node_bytes == 112
    best = heuristic_best(m)
    eng = gpu_engine(m)
    eng.begin(mixed_frontier(m, best), best)
    check(m, eng)
    deep = m.to_engine_layout(random_perm_nodes(m.jobs, 500, 9)[0])
    eng.begin(deep, spread_cap(m, deep))
    check(m, eng, bins=4096)
    eng.begin(m.root(), INT_MAX)
    got, _ = check(m, eng)
    assert got["lower"] == own_bounds(m, m.root())[0]


@pytest.mark.parametrize("lb", [0, 2])
def test_two_streams_merge(lb):
    m = PfspModel(14, lb)
    eng = gpu_engine(m, streams=2)
    nodes, _, _, best = m.warmup(m.best_known, 25)
    eng.begin(nodes, int(best))
    eng.run(max_launches=1)
    got, back = check(m, eng, bins=32)
    print(lb, got["nodes"], got["lower"])


def test_nqueens_engine_has_no_node_bound():
    q = QueensModel(8)
    eng = q.make_engine("gpu", 0, EngineOptions(max_parents=256, ring_bytes=1 << 20))
    eng.begin(q.root(), 0)
    with pytest.raises(RuntimeError, match="no node bound"):
        eng.pool_bound()
    assert eng.size() == 1


# ---- the search is not disturbed -----------------------------------------------------------------------

@pytest.mark.parametrize("use_graphs", [True, False])
def test_bound_between_every_launch(use_graphs):
    m = PfspModel(14, 1)
    eng = gpu_engine(m, max_parents=1 << 12, ring_bytes=1 << 26, use_graphs=use_graphs)
    nodes, tree1, sol1, best = m.warmup(m.best_known, 25)
    eng.begin(nodes, int(best))
    lowers = [eng.pool_bound()["lower"]]
    while eng.size():
        eng.run(max_launches=1)
        pb = eng.pool_bound()
        assert pb["nodes"] == eng.size()
        lowers.append(pb["lower"])
    st = eng.stats()
    assert (tree1 + st["tree"], sol1 + st["sol"], st["best"]) == GOLDEN_TA014
    assert lowers == sorted(lowers) and lowers[-1] == 1377 and len(lowers) > 3
    assert pb["nodes"] == 0 and pb["cap"] == 1377


# ---- whole time-limited solves ---------------------------------------------------------------------------

def test_time_limited_solve_and_resume():
    m = PfspModel(21, 0)
    r = solve_gpu(m, time_limit=0.2, opts=EngineOptions(max_parents=1 << 12, ring_bytes=1 << 28))
    eng = r.extra["engine"]
    assert not r.complete and r.open_nodes == eng.size() > 0
    assert own_bounds(m, m.root())[0] <= r.lower_bound <= 2297 and 0.0 <= r.gap < 1.0
    eng.run(max_seconds=0.2)
    again = eng.pool_bound()
    print(r.open_nodes, r.lower_bound, again["nodes"], again["lower"])
    assert again["lower"] >= r.lower_bound and again["nodes"] == eng.size()


def test_generous_limit_is_the_golden_solve():
    r = solve_gpu(PfspModel(14, 1), time_limit=30, opts=EngineOptions(max_parents=1 << 12, ring_bytes=1 << 26))
    assert r.complete and (r.tree, r.sol, r.best) == GOLDEN_TA014
    assert r.lower_bound == 1377 and r.open_nodes == 0 and r.gap == 0.0 and "engine" not in r.extra


def test_cli_time_limit(tmp_path):
    out = tmp_path / "r.json"
    p = subprocess.run([sys.executable, "-m", "dist_gpu_accelerated_tree_search_amd", "pfsp", "-i", "56", "-l", "2",
                        "-D", "1", "-C", "0", "--time-limit", "2", "--max-parents", "4096", "--ring-gb", "1",
                        "--no-csv", "--json", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["complete"] is False and rec["open_nodes"] > 0
    assert rec["lower_bound"] <= PfspModel(56, 2).best_known and 0.0 <= rec["gap"] < 1.0
    lines = p.stdout.splitlines()
    at = next(i for i, x in enumerate(lines) if x.startswith("Time limit reached after "))
    assert lines[at].endswith(" s: exploration not completed.")
    assert lines[at + 1] == "Open nodes: %d" % rec["open_nodes"]
    assert lines[at + 2] == "Proven lower bound: %d" % rec["lower_bound"]
    assert lines[at + 3] == "Gap to best makespan: %.2f %%" % (100.0 * rec["gap"])
    assert any(x.startswith("Optimal makespan: ") for x in lines[:at])  # after the unchanged results block
