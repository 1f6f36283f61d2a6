"""engine.pool_bound on the host engines and the time-limited solves built on it: what an
unfinished PFSP search has proved (csrc/core/engine_api.hpp PoolBound).

The reference is an oracle written here from the processing times alone: permutation nodes
through ops.cpu().lb1 / lb2(..., INT_MAX), front nodes decoded with numpy from their byte
layout (utils/nodes.py) and bounded by the machine-bound chain over front + remain + minimum
tail. Every node's bound is checked, not only the smallest: lower, nodes and every bin of the
histogram must agree. tests/test_gpu_pool_bound.py reuses the oracle for the device engines."""
import json
import subprocess
import sys

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.nqueens import QueensModel
from dist_gpu_accelerated_tree_search_amd.models.pfsp import EngineOptions, PfspModel
from dist_gpu_accelerated_tree_search_amd.search import SolveResult, solve_engine
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import report
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

INT_MAX = 2**31 - 1
GOLDEN_TA014 = (2573652, 2648, 1377)  # tree, sol, best of ta014 -u 1 (LB1 / LB1_d)


# ---- the oracle ------------------------------------------------------------------------------

def machine_bucket(machines):
    return 5 if machines <= 5 else 10 if machines <= 10 else 20


def p_matrix(model):
    return np.asarray(model.native.p, dtype=np.int64).reshape(model.machines, model.jobs)


def min_tails(p):
    """min over the jobs of the work after machine m (c_bound_simple.c fill_min_heads_tails)."""
    after = np.cumsum(p[::-1], axis=0)[::-1] - p  # [m, j]: sum of p[k, j], k > m
    return after.min(axis=1)


def chain(front, remain, tails):
    run = front[0] + remain[0]
    lb = run + tails[0]
    for m in range(1, len(front)):
        run = max(run, front[m] + remain[m])
        lb = max(lb, run + tails[m])
    return int(lb)


def own_bounds(model, nodes):
    """The own bound of every node of `nodes` (engine layout), from p alone."""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint8)
    if len(nodes) == 0:
        return []
    if not model.front_layout:
        C = ops.cpu()
        depths, perms = nd.pfsp_unpack(nodes, model.jobs)
        if model.lb == 2:
            return [int(C.lb2(model.native, q.tolist(), int(d), INT_MAX)) for d, q in zip(depths, perms)]
        return [int(C.lb1(model.native, q.tolist(), int(d))) for d, q in zip(depths, perms)]
    p = p_matrix(model)
    M = model.machines
    tails = min_tails(p)
    _, rest, fronts = nd.pfsp_front_unpack(nodes, machine_bucket(M), jobs=model.jobs)
    out = []
    for r, f in zip(rest, fronts):
        r = int(r)
        jobs = [j for j in range(model.jobs) if (r >> j) & 1]
        remain = p[:, jobs].sum(axis=1) if jobs else np.zeros(M, dtype=np.int64)
        out.append(chain([int(x) for x in f[:M]], [int(x) for x in remain], [int(x) for x in tails]))
    return out


def oracle(model, nodes, cap, bins):
    """{"lower", "cap", "nodes", "hist"} of a pool holding `nodes` under the incumbent cap."""
    hist = np.zeros(bins, dtype=np.uint64)
    lower = cap
    for own in own_bounds(model, nodes):
        b = min(own, cap)
        hist[min(cap - b, bins - 1)] += 1
        lower = min(lower, b)
    return {"lower": int(lower), "cap": int(cap), "nodes": int(hist.sum()), "hist": hist}


def same(got, want):
    assert (got["lower"], got["cap"], got["nodes"]) == (want["lower"], want["cap"], want["nodes"]), (got, want)
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == want["hist"].shape
    assert np.array_equal(got["hist"], want["hist"]), (got["hist"], want["hist"])
    assert int(got["hist"].sum()) == got["nodes"]


def mixed_frontier(model, best, targets=(1, 30, 300)):
    """Frontiers of the host warm-up at several targets: the root and nodes of several depths."""
    return np.ascontiguousarray(np.concatenate([model.warmup(best, t)[0] for t in targets]))


def heuristic_best(model):
    """An incumbent for instances without a best-known makespan: a heuristic schedule's
    makespan plus 2 %, so that the tree under it is not pruned at the root."""
    return int(ops.cpu().pfsp_neh(model.native, 200000) * 1.02) + 1


def cpu_engine(model, batch=64, threads=1):
    return model.make_engine("cpu", opts=EngineOptions(cpu_batch=batch, cpu_threads=threads))


def check_engine(model, eng, nodes, best, bins_list=(64,)):
    eng.begin(nodes, int(best))
    for bins in bins_list:
        same(eng.pool_bound(bins), oracle(model, nodes, int(best), bins))
    got = eng.pool_bound()
    assert len(got["hist"]) == 64  # the default


# ---- layouts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("inst,lb", [(14, 0), (14, 1), (14, 2), (1, 1), (21, 0), (21, 2), (31, 1), (41, 0), (51, 1),
                                     (31, 2), (56, 2)])
def test_taillard_layouts(inst, lb):
    """20- and 50-job front layouts for 5 / 10 / 20 machines, and LB2's permutation nodes."""
    m = PfspModel(inst, lb)
    assert m.front_layout == (lb != 2)
    nodes = mixed_frontier(m, m.best_known, (1, 30, 200) if lb != 2 else (1, 30, 120))
    depths = set(nodes[:, 0].tolist())
    assert len(depths) >= 3  # mixed depths, the root among them
    check_engine(m, cpu_engine(m), nodes, m.best_known, (64, 2, 5000))


@pytest.mark.parametrize("jobs,machines,level", [(64, 5, 1), (65, 10, 1), (100, 20, 1), (128, 5, 2), (129, 10, 2),
                                                 (200, 20, 2), (256, 5, 2), (257, 10, 2), (500, 20, 2)])
@pytest.mark.parametrize("lb", [0, 1])
def test_wide_front_layouts(jobs, machines, level, lb, monkeypatch):
    """Front nodes of 51-500 jobs (TTS_FRONT_WIDE), job counts on both sides of a word boundary."""
    monkeypatch.setenv("TTS_FRONT_WIDE", str(level))
    m = PfspModel.synthetic(jobs, machines, 11, lb=lb)
    assert m.front_layout
    best = heuristic_best(m)
    nodes = mixed_frontier(m, best, (1, 20, 2 * jobs + 40))
    assert len(nodes) > jobs
    check_engine(m, cpu_engine(m), nodes, best, (64, 3))


@pytest.mark.parametrize("inst,lb", [(61, 1), (61, 0), (91, 1), (111, 1), (61, 2)])
def test_permutation_layouts(inst, lb, monkeypatch):
    """Permutation nodes of 100 / 200 / 500 jobs (the default above 50 jobs), LB1 and LB2."""
    monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
    m = PfspModel(inst, lb)
    assert not m.front_layout
    nodes = mixed_frontier(m, m.best_known, (1, 20, m.jobs + 60))
    check_engine(m, cpu_engine(m), nodes, m.best_known, (64, 2))


@pytest.mark.parametrize("machines", [7, 13])
@pytest.mark.parametrize("lb", [0, 1, 2])
def test_padded_machine_buckets(machines, lb):
    """7 and 13 machines run in the 10- and 20-machine buckets: the padding machines change no bound."""
    m = PfspModel.synthetic(18, machines, 5, lb=lb)
    assert m.front_layout == (lb != 2)
    best = heuristic_best(m)
    nodes = mixed_frontier(m, best)
    check_engine(m, cpu_engine(m), nodes, best, (64, 2, 4096))


@pytest.mark.parametrize("machines", [7, 13])
def test_padded_machine_buckets_permutation_lb1(machines, monkeypatch):
    """Above 50 jobs (no front layout) LB1 runs on permutation nodes: the root included,
    whose padding machines carry the cheapest job's whole route as their head."""
    monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
    m = PfspModel.synthetic(60, machines, 5, lb=1)
    assert not m.front_layout and m.node_bytes == 112
    best = heuristic_best(m)
    check_engine(m, cpu_engine(m), mixed_frontier(m, best), best, (64, 4096))
    check_engine(m, cpu_engine(m), m.root(), INT_MAX)


def test_near_limit_values(monkeypatch):
    """Instances at the top of the 16-bit value range: the sums are 32-bit. Front nodes of a
    near_limit instance (bounds just below 65536), permutation nodes of a near_limit one, and
    an over_limit instance on permutation LB1 nodes, whose bounds pass 65535."""
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    m = PfspModel(None, 1, p=tl.near_limit(60, 10, 3))
    assert m.front_layout
    best = heuristic_best(m)
    nodes = mixed_frontier(m, best, (1, 30, 200))
    assert max(own_bounds(m, nodes)) > 60000
    check_engine(m, cpu_engine(m), nodes, best)
    monkeypatch.delenv("TTS_FRONT_WIDE")
    for p, lb, over in ((tl.near_limit(20, 10, 3), 1, False), (tl.near_limit(20, 10, 3), 2, False),
                        (tl.over_limit(100, 10, 3), 1, True)):
        m = PfspModel(None, lb, p=p)
        assert not m.front_layout
        best = heuristic_best(m)
        nodes = mixed_frontier(m, best, (1, 30, 200))
        assert (max(own_bounds(m, nodes)) > 65535) == over
        check_engine(m, cpu_engine(m), nodes, best)


# ---- cap and bins ----------------------------------------------------------------------------

@pytest.mark.parametrize("lb", [0, 1, 2])
def test_stale_nodes_after_a_lower_incumbent(lb):
    m = PfspModel(14, lb)
    nodes = mixed_frontier(m, m.best_known)
    own = sorted(own_bounds(m, nodes))
    cap = own[len(own) // 2]  # the median bound: about half the pool is stale, some nodes sit exactly at cap
    eng = cpu_engine(m)
    eng.begin(nodes, m.best_known)
    eng.best = cap
    want = oracle(m, nodes, cap, 16)
    assert 0 < want["hist"][0] < len(nodes) and want["hist"][0] == sum(b >= cap for b in own)
    same(eng.pool_bound(16), want)
    eng.best = own[0]  # everything stale: lower == cap
    got = eng.pool_bound(4)
    same(got, oracle(m, nodes, own[0], 4))
    assert got["lower"] == got["cap"] == own[0] and got["hist"][0] == len(nodes)


@pytest.mark.parametrize("lb", [1, 2])
def test_no_incumbent(lb):
    """cap == INT_MAX (-u 0 before the first leaf): everything in the last bin, lower still exact."""
    m = PfspModel(14, lb)
    nodes = mixed_frontier(m, INT_MAX, (1, 30, 100))
    eng = cpu_engine(m)
    eng.begin(nodes, INT_MAX)
    got = eng.pool_bound(8)
    same(got, oracle(m, nodes, INT_MAX, 8))
    assert got["cap"] == INT_MAX and got["hist"][7] == len(nodes) and got["lower"] == min(own_bounds(m, nodes))


def test_bins_and_empty_pool():
    m = PfspModel(14, 1)
    eng = cpu_engine(m)
    eng.begin(m.root()[:0], 1377)
    got = eng.pool_bound()
    assert (got["lower"], got["cap"], got["nodes"]) == (1377, 1377, 0) and not got["hist"].any()
    eng.begin(m.root(), 1377)
    for bins in (1, 0, -3):
        with pytest.raises(ValueError):
            eng.pool_bound(bins)
    wide = eng.pool_bound(100000)  # far more bins than the bound range
    same(wide, oracle(m, m.root(), 1377, 100000))
    assert wide["hist"][1377 - wide["lower"]] == 1


@pytest.mark.parametrize("lb", [0, 2])
def test_host_threads_agree(lb):
    """Pools from 4096 nodes on are shared out over the host engine's threads."""
    m = PfspModel(14, lb)
    frontier = mixed_frontier(m, m.best_known)
    nodes = np.ascontiguousarray(np.tile(frontier, (5000 // len(frontier) + 1, 1))[:5000])
    one, four = cpu_engine(m, threads=1), cpu_engine(m, threads=4)
    one.begin(nodes, m.best_known - 20)
    four.begin(nodes, m.best_known - 20)
    same(four.pool_bound(32), one.pool_bound(32))
    assert one.pool_bound(32)["nodes"] == 5000 and one.pool_bound(32)["hist"][0] > 0


# ---- the pool is left alone ------------------------------------------------------------------

@pytest.mark.parametrize("lb", [0, 1])
def test_pool_unchanged_and_solve_continues(lb):
    m = PfspModel(14, lb)
    eng = cpu_engine(m, batch=4096)
    nodes, tree1, sol1, best = m.warmup(m.best_known, 25)
    eng.begin(nodes, best)
    eng.run(max_launches=5)
    before = (eng.size(), eng.stats(), eng.best)
    for bins in (64, 2):
        eng.pool_bound(bins)
    st = eng.stats()
    assert (eng.size(), eng.best) == (before[0], before[2])
    assert all(st[k] == before[1][k] for k in ("tree", "sol", "parents", "iters", "launches", "best", "device_nodes"))
    lowers = []
    while eng.size():
        eng.run(max_launches=50)
        lowers.append(eng.pool_bound()["lower"])
    st = eng.stats()
    assert (tree1 + st["tree"], sol1 + st["sol"], st["best"]) == GOLDEN_TA014
    assert lowers == sorted(lowers) and lowers[-1] == 1377  # LB1: a child's bound is never below its parent's


@pytest.mark.parametrize("lb", [0, 2])
def test_multi_engine_equals_single(lb):
    """Two CPU sub-engines as one (streams=2): the merged result is the single engine's on the same nodes."""
    m = PfspModel(14, lb)
    nodes = mixed_frontier(m, m.best_known)
    multi = m.make_engine("cpu", opts=EngineOptions(cpu_batch=16, cpu_threads=1, streams=2))
    multi.begin(nodes, m.best_known)
    same(multi.pool_bound(32), oracle(m, nodes, m.best_known, 32))
    multi.run(max_launches=3)  # the sub-engines share the pool out and lower their incumbents apart
    if lb == 0:
        multi.best = 1400 if multi.best > 1400 else multi.best
    n, cap = multi.size(), multi.best
    got = multi.pool_bound(32)
    assert (multi.size(), multi.best) == (n, cap)
    rest = multi.pop(n)
    assert len(rest) == n and multi.size() == 0
    same(got, oracle(m, rest, cap, 32))
    single = cpu_engine(m)
    single.begin(rest, cap)
    same(got, single.pool_bound(32))


def test_hybrid_engine_merges_both_sides():
    m = PfspModel(14, 1)
    nodes = mixed_frontier(m, m.best_known)
    a, b = cpu_engine(m), cpu_engine(m)
    hyb = m.make_hybrid(a, "cpu", 1)
    hyb.begin(nodes, m.best_known)
    hyb.run(max_launches=2)
    n, cap = hyb.size(), hyb.best
    got = hyb.pool_bound(16)
    assert (hyb.size(), hyb.best) == (n, cap) and got["nodes"] == n
    same(got, oracle(m, hyb.pop(n), cap, 16))
    del b


def test_nqueens_engine_has_no_node_bound():
    q = QueensModel(8)
    eng = q.make_engine("cpu")
    eng.begin(q.root(), 0)
    with pytest.raises(RuntimeError, match="no node bound"):
        eng.pool_bound()
    assert eng.size() == 1


# ---- time-limited solves -----------------------------------------------------------------------

def test_time_limited_solve_is_incomplete_and_resumes():
    """ta021 LB1_d explores 2.6e11 nodes: no host finishes it in 0.05 s."""
    m = PfspModel(21, 0)
    eng = cpu_engine(m, batch=512)
    r = solve_engine(m, eng, time_limit=0.05)
    assert not r.complete and r.open_nodes == eng.size() > 0
    root = own_bounds(m, m.root())[0]
    assert root <= r.lower_bound <= 2297 and r.best == 2297
    assert r.gap == (r.best - r.lower_bound) / r.best and 0.0 <= r.gap < 1.0
    pb = r.extra["pool_bound"]
    assert pb["lower"] == r.lower_bound and pb["nodes"] == r.open_nodes and pb["cap"] == 2297
    lowers = [r.lower_bound]
    for _ in range(3):
        eng.run(max_launches=20)
        lowers.append(eng.pool_bound()["lower"])
    assert lowers == sorted(lowers)  # LB1 only: a child's LB1 is never below its parent's
    with pytest.raises(ValueError):
        solve_engine(m, eng, time_limit=0.0)


@pytest.mark.parametrize("lb", [0, 2])
def test_generous_limit_is_a_complete_solve(lb):
    m = PfspModel.synthetic(10, 5, 3, lb=lb)
    best = heuristic_best(m)
    eng = cpu_engine(m, batch=256)
    plain = solve_engine(m, eng, best=best)
    timed = solve_engine(m, eng, best=best, time_limit=60.0)
    assert plain.complete and timed.complete and timed.open_nodes == 0 and eng.size() == 0
    assert (timed.best, timed.tree, timed.sol) == (plain.best, plain.tree, plain.sol) and plain.tree > 0
    assert timed.lower_bound == timed.best == plain.lower_bound and timed.gap == plain.gap == 0.0
    assert "pool_bound" not in timed.extra


def test_ranks_stopped_early_claim_no_bound():
    """The distributed paths have no pool bound: a run that its time box stopped is not
    complete and proves nothing (lower_bound and gap None); a finished one has gap 0."""
    from dist_gpu_accelerated_tree_search_amd.parallel.launch import spawn_local
    from dist_gpu_accelerated_tree_search_amd.parallel.workers import solve_rank

    for session in (True, False):
        spec = {"problem": "pfsp", "inst": 56, "lb": 2, "backend": "cpu", "session": session,
                "dist": {"time_limit_s": 0.2}}
        r = spawn_local(1, solve_rank, (spec,), timeout=300)[0]
        assert r["extra"]["complete"] is False and r["complete"] is False
        assert r["lower_bound"] is None and r["gap"] is None and r["best"] == 3679
    spec = {"problem": "pfsp", "inst": 14, "lb": 0, "backend": "cpu", "dist": {"max_rounds": 1}}
    r = spawn_local(1, solve_rank, (spec,), timeout=300)[0]
    assert r["extra"]["complete"] is False and r["complete"] is False and r["lower_bound"] is None and r["gap"] is None
    spec = {"problem": "pfsp", "inst": 14, "lb": 0, "backend": "cpu", "session": True}
    r = spawn_local(1, solve_rank, (spec,), timeout=300)[0]
    assert (r["tree"], r["sol"], r["best"]) == GOLDEN_TA014
    assert r["complete"] is True and r["lower_bound"] == 1377 and r["gap"] == 0.0


def test_solve_result_defaults():
    r = SolveResult(best=100, tree=1, sol=1, elapsed=1.0)
    assert r.complete and r.lower_bound == 100 and r.open_nodes == 0 and r.gap == 0.0
    r = SolveResult(best=INT_MAX, tree=1, sol=0, elapsed=1.0, complete=False, lower_bound=90, open_nodes=5)
    assert r.gap is None
    r = SolveResult(best=100, tree=1, sol=0, elapsed=1.0, complete=False, lower_bound=90, open_nodes=5)
    assert r.gap == 0.1


# ---- strings and flags -----------------------------------------------------------------------

def test_time_limit_block():
    assert report.pfsp_time_limit(1.23456, 42, 3600, 3679) == (
        "Time limit reached after 1.2346 s: exploration not completed.\n"
        "Open nodes: 42\n"
        "Proven lower bound: 3600\n"
        "Gap to best makespan: 2.15 %")
    for none in (INT_MAX, None):
        assert report.pfsp_time_limit(10.0, 7, 1234, none) == (
            "Time limit reached after 10.0000 s: exploration not completed.\n"
            "Open nodes: 7\n"
            "Proven lower bound: 1234\n"
            "Gap to best makespan: unknown (no schedule found)")


def run_cli(*args):
    return subprocess.run([sys.executable, "-m", "dist_gpu_accelerated_tree_search_amd", "pfsp", *args],
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [("-D", "0", "-C", "0"), ("-D", "0", "-C", "4"), ("-D", "1", "-C", "1"), ("-D", "1"),
                                  ("-D", "2", "-C", "0"), ("-D", "1", "-C", "0", "--single-process"),
                                  ("-D", "1", "-C", "0", "--gpus-list", "0")])
def test_cli_time_limit_needs_one_plain_gpu(args):
    r = run_cli("-i", "14", "--no-csv", "--time-limit", "1", *args)
    assert r.returncode == 1 and r.stderr.strip() == "Error: --time-limit needs -D 1 -C 0" and r.stdout == ""


@pytest.mark.parametrize("s", ["0", "-2.5"])
def test_cli_time_limit_must_be_positive(s):
    r = run_cli("-i", "14", "--no-csv", "-D", "1", "-C", "0", f"--time-limit={s}")
    assert r.returncode == 1 and r.stderr.strip() == "Error: --time-limit must be positive" and r.stdout == ""


def test_cli_cpu_run_untouched(tmp_path):
    """-D 0 without the flag: the results block as before, the JSON record with the new keys."""
    out = tmp_path / "r.json"
    r = run_cli("-i", "14", "-l", "1", "-D", "0", "-C", "0", "--no-csv", "--json", str(out))
    assert r.returncode == 0 and "Time limit" not in r.stdout and "Proven lower bound" not in r.stdout
    assert "Size of the explored tree: 2573652" in r.stdout and "Optimal makespan: 1377" in r.stdout
    rec = json.loads(out.read_text().splitlines()[-1])
    assert (rec["tree"], rec["sol"], rec["best"]) == GOLDEN_TA014
    assert rec["complete"] is True and rec["lower_bound"] == 1377 and rec["open_nodes"] == 0 and rec["gap"] == 0.0
