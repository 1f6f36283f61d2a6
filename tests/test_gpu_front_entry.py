"""Engine solves through the front kernel's entry code (pool_begin, pool_device.hpp).

Every workgroup of every dependent kernel runs the entry code before its first bound: it
reads the control line, rebuilds the prefix of the previous iteration's per-chunk counts
and deals the parent window over the chunks (32-bit arithmetic, core/pool_window.hpp). A
mistake there shows as a wrong tree, so complete solves are compared with the host
engine's (tree, sol, best) under settings that drive the number of chunks an iteration
reads (nch_in) to 1, to exactly the grid's chunk count and above it, through the learned
first replay (one graph launch per solve, both host mirrors) with iteration counts of
every residue mod 3, from warm-up nodes whose children are leaves, from +inf after a
solve with the optimum, with several engines on the GPU and with a rank split pending.
"""
import functools

import pytest

from dist_gpu_accelerated_tree_search_amd.models.pfsp import EngineOptions, PfspModel
from dist_gpu_accelerated_tree_search_amd.parallel.launch import spawn_local
from dist_gpu_accelerated_tree_search_amd.parallel.workers import solve_rank
from dist_gpu_accelerated_tree_search_amd.search import solve_engine

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
GOLDEN = {(14, 1): (2573652, 2648, 1377), (3, 1): (2573133, 5689, 1081)}
KNOBS = ("TTS_LOCAL_STEPS", "TTS_FUSE_MAX", "TTS_LOCAL_MIN", "TTS_WIDE_LEVELS", "TTS_DYN_US", "TTS_BLOCKS_PER_CU")


def result(r):
    return (r.tree, r.sol, r.best)


@functools.lru_cache(maxsize=None)
def taillard(inst, lb=1):
    return PfspModel(inst, lb)


@functools.lru_cache(maxsize=None)
def host(inst, lb=1, m=25):
    """The host engine's solve of a Taillard instance (computed once per instance)."""
    model = taillard(inst, lb)
    r = result(solve_engine(model, model.make_engine("cpu"), ub=1, m=m))
    if (inst, lb) in GOLDEN:
        assert r == GOLDEN[(inst, lb)]
    return r


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- nch_in = 1, = the grid's chunk count, > the grid's chunk count ----------------------

@pytest.mark.parametrize("inst", [14, 3])
@pytest.mark.parametrize("setting", ["window256", "default", "one_level_wide"])
def test_chunk_counts_read(monkeypatch, inst, setting):
    if setting == "window256":
        # one chunk per iteration: every iteration reads one count
        opts = EngineOptions(max_parents=256, ring_bytes=1 << 28)
    elif setting == "default":
        # local DFS iterations write exactly one chunk per workgroup of the grid
        opts = EngineOptions(max_parents=1 << 19, ring_bytes=1 << 30)
    else:
        # local DFS off: one-level iterations over the 2^19 window leave up to 2048 chunks,
        # more than the grid has workgroups
        monkeypatch.setenv("TTS_LOCAL_STEPS", "0")
        opts = EngineOptions(max_parents=1 << 19, ring_bytes=1 << 30)
    model = taillard(inst)
    eng = model.make_engine("gpu", 0, opts)
    for _ in range(2):
        r = solve_engine(model, eng, ub=1)
        print(setting, inst, result(r), "iters", r.extra["iters"], "parents", r.extra["parents"])
        assert result(r) == host(inst)
    if setting == "window256":
        assert r.extra["parents"] <= 256 * r.extra["iters"]


# ---- the learned first replay, twice in a row, K % 3 in {0, 1, 2} -------------------------

def test_learned_replay_every_residue():
    # the iteration count of a -u 1 solve depends on the instance and on where the host
    # warm-up hands over (m nodes): try them until every residue mod 3 was a learned count
    seen = {}
    for inst, lb, m in [(14, 1, 25), (14, 1, 1), (14, 1, 400), (3, 1, 25), (3, 1, 1), (3, 1, 400), (14, 0, 25),
                        (14, 0, 3000), (3, 1, 3000), (14, 1, 3000)]:
        model = taillard(inst, lb)
        eng = model.make_engine("gpu", 0, EngineOptions(max_parents=1 << 19, ring_bytes=1 << 30))
        its, launches = [], []
        for _ in range(5):
            r = solve_engine(model, eng, ub=1, m=m)
            assert result(r) == host(inst, lb), (inst, lb, m)
            its.append(r.extra["iters"])
            launches.append(r.extra["launches"])  # (cumulative over the engine's life)
        del eng
        print(f"ta{inst:03d} lb {lb} m {m}: iterations {its} launches {launches}")
        # solves 3, 4 and 5 are the learned replay (one launch each): both mirrors used
        assert its[2] == its[3] == its[4]
        assert launches[4] - launches[3] == launches[3] - launches[2] == 1, launches
        seen.setdefault(its[4] % 3, (inst, lb, m, its[4]))
        if len(seen) == 3:
            break
    print("learned counts by residue:", seen)
    assert sorted(seen) == [0, 1, 2], seen


# ---- warm-up nodes whose children are leaves ----------------------------------------------

@pytest.mark.parametrize("jobs,machines,m", [(3, 5, 3), (4, 7, 12), (6, 10, 25), (6, 15, 300)])
def test_tiny_generated_instance(jobs, machines, m):
    # the first device iteration (all its fused levels) reaches the leaves: they lower the
    # incumbent in the very first kernel of the solve
    model = PfspModel.synthetic(jobs, machines, seed=7, lb=1)
    want = result(solve_engine(model, model.make_engine("cpu"), ub=0, m=m, best=INT_MAX))
    eng = model.make_engine("gpu", 0, EngineOptions(max_parents=1 << 19, ring_bytes=1 << 28))
    for _ in range(4):
        r = solve_engine(model, eng, ub=0, m=m, best=INT_MAX)
        print(jobs, machines, m, result(r), "iters", r.extra["iters"])
        # (from +inf the tree depends on the order of search: the optimum is what counts)
        assert r.best == want[2]
    # with the optimum as the incumbent the tree is deterministic
    wantu1 = result(solve_engine(model, model.make_engine("cpu"), ub=1, m=m, best=want[2]))
    for _ in range(4):
        assert result(solve_engine(model, eng, ub=1, m=m, best=want[2])) == wantu1


# ---- -u 0 from +inf straight after a -u 1 solve -------------------------------------------

def test_unknown_optimum_after_known():
    model = taillard(14)
    eng = model.make_engine("gpu", 0, EngineOptions(max_parents=1 << 19, ring_bytes=1 << 30))
    for _ in range(3):
        assert result(solve_engine(model, eng, ub=1)) == host(14)
    # the -u 0 solve starts from its own incumbent (+inf), not the one the -u 1 solves left:
    # it has to find the optimum itself, in a far bigger tree
    r0 = solve_engine(model, eng, ub=0, best=INT_MAX)
    print("-u 0:", result(r0))
    assert r0.best == 1377 and r0.tree > host(14)[0]
    for _ in range(2):
        assert result(solve_engine(model, eng, ub=1)) == host(14)


# ---- several engines on one GPU, and a pending rank split ---------------------------------

def test_three_streams():
    model = taillard(14)
    eng = model.make_engine("gpu", 0, EngineOptions(streams=3, ring_bytes=3 << 30, max_parents=1 << 19))
    for _ in range(3):
        assert result(solve_engine(model, eng)) == host(14)


def test_two_ranks_pending_split():
    # two ranks share the GPU over gloo; each solve begins replicated with a split armed
    spec = {"problem": "pfsp", "inst": 14, "lb": 1, "backend": "gpu", "comm": "gloo", "device": 0, "session": True,
            "repeat": 3, "engine": {"ring_bytes": 1 << 28, "max_parents": 1 << 19}}
    res = spawn_local(2, solve_rank, (spec,), timeout=600)
    for r in res:
        assert (r["tree"], r["sol"], r["best"]) == host(14)
