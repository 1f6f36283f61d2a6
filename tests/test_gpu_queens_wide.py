"""Whole N-Queens device engines on boards of 16 to 32 rows (attack-mask bits 15..31),
against the host engine: solves from a deep frontier handed to begin() at three finishing
depths, tiny and wide parent windows, a ring small enough to spill the 16-byte nodes, the
in-search rank split, boards the root's own lane finishes, and the N = 16 / 17 goldens."""
import functools
import random

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import EngineOptions, QueensModel, solve_cpu, solve_gpu
from dist_gpu_accelerated_tree_search_amd.utils import queens_oracle as qo
from test_queens_oracle import drain, pack

pytestmark = pytest.mark.gpu

OPTS = EngineOptions(max_parents=1 << 20, ring_bytes=1 << 30)
# N -> (columns left, nodes)
FRONTIERS = {16: (13, 512), 20: (14, 256), 24: (14, 256), 31: (13, 512), 32: (13, 512)}


@functools.lru_cache(maxsize=None)
def frontier(N):
    """The packed frontier and the host engine's (tree, sol) below it."""
    left, n = FRONTIERS[N]
    nodes = qo.random_nodes(N, N - left, n, random.Random(7000 + N))
    return pack(nodes), drain(N, nodes)


def run_from(eng, nodes):
    eng.begin(nodes, 0)
    eng.run()
    st = eng.stats()
    assert eng.size() == 0
    return st["tree"], st["sol"]


@pytest.mark.parametrize("finish", [0, 9, 12])
@pytest.mark.parametrize("N", sorted(FRONTIERS))
def test_from_a_deep_frontier(N, finish, monkeypatch):
    monkeypatch.setenv("TTS_QUEENS_FINISH", str(finish))
    nodes, want = frontier(N)
    eng = QueensModel(N).make_engine("gpu", 0, OPTS)
    for _ in range(2):
        assert run_from(eng, nodes) == want, (N, finish)


def test_from_a_deep_frontier_with_g_work(monkeypatch):
    monkeypatch.setenv("TTS_QUEENS_FINISH", "9")
    nodes, want = frontier(32)
    eng = QueensModel(32, 2).make_engine("gpu", 0, OPTS)
    for _ in range(2):
        assert run_from(eng, nodes) == want


@pytest.mark.parametrize("finish", [0, 9, 12])
def test_one_chunk_window(finish, monkeypatch):
    """max_parents = 256: one workgroup per kernel (the wide window, 2^20 parents, is the one
    of the tests above). One workgroup explores about a million nodes in a millisecond, and
    without finishing it expands 256 parents per kernel: the first 32 frontier nodes (some
    20 M nodes below them), 2 level by level (a million nodes, a few thousand kernels)."""
    monkeypatch.setenv("TTS_QUEENS_FINISH", str(finish))
    nodes = frontier(20)[0][:2 if finish == 0 else 32]
    want = tuple(int(x) for x in QueensModel(20).drain(0, nodes)[:2])
    assert want[0] > 100_000
    eng = QueensModel(20).make_engine("gpu", 0, EngineOptions(max_parents=256, ring_bytes=1 << 30))
    for _ in range(2):
        assert run_from(eng, nodes) == want, finish


def test_spill_and_refill_of_16_byte_nodes(monkeypatch):
    monkeypatch.delenv("TTS_QUEENS_FINISH", raising=False)
    # a 2^18-node ring (the smallest for a 1024-parent window): a frontier of more than half of
    # it is spilled to the host on begin() and refilled while the device drains
    N = 32
    few = qo.random_nodes(N, N - 11, 512, random.Random(32))
    tree, sol = drain(N, few)
    reps = 300
    nodes = np.tile(pack(few), (reps, 1))
    eng = QueensModel(N).make_engine("gpu", 0, EngineOptions(max_parents=1 << 10, ring_bytes=1 << 20))
    for _ in range(2):
        assert run_from(eng, nodes) == (reps * tree, reps * sol)
        st = eng.stats()
        assert st["spilled"] > 0 and st["refilled"] > 0, st


def test_in_search_split_from_a_deep_frontier(monkeypatch):
    monkeypatch.delenv("TTS_QUEENS_FINISH", raising=False)
    nodes, want = frontier(20)
    tree = sol = 0
    per = []
    for r in range(3):
        e = QueensModel(20).make_engine("gpu", 0, OPTS)
        e.set_split(r, 3, 2048)
        e.begin(nodes, 0)
        assert e.split_pending()
        e.run()
        assert not e.split_pending()
        st = e.stats()
        tree += st["tree"]
        sol += st["sol"]
        per.append(st["tree"])
        del e
    assert (tree, sol) == want
    assert min(per) > 0


@pytest.mark.parametrize("N", range(1, 8))
def test_tiny_boards_finished_by_the_roots_lane(N, monkeypatch):
    # at most 9 columns: the default finishing depth finishes the root in one lane
    monkeypatch.delenv("TTS_QUEENS_FINISH", raising=False)
    want = solve_cpu(QueensModel(N))
    m = QueensModel(N)
    eng = m.make_engine("gpu", 0, EngineOptions(max_parents=1 << 16, ring_bytes=1 << 28))
    for _ in range(2):
        assert run_from(eng, m.root()) == (want.tree, want.sol)
    assert (want.tree, want.sol) == qo.subtree(N, (0, 0, 0, 0))


@pytest.mark.parametrize("N,gold", [(16, (1141190302, 14772512)), (17, (8017021931, 95815104))])
def test_golden_whole_solves(N, gold, monkeypatch):
    monkeypatch.delenv("TTS_QUEENS_FINISH", raising=False)
    r = solve_gpu(QueensModel(N))  # default options
    assert (r.tree, r.sol) == gold
