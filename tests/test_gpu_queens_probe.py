"""What ONE iteration of the production N-Queens kernel writes (queens_expand_probe), child
by child against the pure-Python oracle (utils/queens_oracle.py): the child->parent map,
the r-th-free-row search, the per-chunk counts and leaf words on boards up to N = 32 (mask
bits 15..31), a chunk that fills its slot region, the rank-split mask, and the subtrees
finished inside the kernel (wave stacks and the register-walk fallback) against the
oracle and the host engine. Every comparison is exact; no expected value comes from the
kernel."""
import functools
import random

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.utils import queens_oracle as qo
from test_queens_oracle import FINISH_SETS, ROOT, drain, finish_set, pack, subtree_sum, verdict

pytestmark = pytest.mark.gpu

BP = 256          # parents per chunk
MAXCH = BP * 32   # children a chunk's slot region holds
FINISH_MAX = 12   # deepest finishing the kernel has (kQueensFinishMax)


def probe(N, G, nodes, **kw):
    return ops.require_gpu(0).queens_expand_probe(N, G, pack(nodes), **kw)


def row_of(parent, child):
    return (parent[0] ^ child[0]).bit_length() - 1


def check_level(r, N, nodes, expands=lambda p: True, keep=lambda gi, row: True, leaves=None):
    """The probe's children / counts / leaves against the oracle: chunk c holds the
    children of parents [256 c, 256 c + 256) that expand, in parent order, rows ascending."""
    kids, counts = [], []
    for c0 in range(0, len(nodes), BP):
        k = [c for gi, p in enumerate(nodes[c0:c0 + BP], c0) if expands(p)
             for c in qo.children(N, p) if keep(gi, row_of(p, c))]
        kids += k
        counts.append(len(k))
    assert max(counts) <= MAXCH
    assert list(r["counts"]) == counts
    got, want = r["children"], pack(kids)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (int(bad[0]), got[bad[0]].view(np.uint32), want[bad[0]].view(np.uint32))
    assert r["leaves"] == (sum(1 for p in nodes if p[3] == N) if leaves is None else leaves)
    return kids


@functools.lru_cache(maxsize=None)
def mixed_parents(N, n=1000):
    """n random valid parents, depths over the whole range [0, N] (complete boards
    included), one in 16 a dead end, shuffled."""
    rng = random.Random(1000 + N)
    out = []
    for d in range(N + 1):
        out += qo.random_nodes(N, d, len(range(d, n, N + 1)), rng)
    rng.shuffle(out)
    out[::16] = qo.random_dead_ends(N, len(out[::16]), rng)
    return tuple(out)


def is_dead_end(N, p):
    return p[3] < N and qo.free_rows(N, p) == 0


LEVEL_BOARDS = [(5, 1), (16, 1), (17, 1), (17, 3), (24, 1), (31, 1), (32, 1), (32, 3)]


@pytest.mark.parametrize("n", [255, 256, 257, 1000])
@pytest.mark.parametrize("N,G", LEVEL_BOARDS)
def test_one_level_byte_for_byte(N, G, n):
    nodes = list(mixed_parents(N)[:n])
    assert any(p[3] == N for p in nodes) and any(is_dead_end(N, p) for p in nodes)
    assert {p[3] for p in nodes} == set(range(N + 1))
    r = probe(N, G, nodes)
    kids = check_level(r, N, nodes)
    assert r["fin_tree"] == r["fin_sol"] == 0
    if N == 32:
        # the top mask bit: a queen already on row 31, and a child that places one there
        # (a child's anti mask has bit 30 only when its queen went to row 31), and an expanding
        # parent whose left diagonal loses bit 31 in the children
        assert any(p[0] >> 31 for p in nodes)
        assert any(c[2] >> 30 for c in kids)
        assert any(p[1] >> 31 and qo.free_rows(N, p) for p in nodes)


@pytest.mark.parametrize("N,G", LEVEL_BOARDS)
def test_one_parent(N, G):
    pool = mixed_parents(N)
    leaf = next(p for p in pool if p[3] == N)
    dead = next(p for p in pool if is_dead_end(N, p))
    inner = next(p for p in pool if 0 < p[3] < N and qo.free_rows(N, p))
    for p in (ROOT, inner, leaf, dead):
        r = probe(N, G, [p])
        check_level(r, N, [p])
        assert r["fin_tree"] == r["fin_sol"] == 0


@pytest.mark.parametrize("N", [32, 31])
@pytest.mark.parametrize("n", [256, 257])
def test_a_chunk_that_fills_its_slot_region(N, n):
    # N children per root: at N = 32 one chunk of 256 roots writes exactly MAXCH children
    r = probe(N, 1, [ROOT] * n)
    kids = check_level(r, N, [ROOT] * n)
    assert list(r["counts"]) == ([BP * N] if n == BP else [BP * N, N])
    assert (BP * N == MAXCH) == (N == 32)
    assert [row_of(ROOT, c) for c in kids[-N:]] == list(range(N))


def test_probe_rejects_nodes_the_kernel_cannot_take():
    H = ops.require_gpu(0)
    with pytest.raises(ValueError):
        H.queens_expand_probe(8, 1, pack([(0b11, 0, 0, 3)]), finish_k=9)  # depth is not the queens placed
    with pytest.raises(ValueError):
        H.queens_expand_probe(8, 1, pack([(1 << 8, 0, 0, 1)]))  # a row outside the board
    with pytest.raises(ValueError):
        H.queens_expand_probe(8, 1, pack([ROOT]), split_rank=2, split_world=2)
    assert H.queens_stack_nodes() >= 64  # a wave's finishing parents must fit its stack


# ---- finishing --------------------------------------------------------------------------

def check_finishing(N, G, nodes, k, sample_rng=None):
    """One iteration with finishing from k columns left: children only from the parents
    above the finishing depth, the finished subtrees' counts from the host engine (and
    from the Python oracle on a sample of the finishing parents)."""
    fin = [p for p in nodes if N - k <= p[3] < N]
    r = probe(N, G, nodes, finish_k=k)
    check_level(r, N, nodes, expands=lambda p: p[3] < N - k)
    want = drain(N, fin, G) if fin else (0, 0)
    assert (r["fin_tree"], r["fin_sol"]) == want
    if sample_rng is not None:
        sample = sample_rng.sample(fin, min(len(fin), 32))
        assert subtree_sum(N, sample) == drain(N, sample)
    return r


@pytest.mark.parametrize("k", [1, 2, 9, 12])
@pytest.mark.parametrize("N", [16, 17, 24, 32])
def test_finishing_in_a_mixed_window(N, k):
    rng = random.Random(N * 100 + k)
    nodes = list(mixed_parents(N)) + qo.random_nodes(N, N - k, 40, rng)
    rng.shuffle(nodes)
    # above the finishing depth, exactly at it, below it, complete boards; dead ends among the
    # expanding parents (they exist deep in the tree only) and among the finishing ones
    assert {p[3] for p in nodes} == set(range(N + 1))
    assert any(is_dead_end(N, p) and p[3] < N - k for p in nodes) or k > 2
    assert any(is_dead_end(N, p) and p[3] >= N - k for p in nodes) or k < 9
    assert sum(1 for p in nodes if N - k <= p[3] < N) >= 32
    check_finishing(N, 1, nodes, k, rng)


def test_finishing_keeps_the_g_work():
    check_finishing(17, 3, list(mixed_parents(17)[:600]), 9)
    check_finishing(32, 3, list(mixed_parents(32)[:300]), 12)


def test_finishing_depth_is_clamped():
    # 20 columns: clamped to the deepest finishing the kernel has
    nodes = list(mixed_parents(24)[:300])
    r = probe(24, 1, nodes, finish_k=20)
    check_level(r, 24, nodes, expands=lambda p: p[3] < 24 - FINISH_MAX)
    assert (r["fin_tree"], r["fin_sol"]) == drain(24, [p for p in nodes if 24 - FINISH_MAX <= p[3] < 24])


@pytest.mark.parametrize("N,k", [(17, 9), (32, 12), (16, 2)])
def test_finishing_parents_by_position(N, k):
    rng = random.Random(N + k)
    above = qo.random_nodes(N, N - k - 1, BP, rng)  # expand level by level
    at = qo.random_nodes(N, N - k, BP + 1, rng)     # finish
    # one finishing parent alone
    check_finishing(N, 1, at[:1], k, rng)
    # one finishing parent in a window of expanding ones
    check_finishing(N, 1, above[:100] + at[:1] + above[100:255], k)
    # finishing parents only in the lanes of the workgroup's last wave
    check_finishing(N, 1, above[:192] + at[:64], k, rng)
    # ... and only in some lanes of the last wave of a second, partial chunk
    check_finishing(N, 1, above + above[:70] + at[:9], k)
    # 64 finishing parents filling one wave; 257: a second chunk with one parent
    check_finishing(N, 1, at[:64], k, rng)
    mixed = [p for d in range(N - k, N) for p in qo.random_nodes(N, d, BP // k + 1, rng)][:BP] + at[-1:]
    assert len(mixed) == BP + 1
    check_finishing(N, 1, mixed, k, rng)


@pytest.mark.parametrize("name", sorted(FINISH_SETS))
def test_finishing_sets_that_fit_or_overflow_the_stack(name):
    """The stack model tells on the host whether a wave's stack overflows into the register
    walk on this input at the built stack size: asserted before the GPU is asked, so a build
    with another stack size fails here instead of no longer covering the fallback."""
    N, parents = finish_set(name)
    parents = list(parents)
    k = FINISH_SETS[name][4]
    stack = ops.require_gpu(0).queens_stack_nodes()
    assert verdict(N, parents, stack) == ("fits" if name.endswith("fits") else "overflows")
    want = subtree_sum(N, parents)
    r = probe(N, 1, parents, finish_k=k)
    assert list(r["counts"]) == [0] and len(r["children"]) == 0 and r["leaves"] == 0
    assert (r["fin_tree"], r["fin_sol"]) == want
    # the same wave as the third of a workgroup whose other lanes expand or hold leaves
    rng = random.Random(5)
    other = qo.random_nodes(N, N - k - 1, 100, rng) + qo.random_nodes(N, N, 28, rng)
    window = other[:64] + other[100:] + [other[64]] * (64 - 28) + parents + other[64:100]
    assert window[128:128 + len(parents)] == parents
    r = probe(N, 1, window, finish_k=k)
    check_level(r, N, window, expands=lambda p: p[3] < N - k)
    assert (r["fin_tree"], r["fin_sol"]) == want


# ---- the rank split ---------------------------------------------------------------------

M64 = (1 << 64) - 1


def split_owner(gi, row, world):
    """Owner of child `row` of window parent gi (pool_device.hpp split_keep)."""
    x = (gi * 1024 + row + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x % world


@functools.lru_cache(maxsize=None)
def split_parents():
    rng = random.Random(20)
    nodes = [p for d in range(11, 20) for p in qo.random_nodes(20, d, 32, rng)]
    nodes += qo.random_nodes(20, 20, 12, rng)
    rng.shuffle(nodes)
    assert len(nodes) == 300
    return tuple(nodes)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_rank_split_shares(world):
    N = 20
    nodes = list(split_parents())
    leaves = sum(1 for p in nodes if p[3] == N)
    assert leaves == 12 and all(p[3] >= N - 9 for p in nodes)
    whole = probe(N, 1, nodes)  # unsplit, level by level
    all_kids = check_level(whole, N, nodes)
    union, counts = [], np.zeros(len(whole["counts"]), np.int64)
    for rank in range(world):
        # deep enough to be finished at 9 columns left: not while the split is armed
        r = probe(N, 1, nodes, finish_k=9, split_rank=rank, split_world=world)
        assert r["fin_tree"] == r["fin_sol"] == 0
        kids = check_level(r, N, nodes, keep=lambda gi, row: split_owner(gi, row, world) == rank,
                           leaves=leaves if rank == 0 else 0)
        assert kids, rank
        union += kids
        counts += np.asarray(r["counts"])
    assert sorted(union) == sorted(all_kids)  # as multisets: the shares are disjoint and complete
    assert list(counts) == list(whole["counts"])
