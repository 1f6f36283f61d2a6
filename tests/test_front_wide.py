"""Front-carrying nodes for 51-100 jobs (128-bit job sets, csrc/core/pfsp_node.hpp JobSet):
opt-in with TTS_FRONT_WIDE=1. Host side: layout, the unchanged defaults, bounds against the
permutation-node bounds, trees against the permutation layout's, and the staircase range
rule that replaces the sum rule of the smaller buckets (csrc/core/pfsp_front.hpp)."""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

INT_MAX = 2**31 - 1
SEED = 3  # of the near_limit / over_limit instances


def random_perm_nodes(jobs, n, seed, dmax=None):
    rng = np.random.default_rng(seed)
    depths = rng.integers(0, (dmax or jobs - 1) + 1, size=n)
    perms = np.stack([rng.permutation(jobs) for _ in range(n)])
    return nd.pfsp_pack(depths, perms, jobs), depths, perms


def root_lb1(native):
    return ops.cpu().lb1(native, list(range(native.jobs)), 0)


# ---- layout ------------------------------------------------------------------------------

@pytest.mark.parametrize("lb", [0, 1])
@pytest.mark.parametrize("inst,machines,nbytes", [(61, 5, 48), (71, 10, 64), (81, 20, 80)])
def test_layout(inst, machines, nbytes, lb, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    C = ops.cpu()
    m = PfspModel(inst, lb)
    assert m.front_layout and m.node_bytes == nbytes
    assert m.describe()["layout"] == "front"
    assert C.pfsp_node_bytes(m.jobs) == 112  # the permutation node the bucket replaces
    p2 = PfspModel(inst, 2)
    assert not p2.front_layout and p2.node_bytes == 112  # LB2 stays on permutation nodes
    d, rest, fr = nd.pfsp_front_unpack(m.root(), machines, jobs=100)
    assert d[0] == 0 and int(rest[0]) == (1 << 100) - 1
    assert list(fr[0]) == list(C.PfspInstance.taillard(inst).min_heads)
    w = nd.pfsp_front_set_words(m.root())
    assert w.dtype == np.uint64 and w.shape == (1, 2)
    assert int(w[0, 0]) == (1 << 64) - 1 and int(w[0, 1]) == (1 << 36) - 1


@pytest.mark.parametrize("jobs", [51, 64, 65, 100])
def test_root_set_has_exactly_the_jobs(jobs, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    m = PfspModel.synthetic(jobs, 4, 7, lb=0)
    assert m.front_layout and m.node_bytes == 48
    _, rest, _ = nd.pfsp_front_unpack(m.root(), 5, jobs=jobs)
    assert int(rest[0]) == (1 << jobs) - 1


def test_defaults_unchanged(monkeypatch):
    monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
    m = PfspModel(61, 1)
    assert m.node_bytes == 112 and not m.front_layout and m.describe()["layout"] == "perm"
    monkeypatch.setenv("TTS_FRONT_WIDE", "0")
    assert not PfspModel(61, 1).front_layout
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    monkeypatch.setenv("TTS_FRONT", "0")
    m = PfspModel(61, 1)
    assert m.node_bytes == 112 and not m.front_layout
    # the smaller buckets do not look at the opt-in
    monkeypatch.delenv("TTS_FRONT")
    assert PfspModel(56, 1).node_bytes == 64 and PfspModel(14, 1).node_bytes == 32
    assert PfspModel.synthetic(101, 5, 1, lb=1).front_layout is False  # 200-job bucket: permutation


# ---- bounds ------------------------------------------------------------------------------

def bounds_equal_permutation_bounds(model):
    C = ops.cpu()
    perm_nodes, depths, perms = random_perm_nodes(model.jobs, 200, 11)
    ref = model.child_bounds_cpu(perm_nodes)  # child order k = depth..N-1
    front = model.to_engine_layout(perm_nodes)
    assert front.shape == (200, model.node_bytes)
    got = np.asarray(C.pfsp_children_bounds(model.native, 0, front))  # ascending job order
    off = 0
    for d, q in zip(depths, perms):
        kids = list(q[d:])
        mine = ref[off:off + len(kids)]
        by_job = dict(zip(kids, mine))
        assert list(got[off:off + len(kids)]) == [by_job[j] for j in sorted(kids)]
        off += len(kids)
    assert off == len(got)


# job counts on either side of each 32-bit word boundary of the set and at both ends of the
# bucket; 4 / 9 / 13 / 17 machines: padding machines in every machine bucket
@pytest.mark.parametrize("spec", [(61, None), (71, None), (81, None), (None, (51, 4, 8)), (None, (64, 9, 9)),
                                  (None, (65, 13, 10)), (None, (96, 20, 11)), (None, (100, 17, 12))])
def test_front_bounds_equal_permutation_bounds(spec, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    inst, syn = spec
    model = PfspModel(inst, 0) if inst else PfspModel.synthetic(*syn, lb=0)
    assert model.front_layout
    bounds_equal_permutation_bounds(model)


def test_converted_nodes_hold_the_unscheduled_set(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    model = PfspModel.synthetic(100, 17, 12, lb=0)
    perm_nodes, depths, perms = random_perm_nodes(100, 50, 5)
    d, rest, fr = nd.pfsp_front_unpack(model.to_engine_layout(perm_nodes), 20, jobs=100)
    p = np.asarray(model.native.p).reshape(model.machines, model.jobs)
    for i in range(50):
        assert d[i] == depths[i]
        assert int(rest[i]) == sum(1 << int(j) for j in perms[i][depths[i]:])
        if depths[i] > 0:
            f = np.zeros(model.machines, dtype=np.int64)
            for j in perms[i][:depths[i]]:
                f[0] += p[0, j]
                for k in range(1, model.machines):
                    f[k] = max(f[k - 1], f[k]) + p[k, j]
            assert list(fr[i][:model.machines]) == list(f)


# ---- trees -------------------------------------------------------------------------------

# Start nodes and incumbents of the tree comparisons here and of the device solves
# (tests/test_gpu_front_wide.py), picked on the host with the permutation layout (LB1_d).
#
# "root": the incumbent is the root's LB1 plus delta, the tree is run_pfsp's from the root.
# The trees of these instances grow in jumps with delta, and only ta081 has a delta whose
# tree lies between 2 * 10^3 and 2 * 10^5 nodes:
#   ta081     delta 128: 29,182 nodes (delta 64: 10, delta 140: 297,904, delta 150: 2.5 M)
#   syn65x13  (seed 5) delta 114: 498 nodes; delta 112: 356, delta 116 and above did not
#             finish in 8 s on two threads (seeds 1-4 and 6-9 jump the same way)
#   ta071     delta 8: 4 nodes, delta 9 to 16: not finished in 15 s
#   ta061     delta 0: no node, delta 1: not finished in 15 s (nor did the subtree of any
#             single node of a 239-node warm-up in 4 s: most nodes share the root's bound)
# "deep": ta061 and ta071 therefore start from 64 random nodes of depth jobs - 9 with the
# optimum below them as the incumbent (no leaf improves it, so the tree does not depend on
# the order the children are visited in, which the two layouts do not share):
#   ta071     3,623 nodes, 221 leaves
#   ta061     0 nodes: on 5 machines every child of such a prefix is bounded at the optimum
#             or above; its 576 child bounds are still compared one by one on the device
SOLVES = {
    # name: (kind, model factory, delta or levels above the leaves, (tree, sol))
    "ta081": ("root", lambda: PfspModel(81, 0), 128, (29182, 0)),
    "syn65x13": ("root", lambda: PfspModel.synthetic(65, 13, 5, lb=0), 114, (498, 0)),
    "ta071": ("deep", lambda: PfspModel(71, 0), 9, (3623, 221)),
    "ta061": ("deep", lambda: PfspModel(61, 0), 9, (0, 0)),
}


def deep_nodes(jobs, n, seed, k=7):
    """n permutation nodes of depth jobs - k: k! leaves below each at most."""
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(jobs) for _ in range(n)])
    return nd.pfsp_pack(np.full(n, jobs - k), perms, jobs)


def solve_model(name):
    """(model, start nodes in its engine layout, incumbent) of SOLVES[name], under the
    environment of the caller (TTS_FRONT_WIDE set or not)."""
    kind, make, x, _ = SOLVES[name]
    model = make()
    if kind == "root":
        best = root_lb1(model.native) + x
        return model, model.warmup(best, 25)[0], best
    nodes = model.to_engine_layout(deep_nodes(model.jobs, 64, 21, x))
    return model, nodes, model.drain(INT_MAX, nodes)[2]


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_front_trees_equal_permutation_trees(name, monkeypatch):
    C = ops.cpu()
    kind, _, x, gold = SOLVES[name]
    got = {}
    for wide in ("1", "0"):
        monkeypatch.setenv("TTS_FRONT_WIDE", wide)
        model, nodes, best = solve_model(name)
        assert model.front_layout == (wide == "1")
        if kind == "root":
            r = C.run_pfsp(model.native, 0, best, threads=2)
            got[wide] = (r["tree"], r["sol"], r["best"])
        else:
            got[wide] = tuple(model.drain(best, nodes)) + (best,)
    print(name, x, got)
    assert got["1"] == got["0"]
    assert got["0"][:2] == gold


@pytest.mark.parametrize("k", [7, 10])
def test_front_trees_reach_the_leaves(k, monkeypatch):
    # 64 nodes of depth jobs - 7 (and jobs - 10) on a 100 x 10 instance, drained from +inf:
    # leaves are counted and set the incumbent in both layouts, and both find the same
    # optimum. The tree and the leaf count of a search from +inf depend on the order the
    # leaves are met in (permutation nodes visit children by position, front nodes by job:
    # the counts differ here), so those are compared from that optimum, as
    # test_front_layout.py does for 20 jobs. From jobs - 10 the tree from the optimum still
    # reaches leaves (5,918 nodes, 255 leaves)
    perm = deep_nodes(100, 64, 21, k)
    got, first = {}, {}
    for wide in ("1", "0"):
        monkeypatch.setenv("TTS_FRONT_WIDE", wide)
        m = PfspModel.synthetic(100, 10, 14, lb=0)
        assert m.front_layout == (wide == "1")
        nodes = m.to_engine_layout(perm)
        first[wide] = m.drain(INT_MAX, nodes)
        got[wide] = m.drain(first[wide][2], nodes)
    print(first, got)
    assert first["1"][2] == first["0"][2] < INT_MAX and first["1"][1] > 0 and first["0"][1] > 0
    assert got["1"] == got["0"] and got["1"][2] == first["1"][2]
    if k == 10:
        assert got["1"][:2] == (5918, 255)


# ---- the range rule ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def near():
    return tl.near_limit(100, 10, SEED)


def test_near_limit_is_accepted(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    p = near()
    assert int(p.sum()) > 65535                      # the sum rule of the smaller buckets would refuse it
    assert (100 + 10 - 1) * int(p.max()) < 65536     # the staircase bound holds
    m = PfspModel(None, 0, p=p)
    assert m.front_layout and m.node_bytes == 64
    bounds_equal_permutation_bounds(m)


def test_over_limit_falls_back(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "1")
    p = tl.over_limit(100, 20, SEED)
    assert (100 + 20 - 1) * int(p.max()) >= 65536
    m = PfspModel(None, 0, p=p)  # no exception: the permutation layout
    assert not m.front_layout and m.node_bytes == 112
    assert m.root().shape == (1, 112)
    perm_nodes, _, _ = random_perm_nodes(100, 4, 2)
    assert np.array_equal(m.to_engine_layout(perm_nodes), perm_nodes)


# ---- the command line --------------------------------------------------------------------

def test_cli_front_wide_sets_the_variable_first(monkeypatch):
    import os

    from dist_gpu_accelerated_tree_search_amd import cli

    monkeypatch.setenv("TTS_FRONT_WIDE", "0")
    seen = []
    monkeypatch.setattr(cli, "pfsp_main", lambda argv: seen.append(os.environ.get("TTS_FRONT_WIDE")) or 0)
    assert cli.main(["pfsp", "-i", "61", "-D", "0"]) == 0
    assert cli.main(["pfsp", "-i", "61", "-D", "0", "--front-wide"]) == 0
    assert seen == ["0", "1"]
    assert cli._pfsp_parser().parse_args(["--front-wide"]).front_wide is True
    assert cli._pfsp_parser().parse_args([]).front_wide is False
