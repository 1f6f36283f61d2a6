"""Front-carrying nodes for 101-500 jobs (256- and 512-bit job sets, csrc/core/pfsp_node.hpp
JobSet<4> / JobSet<8>, a 16-byte header with a u16 depth): opt-in with TTS_FRONT_WIDE=2.
Host side: layout, the unchanged defaults, bounds against the permutation-node bounds, the
layout conversion, trees against the permutation layout's, the staircase range rule and the
command line. The reference everywhere is the host permutation-layout code."""
import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl
from test_front_wide import SEED, bounds_equal_permutation_bounds, deep_nodes, random_perm_nodes, root_lb1

INT_MAX = 2**31 - 1

# job counts on both sides of every 64-bit word boundary of the set and at both ends of
# both buckets
JOBS_200 = (101, 128, 129, 192, 193, 200)
JOBS_500 = (201, 256, 257, 320, 321, 384, 385, 448, 449, 500)
BYTES = {200: {5: 64, 10: 80, 20: 96}, 500: {5: 96, 10: 112, 20: 128}}
PERM_BYTES = {200: 208, 500: 1008}


def bucket_of(machines):
    return 5 if machines <= 5 else 10 if machines <= 10 else 20


def job_bucket(jobs):
    return 200 if jobs <= 200 else 500


# ---- layout ------------------------------------------------------------------------------

@pytest.mark.parametrize("lb", [0, 1])
@pytest.mark.parametrize("inst,jobs,machines", [(91, 200, 10), (101, 200, 20), (111, 500, 20)])
def test_layout_taillard(inst, jobs, machines, lb, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    C = ops.cpu()
    m = PfspModel(inst, lb)
    assert (m.jobs, m.machines) == (jobs, machines)
    assert m.front_layout and m.node_bytes == BYTES[jobs][machines]
    assert m.describe()["layout"] == "front"
    assert C.pfsp_node_bytes(m.jobs) == PERM_BYTES[jobs]  # the permutation node the bucket replaces
    p2 = PfspModel(inst, 2)
    assert not p2.front_layout and p2.node_bytes == PERM_BYTES[jobs]  # LB2 stays on permutation nodes
    assert p2.describe()["layout"] == "perm"
    d, rest, fr = nd.pfsp_front_unpack(m.root(), machines, jobs=jobs)
    assert d[0] == 0 and int(rest[0]) == (1 << jobs) - 1
    assert list(fr[0]) == list(C.PfspInstance.taillard(inst).min_heads)
    w = nd.pfsp_front_set_words(m.root(), jobs)
    assert w.dtype == np.uint64 and w.shape == (1, 4 if jobs == 200 else 8)
    root = np.asarray(m.root())
    assert not root[0, :16].any()  # depth 0 and a zero header


@pytest.mark.parametrize("machines", [4, 9, 17])
@pytest.mark.parametrize("jobs", JOBS_200 + JOBS_500)
def test_root_set_has_exactly_the_jobs(jobs, machines, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    m = PfspModel.synthetic(jobs, machines, 7, lb=0)
    mb = bucket_of(machines)
    assert m.front_layout and m.node_bytes == BYTES[job_bucket(jobs)][mb]
    assert m.describe()["layout"] == "front"
    _, rest, _ = nd.pfsp_front_unpack(m.root(), mb, jobs=jobs)
    assert int(rest[0]) == (1 << jobs) - 1
    w = nd.pfsp_front_set_words(m.root(), jobs)
    assert sum(bin(int(x)).count("1") for x in w[0]) == jobs


# ---- defaults ----------------------------------------------------------------------------

def test_defaults_unchanged(monkeypatch):
    for v in (None, "0", "1"):
        if v is None:
            monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)
        else:
            monkeypatch.setenv("TTS_FRONT_WIDE", v)
        for inst, nbytes in ((91, 208), (101, 208), (111, 1008)):
            m = PfspModel(inst, 1)
            assert not m.front_layout and m.node_bytes == nbytes and m.describe()["layout"] == "perm"
        assert PfspModel.synthetic(101, 5, 1, lb=1).front_layout is False
    # 2 includes what 1 does: the 51-100-job nodes at their existing sizes
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    for inst, nbytes in ((61, 48), (71, 64), (81, 80)):
        m = PfspModel(inst, 1)
        assert m.front_layout and m.node_bytes == nbytes
    assert PfspModel(56, 1).node_bytes == 64 and PfspModel(14, 1).node_bytes == 32
    assert PfspModel(101, 1).front_layout
    # TTS_FRONT=0 wins
    monkeypatch.setenv("TTS_FRONT", "0")
    for inst, nbytes in ((61, 112), (101, 208), (111, 1008)):
        m = PfspModel(inst, 1)
        assert not m.front_layout and m.node_bytes == nbytes


# ---- bounds ------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", [91, 101, 111])
def test_front_bounds_equal_permutation_bounds_taillard(inst, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    model = PfspModel(inst, 0)
    assert model.front_layout
    bounds_equal_permutation_bounds(model)


@pytest.mark.parametrize("jobs", JOBS_200 + JOBS_500)
def test_front_bounds_equal_permutation_bounds(jobs, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    machines = (4, 9, 17, 20, 13)[jobs % 5]  # padding machines in every machine bucket
    model = PfspModel.synthetic(jobs, machines, 8 + jobs % 7, lb=0)
    assert model.front_layout
    bounds_equal_permutation_bounds(model)


def around_256(jobs, seed, depth_list):
    """Permutation parents of the given depths whose unscheduled jobs include 255 and 256:
    depths and job ids on both sides of 8 bits."""
    rng = np.random.default_rng(seed)
    depths, perms = [], []
    for d in depth_list:
        for _ in range(4):
            others = rng.permutation([j for j in range(jobs) if j not in (255, 256)])
            tail = np.concatenate([others[d:], [255, 256]])
            perms.append(np.concatenate([others[:d], rng.permutation(tail)]).astype(np.int64))
            depths.append(d)
    return nd.pfsp_pack(np.array(depths), np.stack(perms), jobs), np.array(depths), np.stack(perms)


# (257 jobs: at depth 255 the two jobs left are 255 and 256)
@pytest.mark.parametrize("jobs,machines,depth_list", [(257, 4, (255,)), (300, 9, (254, 255, 256, 257, 258)),
                                                      (500, 20, (254, 255, 256, 257, 258))])
def test_bounds_around_depth_and_job_256(jobs, machines, depth_list, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    C = ops.cpu()
    model = PfspModel.synthetic(jobs, machines, 3, lb=0)
    perm_nodes, depths, perms = around_256(jobs, 5, depth_list)
    ref = model.child_bounds_cpu(perm_nodes)
    front = model.to_engine_layout(perm_nodes)
    d, rest, _ = nd.pfsp_front_unpack(front, bucket_of(machines), jobs=jobs)
    assert list(d) == list(depths)
    got = np.asarray(C.pfsp_children_bounds(model.native, 0, front))
    off = 0
    for i, (dp, q) in enumerate(zip(depths, perms)):
        kids = [int(j) for j in q[dp:]]
        assert 255 in kids and 256 in kids
        assert int(rest[i]) == sum(1 << j for j in kids)
        by_job = dict(zip(kids, ref[off:off + len(kids)]))
        assert list(got[off:off + len(kids)]) == [by_job[j] for j in sorted(kids)]
        off += len(kids)
    assert off == len(got) == len(ref)
    # the children appending jobs 255 and 256 carry depth + 1 past a byte
    kids, leaves, low = C.pfsp_front_expand(model.native, 0, front, INT_MAX)
    dk, rk, _ = nd.pfsp_front_unpack(kids, bucket_of(machines), jobs=jobs)
    assert leaves == 0 and low is None and len(kids) == len(ref)
    at = 0
    for i, dp in enumerate(depths):
        n = jobs - dp
        assert set(dk[at:at + n]) == {dp + 1}
        assert [int(rest[i]) & ~int(r) for r in rk[at:at + n]] == [1 << j for j in sorted(int(j) for j in perms[i][dp:])]
        at += n


# ---- conversion --------------------------------------------------------------------------

@pytest.mark.parametrize("jobs,machines", [(200, 17), (500, 17)])
def test_converted_nodes_hold_the_unscheduled_set(jobs, machines, monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    model = PfspModel.synthetic(jobs, machines, 12, lb=0)
    perm_nodes, depths, perms = random_perm_nodes(jobs, 40, 5)
    if jobs == 500:
        assert (depths > 255).sum() >= 5  # nodes deeper than a byte counts
    front = model.to_engine_layout(perm_nodes)
    assert front.shape == (40, BYTES[jobs][20])
    d, rest, fr = nd.pfsp_front_unpack(front, 20, jobs=jobs)
    assert not np.asarray(front)[:, 2:16].any()  # the header past the depth is zero
    p = np.asarray(model.native.p).reshape(model.machines, model.jobs)
    for i in range(40):
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
# (tests/test_gpu_front_xwide.py), computed with the permutation layout (LB1_d, run_pfsp on
# two threads / drain). None has an improving leaf, so none depends on the order children
# are visited in, which the two layouts do not share.
#   "root": the incumbent is the root's LB1 plus delta, the tree is run_pfsp's from the root
#     ta101 (root LB1 10,979)      +140: 233, +150: 4,832, +160: 68,396 nodes (+170 does not
#                                  finish in 12 s)
#     ta111 (root LB1 25,922)      +24: 60 nodes (+32 does not finish)
#     syn193x20 (seed 5, 11,186)   +24: 207 nodes
#   "deep": 64 random nodes of depth jobs - k, the optimum below them as the incumbent
#     ta111 k = 9 (29,557)         18,739 nodes, 6,923 leaves; k = 10: 77,655 / 28,342
#     ta101 k = 7 (13,183)         170 nodes, 36 leaves
XSOLVES = {
    # name: (kind, model factory, delta or levels above the leaves, (tree, sol))
    "ta101+140": ("root", lambda: PfspModel(101, 0), 140, (233, 0)),
    "ta101+150": ("root", lambda: PfspModel(101, 0), 150, (4832, 0)),
    "ta101+160": ("root", lambda: PfspModel(101, 0), 160, (68396, 0)),
    "ta111+24": ("root", lambda: PfspModel(111, 0), 24, (60, 0)),
    "syn193x20+24": ("root", lambda: PfspModel.synthetic(193, 20, 5, lb=0), 24, (207, 0)),
    "ta111k9": ("deep", lambda: PfspModel(111, 0), 9, (18739, 6923)),
    "ta111k10": ("deep", lambda: PfspModel(111, 0), 10, (77655, 28342)),
    "ta101k7": ("deep", lambda: PfspModel(101, 0), 7, (170, 36)),
}
ROOT_LB1 = {"ta101": 10979, "ta111": 25922, "syn193x20": 11186}
DEEP_OPT = {"ta111k9": 29557, "ta111k10": 29557, "ta101k7": 13183}


def xsolve_model(name, best=None):
    """(model, start nodes in its engine layout, incumbent) of XSOLVES[name], under the
    environment of the caller (TTS_FRONT_WIDE set or not). "root": the root node itself (a
    25-node warm-up already is the whole 60-node tree of ta111). "deep": the incumbent is the
    optimum below the nodes, drained from +inf unless `best` is given."""
    kind, make, x, _ = XSOLVES[name]
    model = make()
    if kind == "root":
        return model, model.root(), root_lb1(model.native) + x
    nodes = model.to_engine_layout(deep_nodes(model.jobs, 64, 21, x))
    return model, nodes, model.drain(INT_MAX, nodes)[2] if best is None else best


@pytest.mark.parametrize("name", sorted(XSOLVES))
def test_front_trees_equal_permutation_trees(name, monkeypatch):
    C = ops.cpu()
    kind, _, x, gold = XSOLVES[name]
    got = {}
    for wide in ("2", "1"):
        monkeypatch.setenv("TTS_FRONT_WIDE", wide)
        # (from +inf the permutation layout takes 12 s on ta111 k = 10: there the front
        # layout alone finds the optimum, the same 29,557 as below k = 9)
        model, nodes, best = xsolve_model(name, DEEP_OPT[name] if (name, wide) == ("ta111k10", "1") else None)
        assert model.front_layout == (wide == "2")
        if kind == "root":
            assert best - x == ROOT_LB1[name.split("+")[0]]
            r = C.run_pfsp(model.native, 0, best, threads=2)
            got[wide] = (r["tree"], r["sol"], r["best"])
            # the same tree from the root node through drain (what the device solves start from)
            assert tuple(model.drain(best, nodes)) == (r["tree"], r["sol"], best)
        else:
            assert best == DEEP_OPT[name]  # both layouts find it from +inf
            got[wide] = tuple(model.drain(best, nodes)) + (best,)
    print(name, x, got)
    assert got["2"] == got["1"]
    assert got["1"][:2] == gold


def test_front_trees_reach_the_leaves(monkeypatch):
    # 64 nodes of depth jobs - 9 of a 257 x 13 instance drained from +inf: tree and sol then
    # depend on the order the leaves are met in (tests/test_front_wide.py), so only the
    # optimum found is compared
    perm = deep_nodes(257, 64, 21, 9)
    first = {}
    for wide in ("2", "1"):
        monkeypatch.setenv("TTS_FRONT_WIDE", wide)
        m = PfspModel.synthetic(257, 13, 5, lb=0)
        assert m.front_layout == (wide == "2")
        first[wide] = m.drain(INT_MAX, m.to_engine_layout(perm))
    print(first)
    assert first["2"][2] == first["1"][2] == 15510 and first["2"][1] > 0 and first["1"][1] > 0


# ---- the host expansion used by the device tests -------------------------------------------

def test_front_expand_equals_children_bounds(monkeypatch):
    # the binding the device tests compare with: its survivors are exactly the children whose
    # pfsp_children_bounds value is below the incumbent, in order, and their bytes convert
    # back from the permutation layout
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    C = ops.cpu()
    m = PfspModel.synthetic(129, 9, 6, lb=0)
    perm_nodes, depths, perms = random_perm_nodes(129, 60, 9)
    front = m.to_engine_layout(perm_nodes)
    lbs = np.asarray(C.pfsp_children_bounds(m.native, 0, front))
    best = int(np.median(lbs))
    kids, leaves, low = C.pfsp_front_expand(m.native, 0, front, best)
    want, at, nleaf, lo = [], 0, 0, None
    for d, q in zip(depths, perms):
        jobs = sorted(int(j) for j in q[d:])
        mine = lbs[at:at + len(jobs)]
        at += len(jobs)
        if d + 1 == m.jobs:
            nleaf += len(jobs)
            lo = int(mine.min()) if lo is None else min(lo, int(mine.min()))
            continue
        for j, lb in zip(jobs, mine):
            if lb < best:
                want.append((d + 1, list(q[:d]) + [j] + [x for x in q[d:] if x != j]))
    assert (leaves, low) == (nleaf, lo) and len(kids) == len(want) > 0
    exp = m.to_engine_layout(nd.pfsp_pack([w[0] for w in want], [w[1] for w in want], 129))
    assert np.array_equal(kids, exp)


# ---- the range rule ----------------------------------------------------------------------

def test_near_limit_is_accepted(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    p = tl.near_limit(500, 20, SEED)
    assert int(p.sum()) > 65535                      # the sum rule of the smaller buckets would refuse it
    assert (500 + 20 - 1) * int(p.max()) < 65536     # the staircase bound holds
    m = PfspModel(None, 0, p=p)
    assert m.front_layout and m.node_bytes == 128
    bounds_equal_permutation_bounds(m)


def test_over_limit_falls_back(monkeypatch):
    monkeypatch.setenv("TTS_FRONT_WIDE", "2")
    p = tl.over_limit(500, 20, SEED)
    assert (500 + 20 - 1) * int(p.max()) >= 65536
    m = PfspModel(None, 0, p=p)  # no exception: the permutation layout
    assert not m.front_layout and m.node_bytes == 1008
    assert m.root().shape == (1, 1008)
    perm_nodes, _, _ = random_perm_nodes(500, 4, 2)
    assert np.array_equal(m.to_engine_layout(perm_nodes), perm_nodes)


# ---- the command line --------------------------------------------------------------------

def test_cli_front_all_sets_the_variable_first(monkeypatch):
    import os

    from dist_gpu_accelerated_tree_search_amd import cli

    monkeypatch.setenv("TTS_FRONT_WIDE", "0")
    seen = []
    monkeypatch.setattr(cli, "pfsp_main", lambda argv: seen.append(os.environ.get("TTS_FRONT_WIDE")) or 0)
    assert cli.main(["pfsp", "-i", "101", "-D", "0"]) == 0
    assert cli.main(["pfsp", "-i", "101", "-D", "0", "--front-all"]) == 0
    monkeypatch.setenv("TTS_FRONT_WIDE", "0")
    assert cli.main(["pfsp", "-i", "101", "-D", "0", "--front-wide"]) == 0
    assert seen == ["0", "2", "1"]
    assert cli._pfsp_parser().parse_args(["--front-all"]).front_all is True
    assert cli._pfsp_parser().parse_args(["--front-all"]).front_wide is False
    assert cli._pfsp_parser().parse_args([]).front_all is False
    assert cli._pfsp_parser().parse_args([]).front_wide is False
