"""The cases of the whole device solves on permutation nodes (tests/test_gpu_perm_engines.py)
and their host references. Every Taillard instance from ta061 on runs by default on
DeviceEngine<PfspTraits<NJ, M, LBK>> with NJ = 100 / 200 / 500 (nodes of 112 / 208 / 1008 B):
the front layouts of these sizes are opt-in (TTS_FRONT_WIDE). Each gold below is a constant
that this file recomputes with the host engine on permutation nodes (ops.cpu().run_pfsp on
two threads, PfspModel.drain); nothing here comes from a device."""
import time

import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd
from test_front_wide import SOLVES, deep_nodes, root_lb1
from test_front_xwide import DEEP_OPT, ROOT_LB1, XSOLVES

INT_MAX = 2**31 - 1


def ta(inst):
    return lambda lb: PfspModel(inst, lb)


def syn(jobs, machines, seed):
    return lambda lb: PfspModel.synthetic(jobs, machines, seed, lb=lb)


# name: (kind, model factory (lb), lb, delta or levels above the leaves, node bytes,
#        (tree, sol, best))
#   "root": from the root node, the incumbent is the root's LB1 plus delta (no leaf improves
#           it); run_pfsp on two threads
#   "deep": from 64 random nodes of depth jobs - k (deep_nodes(jobs, 64, 21, k)), the
#           incumbent is the optimum below them; drain
# LB1_d / LB1: the trees tests/test_front_wide.py SOLVES and tests/test_front_xwide.py XSOLVES
# verify on the host, once per node size, two LB1 twins (LB1 and LB1_d are one kernel and
# equal values) and a 13-machine instance (20-machine bucket, padding machines).
# LB2: root starts, the delta the largest (in steps of 2) whose host solve took at most 5 s
# on two threads; the trees grow in jumps with delta (host seconds in the comments):
#   ta081 100x20  +160: 7,084 nodes 2.7 s, +162: 9,724 nodes 4.3 s, +164: 13,747 nodes 6.6 s
#   ta101 200x20  +152: 6,152 nodes 4.5 s, +154: 8,565 nodes 4.2 s, +156: 11,820 nodes 6.4 s
#   ta111 500x20  +32: 15 nodes 0.5 s, +34: not finished in 14 s (a 15-node tree still
#                 spans several device iterations at 2 parents per chunk)
#   ta071 100x10  +8: 3 nodes 0.05 s, +10: not finished in 14 s
#   ta091 200x10  +20: no node (every child of the root is bounded at the incumbent or
#                 above: one device iteration) 0.08 s, +22: not finished in 14 s
CASES = {
    "ta081": ("root", ta(81), 0, 128, 112, (29182, 0, 5979)),
    "ta081lb1": ("root", ta(81), 1, 128, 112, (29182, 0, 5979)),
    "syn65x13": ("root", syn(65, 13, 5), 0, 114, 112, (498, 0, 3856)),
    "ta071k9": ("deep", ta(71), 0, 9, 112, (3623, 221, 6586)),
    "ta101+150": ("root", ta(101), 0, 150, 208, (4832, 0, 11129)),
    "syn193x20+24": ("root", syn(193, 20, 5), 0, 24, 208, (207, 0, 11210)),
    "ta101k7": ("deep", ta(101), 0, 7, 208, (170, 36, 13183)),
    "ta101k7lb1": ("deep", ta(101), 1, 7, 208, (170, 36, 13183)),
    "ta111k9": ("deep", ta(111), 0, 9, 1008, (18739, 6923, 29557)),
    "ta081lb2+162": ("root", ta(81), 2, 162, 112, (9724, 0, 6013)),
    "ta101lb2+154": ("root", ta(101), 2, 154, 208, (8565, 0, 11133)),
    "ta111lb2+32": ("root", ta(111), 2, 32, 1008, (15, 0, 25954)),
    "ta071lb2+8": ("root", ta(71), 2, 8, 112, (3, 0, 5767)),
    "ta091lb2+20": ("root", ta(91), 2, 20, 208, (0, 0, 10836)),
}
# used by one device test each: the longer tree of a second solve on one engine, and the
# largest 1008-B tree (tests/test_front_xwide.py verifies both on the host)
LONGER = {"ta101+160": ("root", ta(101), 0, 160, 208, XSOLVES["ta101+160"][3] + (ROOT_LB1["ta101"] + 160,)),
          "ta111k10": ("deep", ta(111), 0, 10, 1008, XSOLVES["ta111k10"][3] + (DEEP_OPT["ta111k10"],))}

# From +inf the counts depend on the order the leaves are met in; the optimum does not.
# 64 nodes of depth jobs - 7: name: (model factory, lb, the optimum below them). The host's
# drain from +inf took 0.01 s (ta071) to 0.14 s (ta111 LB2).
FROM_INF = {
    "ta071": (ta(71), 0, 6587), "ta071lb2": (ta(71), 2, 6587),
    "ta101": (ta(101), 0, 13183), "ta101lb2": (ta(101), 2, 13183),
    "ta111": (ta(111), 0, 29565), "ta111lb2": (ta(111), 2, 29565),
}
INF_K = 7


def case_model(name, table=None):
    """(model, start nodes, incumbent, gold) of a case, on permutation nodes whatever the
    environment says about the front layouts."""
    kind, make, lb, x, nbytes, gold = (table or {**CASES, **LONGER})[name]
    model = make(lb)
    assert model.describe()["layout"] == "perm" and model.node_bytes == nbytes, (name, model.describe())
    nodes = model.root() if kind == "root" else model.to_engine_layout(deep_nodes(model.jobs, 64, 21, x))
    return model, nodes, gold[2], gold


def inf_model(name):
    make, lb, opt = FROM_INF[name]
    model = make(lb)
    assert model.describe()["layout"] == "perm"
    return model, model.to_engine_layout(deep_nodes(model.jobs, 64, 21, INF_K)), opt


@pytest.fixture(autouse=True)
def perm_layout(monkeypatch):
    monkeypatch.delenv("TTS_FRONT_WIDE", raising=False)


def test_the_table_reuses_the_verified_trees():
    for name, src in (("ta081", SOLVES["ta081"]), ("ta071k9", SOLVES["ta071"]), ("ta101+150", XSOLVES["ta101+150"]),
                      ("syn193x20+24", XSOLVES["syn193x20+24"]), ("ta101k7", XSOLVES["ta101k7"]),
                      ("ta111k9", XSOLVES["ta111k9"]), ("syn65x13", SOLVES["syn65x13"])):
        kind, _, lb, x, _, gold = CASES[name]
        assert (kind, x, gold[:2]) == (src[0], src[2], src[3]) and lb == 0, name
    assert CASES["ta081lb1"][3:] == CASES["ta081"][3:] and CASES["ta101k7lb1"][3:] == CASES["ta101k7"][3:]
    assert {c[4] for c in CASES.values() if c[2] != 2} == {112, 208, 1008}
    assert {(c[1](2).jobs, c[1](2).machines) for c in CASES.values() if c[2] == 2} >= {(100, 20), (200, 20), (500, 20)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_gold_is_the_host_tree(name):
    kind, _, lb, x, _, _ = CASES[name]
    model, nodes, best, gold = case_model(name)
    t0 = time.perf_counter()
    if kind == "root":
        assert best == root_lb1(model.native) + x
        r = ops.cpu().run_pfsp(model.native, model.host_lb, best, threads=2)
        got = (r["tree"], r["sol"], r["best"])
    else:
        # the optimum below the nodes, found from +inf, is the incumbent
        assert model.drain(INT_MAX, nodes)[2] == best
        got = tuple(model.drain(best, nodes))
    print(name, got, f"{time.perf_counter() - t0:.2f} s")
    assert got == gold
    depth = nd.pfsp_unpack(nodes, model.jobs)[0]
    assert set(depth) == ({0} if kind == "root" else {model.jobs - x})


@pytest.mark.parametrize("name", sorted(FROM_INF))
def test_optimum_from_infinity(name):
    model, nodes, opt = inf_model(name)
    t0 = time.perf_counter()
    tree, sol, best = model.drain(INT_MAX, nodes)
    print(name, (tree, sol, best), f"{time.perf_counter() - t0:.2f} s")
    assert best == opt and sol > 0
