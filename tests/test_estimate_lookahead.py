"""Lookahead tree-size probes on the host (csrc/core/estimate.hpp lookahead_estimate_indexed):
the twin against a pure-Python oracle written from the specification, its unbiasedness on a
tree the solver counts, the exact cases, and the interface (keywords, CLI, report)."""
import json
from math import factorial
from types import SimpleNamespace

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import PfspModel, estimate_tree, ops, solve_cpu
from dist_gpu_accelerated_tree_search_amd.utils import report
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

INT_MAX = 2**31 - 1
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def twin(model, best, probes, seed, **kw):
    kw.setdefault("method", "lookahead")
    return ops.cpu().tree_estimate_indexed(model, int(best), probes, seed, **kw)


def small(jobs, machines, seed=3, lb=0):
    """A stand-in model (jobs, machines, lb, machine-major p): the only way to one job."""
    p = tl.synthetic(max(jobs, 2), machines, seed)[:, :jobs]
    return SimpleNamespace(jobs=jobs, machines=machines, lb=lb, p=np.ascontiguousarray(p).reshape(-1).tolist(),
                           kind="pfsp", best_known=INT_MAX)


def neh(model):
    C = ops.cpu()
    return int(C.pfsp_neh(C.PfspInstance.from_matrix(model.jobs, model.machines, model.p), 200000))


# ---- the oracle: one lookahead probe under LB1, Python ints and floats only ----

class Oracle:
    def __init__(self, model):
        self.N, self.M = model.jobs, model.machines
        self.p = [[int(model.p[m * self.N + j]) for j in range(self.N)] for m in range(self.M)]
        self.tails = [min(sum(self.p[k][j] for k in range(m + 1, self.M)) for j in range(self.N))
                      for m in range(self.M)]

    def survivors(self, node, best):
        """Jobs, ascending, whose child has lb < best; none below a parent whose children are leaves."""
        front, remain, rest = node
        if len(rest) <= 1:
            return []
        out = []
        for j in rest:
            lb = front[0] + remain[0] + self.tails[0]
            t = front[0] + self.p[0][j]
            for m in range(1, self.M):
                s = max(t, front[m])
                lb = max(lb, s + remain[m] + self.tails[m])
                t = s + self.p[m][j]
            if lb < best:
                out.append(j)
        return out

    def child(self, node, j):
        front, remain, rest = node
        f, t = [], 0
        for m in range(self.M):
            t = max(t, front[m]) + self.p[m][j]
            f.append(t)
        return f, [remain[m] - self.p[m][j] for m in range(self.M)], [x for x in rest if x != j]

    def probe(self, best, seed, index, power):
        N = self.N
        node = ([0] * self.M, [sum(row) for row in self.p], list(range(N)))
        h = mix((seed + G * (index + 1)) & M64)
        w, est, depth, jobs = 1.0, 0.0, 0, []
        while depth < N - 1:
            surv = self.survivors(node, best)
            if not surv:
                break
            wk = w * float(len(surv))
            est = est + wk
            level = depth
            depth += 1
            kids = [self.child(node, j) for j in surv]
            wt = [len(self.survivors(c, best)) ** power for c in kids]
            T = sum(wt)
            if T == 0:
                break
            x = (mix((h + G * (level + 1)) & M64) * T) >> 64
            acc = 0
            for i, v in enumerate(wt):
                acc += v
                if acc > x:
                    break
            jobs.append(surv[i])
            wT = w * float(T)
            w = wT / float(wt[i])
            node = kids[i]
        return est, depth, jobs


@pytest.mark.parametrize("lb", [0, 1])
@pytest.mark.parametrize("jobs,machines", [(9, 4), (20, 5)])
def test_twin_equals_the_pure_python_oracle(jobs, machines, lb):
    m = small(jobs, machines, seed=40 + jobs, lb=lb)
    o = Oracle(m)
    h = neh(m)
    for best in (int(1.02 * h), int(1.05 * h)):
        for power in (1, 2, 3):
            r = twin(m, best, 256, 77, first_probe=5, records=True, power=power)["records"]
            assert r["depth"].max() >= 2  # the probes do walk
            for i in range(256):
                est, depth, chosen = o.probe(best, 77, 5 + i, power)
                assert r["depth"][i] == depth, (best, power, i)
                assert r["est"][i] == est, (best, power, i)  # both are exact doubles
                assert r["jobs"][i].tolist() == chosen + [-1] * (jobs - len(chosen)), (best, power, i)


_exact = {}


def exact_tree(lb):
    """A generated 10 x 5 instance and its -u 1 tree: the incumbent is the optimum, so the
    tree the solver counts is the one the probes sample."""
    if lb not in _exact:
        p = tl.synthetic(10, 5, 31)
        opt = solve_cpu(PfspModel(None, lb, p=p), ub=0).best
        m = PfspModel(None, lb, p=p, best_known=opt)
        r = solve_cpu(m, ub=1)
        assert r.best == opt
        _exact[lb] = (m, r.tree)
    return _exact[lb]


@pytest.mark.parametrize("power", [1, 2, 3])
@pytest.mark.parametrize("lb,look", [(0, "own"), (0, "lb1"), (2, "own"), (2, "lb1")])
def test_mean_is_the_exact_tree(lb, look, power):
    m, tree = exact_tree(lb)
    assert tree > 50
    e = twin(m, m.best_known, 200000, 2024 + power, threads=8, power=power, look=look)
    assert e["stderr"] > 0
    assert abs(e["tree"] - tree) <= 4 * e["stderr"], (e["tree"], tree, e["stderr"])


@pytest.mark.parametrize("lb", [0, 2])
def test_knuth_mean_is_the_exact_tree(lb):
    m, tree = exact_tree(lb)
    e = twin(m, m.best_known, 200000, 2024, threads=8, method="knuth")
    assert e["stderr"] > 0
    assert abs(e["tree"] - tree) <= 4 * e["stderr"], (e["tree"], tree, e["stderr"])


@pytest.mark.parametrize("power", [1, 2, 3])
@pytest.mark.parametrize("lb", [0, 1, 2])
def test_unpruned_12_jobs_is_exact(lb, power):
    # nothing pruned: every weight of a level is the same, T / wt_c = k, all below 2^53
    want = sum(factorial(12) // factorial(12 - d) for d in range(1, 12))
    e = twin(small(12, 3, lb=lb), INT_MAX, 40, 6, records=True, power=power)
    assert (e["records"]["est"] == float(want)).all() and (e["records"]["depth"] == 11).all()
    assert (e["records"]["jobs"][:, :10] >= 0).all() and (e["records"]["jobs"][:, 10:] == -1).all()
    assert e["tree"] == float(want) and e["stderr"] == 0.0


def childless_case(jobs=8, machines=6, seed=2):
    """(best, k): under `best` the root has k survivors and none of them has a
    surviving child (LB1; LB2 is at least LB1, so the survivors' children are gone there too)."""
    m = small(jobs, machines, seed=seed)
    C = ops.cpu()
    inst = C.PfspInstance.from_matrix(jobs, machines, m.p)
    root = C.lb1_children(inst, list(range(jobs)), 0)
    for best in sorted({b + 1 for b in root}):
        surv = [j for j in range(jobs) if root[j] < best]
        grand = []
        for j in surv:
            prmu = [j] + [x for x in range(jobs) if x != j]
            by_job = C.lb1_children(inst, prmu, 1)
            grand += [by_job[x] for x in prmu[1:]]
        if surv and min(grand) >= best:
            return best, len(surv)
    raise AssertionError("no incumbent with childless survivors on this instance")


@pytest.mark.parametrize("lb", [0, 1])
def test_all_survivors_childless(lb):
    best, k = childless_case()
    assert k == 2
    e = twin(small(8, 6, seed=2, lb=lb), best, 30, 4, records=True)
    assert (e["records"]["depth"] == 1).all() and (e["records"]["est"] == float(k)).all()
    assert (e["records"]["jobs"] == -1).all()
    assert e["tree"] == float(k) and e["per_level"] == [float(k)]


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_one_and_two_jobs(lb):
    e1 = twin(small(1, 3, lb=lb), INT_MAX, 10, 1, records=True)
    assert e1["tree"] == 0.0 and (e1["records"]["depth"] == 0).all() and e1["per_level"] == []
    e2 = twin(small(2, 3, lb=lb), INT_MAX, 10, 1, records=True)
    assert (e2["records"]["est"] == 2.0).all() and (e2["records"]["depth"] == 1).all()
    assert (e2["records"]["jobs"] == -1).all()  # the two survivors' children are leaves: T = 0
    assert e2["tree"] == 2.0 and e2["per_level"] == [2.0]


def test_threads_and_splits_change_nothing():
    m = PfspModel(14, 0)
    a = twin(m, m.best_known, 3000, 4, threads=1, records=True)
    b = twin(m, m.best_known, 3000, 4, threads=8, records=True)
    assert {k: b[k] for k in ("tree", "stderr", "depth", "per_level")} == \
           {k: a[k] for k in ("tree", "stderr", "depth", "per_level")}
    for k in ("est", "depth", "jobs"):
        assert (a["records"][k] == b["records"][k]).all()
    lo = twin(m, m.best_known, 1200, 4, records=True)["records"]
    hi = twin(m, m.best_known, 1800, 4, first_probe=1200, records=True)["records"]
    for k in ("est", "depth", "jobs"):
        assert (a["records"][k] == np.concatenate([lo[k], hi[k]])).all()


@pytest.mark.parametrize("lb", [0, 2])
def test_knuth_keyword_is_the_old_call(lb):
    m = PfspModel(14, lb)
    old = ops.cpu().tree_estimate_indexed(m, m.best_known, 2000, 9, first_probe=3, threads=2, records=True)
    new = ops.cpu().tree_estimate_indexed(m, m.best_known, 2000, 9, first_probe=3, threads=2, records=True,
                                          method="knuth", power=3, look="own")
    assert {k: new[k] for k in ("tree", "stderr", "depth", "per_level", "probes")} == \
           {k: old[k] for k in ("tree", "stderr", "depth", "per_level", "probes")}
    for k in ("est", "depth", "jobs"):
        assert (old["records"][k] == new["records"][k]).all()
    a = estimate_tree(m, probes=2000, seed=9, device=None)
    assert a["tree"] == estimate_tree(m, probes=2000, seed=9, device=None, method="knuth")["tree"]
    assert (a["method"], a["power"], a["look"]) == ("knuth", 2, "lb1" if lb == 2 else "own")


def test_lookahead_differs_from_knuth_and_lb1_look_is_own_for_lb1():
    m = PfspModel(14, 1)
    k = twin(m, m.best_known, 500, 2, method="knuth")
    own = twin(m, m.best_known, 500, 2, look="own", records=True)
    lb1 = twin(m, m.best_known, 500, 2, look="lb1", records=True)
    assert own["tree"] != k["tree"] and own["depth"] > k["depth"]
    assert (own["records"]["est"] == lb1["records"]["est"]).all()
    m2 = PfspModel(14, 2)
    d = twin(m2, m2.best_known, 500, 2, records=True)  # look None: lb1 for LB2
    assert (d["records"]["est"] == twin(m2, m2.best_known, 500, 2, look="lb1", records=True)["records"]["est"]).all()


def test_unknown_values_raise():
    m = PfspModel(14, 0)
    for kw in (dict(power=0), dict(power=4), dict(method="chen"), dict(look="lb2")):
        with pytest.raises(ValueError):
            estimate_tree(m, probes=10, device=None, **{"method": "lookahead", **kw})
        with pytest.raises(ValueError):
            ops.cpu().tree_estimate_indexed(m, m.best_known, 10, 1, **{"method": "lookahead", **kw})
    with pytest.raises(ValueError):
        estimate_tree(m, probes=10, device=None, method="knuth", power=0)


def test_estimate_tree_cli_and_report(tmp_path, capsys):
    from dist_gpu_accelerated_tree_search_amd import cli

    m = PfspModel(14, 2)
    e = estimate_tree(m, probes=600, seed=3, device=None, method="lookahead", power=3)
    assert (e["method"], e["power"], e["look"]) == ("lookahead", 3, "lb1") and e["launch"] is None
    assert e["tree"] == twin(m, m.best_known, 600, 3, power=3, look="lb1")["tree"]
    assert set(e) == set(estimate_tree(m, probes=10, device=None))
    first = report.pfsp_estimate(14, 2, e).splitlines()[2]
    assert first.startswith("Lookahead (power 3, look lb1) tree-size estimate of ta14")
    assert report.pfsp_estimate(14, 2, estimate_tree(m, probes=10, device=None)).splitlines()[2].startswith("Knuth ")
    out = tmp_path / "e.json"
    assert cli.main(["pfsp", "-i", "14", "-l", "2", "-D", "0", "--estimate", "600", "--estimate-seed", "3",
                     "--estimate-method", "lookahead", "--estimate-power", "3", "--estimate-look", "lb1",
                     "--no-csv", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert "Lookahead (power 3, look lb1) tree-size estimate of ta14" in text and "Mean probe depth" in text
    rec = json.loads(out.read_text().splitlines()[-1])
    assert (rec["method"], rec["power"], rec["look"]) == ("lookahead", 3, "lb1")
    assert rec["tree"] == e["tree"] and rec["per_level"] == e["per_level"]
    with pytest.raises(SystemExit):
        cli.main(["pfsp", "-i", "14", "-D", "0", "--estimate", "10", "--estimate-power", "4", "--no-csv"])
