"""Device lookahead probes (csrc/hip/estimate_kernels.hpp lookahead_probe_kernel) against their
host twin (csrc/core/estimate.hpp lookahead_estimate_indexed), probe by probe: est bit for
bit, depth and every chosen job; the weighted pick where weights of zero sit beside others;
and the independence of the result from how the probes are dealt over waves, grids, launches
and calls."""
from concurrent.futures import ThreadPoolExecutor
from math import factorial
from types import SimpleNamespace

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import PfspModel, estimate_tree, ops
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
SEED = 20261
_twin_cache = {}


def gen(jobs, machines, seed, lb):
    """Generated instance as a stand-in model (jobs, machines, lb, machine-major p); cut from
    a 2-job matrix below two jobs."""
    p = tl.synthetic(max(jobs, 2), machines, seed)[:, :jobs]
    return SimpleNamespace(jobs=jobs, machines=machines, lb=lb, p=np.ascontiguousarray(p).reshape(-1).tolist(),
                           kind="pfsp", best_known=INT_MAX, key=("gen", jobs, machines, seed, lb))


def incumbent(model):
    """An incumbent of a generated instance under which the probes walk: 2 % above the NEH +
    iterated-greedy makespan (at the heuristic's own value LB1 closes a 5-machine root)."""
    C = ops.cpu()
    return int(1.02 * C.pfsp_neh(C.PfspInstance.from_matrix(model.jobs, model.machines, model.p), 200000))


def _twin_call(model, best, probes, seed, first, how):
    return ops.cpu().tree_estimate_indexed(model, int(best), probes, seed, first_probe=first, records=True, **how)


def twin(model, best, probes, seed=SEED, first=0, power=2, look=None, method="lookahead"):
    """Host twin records and aggregates, computed once per case and shared. The twin reduces
    1024 probes per chunk, so a call of fewer runs on one thread; from 32 probes on, eight
    calls over consecutive probe ranges run side by side instead (probe i is the same walk in
    any call) and their records are joined. The aggregates of the joined call are then those
    of finish_estimate over the records, and the per-level means the slices' weighted by
    their probes: the same sums in another order, which is what close_aggregates allows for."""
    how = dict(method=method, power=power, look=look)
    key = (getattr(model, "key", None) or ("ta", model.inst_id, model.lb), best, probes, seed, first, power, look,
           method)
    if key in _twin_cache:
        return _twin_cache[key]
    if probes < 32:
        r = _twin_call(model, best, probes, seed, first, how)
    else:
        cuts = [probes * i // 8 for i in range(9)]
        with ThreadPoolExecutor(8) as ex:
            parts = list(ex.map(lambda i: _twin_call(model, best, cuts[i + 1] - cuts[i], seed, first + cuts[i], how),
                                range(8)))
        rec = {k: np.concatenate([q["records"][k] for q in parts]) for k in ("est", "depth", "jobs")}
        n = float(probes)
        tree = float(rec["est"].sum()) / n
        with np.errstate(over="ignore", invalid="ignore"):
            var = float((rec["est"] * rec["est"]).sum()) / n - tree * tree
        var = var if var > 0 else 0.0  # as std::max(0.0, var): a NaN gives 0
        levels = max(len(q["per_level"]) for q in parts)
        per_level = [sum(q["per_level"][d] * q["probes"] for q in parts if d < len(q["per_level"])) / n
                     for d in range(levels)]
        r = dict(tree=tree, stderr=float(np.sqrt(var / n)), depth=float(rec["depth"].sum()) / n, probes=probes,
                 per_level=per_level, records=rec)
    for a in r["records"].values():
        a.setflags(write=False)
    _twin_cache[key] = r
    return r


def device(model, best, probes, seed=SEED, first=0, power=2, look=None, method="lookahead", **kw):
    p = model.native.p if hasattr(model, "native") else model.p
    return ops.hip().tree_estimate(model.jobs, model.machines, list(p), model.lb, int(best), probes, seed,
                                   first_probe=first, records=True, method=method, power=power, look=look, **kw)


def same_records(d, t):
    d, t = d["records"], t["records"]
    assert d["est"].shape == t["est"].shape
    assert (d["jobs"] == t["jobs"]).all(), np.argwhere(d["jobs"] != t["jobs"])[:4]
    assert (d["depth"] == t["depth"]).all()
    assert (d["est"].view(np.uint64) == t["est"].view(np.uint64)).all()  # bit for bit


def close_aggregates(d, t, n):
    """The sums are of the same positive terms in another order: n additions, each rounding
    by at most 2^-53 relative, on either side. The standard error divides a difference,
    var = s2 / n - mean^2, whose relative error is that of its terms times their size over var."""
    tol = n * 2.0**-52
    assert d["probes"] == t["probes"]
    assert abs(d["tree"] - t["tree"]) <= tol * t["tree"] or d["tree"] == t["tree"]
    assert abs(d["depth"] - t["depth"]) <= tol * t["depth"]
    assert len(d["per_level"]) == len(t["per_level"])
    for a, b in zip(d["per_level"], t["per_level"]):
        assert abs(a - b) <= tol * b if np.isfinite(b) else a == b  # a tree past 1.8e308 is inf on both
    if not (np.isfinite(t["tree"]) and np.isfinite(t["stderr"])):
        assert d["tree"] == t["tree"] and d["stderr"] == t["stderr"]
    elif t["stderr"] > 0:
        var = t["stderr"] ** 2 * n
        amp = (var + 3 * t["tree"] ** 2) / var  # s2 / n = var + mean^2, and mean^2 twice more
        assert abs(d["stderr"] - t["stderr"]) <= tol * amp * t["stderr"]
    else:
        assert d["stderr"] == 0.0


def check(model, best, probes, power=2, look=None, **kw):
    d, t = device(model, best, probes, power=power, look=look, **kw), twin(model, best, probes, power=power, look=look)
    same_records(d, t)
    close_aggregates(d, t, probes)
    return d, t


SHAPES = [(20, 5, 512), (20, 20, 256), (50, 10, 128), (30, 7, 128)]
CASES = [(j, m, n, lb, power, look) for (j, m, n) in SHAPES for lb, look in [(0, None), (1, None), (2, "own"), (2, "lb1")]
         for power in ((1, 2, 3) if j == 30 else (2,))]


@pytest.mark.parametrize("jobs,machines,probes,lb,power,look", CASES)
def test_records_equal_the_twin(jobs, machines, probes, lb, power, look):
    m = gen(jobs, machines, 100 + jobs + machines, lb)
    d, t = check(m, incumbent(m), probes, power=power, look=look)
    assert t["depth"] > 2.0  # the probes do walk, and deeper than one lookahead
    if jobs >= 50:  # weights beyond 2^53 round at every level: w * k then est + w k, w * T then / wt
        assert t["records"]["est"].max() > 2.0**60


@pytest.mark.parametrize("lb", [0, 2])
@pytest.mark.parametrize("jobs", [63, 64, 65])
def test_lane_passes_and_set_words(jobs, lb):
    m = gen(jobs, 5, 7 * jobs, lb)
    d, t = check(m, incumbent(m), 64)
    assert t["records"]["jobs"].max() == jobs - 1  # the last lane of the word, the first of the next


def test_three_set_words_lb1():
    m = gen(129, 10, 129, 1)
    d, t = check(m, incumbent(m), 16)
    assert t["records"]["jobs"].max() >= 128  # a job of the third word is chosen


def test_five_set_words_lb1():
    m = gen(257, 5, 257, 1)
    d, t = check(m, incumbent(m), 8)
    assert t["records"]["jobs"].max() >= 256


def root_weights(model, best):
    """{job: k_c} of the root's survivors under LB1, from the host's child bounds."""
    C = ops.cpu()
    n = model.jobs
    inst = C.PfspInstance.from_matrix(n, model.machines, model.p)
    root = C.lb1_children(inst, list(range(n)), 0)
    out = {}
    for j in range(n):
        if root[j] < best:
            prmu = [j] + [x for x in range(n) if x != j]
            by_job = C.lb1_children(inst, prmu, 1)
            out[j] = sum(by_job[x] < best for x in prmu[1:])
    return out


def mixed_case():
    """An incumbent of a 12 x 5 instance under which some of the root's survivors have
    surviving children and others have none."""
    m = gen(12, 5, 10, 0)
    C = ops.cpu()
    root = C.lb1_children(C.PfspInstance.from_matrix(12, 5, m.p), list(range(12)), 0)
    for best in sorted({b + 1 for b in root}):
        kc = root_weights(m, best)
        if sum(v == 0 for v in kc.values()) >= 2 and len({v for v in kc.values() if v > 0}) >= 2:
            return m, best, kc
    raise AssertionError("no incumbent with mixed weights on this instance")


def test_weighted_pick_skips_the_weightless():
    m, best, kc = mixed_case()
    live = {j for j, v in kc.items() if v > 0}
    t = twin(m, best, 256)
    first = t["records"]["jobs"][:, 0]
    assert set(first.tolist()) <= live and len(set(first.tolist())) >= 3
    uniform = twin(m, best, 256, method="knuth")["records"]["jobs"][:, 0]
    assert set(uniform.tolist()) - live  # a pick that ignores the weights follows the weightless too
    check(m, best, 256)
    for power in (1, 3):
        check(m, best, 256, power=power)


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_ta014(lb):
    m = PfspModel(14, lb)
    check(m, m.best_known, 1024)


@pytest.mark.parametrize("look,probes", [("lb1", 128), ("own", 32)])
def test_ta056_lb2(look, probes):
    m = PfspModel(56, 2)
    d, t = check(m, m.best_known, probes, look=look)
    assert d["launch"]["lds_bytes"] <= 65536 and t["depth"] > 8.0


def childless_case():
    """(best, k): under `best` the root of the 8 x 6 instance has k survivors and none of them
    has a surviving child."""
    m = gen(8, 6, 2, 0)
    C = ops.cpu()
    root = C.lb1_children(C.PfspInstance.from_matrix(8, 6, m.p), list(range(8)), 0)
    for best in sorted({b + 1 for b in root}):
        kc = root_weights(m, best)
        if kc and max(kc.values()) == 0:
            return best, len(kc)
    raise AssertionError("no incumbent with childless survivors on this instance")


@pytest.mark.parametrize("lb", [0, 1])
def test_all_survivors_childless(lb):
    best, k = childless_case()
    d, t = check(gen(8, 6, 2, lb), best, 70)
    assert k == 2 and (d["records"]["depth"] == 1).all() and (d["records"]["est"] == float(k)).all()
    assert (d["records"]["jobs"] == -1).all() and d["tree"] == float(k)


@pytest.mark.parametrize("power", [1, 2, 3])
@pytest.mark.parametrize("lb", [0, 2])
def test_unpruned_12_jobs(lb, power):
    want = sum(factorial(12) // factorial(12 - k) for k in range(1, 12))
    d, _ = check(gen(12, 3, 3, lb), INT_MAX, 70, power=power, look="own")
    assert (d["records"]["est"] == float(want)).all() and (d["records"]["depth"] == 11).all()


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_one_and_two_jobs(lb):
    d1, _ = check(gen(1, 3, 3, lb), INT_MAX, 10)
    assert d1["tree"] == 0.0 and d1["per_level"] == []
    d2, _ = check(gen(2, 3, 3, lb), INT_MAX, 10)
    assert (d2["records"]["est"] == 2.0).all() and (d2["records"]["jobs"] == -1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_probe_counts(n):
    m = PfspModel(14, 0)
    check(m, m.best_known, n)


def test_more_probes_than_one_grid_pass():
    m = PfspModel(14, 2)
    d, _ = check(m, m.best_known, 500, batch=500, max_blocks=3)
    assert d["launch"]["grid"] * d["launch"]["waves"] < 500 and d["launch"]["launches"] == 1


def test_first_probe_split_and_batches():
    m = PfspModel(14, 0)
    best, n = m.best_known, 1024
    whole = twin(m, best, n)
    lo, hi = device(m, best, 400), device(m, best, 624, first=400)
    for k in ("est", "depth", "jobs"):
        assert (np.concatenate([lo["records"][k], hi["records"][k]]) == whole["records"][k]).all()
    small = device(m, best, n, batch=64)
    assert small["launch"]["launches"] == 16 and small["launch"]["batch"] == 64
    same_records(small, whole)
    close_aggregates(small, whole, n)
    close_aggregates(small, device(m, best, n), n)


def test_knuth_keyword_is_the_old_call():
    m = PfspModel(14, 2)
    p = list(m.native.p)
    old = ops.hip().tree_estimate(m.jobs, m.machines, p, 2, m.best_known, 512, 7, records=True)
    new = ops.hip().tree_estimate(m.jobs, m.machines, p, 2, m.best_known, 512, 7, records=True, method="knuth",
                                  power=3, look="own")
    same_records(new, old)
    assert {k: new[k] for k in ("tree", "stderr", "depth", "per_level")} == \
           {k: old[k] for k in ("tree", "stderr", "depth", "per_level")}


def test_lookahead_state_past_lds_raises():
    # 512 x 26 LB1: 55 KB of tables; the Knuth wave state (4.4 KB) fits beside them, the
    # lookahead state (another 6.3 KB: prefix sums, k_c, the second node) does not
    m = gen(512, 26, 5, 1)
    assert device(m, 0, 4, method="knuth")["tree"] == 0.0
    with pytest.raises(ValueError, match="lookahead state"):
        device(m, 0, 4)
    for bad in (dict(power=0), dict(power=4), dict(look="lb2"), dict(method="chen")):
        with pytest.raises(ValueError):
            device(PfspModel(14, 0), 1377, 4, **bad)
    m2 = gen(100, 20, 220, 2)  # the LB2 tables leave room for two lookahead waves, as for two Knuth waves
    assert device(m2, 0, 4)["launch"]["waves"] == 2


def test_estimate_tree_interface():
    m = PfspModel(14, 0)
    a = estimate_tree(m, probes=512, seed=5, device=0, method="lookahead", power=3)
    b = estimate_tree(m, probes=512, seed=5, device=None, method="lookahead", power=3)
    assert set(a) == set(b)
    assert (a["method"], a["power"], a["look"]) == (b["method"], b["power"], b["look"]) == ("lookahead", 3, "own")
    close_aggregates(a, b, 512)
    assert a["launch"]["batch"] >= 1 and a["launch"]["rate"] > 0
    with pytest.raises(ValueError):
        estimate_tree(m, probes=8, device=0, method="lookahead", power=4)


def test_cli_estimates_on_the_device(tmp_path, capsys):
    import json

    from dist_gpu_accelerated_tree_search_amd import cli

    out = tmp_path / "e.json"
    assert cli.main(["pfsp", "-i", "14", "-l", "2", "-D", "1", "--estimate", "1024", "--estimate-seed", "9",
                     "--estimate-method", "lookahead", "--no-csv", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert "Lookahead (power 2, look lb1) tree-size estimate of ta14" in text and "on the device 0" in text
    rec = json.loads(out.read_text().splitlines()[-1])
    m = PfspModel(14, 2)
    t = ops.cpu().tree_estimate_indexed(m, m.best_known, 1024, 9, method="lookahead")
    assert rec["device"] == 0 and rec["probes"] == 1024
    assert (rec["method"], rec["power"], rec["look"]) == ("lookahead", 2, "lb1")
    close_aggregates(rec, t, 1024)
