"""Device Knuth estimator (csrc/hip/estimate_kernels.hpp) against its host twin, probe by
probe: est bit for bit, depth and every chosen job; and the independence of the result
from how the probes are dealt over waves, grids, launches and calls."""
from types import SimpleNamespace

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import PfspModel, estimate_tree, ops
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
SEED = 20251
_twin_cache = {}


def gen(jobs, machines, seed, lb):
    """Generated instance as a stand-in model (jobs, machines, lb, machine-major p); cut from
    a 2-job matrix below two jobs."""
    p = tl.synthetic(max(jobs, 2), machines, seed)[:, :jobs]
    return SimpleNamespace(jobs=jobs, machines=machines, lb=lb, p=np.ascontiguousarray(p).reshape(-1).tolist(),
                           kind="pfsp", best_known=INT_MAX, key=("gen", jobs, machines, seed, lb))


def from_matrix(p, lb, key):
    mm, n = p.shape
    return SimpleNamespace(jobs=n, machines=mm, lb=lb, p=np.ascontiguousarray(p).reshape(-1).tolist(), kind="pfsp",
                           best_known=INT_MAX, key=(key, lb))


def incumbent(model):
    """An incumbent of a generated instance under which the probes walk: 2 % above the NEH +
    iterated-greedy makespan (at the heuristic's own value LB1 closes a 5-machine root)."""
    C = ops.cpu()
    return int(1.02 * C.pfsp_neh(C.PfspInstance.from_matrix(model.jobs, model.machines, model.p), 200000))


def twin(model, best, probes, seed=SEED, first=0):
    """Host twin records, computed once per (instance, best, probes, seed, first) and shared."""
    key = (getattr(model, "key", None) or ("ta", model.inst_id, model.lb), best, probes, seed, first)
    if key not in _twin_cache:
        r = ops.cpu().tree_estimate_indexed(model, int(best), probes, seed, first_probe=first, threads=8, records=True)
        for a in r["records"].values():
            a.setflags(write=False)
        _twin_cache[key] = r
    return _twin_cache[key]


def device(model, best, probes, seed=SEED, first=0, **kw):
    p = model.native.p if hasattr(model, "native") else model.p
    return ops.hip().tree_estimate(model.jobs, model.machines, list(p), model.lb, int(best), probes, seed,
                                   first_probe=first, records=True, **kw)


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


def check(model, best, probes, **kw):
    d, t = device(model, best, probes, **kw), twin(model, best, probes)
    same_records(d, t)
    close_aggregates(d, t, probes)
    return d, t


@pytest.mark.parametrize("lb", [0, 1, 2])
@pytest.mark.parametrize("jobs,machines,probes", [(20, 5, 1024), (20, 20, 512), (50, 10, 256), (100, 20, 32),
                                                  (30, 7, 256)])
def test_records_equal_the_twin(jobs, machines, probes, lb):
    m = gen(jobs, machines, 100 + jobs + machines, lb)
    d, t = check(m, incumbent(m), probes)
    assert t["depth"] > 1.0  # the probes do walk
    if jobs >= 50:  # weights beyond 2^53 round at every level: w * k then est + w, never one fma
        assert t["records"]["est"].max() > 2.0**60


@pytest.mark.parametrize("lb", [0, 2])
@pytest.mark.parametrize("jobs", [63, 64, 65])
def test_lane_passes_and_set_words(jobs, lb):
    m = gen(jobs, 5, 7 * jobs, lb)
    check(m, incumbent(m), 64)


@pytest.mark.parametrize("jobs,machines,probes", [(129, 10, 32), (257, 5, 16)])
def test_many_set_words_lb1(jobs, machines, probes):
    m = gen(jobs, machines, jobs, 1)
    d, t = check(m, incumbent(m), probes)
    assert t["records"]["jobs"].max() >= 128  # jobs of the third word and beyond are chosen


def test_ta056_lb2():
    m = PfspModel(56, 2)
    d, t = check(m, m.best_known, 256)
    assert d["launch"]["waves"] == 4 and d["launch"]["lds_bytes"] <= 65536


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_ta014(lb):
    m = PfspModel(14, lb)
    check(m, m.best_known, 2048)


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_tiny_and_empty(lb):
    d1, _ = check(gen(1, 3, 3, lb), INT_MAX, 10)
    assert d1["tree"] == 0.0 and d1["per_level"] == []
    d2, _ = check(gen(2, 3, 3, lb), INT_MAX, 10)
    assert (d2["records"]["est"] == 2.0).all()
    m = gen(10, 5, 9, lb)
    C = ops.cpu()
    lo = min(C.lb1_children(C.PfspInstance.from_matrix(10, 5, m.p), list(range(10)), 0))
    d0, _ = check(m, lo, 70)  # LB2 >= LB1, so no root child survives under any bound
    assert d0["tree"] == 0.0 and (d0["records"]["depth"] == 0).all()


@pytest.mark.parametrize("lb", [0, 2])
def test_unpruned_20_jobs_beyond_2_53(lb):
    # 20 jobs, nothing pruned: est passes 2^53 at level 17 and its additions round from there.
    # The weights themselves stay exact (20! / k! is 2^18 times a 43-bit odd number at most),
    # so a fused multiply-add rounds as two operations here; the contraction is caught where
    # the weights round too: the pruned trees of 50 jobs and more (test_records_equal_the_twin).
    m = gen(20, 5, 77, lb)
    d, t = check(m, INT_MAX, 64)
    assert (t["records"]["depth"] == 19).all() and t["records"]["est"].min() > 2.0**53
    assert len(set(t["records"]["est"].tolist())) == 1  # the same tree from every probe


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_probe_counts(n):
    m = PfspModel(14, 0)
    check(m, m.best_known, n)


def test_more_probes_than_one_grid_pass():
    m = PfspModel(14, 2)
    d, _ = check(m, m.best_known, 500, batch=500, max_blocks=3)
    assert d["launch"]["grid"] * d["launch"]["waves"] < 500 and d["launch"]["launches"] == 1


def test_first_launch_is_one_grid_pass_and_sizes_the_rest():
    m = PfspModel(14, 0)
    d, _ = check(m, m.best_known, 300, max_blocks=2)
    la = d["launch"]
    assert la["grid"] == 2 and la["launches"] >= 2 and la["rate"] > 0 and 0 < la["first_seconds"] < 1.0
    assert la["batch"] == max(1, min(1 << 22, int(la["rate"] * 0.2)))  # from the rate alone, above or below 8
    full = device(m, m.best_known, 300)["launch"]
    assert full["grid"] * full["waves"] >= 300 and full["launches"] == 1  # within the first pass


def test_100x20_lb2_runs_two_waves_and_larger_lb2_raises():
    m = gen(100, 20, 220, 2)
    assert device(m, incumbent(m), 4)["launch"]["waves"] == 2
    for jobs in (200, 500):  # the Johnson orders alone pass 64 KB: refused, never read from elsewhere
        with pytest.raises(ValueError, match="LB2 tables"):
            device(gen(jobs, 20, jobs, 2), INT_MAX, 4)


@pytest.mark.parametrize("jobs,machines,lb", [(500, 20, 0), (200, 20, 1), (200, 10, 2)])
def test_largest_accepted_shapes(jobs, machines, lb):
    # 500 x 20 LB1_d: eight set words and the largest tables that fit (42 KB of cum, 4 waves)
    m = gen(jobs, machines, jobs + machines, lb)
    d, t = check(m, incumbent(m), 8)
    assert t["depth"] > 1.0


def test_first_probe_split_and_batches():
    m = PfspModel(14, 0)
    best, n = m.best_known, 1000
    whole = twin(m, best, n)
    lo, hi = device(m, best, 400), device(m, best, 600, first=400)
    for k in ("est", "depth", "jobs"):
        assert (np.concatenate([lo["records"][k], hi["records"][k]]) == whole["records"][k]).all()
    same_records(hi, twin(m, best, 600, first=400))
    small = device(m, best, n, batch=64)
    assert small["launch"]["launches"] == 16 and small["launch"]["batch"] == 64
    same_records(small, whole)
    close_aggregates(small, whole, n)
    close_aggregates(small, device(m, best, n), n)


@pytest.mark.parametrize("lb", [0, 1, 2])
@pytest.mark.parametrize("make", [tl.near_limit, tl.over_limit])
@pytest.mark.parametrize("jobs,machines", [(20, 10), (50, 20)])
def test_value_range_equals_the_twin_or_raises(jobs, machines, make, lb):
    m = from_matrix(make(jobs, machines, 5), lb, (make.__name__, jobs, machines))
    best = incumbent(m)
    try:
        d = device(m, best, 48)
    except ValueError:
        return
    same_records(d, twin(m, best, 48))


def test_values_beyond_31_bits_raise():
    p = tl.synthetic(20, 5, 1).astype(np.int64) * 150000  # three times the sum of p passes 2^31
    assert 3 * int(p.sum()) > INT_MAX > int(p.sum())
    m = from_matrix(p, 0, "huge")
    with pytest.raises(ValueError, match="too large"):
        device(m, INT_MAX, 4)
    with pytest.raises(ValueError):
        ops.hip().tree_estimate(20, 65, [1] * (20 * 65), 0, INT_MAX, 4, 1)  # machines


def test_estimate_tree_interface():
    m = PfspModel(14, 0)
    a = estimate_tree(m, probes=512, seed=5, device=0)
    b = estimate_tree(m, probes=512, seed=5, device=None)
    assert set(a) == set(b)
    assert a["best"] == b["best"] == m.best_known and a["device"] == 0 and b["device"] is None
    close_aggregates(a, b, 512)
    assert a["launch"]["batch"] >= 1 and a["launch"]["rate"] > 0


def test_cli_estimates_on_the_device(tmp_path, capsys):
    import json

    from dist_gpu_accelerated_tree_search_amd import cli

    out = tmp_path / "e.json"
    assert cli.main(["pfsp", "-i", "14", "-l", "2", "-D", "1", "--estimate", "2048", "--estimate-seed", "9",
                     "--no-csv", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert "on the device 0" in text and "Estimated nodes per level:" in text
    rec = json.loads(out.read_text().splitlines()[-1])
    m = PfspModel(14, 2)
    t = ops.cpu().tree_estimate_indexed(m, m.best_known, 2048, 9)
    assert rec["device"] == 0 and rec["n_gpus"] == 1 and rec["probes"] == 2048
    close_aggregates(rec, t, 2048)
