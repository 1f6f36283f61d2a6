"""Host twin of the device tree-size estimator (csrc/core/estimate.hpp knuth_estimate_indexed,
csrc/core/probe_rng.hpp): the choices are a pure function of (seed, probe, level), the
estimate is Knuth's, and nothing depends on threads or on how the probes are split."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import PfspModel, estimate_tree, ops
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


def pick(seed, probe, level, k):
    """csrc/core/probe_rng.hpp, rebuilt from its header comment."""
    h = mix((seed + G * (probe + 1)) & M64)
    r = mix((h + G * (level + 1)) & M64)
    return ((r >> 32) * k) >> 32


def twin(model, best, probes, seed, **kw):
    return ops.cpu().tree_estimate_indexed(model, int(best), probes, seed, **kw)


def small(jobs, machines, seed=3, lb=0):
    """A stand-in model (jobs, machines, lb, machine-major p): the only way to one job."""
    p = tl.synthetic(max(jobs, 2), machines, seed)[:, :jobs]
    return SimpleNamespace(jobs=jobs, machines=machines, lb=lb, p=p.reshape(-1).tolist(), kind="pfsp",
                           best_known=INT_MAX)


def test_choices_are_the_documented_formula():
    # best = INT_MAX: every child survives, so the survivors are the unscheduled jobs in
    # ascending order and the chosen job follows from the formula alone
    m = PfspModel.synthetic(8, 3, 5, lb=0)
    seed, first = 11, 40
    r = twin(m, INT_MAX, 64, seed, first_probe=first, records=True)["records"]
    for i in range(64):
        rest = list(range(8))
        for lvl in range(7):
            j = rest.pop(pick(seed, first + i, lvl, len(rest)))
            assert r["jobs"][i, lvl] == j, (i, lvl)
        assert r["jobs"][i, 7] == -1


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_unpruned_tree_is_exact(lb):
    m = PfspModel.synthetic(8, 3, 5, lb=lb)
    e = twin(m, INT_MAX, 100, 1, records=True)
    want = sum(40320 // int(np.prod(range(1, 8 - d + 1))) for d in range(1, 8))
    assert want == 69280
    assert (e["records"]["est"] == 69280.0).all() and (e["records"]["depth"] == 7).all()
    assert e["tree"] == 69280.0 and e["stderr"] == 0.0 and e["depth"] == 7.0
    assert e["per_level"] == [8.0, 56.0, 336.0, 1680.0, 6720.0, 20160.0, 40320.0]


@pytest.mark.parametrize("lb", [0, 1, 2])
def test_one_and_two_jobs(lb):
    e1 = twin(small(1, 3, lb=lb), INT_MAX, 10, 1, records=True)
    assert e1["tree"] == 0.0 and (e1["records"]["depth"] == 0).all() and e1["per_level"] == []
    e2 = twin(small(2, 3, lb=lb), INT_MAX, 10, 1, records=True)
    assert (e2["records"]["est"] == 2.0).all() and (e2["records"]["depth"] == 1).all()
    assert e2["tree"] == 2.0 and e2["per_level"] == [2.0]


def test_empty_root():
    m = PfspModel.synthetic(10, 5, 9, lb=0)
    lo = min(ops.cpu().lb1_children(m.native, list(range(10)), 0))
    for best in (lo, lo - 1):
        e = twin(m, best, 50, 2, records=True)
        assert e["tree"] == 0.0 and e["depth"] == 0.0 and (e["records"]["jobs"] == -1).all()
    assert twin(m, lo + 1, 50, 2)["tree"] > 0.0


def test_threads_and_splits_change_nothing():
    m = PfspModel(14, 0)
    a = twin(m, m.best_known, 3000, 4, threads=1, records=True)
    for t in (3, 6):
        b = twin(m, m.best_known, 3000, 4, threads=t, records=True)
        assert {k: b[k] for k in ("tree", "stderr", "depth", "per_level")} == \
               {k: a[k] for k in ("tree", "stderr", "depth", "per_level")}
        for k in ("est", "depth", "jobs"):
            assert (a["records"][k] == b["records"][k]).all()
    whole = twin(m, m.best_known, 1000, 4, records=True)["records"]
    lo = twin(m, m.best_known, 500, 4, records=True)["records"]
    hi = twin(m, m.best_known, 500, 4, first_probe=500, records=True)["records"]
    for k in ("est", "depth", "jobs"):
        assert (whole[k] == np.concatenate([lo[k], hi[k]])).all()


def test_mean_is_the_exact_tree_of_a_small_instance():
    # 6 jobs: the host solver gives the -u 1 tree exactly (the incumbent is the optimum, so
    # it never moves and the explored tree is the one the probes sample)
    C = ops.cpu()
    m = PfspModel.synthetic(6, 4, 21, lb=0)
    opt = C.run_pfsp(m.native, 0, INT_MAX, threads=0)["best"]
    exact = C.run_pfsp(m.native, 0, opt, threads=0)["tree"]
    e = twin(m, opt, 200000, 12345, threads=4)
    assert exact > 6 and e["stderr"] > 0
    assert abs(e["tree"] - exact) <= 4 * e["stderr"], (e["tree"], exact, e["stderr"])


def test_ta014_bracket_and_first_level():
    m = PfspModel(14, 0)
    e = twin(m, m.best_known, 200000, 12345, threads=6)
    assert 0.5 * 2573652 < e["tree"] < 2.0 * 2573652, e["tree"]
    assert e["per_level"][0] == float(len(m.warmup(m.best_known, 2)[0]))


def test_estimate_tree_host_and_cli(tmp_path, capsys):
    from dist_gpu_accelerated_tree_search_amd import cli

    m = PfspModel(14, 0)
    e = estimate_tree(m, probes=1000, seed=3, device=None)
    assert e["best"] == m.best_known and e["probes"] == 1000 and e["launch"] is None
    assert e["tree"] == twin(m, m.best_known, 1000, 3)["tree"]
    out = tmp_path / "e.json"
    assert cli.main(["pfsp", "-i", "14", "-l", "0", "-D", "0", "--estimate", "1000", "--estimate-seed", "3",
                     "--no-csv", "--json", str(out)]) == 0
    text = capsys.readouterr().out
    assert "Knuth tree-size estimate of ta14" in text and "Mean probe depth" in text
    assert "Size of the explored tree:" not in text  # no search ran
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["estimate"] is True and rec["probes"] == 1000 and rec["tree"] == e["tree"]
    assert rec["per_level"] == e["per_level"] and rec["inst"] == 14


def test_records_are_capped():
    m = PfspModel.synthetic(8, 3, 5, lb=0)
    with pytest.raises(ValueError, match="records"):
        twin(m, INT_MAX, (1 << 20) + 1, 1, records=True)
    with pytest.raises(ValueError, match="records"):
        twin(small(300, 3), 0, 1 << 18, 1, records=True)  # 2^18 probes x 300 jobs pass 2^26 cells
