"""The two timing entry points (pfsp_expand_time: one LB2 expand iteration, pfsp_front_time:
one front-kernel iteration): the structure of what they return, never a time, and that a
timing call leaves no state behind for the next probe."""
import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel
from dist_gpu_accelerated_tree_search_amd.utils import nodes as nd

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1


def _parents(jobs, n, seed, leaf_parents=3):
    # as test_gpu_lb1_expand.py builds them
    rng = np.random.default_rng(seed)
    depths = rng.integers(0, jobs - 1, size=n)
    depths[:leaf_parents] = jobs - 1  # parents whose children are leaves
    perms = np.stack([rng.permutation(jobs) for _ in range(n)])
    return nd.pfsp_pack(depths, perms, jobs)


@pytest.mark.parametrize("variant", [1, 2])
def test_expand_time_structure_and_no_state_left(variant):
    model = PfspModel(1, 2)  # ta001, 20 x 5
    nodes = _parents(model.jobs, 40, 1)
    best = int(np.median(model.child_bounds_cpu(nodes, INT_MAX)))
    H = ops.require_gpu(0)
    args = (model.jobs, model.machines, list(model.native.p), 2, nodes, best, 0, variant)
    before = H.pfsp_expand_probe(*args)
    t = H.pfsp_expand_time(*args, 2)
    after = H.pfsp_expand_probe(*args)
    assert set(t) == {"ms_min", "ms_median", "clk_a", "clk_b1", "clk_b2", "clk_c", "chunks", "clk_block_max",
                      "clk_block_mean", "grid", "timeline_us"}
    assert 0 < t["ms_min"] <= t["ms_median"]
    assert t["grid"] >= 1
    assert t["timeline_us"].shape == (t["grid"], 3)
    assert np.array_equal(before, after)


@pytest.mark.parametrize("knobs", [{}, {"local_min": 1, "local_steps": 2}], ids=["defaults", "local_dfs"])
def test_front_time_structure(knobs):
    model = PfspModel(14, 1)  # ta014, 20 x 10
    best = model.best_known
    nodes = ops.cpu().pfsp_bfs_level(model.native, model.host_lb, best, 3)
    assert len(nodes) > 0
    t = ops.require_gpu(0).pfsp_front_time(model.jobs, model.machines, list(model.native.p), 1, nodes, best,
                                           max_parents=4096, reps=2, dyn_us=0, **knobs)
    assert 0 < t["ms_min"] <= t["ms_median"]
    assert t["grid"] >= 1
    assert t["nch_out"] >= 1
    st = t["stamps_us"]
    assert st.shape == (t["grid"], 16)
    assert np.any((st[:, 15] > 0) & (st[:, 15] >= st[:, 0]))
