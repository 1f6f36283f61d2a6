"""What the front kernel WRITES (the bounds probe checks what it evaluates).

`pfsp_front_expand_probe` runs exactly one front-kernel iteration of a requested shape
over given parents with a given incumbent and returns each output chunk's nodes in the
order the kernel laid them out. Expected children come from the host: which children
survive from `pfsp_children_bounds` (PfspFrontProblem, ref add_front_and_bound), the child
nodes from the max-plus chain of the parent's front (`children_of`, itself checked
against `pfsp_bfs_level` without a GPU).

One level per kernel and local DFS with one step: byte for byte and in order — chunk by
chunk, parents in order, jobs ascending (ref generate_children, PFSP_lib.h:51-95). Local
DFS with several steps: the stack each chunk leaves as a multiset, the nodes it pushed
and expanded itself, leaves and incumbent, against a host replay of the chunk's steps.

The cases aim at the wave-balanced emit (front_emit_balanced): one survivor per lane and
round, descriptors in windows of 256 per wave, parents fetched across lanes.
"""
import functools

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops
from dist_gpu_accelerated_tree_search_amd.models.pfsp import PfspModel

INT_MAX = 2**31 - 1
BP = 256          # parents per chunk (FrontGeom::BP)
SLOT = 2 * BP * 20  # 20-job chunk slot region (FrontGeom::SLOT)


# ---- host side -------------------------------------------------------------------------

def layout(model):
    """(offset of the job set, its bytes, offset of the fronts, machine bucket)."""
    mb = 8 if model.jobs > 20 else 4
    bucket = 5 if model.machines <= 5 else 10 if model.machines <= 10 else 20
    return mb, mb, 2 * mb, bucket


def unpack(model, nodes):
    ro, rb, fo, bucket = layout(model)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint8)
    depth = nodes[:, 0].astype(np.int64)
    rest = nodes[:, ro:ro + rb].copy().view("<u4" if rb == 4 else "<u8").reshape(-1).astype(np.uint64)
    front = nodes[:, fo:fo + 2 * bucket].copy().view("<u2").reshape(len(nodes), bucket).astype(np.int64)
    return depth, rest, front


def pack(model, depth, rest, front):
    ro, rb, fo, bucket = layout(model)
    out = np.zeros((len(depth), model.node_bytes), dtype=np.uint8)
    out[:, 0] = depth
    out[:, ro:ro + rb] = np.asarray(rest, dtype="<u4" if rb == 4 else "<u8").reshape(-1, 1).view(np.uint8)
    out[:, fo:fo + 2 * bucket] = np.ascontiguousarray(front, dtype="<u2").view(np.uint8)
    return out


def ptable(model):
    _, _, _, bucket = layout(model)
    p = np.zeros((model.jobs, bucket), dtype=np.int64)  # job-major, padded machines 0
    p[:, :model.machines] = np.asarray(model.native.p, dtype=np.int64).reshape(model.machines, model.jobs).T
    return p


def child_bounds(model, nodes):
    """Per parent: (jobs ascending, their child bounds)."""
    _, rest, _ = unpack(model, nodes)
    flat = np.asarray(ops.cpu().pfsp_children_bounds(model.native, model.lb,
                                                     np.ascontiguousarray(nodes, dtype=np.uint8)), dtype=np.int64)
    out, at = [], 0
    for r in rest:
        jobs = [j for j in range(model.jobs) if (int(r) >> j) & 1]
        out.append((jobs, flat[at:at + len(jobs)]))
        at += len(jobs)
    assert at == len(flat)
    return out


def children_of(model, nodes, best):
    """One expansion of `nodes` in order: (surviving children, parents in order and jobs
    ascending; leaves evaluated; the lowest leaf bound or None; survivors per parent)."""
    depth, rest, front = unpack(model, nodes)
    p = ptable(model)
    cd, cr, cf, per = [], [], [], []
    leaves, low = 0, None
    for i, (jobs, lbs) in enumerate(child_bounds(model, nodes)):
        if depth[i] + 1 == model.jobs:
            leaves += len(jobs)
            if len(lbs):
                low = int(lbs.min()) if low is None else min(low, int(lbs.min()))
            per.append(0)
            continue
        n = 0
        for j, lb in zip(jobs, lbs):
            if lb >= best:
                continue
            f = np.zeros(front.shape[1], dtype=np.int64)
            src = np.zeros_like(f) if depth[i] == 0 else front[i]  # a root's front holds the minimum heads
            t = 0
            for m in range(len(f)):
                t = max(t, src[m]) + p[j, m]
                f[m] = t
            cd.append(depth[i] + 1)
            cr.append(int(rest[i]) & ~(1 << j))
            cf.append(f)
            n += 1
        per.append(n)
    kids = pack(model, np.asarray(cd, dtype=np.int64), np.asarray(cr, dtype=np.uint64),
                np.asarray(cf, dtype=np.int64).reshape(len(cd), front.shape[1]))
    return kids, leaves, low, np.asarray(per, dtype=np.int64)


def replay_local(model, parents, best, steps, slot):
    """Host replay of one chunk's local DFS (front_local): its stack left, the nodes it
    pushed, the leaves it evaluated."""
    stack = np.zeros((0, model.node_bytes), dtype=np.uint8)
    pushed = leaves = 0
    cur = parents
    for s in range(steps):
        if s > 0:
            if len(stack) == 0:
                break
            npop = min(len(stack), BP)
            cur, stack = stack[len(stack) - npop:], stack[:len(stack) - npop]
        kids, lf, _, _ = children_of(model, cur, best)
        stack = np.concatenate([stack, kids])
        pushed += len(kids)
        leaves += lf
        if not (s + 1 < steps and len(stack) > 0 and len(stack) + BP * (20 if model.jobs <= 20 else 50) <= slot):
            break
    return stack, pushed, leaves


@functools.lru_cache(maxsize=None)
def model_of(inst, lb=1):
    return PfspModel(inst, lb)


@functools.lru_cache(maxsize=None)
def level(inst, depth, best, lb=1):
    m = model_of(inst, lb)
    return ops.cpu().pfsp_bfs_level(m.native, m.lb, int(best), depth)


def leaf_parents(model, n, seed=5):
    """n nodes of depth jobs - 1 (one unscheduled job each) from random prefixes."""
    rng = np.random.default_rng(seed)
    p = ptable(model)
    _, _, _, bucket = layout(model)
    d, r, f = [], [], []
    for _ in range(n):
        perm = rng.permutation(model.jobs)
        fr = np.zeros(bucket, dtype=np.int64)
        for j in perm[:-1]:
            t = 0
            for m in range(bucket):
                t = max(t, fr[m]) + p[j, m]
                fr[m] = t
        d.append(model.jobs - 1)
        r.append(1 << int(perm[-1]))
        f.append(fr)
    return pack(model, np.asarray(d), np.asarray(r, dtype=np.uint64), np.asarray(f))


# ---- the host expectation itself (no GPU) ----------------------------------------------

@pytest.mark.parametrize("inst,depth", [(14, 1), (14, 4), (21, 2), (31, 2)])
def test_children_of_reproduces_the_host_levels(inst, depth):
    m = model_of(inst)
    best = m.best_known
    cur = level(inst, depth, best)
    kids, _, _, per = children_of(m, cur[:300], best)
    nxt = level(inst, depth + 1, best)
    assert per.sum() == len(kids) > 0
    assert np.array_equal(kids, nxt[:len(kids)])


# ---- the device ------------------------------------------------------------------------

def expand(model, parents, best, steps):
    H = ops.require_gpu(0)
    return H.pfsp_front_expand_probe(model.jobs, model.machines, list(model.native.p), model.lb,
                                     np.ascontiguousarray(parents, dtype=np.uint8), int(best), steps=steps)


def check_one_step(model, parents, best, steps):
    """steps 0 (one level per kernel) or 1 (local DFS, one step): byte for byte, in order."""
    r = expand(model, parents, best, steps)
    bp = r["bp"]
    assert bp == (BP if steps == 0 else min(BP, -(-len(parents) // -(-len(parents) // BP))))
    exp_leaves, exp_low, at = 0, None, 0
    assert len(r["counts"]) == -(-len(parents) // bp)
    for c, cnt in enumerate(r["counts"]):
        kids, lf, low, _ = children_of(model, parents[c * bp:(c + 1) * bp], best)
        got = r["children"][at:at + cnt]
        print(f"chunk {c}: {cnt} nodes written, {len(kids)} expected")
        assert cnt == len(kids), (c, cnt, len(kids))
        bad = np.flatnonzero((got != kids).any(axis=1))
        assert bad.size == 0, (c, int(bad[0]), got[bad[0]].tolist(), kids[bad[0]].tolist())
        assert r["inner"][c] == 0
        at += cnt
        exp_leaves += lf
        if low is not None:
            exp_low = low if exp_low is None else min(exp_low, low)
    assert at == len(r["children"])
    assert r["leaves"] == exp_leaves
    assert r["best"] == (min(best, exp_low) if exp_low is not None else best)
    return r


gpu = pytest.mark.gpu
SHAPES = [0, 1]


@gpu
@pytest.mark.parametrize("steps", SHAPES)
def test_one_parent_root(steps):
    # 20 survivors from a single lane
    m = model_of(14)
    r = check_one_step(m, m.root(), INT_MAX, steps)
    assert r["counts"] == [20]


@gpu
@pytest.mark.parametrize("steps", SHAPES)
def test_overflowing_wave(steps):
    # 64 depth-1 parents (the 20 there are, repeated), no incumbent: every lane has 19
    # survivors, 1216 in the wave — five descriptor windows of 256
    m = model_of(14)
    lv = level(14, 1, INT_MAX)
    assert len(lv) == 20
    r = check_one_step(m, lv[np.arange(64) % 20], INT_MAX, steps)
    assert r["counts"] == [64 * 19]


@gpu
@pytest.mark.parametrize("steps", SHAPES)
@pytest.mark.parametrize("n", [65, 70])
def test_second_wave_nearly_empty(n, steps):
    m = model_of(14)
    check_one_step(m, level(14, 10, m.best_known)[1000:1000 + n], m.best_known, steps)


@gpu
@pytest.mark.parametrize("steps", SHAPES)
def test_two_chunks_last_partial(steps):
    # a typical mix of a wide level: many lanes without a survivor
    m = model_of(14)
    parents = level(14, 10, m.best_known)[5000:5259]
    _, _, _, per = children_of(m, parents, m.best_known)
    assert (per == 0).sum() > 20 and per.max() >= 4
    r = check_one_step(m, parents, m.best_known, steps)
    assert len(r["counts"]) == 2


def wave_with_total(model, pool, best, total):
    """64 parents of `pool` whose survivors sum to `total`, the owners of the last
    survivors in the highest lanes (the low lanes hold parents without a survivor)."""
    _, _, _, per = children_of(model, pool, best)
    zeros = np.flatnonzero(per == 0)
    pick, left = [], total
    for i in np.flatnonzero(per > 0):
        if per[i] <= left:
            pick.append(i)
            left -= per[i]
        if left == 0:
            break
    assert left == 0 and len(pick) < 64 and len(zeros) >= 64 - len(pick)
    idx = np.concatenate([zeros[:64 - len(pick)], np.asarray(pick, dtype=np.int64)])
    assert per[idx].sum() == total and per[idx[-1]] > 0
    return idx


@gpu
@pytest.mark.parametrize("steps", SHAPES)
@pytest.mark.parametrize("total", [64, 65])
def test_wave_total_exactly(total, steps):
    # the first wave's survivors fill exactly one round / one round and one lane; a second
    # wave of ordinary parents follows
    m = model_of(14)
    pool = level(14, 10, m.best_known)[:1500]
    idx = wave_with_total(m, pool, m.best_known, total)
    rest = np.setdiff1d(np.arange(200), idx)[:40]
    check_one_step(m, np.concatenate([pool[idx], pool[rest]]), m.best_known, steps)


@gpu
@pytest.mark.parametrize("steps", SHAPES)
def test_no_survivor(steps):
    m = model_of(14)
    r = check_one_step(m, level(14, 10, m.best_known)[:100], 1, steps)
    assert r["counts"] == [0] and len(r["children"]) == 0


@gpu
@pytest.mark.parametrize("steps", SHAPES)
def test_leaf_parents(steps):
    # depth 19: nothing emitted, one leaf per parent counted, the incumbent lowered
    m = model_of(14)
    parents = leaf_parents(m, 70)
    r = check_one_step(m, parents, INT_MAX, steps)
    assert r["leaves"] == 70 and sum(r["counts"]) == 0 and r["best"] < INT_MAX


def bucket_case(name):
    if name == "syn14x7":
        m = PfspModel.synthetic(14, 7, seed=3, lb=1)
        lv = ops.cpu().pfsp_bfs_level(m.native, m.lb, INT_MAX, 3)
    else:
        inst, depth = {"ta001": (1, 3), "ta021": (21, 3), "ta031": (31, 2)}[name]
        m = model_of(inst)
        lv = level(inst, depth, INT_MAX)
    parents = lv[:600]
    # an incumbent that prunes about half of the children: the median child bound
    best = int(np.median(np.concatenate([lbs for _, lbs in child_bounds(m, parents)])))
    return m, parents, best


@gpu
@pytest.mark.parametrize("steps", SHAPES)
@pytest.mark.parametrize("name", ["ta001", "ta021", "ta031", "syn14x7"])
def test_other_buckets(name, steps):
    # 5 machines, 20 machines (per-lane emit), 50 jobs (64-bit sets), padded machines
    m, parents, best = bucket_case(name)
    assert 256 < len(parents) <= 600
    r = check_one_step(m, parents, best, steps)
    assert 0 < sum(r["counts"]) < sum(len(j) for j, _ in child_bounds(m, parents))


@gpu
@pytest.mark.parametrize("depth,steps", [(10, 3), (17, 4)])
def test_local_dfs_several_steps(depth, steps):
    # the stack each chunk leaves (multiset), what it pushed and expanded itself, leaves
    # and incumbent; from depth 17 the last steps reach the leaves
    m = model_of(14)
    best = m.best_known
    parents = level(14, depth, best)[2000:2259]
    r = expand(m, parents, best, steps)
    bp = r["bp"]
    assert bp == 130 and len(r["counts"]) == 2
    at = leaves = 0
    for c, cnt in enumerate(r["counts"]):
        stack, pushed, lf = replay_local(m, parents[c * bp:(c + 1) * bp], best, steps, SLOT)
        got = r["children"][at:at + cnt]
        print(f"chunk {c}: stack {cnt} (expected {len(stack)}), inner {r['inner'][c]} (expected {pushed - len(stack)})")
        assert cnt == len(stack)
        assert r["inner"][c] == pushed - len(stack)
        key = lambda a: sorted(map(bytes, a))  # noqa: E731
        assert key(got) == key(stack)
        at += cnt
        leaves += lf
    assert r["leaves"] == leaves
    assert r["best"] == best
    if depth == 17:
        assert leaves > 0
