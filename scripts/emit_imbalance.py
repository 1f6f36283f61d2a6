"""Emit imbalance of the front kernel's per-lane survivor loop, from the tree alone.

    python scripts/emit_imbalance.py [--inst 14] [--depths 8-16]

Rebuilds the LB1 tree of a 20-job Taillard instance (default ta014, incumbent = best
known, the headline's -u 1) level by level in numpy, then groups consecutive parents of
each level into waves of 64 as the kernel's thread-per-parent steps do, and prints per
depth:
  * pair passes per wave: ceil(unscheduled jobs / 2), uniform across a wave;
  * emit iterations per wave of the per-lane loop: the largest survivor count of a lane;
  * rounds of the wave-balanced emit: ceil(wave survivors / 64).
No GPU, numpy and utils/taillard.py only; a few seconds. (The kernel's waves hold the
parents of a workgroup's stack top, not a level's consecutive nodes: the table is the
shape of the imbalance, not a count of executed instructions.)
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from dist_gpu_accelerated_tree_search_amd.utils import taillard as tl  # noqa: E402


def expand(p, tails, depth, rest, front, best):
    """One level: survivors (parent-major, jobs ascending) and their count per parent.
    p is (jobs, machines); LB1 of a child = max_m(start_m + remain_m + tail_m)."""
    jobs, mach = p.shape
    n = len(rest)
    unsched = ((rest[:, None] >> np.arange(jobs)) & 1).astype(bool)          # (n, jobs)
    rt = unsched.astype(np.int64) @ p + tails                                 # remain + tail, (n, mach)
    surv = np.zeros((n, jobs), dtype=bool)
    leaves = 0
    for j in range(jobs):
        has = unsched[:, j]
        f = front[has]
        r = rt[has]
        lb = f[:, 0] + r[:, 0]
        tt = f[:, 0] + p[j, 0]
        for m in range(1, mach):
            sv = np.maximum(tt, f[:, m])
            lb = np.maximum(lb, sv + r[:, m])
            tt = sv + p[j, m]
        if depth + 1 == jobs:
            leaves += int(has.sum())
        else:
            surv[has, j] = lb < best
    pi, ji = np.nonzero(surv)
    src = front[pi] if depth > 0 else np.zeros((len(pi), mach), dtype=np.int64)  # the root's front: heads
    cf = np.empty_like(src)
    t = np.zeros(len(pi), dtype=np.int64)
    for m in range(mach):
        t = np.maximum(t, src[:, m]) + p[ji, m]
        cf[:, m] = t
    return rest[pi] & ~(np.int64(1) << ji), cf, surv.sum(axis=1), leaves


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inst", type=int, default=14)
    ap.add_argument("--depths", default="8-16")
    a = ap.parse_args()
    lo, hi = (int(x) for x in a.depths.split("-"))
    pm = np.asarray(tl.processing_times(a.inst), dtype=np.int64)  # (machines, jobs)
    p = pm.T.copy()
    jobs, mach = p.shape
    if jobs > 20:
        raise SystemExit("20-job instances only")
    best = tl.best_known(a.inst)
    heads = np.array([pm[:m].sum(axis=0).min() for m in range(mach)])
    tails = np.array([pm[m + 1:].sum(axis=0).min() for m in range(mach)])
    rest = np.array([(1 << jobs) - 1], dtype=np.int64)
    front = heads[None, :].astype(np.int64)
    tree = sol = 0
    rows = []
    for depth in range(jobs):
        nrest, nfront, per, leaves = expand(p, tails, depth, rest, front, best)
        sol += leaves
        tree += len(nrest)
        if lo <= depth <= hi:
            pad = (-len(per)) % 64
            w = np.concatenate([per, np.zeros(pad, dtype=per.dtype)]).reshape(-1, 64)
            rows.append((depth, len(per), per.mean(), (jobs - depth + 1) // 2, w.max(axis=1).mean(),
                         np.ceil(w.sum(axis=1) / 64).mean(), len(w)))
        rest, front = nrest, nfront
        if len(rest) == 0:
            break
    print(f"ta{a.inst:03d} LB1, incumbent {best}: tree {tree}, sol {sol}\n")
    print("| Depth | Parents | Survivors / parent | Pair passes / wave | Emit iterations / wave, per lane (max over lanes) "
          "| Balanced (ceil(wave survivors / 64)) |\n|---|---|---|---|---|---|")
    tp = te = tb = 0.0
    for d, n, s, pp, e, b, nw in rows:
        print(f"| {d} | {n:,} | {s:.2f} | {pp} | {e:.2f} | {b:.2f} |")
        tp += pp * nw
        te += e * nw
        tb += b * nw
    print(f"\nsummed over depths {lo}-{hi}: {tp / 1e3:.0f} K pair passes, {te / 1e3:.0f} K per-lane emit iterations, "
          f"{tb / 1e3:.0f} K balanced rounds ({te / max(tb, 1):.1f} x fewer)")


if __name__ == "__main__":
    main()
