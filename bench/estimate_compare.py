"""Measurements of the tree-size estimators (search.estimate_tree): Knuth against lookahead.

  cpu      host twin on trees that are known, equal wall time per run, independent seeds:
           median |log2(mean / gold)|, runs within 2x of gold, median relative standard error
  rate     device probes/s of both methods in alternating runs, with the first-launch seconds
  project  one long device estimate from several calls over consecutive probe ranges with
           records, so the largest single probe's share of the total is known

Each prints plain text; redirect it where the record is kept (profiles/).
"""
from __future__ import annotations

import argparse
import math
import statistics
import time

import numpy as np

from dist_gpu_accelerated_tree_search_amd import PfspModel, estimate_tree

KNOWN = [(14, 1, 2573652), (8, 0, 113458723), (21, 0, 260069628524)]  # (Taillard id, lb, -u 1 tree)
LB = {0: "LB1_d", 1: "LB1", 2: "LB2"}


def methods(lb):
    out = [("knuth", dict(method="knuth"))]
    for power in (1, 2, 3):
        for look in (("own", "lb1") if lb == 2 else ("own",)):
            out.append((f"lookahead e={power} look={look}", dict(method="lookahead", power=power, look=look)))
    return out


def cpu(a):
    print(f"Host twin, {a.threads} threads, {a.seeds} seeds per row, every run sized to {a.seconds} s from a pilot run's "
          f"rate; incumbent = best-known makespan (-u 1 tree).")
    for inst, lb, gold in KNOWN:
        m = PfspModel(inst, lb)
        print(f"\nta{inst:03d} {LB[lb]}  gold tree {gold}")
        print(f"  {'method':<28}{'probes/run':>12}{'s/run':>8}{'median |log2(mean/gold)|':>27}{'within 2x':>11}"
              f"{'median s.e./mean':>18}{'mean depth':>12}")
        for name, kw in methods(lb):
            estimate_tree(m, probes=1000, seed=998, device=None, threads=a.threads, **kw)  # one-time set-up
            probes = a.pilot  # pilot runs grow until one lasts a third of the target: thread start-up is no rate
            while True:
                pilot = estimate_tree(m, probes=probes, seed=999, device=None, threads=a.threads, **kw)
                if pilot["seconds"] >= a.seconds / 3:
                    break
                probes = int(probes * max(2.0, 0.5 * a.seconds / pilot["seconds"]))
            for _ in range(2):  # the first calls after an idle spell run slow: size from full-length runs
                probes = max(1000, int(pilot["probes_per_s"] * a.seconds))
                pilot = estimate_tree(m, probes=probes, seed=999, device=None, threads=a.threads, **kw)
            probes = max(1000, int(pilot["probes_per_s"] * a.seconds))
            err, rel, secs, depth = [], [], [], []
            for s in range(a.seeds):
                e = estimate_tree(m, probes=probes, seed=1000 + s, device=None, threads=a.threads, **kw)
                err.append(abs(math.log2(e["tree"] / gold)) if e["tree"] > 0 else float("inf"))
                rel.append(e["stderr"] / e["tree"] if e["tree"] > 0 else float("inf"))
                secs.append(e["seconds"])
                depth.append(e["depth"])
            print(f"  {name:<28}{probes:>12}{statistics.median(secs):>8.2f}{statistics.median(err):>27.3f}"
                  f"{sum(x <= 1.0 for x in err):>8}/{a.seeds}{statistics.median(rel):>18.3f}"
                  f"{statistics.mean(depth):>12.2f}", flush=True)


def one_rate(m, seconds, seed, kw, gauge):
    probes = max(1024, int(gauge * seconds))
    try:
        e = estimate_tree(m, probes=probes, seed=seed, device=0, **kw)
    except ValueError as x:
        return f"refused: {x}", None
    la = e["launch"]
    return (f"{e['probes_per_s']:.0f} probes/s  ({e['seconds']:.3f} s, {probes} probes, {la['launches']} launches of <= "
            f"{la['batch']} sized from {la['rate']:.0f} probes/s of a first launch of {la['first_seconds'] * 1e3:.1f} ms, "
            f"grid {la['grid']} x {la['waves']} waves, lds {la['lds_bytes']} B)  tree {e['tree']:.4g} +- {e['stderr']:.3g}"
            f"  depth {e['depth']:.2f}"), e["probes_per_s"]


def rate(a):
    print("Device estimators, alternating runs, three each, incumbent = best-known makespan. Rates are wall-clock of "
          "search.estimate_tree (table upload, launches, host reduction). The gauge call sizes the runs.")
    for inst, lb in ((21, 0), (56, 2)):
        m = PfspModel(inst, lb)
        rows = [("knuth", dict(method="knuth"))]
        rows += [(f"lookahead e={a.power} look={look}", dict(method="lookahead", power=a.power, look=look))
                 for look in (("lb1", "own") if lb == 2 else ("own",))]
        gauge = {}
        for name, kw in rows:
            try:
                estimate_tree(m, probes=256, seed=1, device=0, batch=256, **kw)  # loads the module, warms the kernel
                g = estimate_tree(m, probes=a.gauge, seed=1, device=0, **kw)
                gauge[name] = g["probes_per_s"]
                print(f"ta{inst:03d} {LB[lb]} {name} gauge: {g['probes_per_s']:.0f} probes/s over {a.gauge}; first launch "
                      f"{g['launch']['first_seconds'] * 1e3:.1f} ms", flush=True)
            except ValueError as x:
                print(f"ta{inst:03d} {LB[lb]} {name} gauge refused: {x}", flush=True)
        got = {name: [] for name in gauge}
        for run in range(3):
            for name, kw in rows:
                if name not in gauge:
                    continue
                text, r = one_rate(m, a.seconds, 100 + run, kw, gauge[name])
                print(f"  run {run} {name}: {text}", flush=True)
                if r:
                    got[name].append(r)
        for name, v in got.items():
            if v:
                print(f"ta{inst:03d} {LB[lb]} {name}: median {statistics.median(v):.0f} probes/s")


def project(a):
    m = PfspModel(a.inst, a.lb)
    kw = dict(method=a.method, power=a.power, look=a.look)
    estimate_tree(m, probes=256, seed=1, device=0, batch=256, **kw)
    g = estimate_tree(m, probes=a.gauge, seed=1, device=0, **kw)
    total = int(g["probes_per_s"] * a.seconds)
    chunk = 1 << 20
    est, depth, lvl, secs, done, launches = [], [], np.zeros(m.jobs), 0.0, 0, 0
    t0 = time.perf_counter()
    while done < total:
        n = min(chunk, total - done)
        e = estimate_tree(m, probes=n, seed=a.seed, device=0, first_probe=done, records=True, **kw)
        est.append(e["records"]["est"])
        depth.append(e["records"]["depth"])
        pl = np.asarray(e["per_level"])
        lvl[:len(pl)] += pl * n
        secs += e["launch"]["seconds"]
        launches += e["launch"]["launches"]
        done += n
    wall = time.perf_counter() - t0
    est, depth = np.concatenate(est), np.concatenate(depth)
    n = float(done)
    mean = est.sum() / n
    var = max(0.0, float((est * est).sum()) / n - mean * mean)
    print(f"ta{a.inst:03d} {LB[a.lb]} {a.method} power {a.power} look {a.look} seed {a.seed}: {done} probes, "
          f"{launches} launches taking {secs:.1f} s ({wall:.1f} s wall with records), gauge {g['probes_per_s']:.0f} probes/s")
    print(f"tree {mean:.4g} +- {math.sqrt(var / n):.3g} (s.e. / mean {math.sqrt(var / n) / mean:.3f}), "
          f"mean depth {depth.mean():.2f}, deepest {depth.max()}")
    top = np.sort(est)[::-1][:5]
    print(f"largest single probe {top[0]:.4g} = {top[0] / est.sum():.4f} of the sum; next four "
          + ", ".join(f"{x / est.sum():.4f}" for x in top[1:]))
    print("level  estimated nodes  probes reaching it")
    for d, v in enumerate(lvl / n):
        if v > 0:
            print(f"{d + 1:5d}  {v:.4g}  {(depth > d).sum()}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("cpu")
    c.add_argument("--threads", type=int, default=16)
    c.add_argument("--seeds", type=int, default=20)
    c.add_argument("--seconds", type=float, default=1.0)
    c.add_argument("--pilot", type=int, default=20000)
    c.set_defaults(f=cpu)
    r = sub.add_parser("rate")
    r.add_argument("--seconds", type=float, default=0.5)
    r.add_argument("--gauge", type=int, default=16384)
    r.add_argument("--power", type=int, default=2)
    r.set_defaults(f=rate)
    p = sub.add_parser("project")
    p.add_argument("--inst", type=int, default=56)
    p.add_argument("--lb", type=int, default=2)
    p.add_argument("--method", default="lookahead")
    p.add_argument("--power", type=int, default=2)
    p.add_argument("--look", default=None)
    p.add_argument("--seconds", type=float, default=46.0)
    p.add_argument("--gauge", type=int, default=16384)
    p.add_argument("--seed", type=int, default=2025)
    p.set_defaults(f=project)
    a = ap.parse_args(argv)
    a.f(a)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
