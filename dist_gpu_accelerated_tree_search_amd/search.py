"""Single-process search drivers (CPU sequential, CPU multi-core, one GPU).

The three-step structure of every reference driver is kept
(ref pfsp_multigpu_cuda.c:55-511, nqueens_gpu_cuda.cu:198-264):
  Step 1  host breadth-first warm-up until the pool holds `m` (x workers) nodes,
  Step 2  the parallel / device search,
  Step 3  host depth-first drain of whatever Step 2 leaves (nothing, on the GPU
          path: the device engine drains its pool completely).
Counting (tree / sol) and the -u incumbent rule are the reference's.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from . import ops
from .models.pfsp import EngineOptions
from .utils.report import WorkerStats

INT_MAX = 2**31 - 1


@dataclass
class SolveResult:
    best: int
    tree: int
    sol: int
    elapsed: float
    t_init: float = 0.0
    t_search: float = 0.0
    t_tail: float = 0.0
    workers: list = field(default_factory=list)
    extra: dict = field(default_factory=dict)
    # a time-limited solve that stopped with nodes still pooled (solve_engine time_limit):
    # complete False, open_nodes the pool left in the engine, lower_bound what the search
    # has proved (optimum >= lower_bound; a complete solve: == best). A run stopped early
    # without a pool bound (ranks under DistConfig time_limit_s / max_rounds): complete
    # False, lower_bound and gap None
    complete: bool = True
    lower_bound: int | None = None
    open_nodes: int = 0

    def __post_init__(self):
        if self.complete and self.lower_bound is None:
            self.lower_bound = self.best

    @property
    def nodes_per_sec(self) -> float:
        return self.tree / self.elapsed if self.elapsed > 0 else float("inf")

    @property
    def gap(self) -> float | None:
        """(best - lower_bound) / best: 0.0 when complete, None while no schedule is known."""
        if self.complete:
            return 0.0
        if self.best >= INT_MAX or self.lower_bound is None:
            return None
        return (self.best - self.lower_bound) / self.best


def progress_weights(model) -> list[float]:
    """w[d] = share of the search space below a node of depth d: 1 / (N (N-1) ... (N-d+1))
    for PFSP permutations (the root stands for all N! of them); for N-Queens the same
    with N rows. 1 - engine.pool_weight(w) is the explored fraction of the space —
    pruned subtrees count as explored — used to project a time to solution."""
    n = model.jobs if model.kind == "pfsp" else model.N
    w, x = [], 1.0
    for d in range(n + 1):
        w.append(x)
        x /= max(1, n - d)
    return w


def estimate_tree(model, best: int | None = None, probes: int = 1 << 16, seed: int = 1, device: int | None = 0,
                  first_probe: int = 0, threads: int = 1, records: bool = False, batch: int = 0,
                  method: str = "knuth", power: int = 2, look: str | None = None) -> dict:
    """Knuth estimate of the tree a PFSP search explores from a fixed incumbent `best`
    (None: model.best_known, the -u 1 tree), from `probes` random root-to-dead-end walks.

    method "knuth": a probe follows a surviving child uniformly. method "lookahead": it
    follows child c in proportion to (c's own surviving children) ** power, power 1, 2 or
    3, and reweights, so it never steps into a dead end one level down (unbiased as well,
    far less skewed; a probe costs about 1 + k child passes per level instead of 1).
    look is the bound that counts c's children: "own" (the model's) or "lb1"; None is own
    for lb 0/1 and lb1 for lb 2. power and look are ignored by "knuth" but still checked.

    device >= 0: the device estimator (csrc/hip/estimate_kernels.hpp, one wave per probe,
    bounded launches); device None: its host twin on `threads` threads
    (csrc/core/estimate.hpp knuth_estimate_indexed). Probe i of (seed, first_probe) is
    the same walk on both, so the two agree probe for probe and differ only in the order
    their sums are added. Returns tree, stderr, depth, probes, per_level (mean estimated
    nodes per level), best, device, seconds, probes_per_s and launch (the device's launch
    record: probes per launch and the rate that sized them; None on the host), method,
    power and look as used (look resolved), plus
    records (per-probe est, depth, jobs) when asked. N-Queens stays on
    ops.cpu().tree_estimate."""
    if getattr(model, "kind", "pfsp") != "pfsp":
        raise ValueError("estimate_tree is for PFSP models; N-Queens uses ops.cpu().tree_estimate")
    if method not in ("knuth", "lookahead"):
        raise ValueError(f"estimate method must be 'knuth' or 'lookahead', not {method!r}")
    if power not in (1, 2, 3):
        raise ValueError(f"estimate power must be 1, 2 or 3, not {power!r}")
    if look is None:
        look = "lb1" if int(model.lb) == 2 else "own"
    if look not in ("own", "lb1"):
        raise ValueError(f"estimate look must be 'own' or 'lb1', not {look!r}")
    how = dict(method=method, power=int(power), look=look)
    best = int(model.best_known if best is None else best)
    t0 = time.perf_counter()
    if device is None:
        r = dict(ops.cpu().tree_estimate_indexed(model, best, int(probes), int(seed), first_probe=int(first_probe),
                                                 threads=int(threads), records=bool(records), **how))
        r["launch"] = None
    else:
        H = ops.require_gpu(device)
        p = model.native.p if hasattr(model, "native") else model.p
        r = dict(H.tree_estimate(int(model.jobs), int(model.machines), [int(x) for x in p], int(model.lb), best,
                                 int(probes), int(seed), first_probe=int(first_probe), device=int(device),
                                 records=bool(records), batch=int(batch), **how))
    r.update(how)
    r["seconds"] = time.perf_counter() - t0
    r["probes_per_s"] = r["probes"] / r["seconds"] if r["seconds"] > 0 else float("inf")
    r["best"] = best
    r["device"] = device
    return r


def solve_cpu(model, ub: int = 1, threads: int = 0, m: int = 25, batch: int = 20000, steal_cap: int = 250000,
              ws: bool = True, verbose: bool = False) -> SolveResult:
    """threads == 0: sequential (ref pfsp_c.c / nqueens_c.c); >0: multi-core WS
    (ref pfsp_omp_c.c)."""
    C = ops.cpu()
    if model.kind == "pfsp":
        r = C.run_pfsp(model.native, model.lb, model.initial_best(ub), threads=threads, m=m, batch=batch,
                       steal_cap=steal_cap, ws=ws, verbose=verbose)
    else:
        r = C.run_queens(model.N, model.G, threads=threads, m=m, batch=batch, steal_cap=steal_cap, ws=ws,
                         verbose=verbose)
    return SolveResult(best=r["best"], tree=r["tree"], sol=r["sol"], elapsed=r["elapsed"], t_init=r["t_init"],
                       t_search=r["t_search"], t_tail=r["t_tail"],
                       workers=[WorkerStats.from_dict(w) for w in r["workers"]])


def solve_engine(model, engine, ub: int = 1, m: int = 25, best: int | None = None,
                 verbose: bool = False, time_limit: float | None = None) -> SolveResult:
    """One complete solve on an existing engine (GPU or CPU backend).

    The engine is reused across solves (allocation and graph capture are setup,
    like model initialisation); its counters are reset here.

    time_limit (seconds, PFSP): the engine search stops after it. If nodes remain, the
    host drain is skipped and the pool stays in the engine — the caller may resume with
    engine.run — and the result is complete False with open_nodes, lower_bound (min of
    the incumbent and engine.pool_bound()["lower"]: the optimum is proved >= it) and gap;
    extra["pool_bound"] holds the whole pool_bound dict."""
    if time_limit is not None and not time_limit > 0:
        raise ValueError("time_limit must be positive")
    t0 = time.perf_counter()
    best = model.search_best(ub) if best is None else best
    nodes, tree1, sol1, best = model.warmup(best, m)
    t1 = time.perf_counter()
    if verbose:
        from .utils.report import phase
        print(phase("Initial search on CPU completed", tree1, sol1, t1 - t0))
    if time_limit is None:
        st = engine.solve(nodes, int(best))  # reset + load + run to exhaustion, one native call
    else:
        engine.begin(nodes, int(best))
        engine.run(-1, float(time_limit), 0)
        st = engine.stats()
    launches = st["launches"]
    best = min(best, st["best"])
    t2 = time.perf_counter()
    tree, sol = tree1 + st["tree"], sol1 + st["sol"]
    if verbose:
        print(phase("Search on GPU completed", tree, sol, t2 - t1))
    # Step 3: the engine drains completely; anything left (none) goes to the host
    left = engine.size()
    bound = None
    if left and time_limit is not None:
        bound = engine.pool_bound()
    elif left:
        rest = engine.pop(left)
        tr, so, best = model.drain(best, rest)
        tree += tr
        sol += so
    t3 = time.perf_counter()
    if verbose:
        if bound is None:
            print(phase("Final on CPU completed", tree, sol, t3 - t2))
            print("\nExploration terminated.")
        else:  # (no host drain: the pool stays in the engine)
            print("\nExploration stopped.")
    w = WorkerStats(tree=st["tree"], sol=st["sol"], gen_child=st["tree"], t_memcpy=st["t_memcpy"],
                    t_malloc=st["t_malloc"], t_kernel=st["t_run"])
    r = SolveResult(best=best, tree=tree, sol=sol, elapsed=t3 - t0, t_init=t1 - t0, t_search=t2 - t1,
                    t_tail=t3 - t2, workers=[w], extra={"launches": launches, "iters": st["iters"],
                                                        "parents": st["parents"], "syncs": st["syncs"]})
    if bound is not None:
        r.complete = False
        r.open_nodes = int(left)
        r.lower_bound = min(int(best), int(bound["lower"]))
        r.extra["pool_bound"] = bound
    return r


def solve_gpu(model, ub: int = 1, device: int = 0, m: int = 25, opts: EngineOptions | None = None,
              verbose: bool = False, time_limit: float | None = None) -> SolveResult:
    """Single-GPU solve (ref pfsp_multigpu_cuda.c with -D 1 -C 0). time_limit: see
    solve_engine; an incomplete result keeps its engine in extra["engine"] (the open pool
    lives there: engine.run resumes it, engine.pool_bound re-evaluates it)."""
    eng = model.make_engine("gpu", device, opts)
    try:
        r = solve_engine(model, eng, ub=ub, m=m, verbose=verbose, time_limit=time_limit)
        if not r.complete:
            r.extra["engine"] = eng
        return r
    finally:
        del eng


def solve_workers(model, devices=(0,), cpu_threads: int = 0, ub: int = 1, m: int = 25, steal_cap: int = 250000,
                  ws: bool = True, opts: EngineOptions | None = None, engines=None, slice_min: float = 0.0005,
                  slice_max: float = 0.05, pin: bool = False, device_steals: bool = True, watchdog_s: float = 0.0,
                  faults: dict | None = None) -> SolveResult:
    """Several engines in ONE process — GPUs (`devices`, repeats allowed) plus an
    optional CPU worker with `cpu_threads` threads (-C 1) — driven by the native
    runner (csrc/core/runner.hpp), the analogue of ref pfsp_multigpu_cuda.c.
    Pass `engines` to reuse engines across solves.

    pin: pin each GPU's host thread to the CPUs of the GPU's NUMA node.
    device_steals: GPU -> GPU transfers through device staging (xGMI peer copies).
    watchdog_s / faults: stuck-phase reporting and fault injection
    ({"delay_us", "steal_fail_pct", "stall_worker", "stall_s", "seed"}; env
    TTS_FAULT_* / TTS_WATCHDOG_* also apply), see csrc/core/runner.hpp."""
    gpu = len(devices) > 0
    mod = ops.require_gpu(max(devices)) if gpu else ops.cpu()
    if engines is None:
        engines = [model.make_engine("gpu", d, opts) for d in devices]
        if cpu_threads > 0:
            engines.append(_cpu_worker(model, mod, cpu_threads, opts))
    W = len(engines)
    if W == 0:
        raise ValueError("no worker")
    t0 = time.perf_counter()
    best = model.search_best(ub)
    nodes, tree1, sol1, best = model.warmup(best, W * m)
    from .parallel.runtime import round_robin_share

    init = [np.ascontiguousarray(nodes[round_robin_share(len(nodes), w, W)]) for w in range(W)]
    # per-worker sharing thresholds: a GPU is needy below a quarter of its parent
    # window and donates from one window; a CPU worker keeps the reference's m / 2m
    # and receives at most 4*T nodes per steal (ref pfsp_multigpu_cuda.c:369-372)
    o = opts or EngineOptions()
    needy, donor, rcap = [], [], []
    for e in engines:
        if e.device >= 0:
            nb = max(m, int(o.max_parents) // 4)
            needy.append(nb)
            donor.append(max(2 * nb, int(o.max_parents)))
            rcap.append(steal_cap)
        else:
            needy.append(m)
            donor.append(2 * m)
            rcap.append(min(steal_cap, 4 * int(o.cpu_batch)))
    t1 = time.perf_counter()
    out = mod.run_workers(engines, init, int(best), m=m, steal_cap=steal_cap, slice_min=slice_min,
                          slice_max=slice_max, ws=ws, pin=pin, device_steals=device_steals,
                          watchdog_s=watchdog_s, faults=dict(faults or {}), needy_below=needy, donor_min=donor,
                          recv_cap=rcap)
    t2 = time.perf_counter()
    ws_ = out["workers"]
    tree = tree1 + sum(int(w["tree"]) for w in ws_)
    sol = sol1 + sum(int(w["sol"]) for w in ws_)
    workers = [WorkerStats(tree=int(w["tree"]), sol=int(w["sol"]), gen_child=int(w["tree"]),
                           steals=int(w["steals"]), success_steals=int(w["success_steals"]),
                           terminations=int(w["idle_rounds"]), t_memcpy=float(w["t_memcpy"]),
                           t_malloc=float(w["t_malloc"]), t_kernel=float(w["t_run_w"]),
                           t_pool_ops=float(w["t_comm"]), t_idle=float(w["t_idle"]),
                           t_termination=float(w["t_termination"])) for w in ws_]
    return SolveResult(best=min(int(best), int(out["best"])), tree=tree, sol=sol, elapsed=t2 - t0,
                       t_init=t1 - t0, t_search=t2 - t1, workers=workers,
                       extra={"rounds": max(int(w["rounds"]) for w in ws_), "engines": engines,
                              "sent_nodes": [int(w["sent"]) for w in ws_],
                              "device_transfers": sum(int(w["device_transfers"]) for w in ws_),
                              "dropped_transfers": sum(int(w["dropped_transfers"]) for w in ws_),
                              "watchdog_events": int(ws_[0]["watchdog_events"]),
                              "pinned": [bool(w["pinned"]) for w in ws_]})


def _cpu_worker(model, mod, threads: int, opts: EngineOptions | None):
    batch = (opts or EngineOptions()).cpu_batch
    if model.kind == "pfsp":
        return mod.make_pfsp_cpu_engine(model.jobs, model.machines, list(model.native.p), model.lb, batch, threads) \
            if hasattr(mod, "make_pfsp_engine") else mod.make_pfsp_cpu_engine(model.native, model.host_lb, batch,
                                                                              threads)
    return mod.make_queens_cpu_engine(model.N, model.G, batch, threads)
