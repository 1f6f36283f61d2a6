"""The device ring's host bookkeeping (csrc/core/pool_ring.hpp) against a plain Python model.

DeviceEngine (csrc/hip/engine.hpp) keeps the ring's host shadow and sizes its replays with
two small host-only types: PoolRing (where a run of ring slots lies, how `bot` and the stack
move when nodes are pushed on top, popped from the bottom or refilled under the bottom) and
ReplayPlan (the worst-case ring growth of a replay and which graph fits). One wrong term in
either loses or duplicates nodes on a GPU run that happens to wrap. The models below are
written out from the formulas the engine had inline before it used the two types; they share
no code with them.
"""
import itertools
import random
from collections import Counter, deque

import numpy as np
import pytest

from dist_gpu_accelerated_tree_search_amd import ops


def pieces(ring, cap, start, n):
    """ring.spans(start, n), each piece checked to lie inside the ring."""
    out = ring.spans(start, n)
    for off, cnt in out:
        assert cnt > 0 and off + cnt <= cap, (cap, start, n, out)
    return out


# ---------------------------------------------------------------- spans


@pytest.mark.parametrize("cap", [1, 2, 8, 64])
def test_spans_cover_the_run_in_order(cap):
    ring = ops.cpu().PoolRing(cap)
    for start, n in itertools.product(range(2 * cap), range(cap + 1)):
        got = pieces(ring, cap, start, n)
        assert [s for off, cnt in got for s in range(off, off + cnt)] == [(start + i) % cap for i in range(n)]
        assert len(got) <= 2
        if len(got) == 2:
            assert got[1][0] == 0
        if n == 0:
            assert got == []


def test_spans_of_a_large_ring():
    cap = 1 << 19
    ring = ops.cpu().PoolRing(cap)
    rng = random.Random(19)
    draws = [(rng.randrange(4 * cap), rng.randrange(cap + 1)) for _ in range(100)]
    # and short runs at both sides of the wrap
    draws += [(cap - rng.randrange(1, 70) + rng.choice((0, cap)), rng.randrange(0, 140)) for _ in range(2000)]
    draws += [(0, cap), (cap - 1, cap), (cap, 1), (cap - 1, 1), (cap - 1, 2), (2 * cap - 1, cap)]
    wrapped = 0
    for start, n in draws:
        got = pieces(ring, cap, start, n)
        slots = np.concatenate([np.arange(off, off + cnt) for off, cnt in got]) if got else np.arange(0)
        assert np.array_equal(slots, (start + np.arange(n)) % cap), (start, n, got)
        assert len(got) <= 2 and (len(got) < 2 or got[1][0] == 0) and (n > 0 or got == [])
        wrapped += len(got) == 2
    assert wrapped > 500


# ---------------------------------------------------------------- shadow


@pytest.mark.parametrize("cap", [8, 64])
def test_shadow_follows_a_random_run_of_the_engine_operations(cap):
    C = ops.cpu()
    rng = random.Random(cap)
    ring = C.PoolRing(cap)
    slots = [None] * cap  # the device ring
    ids = deque()  # what the pool holds, oldest first
    bot = stack = 0  # the shadow as engine.hpp updated it inline
    fresh = itertools.count()
    seen = Counter()

    def read(start, n):
        return [x for off, cnt in pieces(ring, cap, start, n) for x in slots[off : off + cnt]]

    for _ in range(20000):
        op = rng.choice(("push", "push", "pop", "refill", "refill", "export"))
        if op == "push":  # ring_write_top
            n = rng.randrange(cap + 1)
            if stack + n > cap:
                with pytest.raises(RuntimeError, match="device ring capacity exceeded"):
                    ring.push_top(n)
                seen["overfull"] += 1
            else:
                new = [next(fresh) for _ in range(n)]
                top = ring.top()
                assert top == bot + stack
                ring.push_top(n)
                i = 0
                for off, cnt in pieces(ring, cap, top, n):
                    slots[off : off + cnt] = new[i : i + cnt]
                    i += cnt
                assert i == n
                seen["push wraps"] += ((bot + stack) & (cap - 1)) + n > cap
                ids.extend(new)
                stack += n
        elif op == "pop":  # ring_read_bottom, spill_bottom, commit_spill_ahead
            n = rng.randrange(stack + 1)
            assert read(ring.bot, n) == [ids.popleft() for _ in range(n)]
            ring.pop_bottom(n)
            seen["pop wraps"] += bot + n > cap
            bot = (bot + n) & (cap - 1)
            stack -= n
        elif op == "refill":  # start_refill + fold_refill: one contiguous copy under the bottom
            assert ring.contiguous_under_bottom() == (bot if bot else cap)
            room = min(cap - stack, bot if bot else cap)
            if room == 0:
                continue
            k = rng.randrange(1, room + 1)
            dst = ring.under_bottom(k)
            assert dst == (bot + cap - k) & (cap - 1) and dst + k <= cap
            new = [next(fresh) for _ in range(k)]
            slots[dst : dst + k] = new
            ring.extend_bottom(k)
            seen["refill from slot 0"] += bot == 0
            ids.extendleft(reversed(new))
            bot = (bot + cap - k) & (cap - 1)
            stack += k
        else:  # export_ahead from bot + pending, once or more, then commit_export
            pending = 0
            for _ in range(rng.randrange(1, 4)):
                n = rng.randrange(stack - pending + 1)
                assert read(ring.bot + pending, n) == list(itertools.islice(ids, pending, pending + n))
                seen["export wraps"] += n > 0 and ((bot + pending) & (cap - 1)) + n > cap
                pending += n
            ring.pop_bottom(pending)
            for _ in range(pending):
                ids.popleft()
            bot = (bot + pending) & (cap - 1)
            stack -= pending
        assert (ring.bot, ring.stack) == (bot, stack)
        assert ring.bot < cap and ring.stack <= cap
        assert read(ring.bot, ring.stack) == list(ids)
    for what in ("overfull", "push wraps", "pop wraps", "refill from slot 0", "export wraps"):
        assert seen[what] > 50, seen
    ring.reset(3)
    assert (ring.bot, ring.stack, ring.top()) == (0, 3, 3)


# ---------------------------------------------------------------- replay plan

ITERS = (6, 48, 18)  # EngineConfig / EngineOptions iters_small, iters_large, iters_first
# (parents per chunk, children per chunk, chunks at most, node bytes) of the PFSP front engines:
# FrontGeom BP, SLOT = 2 * BP * NJ, MAXCHUNKS, sizeof(PfspFrontNode<M, NJ>)
FRONT = {
    "front20": (256, 2 * 256 * 20, 2048, 32),
    "front20 m20": (256, 2 * 256 * 20, 2048, 48),
    "front100": (256, 2 * 256 * 100, 2048, 80),
    "front500": (256, 2 * 256 * 500, 2048, 128),
}
# (engine, max_parents, ring_bytes): the option defaults, smoke()'s ring, and the small rings
# of tests/test_gpu_transfers.py
CONFIGS = [
    ("front20", 1 << 18, 16 << 30),
    ("front20 m20", 1 << 18, 16 << 30),
    ("front100", 1 << 18, 16 << 30),
    ("front500", 1 << 18, 16 << 30),
    ("front20", 1 << 18, 1 << 30),
    ("front20", 1 << 12, 1 << 28),
    ("front20", 256, 1 << 20),
    ("front20", 1024, 1 << 20),
]


def geometry(engine, max_parents, ring_bytes):
    """(buf_nodes, cap, max_parents) as DeviceEngine's constructor sizes them."""
    bp, slot, max_chunks, node = FRONT[engine]
    chunks = min((max_parents + bp - 1) // bp, max_chunks)
    buf_nodes = chunks * slot
    cap = 1
    while cap * 2 * node <= ring_bytes:
        cap *= 2
    while cap < buf_nodes * 8:
        cap *= 2
    return buf_nodes, cap, chunks * bp


class PlanModel:
    def __init__(self, iters_small, iters_large, iters_first, buf_nodes, cap, max_parents):
        self.iters_first, self.iters_large = iters_first, iters_large
        self.buf_nodes, self.cap, self.max_parents = buf_nodes, cap, max_parents
        self.ks = []
        k = iters_small
        while k <= iters_large:
            self.ks.append(k)
            k *= 2
        if iters_first % 6 == 0 and iters_first < iters_large and iters_first not in self.ks:
            self.ks = sorted(self.ks + [iters_first])

    def growth(self, k):
        return (k + 1) * self.buf_nodes

    def pick(self, total, extra, reserved, fresh, kmax=None):
        want = max(6, self.iters_first) if fresh else 6
        while (want < self.iters_large and total >= (want // 6) * 2 * self.max_parents
               and (kmax is None or want * 2 <= kmax)):
            want *= 2
        for i in reversed(range(len(self.ks))):
            if self.ks[i] > want and i > 0:
                continue
            if total + extra + reserved + (self.ks[i] + 1) * self.buf_nodes <= self.cap:
                return i
        return -1

    def fits(self, total, reserved, k):
        return total + reserved + (k + 1) * self.buf_nodes <= self.cap

    def leave_kmax(self, total):
        return max(6, total // 2 // self.max_parents)

    def exportable_ahead(self, stack, export_pending, inflight_ks):
        safe = (sum(inflight_ks) + 1) * self.max_parents
        left = stack - export_pending
        return left - safe if left > safe else 0

    def refill_limit(self, used):
        growth = (self.ks[0] + 1) * self.buf_nodes
        limit = min(self.cap // 2, self.cap - growth if self.cap > growth else 0)
        return limit - used if limit > used else 0

    def spill_ahead_keep(self):
        return max(self.cap // 2, 2 * (self.ks[-1] + 1) * self.max_parents)


def both(config, iters=ITERS):
    args = (*iters, *geometry(*config))
    return ops.cpu().ReplayPlan(*args), PlanModel(*args)


def around(*xs):
    return sorted({x + d for x in xs for d in (-1, 0, 1) if x + d >= 0})


def test_small_ring_geometry_is_what_the_transfer_tests_say():
    # "a ring (2^19 nodes)"; "window 256: a graph's growth is over half the ring"
    assert geometry("front20", 1024, 1 << 20) == (4 * 10240, 1 << 19, 1024)
    buf_nodes, cap, _ = geometry("front20", 256, 1 << 20)
    assert 7 * buf_nodes > cap // 2


@pytest.mark.parametrize("iters,ks", [((6, 48, 18), [6, 12, 18, 24, 48]), ((6, 48, 6), [6, 12, 24, 48]),
                                      ((6, 48, 48), [6, 12, 24, 48]), ((6, 48, 20), [6, 12, 24, 48]),
                                      ((6, 48, 36), [6, 12, 24, 36, 48]), ((6, 6, 18), [6]),
                                      ((12, 96, 18), [12, 18, 24, 48, 96]), ((6, 48, 54), [6, 12, 24, 48])])
def test_graph_lengths(iters, ks):
    plan, model = both(CONFIGS[0], iters)
    assert plan.ks == model.ks == ks
    for k in (1, 5, 6, 17, 48, 96):
        assert plan.growth(k) == model.growth(k) == (k + 1) * model.buf_nodes


@pytest.mark.parametrize("config,iters",
                         [(c, ITERS) for c in CONFIGS] + [(CONFIGS[0], (6, 48, 6)), (CONFIGS[-1], (6, 48, 36))],
                         ids=lambda v: "-".join(map(str, v)))
def test_pick_matches_the_engine_formula_around_every_threshold(config, iters):
    plan, model = both(config, iters)
    cap, mp = model.cap, model.max_parents
    # every length `want` passes through (6 doubling; iters_first doubling when fresh), and the
    # kmax at which each doubling is still allowed (want * 2 <= kmax)
    wants = sorted({w * 2**j for w in (6, max(6, iters[2])) for j in range(4) if w * 2**j <= 2 * iters[1]})
    kmaxes = [None] + around(6, *(2 * w for w in wants if w < iters[1]))
    n = 0
    picked = Counter()
    for extra in (0, model.growth(6), model.growth(48)):
        for reserved in (0, 1, mp, cap // 4):
            totals = around(0, cap, *((w // 6) * 2 * mp for w in wants),
                            *(cap - model.growth(k) for k in model.ks if cap >= model.growth(k)),
                            *(cap - model.growth(k) - extra - reserved for k in model.ks
                              if cap >= model.growth(k) + extra + reserved))
            for total, fresh, kmax in itertools.product(totals, (False, True), kmaxes):
                args = (total, extra, reserved, fresh) + (() if kmax is None else (kmax,))
                got = plan.pick(*args)
                assert got == model.pick(*args), args
                picked[got] += 1
                n += 1
    # the totals reach "none fits" and every graph the ring can hold at all
    assert n > 10000 and sorted(picked) == [-1] + [i for i, k in enumerate(model.ks) if model.growth(k) <= cap], picked


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_the_other_sizing_rules_match_the_engine_formulas(config):
    plan, model = both(config)
    cap, mp, buf = model.cap, model.max_parents, model.buf_nodes
    # the learned first replay (any count up to 48) and warm_split's 6-iteration passes
    for k, reserved in itertools.product((1, 2, 3, 5, 6, 7, 17, 18, 47, 48), (0, 1, mp, cap // 4)):
        for total in around(0, cap, cap - (k + 1) * buf, cap - (k + 1) * buf - reserved):
            assert plan.fits(total, reserved, k) == model.fits(total, reserved, k), (total, reserved, k)
    # leave_one's cap on the replay left running
    for total in around(0, *(2 * mp * j for j in (1, 5, 6, 7, 12, 13, 24, 48, 49)), cap):
        assert plan.leave_kmax(total) == model.leave_kmax(total), total
    assert plan.leave_kmax(2 * mp * 7 - 1) == 6 and plan.leave_kmax(2 * mp * 7) == 7
    # export from under the replays in flight
    for ks, pending in itertools.product(([], [6], [48], [18, 6], [48, 48], [5], [17, 12]), (0, 1, mp, 3 * mp + 7)):
        safe = (sum(ks) + 1) * mp
        for stack in around(pending, pending + safe, pending + safe + mp, cap):
            if stack < pending:
                continue  # (the pending export is part of the stack)
            args = (stack, pending, ks)
            assert plan.exportable_ahead(*args) == model.exportable_ahead(*args), args
        assert plan.exportable_ahead(pending + safe, pending, ks) == 0
        assert plan.exportable_ahead(pending + safe + 1, pending, ks) == 1
    # refills: within half the ring, and the smallest graph still fits
    limit = min(cap // 2, max(cap - 7 * buf, 0))
    for used in around(0, limit, cap // 2, cap - 7 * buf if cap > 7 * buf else 0, cap):
        assert plan.refill_limit(used) == model.refill_limit(used), used
    assert plan.refill_limit(limit) == 0 and (limit == 0 or plan.refill_limit(limit - 1) == 1)
    assert plan.spill_ahead_keep() == model.spill_ahead_keep() == max(cap // 2, 2 * 49 * mp)
