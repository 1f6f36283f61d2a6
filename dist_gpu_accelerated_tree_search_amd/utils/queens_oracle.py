"""Pure-Python N-Queens oracle: an independent reference for the native engines.

A node is a tuple (cols, diag, anti, depth) of the three 32-bit attack masks of the next
column and the number of queens placed (csrc/core/pfsp_node.hpp QueensNode). The child
rule is QueensProblem::decompose's (csrc/core/problems.hpp): placing row `bit` gives
cols | bit, ((diag | bit) << 1) mod 2^32, (anti | bit) >> 1. Counting rules are the
pool's: every safe child is a tree node, a child in the last column is also a solution, a
parent at depth N is one solution and no tree node. Used by tests to check what the
kernels write child by child; imports nothing native.
"""
from __future__ import annotations

import random

MASK32 = 0xFFFFFFFF
WAVE = 64


def _popcount(x: int) -> int:
    return bin(x).count("1")


def full_mask(N: int) -> int:
    if not 1 <= N <= 32:
        raise ValueError("N-Queens supports 1 <= N <= 32")
    return (1 << N) - 1


def free_rows(N: int, node) -> int:
    """Mask of the safe rows of the next column (0 for a complete board)."""
    cols, diag, anti, depth = node
    if depth == N:
        return 0
    return ~(cols | diag | anti) & full_mask(N)


def children(N: int, node) -> list:
    """The safe children of a node, rows ascending (none for a complete board)."""
    cols, diag, anti, depth = node
    av = free_rows(N, node)
    out = []
    while av:
        bit = av & -av
        av ^= bit
        out.append((cols | bit, ((diag | bit) << 1) & MASK32, (anti | bit) >> 1, depth + 1))
    return out


def _count(full: int, cols: int, diag: int, anti: int, left: int):
    av = ~(cols | diag | anti) & full
    if left == 1:
        c = _popcount(av)
        return c, c
    tree = sol = 0
    while av:
        bit = av & -av
        av ^= bit
        t, s = _count(full, cols | bit, ((diag | bit) << 1) & MASK32, (anti | bit) >> 1, left - 1)
        tree += 1 + t
        sol += s
    return tree, sol


def subtree(N: int, node):
    """(tree, sol) of everything below a node, with the pool's counting rules."""
    cols, diag, anti, depth = node
    if depth == N:
        return 0, 1
    return _count(full_mask(N), cols, diag, anti, N - depth)


def _place(N: int, depth: int, rng: random.Random, budget: int):
    """One random valid placement of `depth` queens by randomised backtracking, or None
    when `budget` steps did not find one."""
    full = full_mask(N)
    path = [(0, 0, 0, 0)]
    todo = []
    while True:
        cols, diag, anti, d = path[-1]
        if d == depth:
            return path[-1]
        if len(todo) < len(path):
            rows = [r for r in range(N) if (~(cols | diag | anti) & full) >> r & 1]
            rng.shuffle(rows)
            todo.append(rows)
        budget -= 1
        if budget < 0:
            return None
        if todo[-1]:
            bit = 1 << todo[-1].pop()
            path.append((cols | bit, ((diag | bit) << 1) & MASK32, (anti | bit) >> 1, d + 1))
        else:
            todo.pop()
            path.pop()
            if not path:
                return None


def random_nodes(N: int, depth: int, n: int, rng: random.Random) -> list:
    """n random valid partial placements of `depth` queens (0 <= depth <= N): column by
    column on a random free row, backing up (and after a while starting over) on a dead end."""
    if not 0 <= depth <= N:
        raise ValueError("depth must be in [0, N]")
    if depth == N and N in (2, 3):
        raise ValueError("no complete board for N = 2 or 3")
    out = []
    while len(out) < n:
        node = _place(N, depth, rng, 50 * N)
        if node is not None:
            out.append(node)
    return out


def random_dead_ends(N: int, n: int, rng: random.Random) -> list:
    """n random partial placements (depth < N) whose next column has no safe row."""
    full = full_mask(N)
    out = []
    while len(out) < n:
        cols = diag = anti = d = 0
        while d < N:
            av = ~(cols | diag | anti) & full
            if not av:
                out.append((cols, diag, anti, d))
                break
            bit = 1 << rng.choice([r for r in range(N) if av >> r & 1])
            cols, diag, anti, d = cols | bit, ((diag | bit) << 1) & MASK32, (anti | bit) >> 1, d + 1
    return out


def finish_wave_model(N: int, parents, stack: int):
    """Model of the stack discipline of one wave's subtree finishing (queens_finish_wave,
    csrc/hip/queens_kernels.hpp) over at most 64 parents of depth < N and a stack of
    `stack` nodes: each pass pops the top <= 64 nodes, counts their safe children, pushes
    the children of nodes above the last column at prefix offsets; when they do not all
    fit, the pass is cut at the first lane whose children do not, and that lane and every
    later lane with children to push walks its node's subtree on its own instead.
    Returns (tree, sol, walks, peak): the counts, the number of walked nodes and the
    largest stack occupancy. Tests use it to tell which inputs overflow a stack; expected
    counts come from subtree()."""
    parents = list(parents)
    if len(parents) > WAVE or len(parents) > stack:
        raise ValueError("one wave holds at most 64 parents (and its stack at least as many)")
    full = full_mask(N)
    st = []
    for cols, diag, anti, depth in parents:
        if depth >= N or _popcount(cols) != depth:
            raise ValueError("a finishing parent has depth < N queens placed")
        st.append((cols, diag, anti))
    tree = sol = walks = 0
    peak = len(st)
    while st:
        n = min(len(st), WAVE)
        base = len(st) - n
        lanes = st[base:]
        del st[base:]
        room = stack - base
        used = 0
        cut = False
        for cols, diag, anti in lanes:
            av = ~(cols | diag | anti) & full
            c = _popcount(av)
            depth = _popcount(cols)
            last = depth + 1 == N
            cpush = 0 if last else c
            if cpush and (cut or used + cpush > room):
                cut = True
                t, s = subtree(N, (cols, diag, anti, depth))
                tree += t
                sol += s
                walks += 1
                continue
            tree += c
            if last:
                sol += c
            while cpush and av:
                bit = av & -av
                av ^= bit
                st.append((cols | bit, ((diag | bit) << 1) & MASK32, (anti | bit) >> 1))
            used += cpush
        peak = max(peak, len(st))
    return tree, sol, walks, peak
