"""numpy views of the node layouts shared by host and device pools.

PFSP node (csrc/core/pfsp_node.hpp): id_t depth; id_t prmu[NJ]; padded to 16 B,
id_t = uint8 for NJ <= 255 else uint16. PFSP front node (LB1 / LB1_d engines on up to
20 jobs): uint8 depth, 3 pad, uint32 unscheduled-job mask, uint16 front[MB] (21-50 jobs:
7 pad and a uint64 mask; 51-100 jobs, with TTS_FRONT_WIDE=1: 15 pad and a 128-bit mask of
two uint64 words, low word first), padded
to 16 B (32 B for MB <= 10 machines, 48 B for 20; 50 jobs: 32 / 48 / 64 B and 100 jobs:
48 / 64 / 80 B for 5 / 10 / 20 machines). 101-500 jobs, with TTS_FRONT_WIDE=2: a 16-byte
header (uint16 depth, 14 zero bytes), a mask of 4 (up to 200 jobs) or 8 uint64 words at byte
16, low word first, then the fronts (200 jobs: 64 / 80 / 96 B, 500 jobs: 96 / 112 / 128 B).
N-Queens node: 4 x uint32
{cols, diag, anti, depth}. Parity: ref pfsp/lib/PFSP_node.h:15-20 (44-B node with
limit1 stored), nqueens/lib/NQueens_node.h:13-17 (board).
"""
from __future__ import annotations

import numpy as np

BUCKETS = (20, 50, 100, 200, 500)


def pfsp_bucket(jobs: int) -> int:
    for b in BUCKETS:
        if jobs <= b:
            return b
    return 500


def pfsp_id_dtype(jobs: int):
    return np.uint16 if pfsp_bucket(jobs) > 255 else np.uint8


def pfsp_node_bytes(jobs: int) -> int:
    nj = pfsp_bucket(jobs)
    isz = np.dtype(pfsp_id_dtype(jobs)).itemsize
    raw = (nj + 1) * isz
    return (raw + 15) // 16 * 16


def pfsp_pack(depths, perms, jobs: int) -> np.ndarray:
    """Pack (depth, permutation) pairs into an (n, node_bytes) uint8 array."""
    depths = np.asarray(depths)
    perms = np.asarray(perms)
    n = len(depths)
    nb = pfsp_node_bytes(jobs)
    dt = pfsp_id_dtype(jobs)
    isz = np.dtype(dt).itemsize
    out = np.zeros((n, nb // isz), dtype=dt)
    out[:, 0] = depths
    out[:, 1 : 1 + jobs] = perms
    return out.view(np.uint8).reshape(n, nb)


def pfsp_unpack(nodes: np.ndarray, jobs: int):
    """Inverse of pfsp_pack: (depths[n], perms[n, jobs])."""
    dt = pfsp_id_dtype(jobs)
    v = np.ascontiguousarray(nodes).view(dt)
    return v[:, 0].astype(np.int64), v[:, 1 : 1 + jobs].astype(np.int64)


def pfsp_root(jobs: int) -> np.ndarray:
    return pfsp_pack([0], [np.arange(jobs)], jobs)


def pfsp_front_unpack(nodes: np.ndarray, machines_bucket: int, jobs: int = 20):
    """Front nodes -> (depths[n], rest masks[n], fronts[n, machines_bucket]). Up to 20
    jobs the unscheduled set is 32 bits at byte 4 and the fronts start at byte 8; up to
    50 jobs it is 64 bits at byte 8 and the fronts start at byte 16; up to 100 jobs it is
    128 bits at byte 16 (two uint64 words, low word first) and the fronts start at byte 32:
    the masks then come back as an object array of Python ints, and pfsp_front_set_words
    gives the two uint64 columns. Up to 200 / 500 jobs the depth is a uint16 in bytes 0-1,
    the set 4 / 8 uint64 words at byte 16 and the fronts start at byte 48 / 80."""
    a = np.ascontiguousarray(nodes, dtype=np.uint8)
    depths = a[:, 0].astype(np.int64)
    if jobs > 100:
        depths = a[:, 0:2].copy().view(np.uint16).reshape(-1).astype(np.int64)
        w = pfsp_front_set_words(a, jobs)
        rest = np.array([sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in w], dtype=object)
        f0 = 16 + 8 * w.shape[1]
    elif jobs <= 20:
        rest = a[:, 4:8].copy().view(np.uint32).reshape(-1).astype(np.int64)
        f0 = 8
    elif jobs > 50:
        w = pfsp_front_set_words(a)
        rest = np.array([int(lo) | (int(hi) << 64) for lo, hi in w], dtype=object)
        f0 = 32
    else:
        rest = a[:, 8:16].copy().view(np.uint64).reshape(-1)
        f0 = 16
    fronts = a[:, f0:f0 + 2 * machines_bucket].copy().view(np.uint16).astype(np.int64)
    return depths, rest, fronts


def pfsp_front_set_words(nodes: np.ndarray, jobs: int = 100) -> np.ndarray:
    """The unscheduled sets of front nodes above 50 jobs as (n, W) uint64 words, low word
    first (bit j of the set: bit j % 64 of word j // 64): W = 2 for 51-100 jobs, 4 for
    101-200, 8 for 201-500."""
    a = np.ascontiguousarray(nodes, dtype=np.uint8)
    w = 2 if jobs <= 100 else 4 if jobs <= 200 else 8
    return a[:, 16:16 + 8 * w].copy().view(np.uint64).reshape(-1, w)


QUEENS_NODE_BYTES = 16


def queens_pack(cols, diag, anti, depth) -> np.ndarray:
    a = np.stack([np.asarray(cols), np.asarray(diag), np.asarray(anti), np.asarray(depth)], axis=1).astype(np.uint32)
    return a.view(np.uint8).reshape(len(a), QUEENS_NODE_BYTES)


def queens_unpack(nodes: np.ndarray):
    v = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)
    return v[:, 0], v[:, 1], v[:, 2], v[:, 3]
