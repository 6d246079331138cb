"""Hand-built trees and the case lists of tests/test_partition_shapes.py: bare (parent, pst)
arrays written down directly, so that the partitioner's data-dependent branches are reached
by construction and not by whatever an elimination tree of a random graph happens to
look like.  Pure numpy, fixed seeds; every array is cached and read-only."""
import functools

import numpy as np

import oracle

INVALID = 0xFFFFFFFF

# constants of sheep_amd/csrc/partition.hip that the cases are built around
EV_ARG = 128          # event tables up to this size travel as a kernel argument
EV_LDS = 4096         # ... up to this size are read from LDS, larger ones from global memory
EV_STAGE = 1 << 16    # kids staged per k_event_kids launch
EVENT_LOOP_CAP = 4096   # sheep_tuning event_loop's default: k_event_loop's table capacity
LW32_LIMIT = 0xFFFFFFFF   # max_component below this: 32-bit rake words
RAKE_TOTAL_LIMIT = 1 << 40   # total weight from this on: no raking
MAX_PARTS = 30000     # every case stays below this (the int16 part limit is 32,767)


def _ro(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------
# 1. generators: parent[i] > i or INVALID
# ------------------------------------------------------------------------------------
def path(n=100_000):
    p = np.arange(1, n + 1, dtype=np.uint32)
    p[-1] = INVALID
    return p


def star(n=70_001):
    p = np.full(n, n - 1, np.uint32)
    p[-1] = INVALID
    return p


def caterpillar(n=100_001):
    """Even ids are leaves under the next (odd) spine node; the last node is the root."""
    i = np.arange(n, dtype=np.int64)
    p = np.where(i % 2 == 0, i + 1, i + 2)
    p[p >= n] = n - 1
    p = p.astype(np.uint32)
    p[-1] = INVALID
    return p


def binary(levels=17):
    """Complete binary tree: heap index h (root 1) is node n - h, so parents come later."""
    n = (1 << levels) - 1
    h = n - np.arange(n, dtype=np.int64)
    p = (n - h // 2).astype(np.uint32)
    p[-1] = INVALID
    return p


def recursive(n=100_000, seed=11):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    p = i + 1 + (rng.random(n) * (n - 1 - i)).astype(np.int64)
    p = np.minimum(p, n - 1).astype(np.uint32)
    p[-1] = INVALID
    return p


def narrow(n=100_000, span=64, seed=12):
    rng = np.random.default_rng(seed)
    p = np.arange(n, dtype=np.int64) + 1 + rng.integers(0, span, n)
    p[p >= n] = INVALID
    return p.astype(np.uint32)


def forest(n=100_000, roots=3000, seed=13):
    p = narrow(n, 64, seed).copy()
    rng = np.random.default_rng(seed + 1)
    p[rng.choice(n, roots, replace=False)] = INVALID
    return p


def two_level(fan=300):
    leaves = fan * fan
    p = np.empty(leaves + fan + 1, np.uint32)
    p[:leaves] = leaves + np.arange(leaves) // fan
    p[leaves:leaves + fan] = leaves + fan
    p[-1] = INVALID
    return p


def three_level(fan=300):
    p2 = two_level(fan)
    n2 = len(p2)
    p = np.concatenate([p2, np.arange(n2 + 1, n2 + 4, dtype=np.uint32)])
    p[n2 - 1] = n2
    p[-1] = INVALID
    return p


def broom(n=100_000):
    """The first half are leaves of node n/2, the bottom of a path up to n - 1."""
    half = n // 2
    p = np.arange(1, n + 1, dtype=np.uint32)
    p[:half] = half
    p[-1] = INVALID
    return p


def tiny1():
    return np.array([INVALID], np.uint32)


def tiny2():
    return np.array([1, INVALID], np.uint32)


def tiny3():
    return np.full(3, INVALID, np.uint32)


GENERATORS = {"path": path, "star": star, "caterpillar": caterpillar, "binary": binary, "recursive": recursive,
              "narrow": narrow, "forest": forest, "two_level": two_level, "three_level": three_level,
              "broom": broom, "tiny1": tiny1, "tiny2": tiny2, "tiny3": tiny3}
BIG_SHAPES = [s for s in GENERATORS if not s.startswith("tiny")]
TINY_SHAPES = ["tiny1", "tiny2", "tiny3"]
MERGE_SHAPES = ["path", "star", "caterpillar", "recursive", "forest", "narrow"]


@functools.lru_cache(maxsize=None)
def shape(name, n=None):
    """The named tree at its table size, or regenerated with n nodes (path, star,
    caterpillar, recursive, narrow and forest take one)."""
    return _ro(GENERATORS[name]() if n is None else GENERATORS[name](n))


# ------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pst_of(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "zero":
        w = np.zeros(n, np.uint32)
    elif kind == "uniform":
        w = rng.integers(0, 50, n).astype(np.uint32)
    elif kind == "heavy":   # Lomax tail (mean about 25), clipped well below total / 1000
        w = np.minimum(rng.pareto(1.2, n) * 8, 1500).astype(np.uint32)
    elif kind == "wide":    # sums and path heights past 2^32
        w = np.full(n, 1 << 26, np.uint32)
    else:
        raise KeyError(kind)
    return _ro(w)


# name -> (vtx_weight, pst_weight, pst kind); "unit" is partition_tree -x alone
MODES = {"unit": (1, 0, "uniform"), "pst_zero": (0, 1, "zero"), "pst_uniform": (0, 1, "uniform"),
         "pst_heavy": (0, 1, "heavy"), "both_zero": (1, 1, "zero"), "both_uniform": (1, 1, "uniform"),
         "both_heavy": (1, 1, "heavy")}
K_DEFAULT = (1, 2, 7, 64, 1000)
K_BIG_FAN = (1, 2, 7, 16)   # one huge kid list: the host first-fit is O(kids * parts^2) there
K_EVENTS = 8192             # unit weights on path / caterpillar: max_component 12, ~8,000 events
BALANCES = (1.0, 2.0)       # beside the default 1.03
BALANCE_SHAPES = ("path", "narrow", "forest", "recursive")


def ks_of(name, mode):
    if name in ("star", "broom"):
        return K_BIG_FAN
    if name.startswith("tiny"):   # a single node must fit max_component: k = 1, or unit weights and k = n
        return (1, len(shape(name))) if mode == "unit" and name != "tiny1" else (1,)
    return K_DEFAULT


def weights(name, mode):
    """(vtx, pstw, pst, per-node weight as the partitioner sums it)."""
    vtx, pstw, kind = MODES[mode]
    pst = pst_of(kind, len(shape(name)))
    return vtx, pstw, pst, vtx + pstw * pst.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def subtree_sums(name, mode):
    """Every node's subtree weight (kids come first, so one ascending pass)."""
    p = shape(name).tolist()
    s = weights(name, mode)[3].tolist()
    for i, par in enumerate(p):
        if par != INVALID:
            s[par] += s[i]
    return _ro(np.array(s, np.uint64))


def max_component_of(total, k, balance):
    return int(float(int(total) // k) * balance)   # partition.cpp:57


def merge_tree(name, n=100_000):
    """(parent, pst) of a merge input: the shape at n nodes, its own small random pst."""
    rng = np.random.default_rng(500 + MERGE_SHAPES.index(name))
    return shape(name, n), _ro(rng.integers(0, 1000, n).astype(np.uint32))


# (shape, mode, balance, ks): each is one run over a persistent kid table, in this k order
SHAPE_CASES = [(s, m, 1.03, ks_of(s, m)) for s in BIG_SHAPES + TINY_SHAPES for m in MODES]
BALANCE_CASES = [(s, m, b, K_DEFAULT) for s in BALANCE_SHAPES for b in BALANCES
                 for m in ("unit", "pst_uniform", "both_heavy")]
EVENT_CASES = [(s, "unit", 1.03, (K_EVENTS,)) for s in ("path", "caterpillar")]
TIE_SHAPES = ("narrow", "recursive", "binary")
TIE_KS = (64, 1000, 7, 256, 2)
TIE_CASES = [(s, "unit", 1.03, TIE_KS) for s in TIE_SHAPES]
SPARSE_CASES = [(s, m, 1.03, (2, 64, 1000)) for s in ("narrow", "forest") for m in ("unit", "pst_heavy")]
EVENT_LOOP_CASES = [("path", "unit", 1.03, (K_EVENTS,)), ("forest", "both_uniform", 1.03, (64, 1000))]
ALL_CASES = SHAPE_CASES + BALANCE_CASES + EVENT_CASES + TIE_CASES


def case_id(c):
    return f"{c[0]}-{c[1]}-b{c[2]}"


def identity_seq(n):
    return np.arange(n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def sparse_seq(n):
    """vid = 3 * perm[j] + 5: pos_size is about 3n and most slots are unsequenced."""
    return _ro((3 * np.random.default_rng(77).permutation(n) + 5).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def oracle_run(name, mode, balance, ks, sparse=False):
    """The oracle's parts and info for every k of one case, in order, on one oracle.Kids
    (forwardPartition's std::sort of a packing node's kids carries over to the next k)."""
    parent = shape(name)
    vtx, pstw, pst, _ = weights(name, mode)
    seq = sparse_seq(len(parent)) if sparse else identity_seq(len(parent))
    kids = oracle.Kids(parent)
    out = []
    for k in ks:
        parts, info = oracle.partition(parent, pst, seq, k, balance, vtx, pstw, kids)
        out.append((_ro(parts), info))
    return out


# ------------------------------------------------------------------------------------
# 3. wide weights on a small narrow tree: (pst, balance, ks, which side of each switch)
# ------------------------------------------------------------------------------------
WIDE_N = 4096


@functools.lru_cache(maxsize=None)
def shape_wide():
    return _ro(narrow(WIDE_N, 16, 21))


@functools.lru_cache(maxsize=None)
def wide_pst(kind):
    if kind == "mixed":
        return _ro(np.random.default_rng(22).integers(0, 1 << 32, WIDE_N, dtype=np.uint64).astype(np.uint32))
    return _ro(np.full(WIDE_N, 1 << int(kind[1:]), np.uint32))


# name -> (pst kind, balance, {k: max_component >= LW32_LIMIT?}, total >= RAKE_TOTAL_LIMIT?)
WIDE_CASES = {
    # total 2^38, raking on; k = 64 gives exactly 2^32, k = 65 is back below 2^32 - 1
    "p26-b1.0": ("p26", 1.0, {2: True, 32: True, 64: True, 65: False}, False),
    "p26-b1.03": ("p26", 1.03, {64: True, 65: True, 66: False, 600: False}, False),
    # total exactly 2^40 and 2^43: no raking, both rake word widths
    "p28": ("p28", 1.03, {2: True, 64: True, 600: False, 2000: False}, True),
    "p31": ("p31", 1.03, {2: True, 64: True, 600: True, 2000: True}, True),
    # random 32-bit weights: every k leaves max_component above the heaviest node
    "mixed": ("mixed", 1.03, {2: True, 64: True, 600: True}, True),
}
WIDE_FLAGS = ((0, 1), (1, 1))
