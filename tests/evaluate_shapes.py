"""Graphs, part vectors and the case list of tests/test_evaluate_shapes.py: the evaluator
(sheep_amd/csrc/evaluate.hip) under arbitrary int16 part vectors, not only the ones a tree
partition produces.  Every graph has at most 2^12 vertex slots and about 70,000 records, so
the evaluator's state (pos_size * (1 + M * W64) * 8 bytes) stays near 67 MB at 32,768 parts.
Pure numpy, fixed seeds; every array is cached and read-only."""
import functools

import numpy as np

import oracle
from conftest import golden_records

import evaluate_model as model

# constants of sheep_amd/csrc/evaluate.hip and common.hpp that the cases are built around
LDS_PARTS = 2048      # balance histograms in LDS up to this many parts, global atomics above
WAVE = 64
WAVE_COUNT_RARE = 8   # wave_count: fewer equal keys than this in a wave -> one atomic per lane
MAX_SLOTS = 1 << 12
STAR_LEAVES = 4000

ALL_K = (1, 2, 63, 64, 65, 128, 129, 2047, 2048, 2049, 4096, 32767, 32768)
MASKS = (0, 1, 2, 4, 3, 5, 6)
FORMS = ("records", "step")


def _ro(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------
# 1. graphs: (tail, head) as uint32
# ------------------------------------------------------------------------------------
def _rmat12():
    import sheep_amd
    r = sheep_amd.rmat_host(12, 16, 12)
    return r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint32)


def _rmat12_mixed():
    """rmat12 plus 500 self-loops on vertices that have edges, plus its first 1,000 records
    again; every second record with its ends swapped, then shuffled: no tail runs."""
    t, h = _rmat12()
    rng = np.random.default_rng(1201)
    loops = rng.choice(np.unique(np.concatenate([t, h])), 500, replace=False).astype(np.uint32)
    t = np.concatenate([t, loops, t[:1000]])
    h = np.concatenate([h, loops, h[:1000]])
    swap = np.arange(len(t)) % 2 == 1
    t, h = np.where(swap, h, t), np.where(swap, t, h)
    order = rng.permutation(len(t))
    return t[order], h[order]


def _star(hub_major):
    """Hub 0 and STAR_LEAVES leaves; hub-major: one run of equal tails over many waves and
    workgroups."""
    leaf = np.arange(1, STAR_LEAVES + 1, dtype=np.uint32)
    hub = np.zeros(STAR_LEAVES, np.uint32)
    return (hub, leaf) if hub_major else (leaf, hub)


def _path(n=MAX_SLOTS):
    v = np.arange(n - 1, dtype=np.uint32)
    return v, v + 1


def _loops_only():
    """A 50-vertex path (vids 0..49) next to 300 vertices (50..349) whose only records are
    self-loops, the first 20 of them twice: nodes without any edge."""
    pt, ph = _path(50)
    lp = np.arange(50, 350, dtype=np.uint32)
    t = np.concatenate([lp[:150], pt, lp[150:], lp[:20]])
    return t, np.concatenate([lp[:150], ph, lp[150:], lp[:20]])


def _edge():
    r = golden_records("edge")
    return r["tail"].astype(np.uint32), r["head"].astype(np.uint32)


GRAPHS = {"rmat12": _rmat12, "rmat12_mixed": _rmat12_mixed, "star_leaf": lambda: _star(False),
          "star_hub": lambda: _star(True), "path": _path, "loops_only": _loops_only, "edge": _edge}
STAR_HUB_VID = 0


@functools.lru_cache(maxsize=None)
def graph(name):
    """(tail, head, seq, pos_size): the records, their degree sequence (every vertex with an
    adjacency entry, as degreeSequence orders them) and the slot count, max vid + 1."""
    t, h = GRAPHS[name]()
    t, h = _ro(np.ascontiguousarray(t, np.uint32)), _ro(np.ascontiguousarray(h, np.uint32))
    pos_size = int(max(t.max(), h.max())) + 1
    assert pos_size <= MAX_SLOTS and len(t) <= 70_000
    return t, h, _ro(oracle.sequence(t, h)), pos_size


def positions(name):
    _, _, seq, pos_size = graph(name)
    pos = np.full(pos_size, -1, np.int64)
    pos[seq] = np.arange(len(seq))
    return pos


def loop_only_nodes(name):
    """Vertices whose every record is a self-loop."""
    t, h, _, _ = graph(name)
    nl = t != h
    return np.setdiff1d(t[~nl], np.concatenate([t[nl], h[nl]]))


def forced_endpoint(name):
    """The edge endpoint every generator puts in part k - 1 (so max part + 1 == k)."""
    t, _, _, _ = graph(name)
    return int(t[len(t) // 2])


# ------------------------------------------------------------------------------------
# 2. part vectors over the pos_size slots, max part + 1 == k
# ------------------------------------------------------------------------------------
GENERATORS = ("random", "mod", "blocks", "by_pos", "one", "sparse", "distinct_leaves")


@functools.lru_cache(maxsize=None)
def parts(name, gen, k):
    _, _, seq, pos_size = graph(name)
    vid = np.arange(pos_size, dtype=np.int64)
    if gen == "random":
        p = np.random.default_rng(7000 + k).integers(0, k, pos_size)
    elif gen == "mod":
        p = vid % k
    elif gen == "blocks":     # long runs of equal parts
        p = vid * k // pos_size
    elif gen == "by_pos":     # the same along the sequence (slots outside it: part 0)
        p = np.maximum(positions(name), 0) * k // len(seq)
    elif gen == "one":
        p = np.full(pos_size, k - 1)
    elif gen == "sparse":     # two parts in use, whatever k: nparts is the maximum + 1
        p = np.where(vid % 3 == 0, k - 1, 0)
    elif gen == "distinct_leaves":   # the star: leaf i in part i % k, the hub in part k - 1
        assert name.startswith("star")
        p = (vid - 1) % k
        p[STAR_HUB_VID] = k - 1
    else:
        raise KeyError(gen)
    p = p.astype(np.int64)
    if gen != "distinct_leaves":
        p[forced_endpoint(name)] = k - 1
    assert p.min() >= 0 and p.max() == k - 1
    return _ro(p.astype(np.int16))


# ------------------------------------------------------------------------------------
# 3. the cases: (graph, generator, k)
# ------------------------------------------------------------------------------------
K_SMALL = tuple(k for k in ALL_K if k <= 4096)
K_EDGES = (2, 64, 65, 2048, 2049)       # one k on each side of the ROW16 / W64 == 1 and the LDS switch
K_SHARDS = (64, 65, 2049, 32768)
SHARD_MASKS = (0, 2, 5)

CASES = (
    [("rmat12_mixed", "random", k) for k in ALL_K]
    + [("star_leaf", "distinct_leaves", k) for k in ALL_K]
    + [("star_hub", "distinct_leaves", k) for k in (1, 64, 65, 2048, 2049, 4096, 32768)]
    + [("rmat12_mixed", g, k) for g in ("one", "sparse") for k in (64, 65, 2048, 2049, 32768)]
    + [("rmat12", "random", k) for k in K_SMALL]
    + [("rmat12", g, k) for g in ("mod", "blocks", "by_pos") for k in K_EDGES]
    + [("path", g, k) for g in ("mod", "blocks", "by_pos") for k in K_EDGES + (129, 4096)]
    + [("loops_only", g, k) for g in ("random", "one", "sparse") for k in (1, 64, 65, 129, 2048, 2049)]
    + [("edge", "mod", k) for k in (1, 2, 3)] + [("edge", "sparse", k) for k in (65, 2049)]
)
SHARD_CASES = [c for c in CASES if c[2] in K_SHARDS and (c[0], c[1]) in
               (("rmat12_mixed", "random"), ("star_hub", "distinct_leaves"), ("loops_only", "sparse"))]
ERROR_CASE = ("rmat12_mixed", "random", 2049)
ERROR_MASKS = (0, 2)


def case_id(c):
    return f"{c[0]}-{c[1]}-k{c[2]}"


def isolated_slot(name):
    """A vertex slot below pos_size without any record (sequenced by hand in the error test)."""
    t, h, _, pos_size = graph(name)
    free = np.setdiff1d(np.arange(pos_size), np.concatenate([t, h]))
    return int(free[len(free) // 2])


@functools.lru_cache(maxsize=None)
def expected(name, gen, k):
    """(the model's eleven fields, the model's per-record owners) of one case."""
    t, h, seq, _ = graph(name)
    p = parts(name, gen, k)
    return model.evaluate(t, h, seq, p), _ro(model.edge_owner(t, h, seq, p))


# ------------------------------------------------------------------------------------
# 4. what a case reaches in the kernels, derived on the host
# ------------------------------------------------------------------------------------
def arrays_of(what):
    """M: the bit arrays of a metric mask (down, up: one each; evaluate(graph): hash and Vcom)."""
    m = what or 7
    return (1 if m & 2 else 0) + (1 if m & 4 else 0) + (2 if m & 1 else 0)


def vcom_width(name, gen, k):
    """The widest Vcom set of the case (neighbours' parts and the own part) and its vertex."""
    t, h, _, pos_size = graph(name)
    p = parts(name, gen, k).astype(np.int64)
    x = np.concatenate([t, h, np.arange(pos_size)]).astype(np.int64)
    y = np.concatenate([h, t, np.arange(pos_size)]).astype(np.int64)
    pairs = np.unique(x * 65536 + p[y])
    width = np.bincount(pairs >> 16, minlength=pos_size)
    return int(width.max()), int(width.argmax())


def coverage(case, what, form):
    name, gen, k = case
    M, W64 = arrays_of(what), (k + 63) // 64
    return {
        "case": case_id(case), "what": what, "form": form, "M": M, "W64": W64,
        "balances": "global" if k > LDS_PARTS else "LDS",
        # the 16-byte row kernel: the record form with one array of one word
        "ROW16": form == "records" and M == 1 and W64 == 1,
        "one_word": W64 == 1,
        "full_vcom": bool((what or 7) & 1) and vcom_width(name, gen, k)[0] == k,
        "loop_only_nodes": len(loop_only_nodes(name)) > 0,
    }


@functools.lru_cache(maxsize=None)
def coverage_table():
    return tuple(coverage(c, w, f) for c in CASES for w in MASKS for f in FORMS)
