"""A plain model of Partition::evaluate(graph) and evaluate(graph, seq) (partition.cpp:428-521)
and of writePartitionedGraph's edge owner (partition.cpp:657-664), behind
tests/test_evaluate_shapes.py.  Set arithmetic over the adjacency entries, straight from the
definition: no bitsets, no histograms in fast memory, no oracle library.  Exact Python ints.

The graph is LLAMA's view of the records: a record (u, v) gives the adjacency entries u->v
and v->u, a self-loop gives one entry, repeated records repeat; a node is a vertex with an
entry; getEdges() is the entry count / 2.  A node X inserts one owner part per entry X->Y
into a set per metric, and the metric is the sum over the nodes of (set size - 1):

  ECV(down)  the part of the endpoint earlier in the sequence
  ECV(up)    the part of the later endpoint
  ECV(hash)  the part of the endpoint with the smaller cormen hash of its vid
  Vcom. vol  Y's part, and X's own part from the start

A self-loop's entry X->X owns X's part in every set.  The balances count each non-loop record
once, at the part that owns it (the vertex balance: each node once, at its part), and are the
maximum over the parts; edges cut counts the non-loop records whose ends differ in part.
"""
import numpy as np

FIELDS = ("edges_cut", "vcom_vol", "max_vertex_bal", "ecv_hash", "max_hash_bal", "ecv_down", "max_down_bal",
          "ecv_up", "max_up_bal", "edges", "nodes")
# metric mask bits of sheep_evaluate: 1 = evaluate(graph), 2 = ECV(down), 4 = ECV(up); 0 = all
MASK_FIELDS = {1: ("edges_cut", "vcom_vol", "max_vertex_bal", "ecv_hash", "max_hash_bal"),
               2: ("ecv_down", "max_down_bal"),
               4: ("ecv_up", "max_up_bal")}
CORMEN_S = 2654435769   # floor(0.5 * (sqrt(5) - 1) * 2^32) (partition.cpp:423-427), odd: k -> k * s is a bijection
assert CORMEN_S == int(0.5 * (5 ** 0.5 - 1) * 2 ** 32) and CORMEN_S % 2 == 1


def cormen_hash(vid):
    return (np.asarray(vid, dtype=np.uint64) * np.uint64(CORMEN_S)) & np.uint64(0xFFFFFFFF)


def _lookup(tail, head, seq, parts):
    """int64 tails, heads, positions by vid (-1: unsequenced) and parts by vid (-1: none)."""
    t, h, seq = (np.asarray(x).astype(np.int64) for x in (tail, head, seq))
    parts = np.asarray(parts).astype(np.int64)
    size = int(max(t.max(initial=-1), h.max(initial=-1), seq.max(initial=-1), len(parts) - 1)) + 1
    pos = np.full(size, -1, dtype=np.int64)
    pos[seq] = np.arange(len(seq))
    pv = np.full(size, -1, dtype=np.int64)
    pv[: len(parts)] = parts
    if ((pos[t] < 0) | (pos[h] < 0) | (pv[t] < 0) | (pv[h] < 0)).any():
        raise IndexError("an edge endpoint has no position or no part")   # pos.at() / the asserts
    return t, h, pos, pv


def _distinct(vertex, owner):
    """Number of distinct (vertex, owner) pairs (owner < 2^16)."""
    return int(len(np.unique(vertex * 65536 + owner)))


def _max_count(owner, nparts):
    return int(np.bincount(owner, minlength=nparts).max())


def evaluate(tail, head, seq, parts):
    """The eleven oracle.EVAL_FIELDS of the records under the vid-indexed `parts`."""
    t, h, pos, pv = _lookup(tail, head, seq, parts)
    nparts = int(np.asarray(parts).max()) + 1   # max part + 1, used or not (partition.cpp:434, 486)
    nl = t != h
    # adjacency entries X -> Y
    x = np.concatenate([t, h[nl]])
    y = np.concatenate([h, t[nl]])
    node_ids = np.unique(x)
    nodes = int(len(node_ids))
    px, py = pv[x], pv[y]
    first = pos[x] < pos[y]    # X is the earlier endpoint (false both ways for a self-loop: Y's part = X's)
    later = pos[x] > pos[y]
    hashed = cormen_hash(x) < cormen_hash(y)
    own_sets = {
        "ecv_down": _distinct(x, np.where(first, px, py)),
        "ecv_up": _distinct(x, np.where(later, px, py)),
        "ecv_hash": _distinct(x, np.where(hashed, px, py)),
        "vcom_vol": _distinct(np.concatenate([x, node_ids]), np.concatenate([py, pv[node_ids]])),
    }
    out = {f: v - nodes for f, v in own_sets.items()}
    # per non-loop record (the reference counts at X < Y, resp. at the entry of the owning side: once)
    tn, hn = t[nl], h[nl]
    ptn, phn = pv[tn], pv[hn]
    t_first = pos[tn] < pos[hn]
    out["max_down_bal"] = _max_count(np.where(t_first, ptn, phn), nparts)
    out["max_up_bal"] = _max_count(np.where(t_first, phn, ptn), nparts)
    out["max_hash_bal"] = _max_count(np.where(cormen_hash(tn) < cormen_hash(hn), ptn, phn), nparts)
    out["max_vertex_bal"] = _max_count(pv[node_ids], nparts)
    out["edges_cut"] = int(np.count_nonzero(ptn != phn))
    out["edges"] = int(len(x)) // 2
    out["nodes"] = nodes
    return {f: int(out[f]) for f in FIELDS}


def masked(result, what):
    """`result` as sheep_evaluate returns it under the metric mask `what`: the fields of the
    metrics outside the mask are 0; edges and nodes always come back."""
    m = what or 7
    keep = {"edges", "nodes"}
    for bit, fields in MASK_FIELDS.items():
        if m & bit:
            keep |= set(fields)
    return {k: (v if k in keep else 0) for k, v in result.items()}


def edge_owner(tail, head, seq, parts):
    """The part each record is written to: that of its earlier-positioned endpoint
    (X_pos < Y_pos ? X_part : Y_part); a self-loop takes its vertex's part."""
    t, h, pos, pv = _lookup(tail, head, seq, parts)
    return np.where(t == h, pv[t], np.where(pos[t] < pos[h], pv[t], pv[h])).astype(np.int16)
