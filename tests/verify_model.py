"""The tree verifier's certificate by its definition (tests/test_verify.py).

A forest over ids 0..n-1 is the elimination tree of the records under a sequence exactly when
  1. structure  every parent is INVALID or lies in (v, n);
  2. descent    for every position edge (lo, hi), hi is an ancestor of lo;
  3. support    every non-root v with parent p has an edge (x, p) with x in v's subtree;
  4. pst        pst[v] = edges with lo == v + records whose only sequenced end is v.
Ancestry is found by walking parents (no tour): `verify_literal` one step at a time,
`verify` in strides of 2^k over a table of 2^k-th ancestors, which is the same walk because
ids grow along every path once (1) holds.  Both return the fields of sheep_verify_t.
"""
import numpy as np

INVALID = 0xFFFFFFFF
NO_ID = 0xFFFFFFFFFFFFFFFF
FIELDS = ("ok", "bad_parent", "not_descendant", "unsupported", "pst_mismatch",
          "first_bad_parent", "first_not_descendant", "first_unsupported", "first_pst_mismatch")


def relabel(tail, head, seq, n):
    """The records in sequence positions, as oracle/sheep_oracle.cpp buildTreeMapReduce reads
    them: (record index, lo, hi) of the records with both ends sequenced, and cnt[v] = those
    with lo == v plus the records whose only sequenced end is v.  A self-loop counts nowhere;
    a neighbour >= pos_size of a sequenced vertex raises IndexError."""
    tail, head, seq = (np.asarray(x, dtype=np.int64) for x in (tail, head, seq))
    pos_size = int(seq.max()) + 1 if len(seq) else 0
    pos = np.full(pos_size + 1, -1, dtype=np.int64)   # the last slot stands for every vid >= pos_size
    pos[seq] = np.arange(len(seq))
    pt, ph = pos[np.minimum(tail, pos_size)], pos[np.minimum(head, pos_size)]
    pt[pt >= n] = -1   # (a position past the tree: no node of it)
    ph[ph >= n] = -1
    if np.any(((pt >= 0) & (head >= pos_size)) | ((ph >= 0) & (tail >= pos_size))):
        raise IndexError("vertex id out of range of the sequence index")
    live = tail != head
    both = live & (pt >= 0) & (ph >= 0)
    idx = np.flatnonzero(both)
    lo, hi = np.minimum(pt[idx], ph[idx]), np.maximum(pt[idx], ph[idx])
    cnt = np.bincount(lo, minlength=n)
    cnt += np.bincount(pt[live & (pt >= 0) & (ph < 0)], minlength=n)
    cnt += np.bincount(ph[live & (ph >= 0) & (pt < 0)], minlength=n)
    return idx, lo, hi, cnt


def _verdict(bad, stray, unsup, pst):
    """The fields from the sorted offender lists of the four classes."""
    first = lambda a: int(a[0]) if len(a) else NO_ID
    v = dict(bad_parent=len(bad), not_descendant=len(stray), unsupported=len(unsup), pst_mismatch=len(pst),
             first_bad_parent=first(bad), first_not_descendant=first(stray), first_unsupported=first(unsup),
             first_pst_mismatch=first(pst))
    v["ok"] = not (len(bad) or len(stray) or len(unsup) or len(pst))
    return v


def bad_parents(parent):
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    return np.flatnonzero((parent != INVALID) & ((parent <= np.arange(n)) | (parent >= n)))


def verify_literal(tail, head, seq, parent, pst):
    """Plain Python, one parent step at a time (small inputs)."""
    parent = [int(p) for p in parent]
    n = len(parent)
    bad = bad_parents(parent)
    if len(bad):   # final: the other classes are not evaluated
        return _verdict(bad, [], [], [])
    idx, lo, hi, cnt = relabel(tail, head, seq, n)
    stray, sup = [], [False] * n
    for i, l, h in zip(idx.tolist(), lo.tolist(), hi.tolist()):
        c = l
        while parent[c] != INVALID and parent[c] < h:
            c = parent[c]
        if parent[c] == h:
            sup[c] = True    # the edge (l, h) leaves c's subtree at c's parent
        else:
            stray.append(i)  # the walk passed h: h is no ancestor of l
    unsup = [v for v in range(n) if parent[v] != INVALID and not sup[v]]
    wrong = [v for v in range(n) if int(pst[v]) != int(cnt[v])]
    return _verdict(bad, stray, unsup, wrong)


def verify(tail, head, seq, parent, pst):
    """The same walk for every edge at once, in strides of 2^k."""
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    bad = bad_parents(parent)
    if len(bad):
        return _verdict(bad, [], [], [])
    idx, lo, hi, cnt = relabel(tail, head, seq, n)
    up = [np.where(parent == INVALID, n, parent)]      # n: above every root
    up[0] = np.append(up[0], n)
    while len(up) < max(1, n.bit_length()):
        up.append(up[-1][up[-1]])
    c = lo.copy()
    for anc in reversed(up):                           # the highest ancestor-or-self below hi
        nxt = anc[c]
        c = np.where(nxt < hi, nxt, c)
    below = up[0][c] == hi
    sup = np.zeros(n, dtype=bool)
    sup[c[below]] = True
    unsup = np.flatnonzero((parent != INVALID) & ~sup)
    wrong = np.flatnonzero(np.asarray(pst, dtype=np.int64) != cnt)
    return _verdict(bad, idx[~below], unsup, wrong)


def counts_line(v):
    """The line verify_tree prints under "ERROR: Tree is not valid."."""
    f = lambda x: "-" if x == NO_ID else str(x)
    return ("bad_parent:%d@%s not_descendant:%d@%s unsupported:%d@%s pst_mismatch:%d@%s\n"
            % (v["bad_parent"], f(v["first_bad_parent"]), v["not_descendant"], f(v["first_not_descendant"]),
               v["unsupported"], f(v["first_unsupported"]), v["pst_mismatch"], f(v["first_pst_mismatch"])))
