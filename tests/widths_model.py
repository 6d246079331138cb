"""Python models behind tests/test_widths.py (true tree widths, graph2tree -k -e -j).

* the elimination game: the definition of width(v) = 1 + |jxn(v)| (jtree.cpp:97,
  jnode.h:230-260), literal and in its merge-into-the-parent form;
* the row-subtree rule the kernels of sheep_amd/csrc/widths.hip implement, pass for pass;
* JNodeTable::Facts (jnode.cpp:256-290) with given widths, and the print formats.
"""
import numpy as np

INVALID = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def position_edges(tail, head, seq):
    """The records in sequence positions, lo < hi; self-loops and records with an
    unsequenced end are dropped as the map drops them.  Repeats are kept."""
    tail, head, seq = (np.asarray(x, dtype=np.int64) for x in (tail, head, seq))
    size = int(max(tail.max(initial=-1), head.max(initial=-1), seq.max(initial=-1))) + 1
    pos = np.full(size, -1, dtype=np.int64)
    pos[seq] = np.arange(len(seq))
    pt, ph = pos[tail], pos[head]
    keep = (tail != head) & (pt >= 0) & (ph >= 0)
    pt, ph = pt[keep], ph[keep]
    return np.minimum(pt, ph), np.maximum(pt, ph)


def etree(n, lo, hi):
    """Liu's elimination tree of the position edges and pst = records with that lo."""
    parent = np.full(n, INVALID, dtype=np.int64)
    anc = [-1] * n
    order = np.argsort(hi, kind="stable")
    for l, h in zip(lo[order].tolist(), hi[order].tolist()):
        r = l
        while anc[r] != -1 and anc[r] != h:   # climb, compressing the path onto h
            up = anc[r]
            anc[r] = h
            r = up
        if anc[r] == -1 and r != h:
            anc[r] = h
            parent[r] = h
    return parent, np.bincount(lo, minlength=n).astype(np.int64)


def game_literal(n, lo, hi):
    """Eliminate the vertices in order; eliminating v joins its later neighbours pairwise."""
    adj = [set() for _ in range(n)]
    for l, h in zip(lo.tolist(), hi.tolist()):
        adj[l].add(h)
        adj[h].add(l)
    width = np.ones(n, dtype=np.int64)
    for v in range(n):
        later = [u for u in adj[v] if u > v]
        width[v] = 1 + len(later)
        for a in later:
            adj[a].update(x for x in later if x != a)
    return width


def game(n, lo, hi):
    """The same widths with the later neighbours handed to the earliest of them only (the
    elimination tree parent): what reaches a vertex is the same set."""
    later = [set() for _ in range(n)]
    for l, h in zip(lo.tolist(), hi.tolist()):
        later[l].add(h)
    width = np.ones(n, dtype=np.int64)
    for v in range(n):
        s = later[v]
        width[v] = 1 + len(s)
        if s:
            p = min(s)
            s.discard(p)
            if len(later[p]) < len(s):
                s |= later[p]
                later[p] = s
            else:
                later[p] |= s
            later[p].discard(p)
        later[v] = None
    return width


def tour(parent):
    """Euler tour of the forest (kids ascending, roots ascending): the node sequence with a
    node repeated after each kid, first[v], and v's subtree as the preorder range
    [tin[v], tout[v])."""
    n = len(parent)
    kids = [[] for _ in range(n)]
    for v in range(n):
        if parent[v] != INVALID:
            kids[parent[v]].append(v)
    seq, first, tin, tout, depth = [], [0] * n, [0] * n, [0] * n, [0] * n
    clock = 0
    for r in range(n):
        if parent[r] != INVALID:
            continue
        stack = [(r, 0)]
        tin[r] = clock
        clock += 1
        first[r] = len(seq)
        seq.append(r)
        while stack:
            v, i = stack.pop()
            if i < len(kids[v]):
                stack.append((v, i + 1))
                c = kids[v][i]
                depth[c] = depth[v] + 1
                tin[c] = clock
                clock += 1
                first[c] = len(seq)
                seq.append(c)
                stack.append((c, 0))
            else:
                tout[v] = clock
                if stack:
                    seq.append(stack[-1][0])
    return (np.array(seq, dtype=np.int64), np.array(first, dtype=np.int64), np.array(tin, dtype=np.int64),
            np.array(tout, dtype=np.int64), np.array(depth, dtype=np.int64))


def sparse_table(keys, op):
    rows = [np.asarray(keys)]
    half = 1
    while 2 * half <= len(keys):
        prev = rows[-1]
        rows.append(op(prev[:-half], prev[half:]))
        half *= 2
    return rows


def range_query(rows, p, q, op):
    k = np.floor(np.log2(q - p + 1)).astype(np.int64)
    out = np.empty(len(p), dtype=np.int64)
    for j in np.unique(k):
        m = k == j
        out[m] = op(rows[j][p[m]], rows[j][q[m] + 1 - (1 << j)])
    return out


def lca_min_depth(seq, depth, p, q):
    """Range-minimum over the tour's depth array (the textbook form)."""
    n1 = len(depth) + 1
    rows = sparse_table(depth[seq] * n1 + seq, np.minimum)
    return range_query(rows, p, q, np.minimum) % n1


def lca_max_id(seq, p, q):
    """The same node as the largest id of the tour range: a parent is later than its kids."""
    return range_query(sparse_table(seq, np.maximum), p, q, np.maximum)


def row_subtree(n, parent, lo, hi, lca="max_id", check=True):
    """The kernels' rule: sort (hi, tour position of lo); +1 per distinct lo, -1 at the lca of
    neighbours in the order, -1 at hi; width = 1 + the subtree sum."""
    seq, first, tin, tout, depth = tour(parent)
    if check:
        assert np.all((tin[hi] < tin[lo]) & (tin[lo] < tout[hi])), "an edge's lo is not below its hi"
    order = np.lexsort((first[lo], hi))
    lo, hi = lo[order], hi[order]
    wt = np.zeros(n, dtype=np.int64)
    np.add.at(wt, lo, 1)
    same = hi[1:] == hi[:-1]
    a, b = first[lo[:-1]][same], first[lo[1:]][same]
    anc = lca_max_id(seq, a, b) if lca == "max_id" else lca_min_depth(seq, depth, a, b)
    np.subtract.at(wt, anc, 1)
    np.subtract.at(wt, np.unique(hi), 1)
    pre = np.zeros(n + 1, dtype=np.int64)
    by_tin = np.zeros(n, dtype=np.int64)
    by_tin[tin] = wt
    pre[1:] = np.cumsum(by_tin)
    return 1 + pre[tout] - pre[tin]


def facts(parent, pst, width=None):
    """JNodeTable::Facts (jnode.cpp:256-290); width None = the placeholder 1 + pst."""
    n = len(parent)
    parent, pst = [int(x) for x in parent], [int(x) for x in pst]
    width = [1 + w for w in pst] if width is None else [int(x) for x in width]
    f = dict(width=0, root_cnt=0, vert_height=0, edge_height=0, vert_cnt=0, edge_cnt=0, halo_id=INVALID,
             core_id=INVALID, fill=0)
    vh, eh = [0] * n, [0] * n
    for i in range(n):
        f["vert_cnt"] += 1
        f["edge_cnt"] += pst[i]
        f["width"] = max(f["width"], width[i])
        f["fill"] = (f["fill"] + width[i] - pst[i] - 1) & MASK64   # size_t arithmetic
        vh[i] += 1
        eh[i] += pst[i]
        p = parent[i]
        if p != INVALID:
            vh[p] = max(vh[p], vh[i])
            eh[p] = max(eh[p], eh[i])
        else:
            f["vert_height"] = max(f["vert_height"], vh[i])
            f["edge_height"] = max(f["edge_height"], eh[i])
            f["root_cnt"] += 1
        if f["halo_id"] == INVALID and width[i] > 3:
            f["halo_id"] = i
        if f["core_id"] == INVALID and width[i] >= f["width"]:
            f["core_id"] = i
    return f


def facts_text(f):   # jnode.h:285-291
    return (f"TREEFAQS: width:{f['width']}\troots:{f['root_cnt']}\n"
            f"\tvheight:{f['vert_height']}\teheight:{f['edge_height']}\n"
            f"\tverts:{f['vert_cnt']}\tedges:{f['edge_cnt']}\n"
            f"\thalo:{f['halo_id']}\tcore:{f['core_id']}\n"
            f"\tfill:{f['fill']}\n")


def print_text(seq, parent, pst, width):   # JTree::print (jtree.h:60-66) + JNodeTable::print (jnode.h:263-267)
    return "".join("%4d:%-8d%6d:w%6d:pre%6d:pst        ->[%4d]\n" % (i, seq[i], width[i], 0, pst[i], parent[i])
                   for i in range(len(parent)))


def random_multigraph(rng, n_max=60):
    """Records over up to n_max vertex slots with self-loops, repeats and isolated slots, and
    a random sequence that leaves some slots out."""
    slots = int(rng.integers(1, n_max + 1))
    m = int(rng.integers(0, 3 * slots + 1))
    tail = rng.integers(0, slots, m)
    head = rng.integers(0, slots, m)
    if m:
        rep = rng.integers(0, m, m // 4)   # repeats, some reversed
        tail = np.concatenate([tail, head[rep[::2]], tail[rep[1::2]]])
        head = np.concatenate([head, tail[rep[::2]], head[rep[1::2]]])
    seq = rng.permutation(slots)[: int(rng.integers(0, slots + 1))]
    return tail.astype(np.uint32), head.astype(np.uint32), seq.astype(np.uint32)
