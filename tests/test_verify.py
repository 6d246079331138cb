"""Verify a tree against its graph (sheep_verify_*, graph2tree -c, verify_tree): a forest is
the elimination tree of the records under the sequence exactly when parents are later, every
edge's earlier end lies below its later end, every non-root's subtree is adjacent to its
parent, and the pst weights are the records' counts (tests/verify_model.py).

CPU: the certificate against the oracle's tree on mutated trees of random multigraphs, the
golden trees, and verify_tree's argument errors.  GPU: the kernels against the model, field
by field (integers: the bar is equality), closed forms past one workgroup of every pass,
a device-built tree, shards, errors and handle lifetime, and the CLIs.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import verify_model as vm
import widths_model as wm
from conftest import GOLDEN, golden_records, golden_seq, golden_tree, ROOT

BIN = os.environ.get("SHEEP_BIN_DIR") or os.path.join(ROOT, "sheep_amd", "bin")
INVALID = vm.INVALID
KINDS = ("none", "to_ancestor", "to_non_ancestor", "attach_root", "detach", "pst", "parent_le_id", "parent_ge_n",
         "drop_record", "add_record")


def ancestors(parent, v):
    out = []
    while parent[v] != INVALID:
        v = int(parent[v])
        out.append(v)
    return out


def mutate(kind, rng, tail, head, seq, parent, pst):
    """One mutation of `kind` applied to copies: (tail, head, parent, pst), or None where the
    input has no place for it (a tree without a non-root cannot be detached, ...)."""
    tail, head, parent, pst = tail.copy(), head.copy(), parent.astype(np.int64), pst.astype(np.int64)
    n = len(parent)
    nonroots = np.flatnonzero(parent != INVALID)
    pick = lambda a: int(a[rng.integers(0, len(a))])
    if kind == "none":
        pass
    elif kind == "to_ancestor":       # a proper ancestor other than the parent
        deep = nonroots[parent[parent[nonroots]] != INVALID] if len(nonroots) else nonroots
        if not len(deep):
            return None
        v = pick(deep)
        parent[v] = pick(ancestors(parent, v)[1:])
    elif kind == "to_non_ancestor":   # a later node that is no ancestor
        for v in rng.permutation(nonroots)[:8].tolist():
            anc = set(ancestors(parent, v))
            others = [u for u in range(v + 1, n) if u not in anc]
            if others:
                parent[v] = pick(others)
                break
        else:
            return None
    elif kind == "attach_root":       # a root's component has no edge to any later node
        roots = np.flatnonzero(parent[: max(n - 1, 0)] == INVALID)
        if not len(roots):
            return None
        r = pick(roots)
        parent[r] = int(rng.integers(r + 1, n))
    elif kind == "detach":
        if not len(nonroots):
            return None
        parent[pick(nonroots)] = INVALID
    elif kind == "pst":
        if not n:
            return None
        v = int(rng.integers(0, n))
        pst[v] += -1 if pst[v] > 0 and rng.integers(0, 2) else 1
    elif kind == "parent_le_id":
        if not n:
            return None
        v = int(rng.integers(0, n))
        parent[v] = int(rng.integers(0, v + 1))
    elif kind == "parent_ge_n":
        if not n:
            return None
        parent[int(rng.integers(0, n))] = n + int(rng.integers(0, 3))
    elif kind == "drop_record":
        if not len(tail):
            return None
        i = int(rng.integers(0, len(tail)))
        tail, head = np.delete(tail, i), np.delete(head, i)
    elif kind == "add_record":        # one more edge between two sequenced vertices
        if len(seq) < 2:
            return None
        a, b = rng.choice(len(seq), 2, replace=False)
        i = int(rng.integers(0, len(tail) + 1))
        tail, head = np.insert(tail, i, seq[a]), np.insert(head, i, seq[b])
    else:
        raise KeyError(kind)
    return tail, head, parent.astype(np.uint32), pst.astype(np.uint32)


def oracle_tree(tail, head, seq):
    """The oracle's (parent, pst), or None where index.at() throws (a neighbour beyond the
    sequence's largest vid)."""
    import oracle
    try:
        return oracle.build_tree(tail, head, seq)
    except RuntimeError as e:
        assert "range" in str(e) or "index" in str(e), e
        return None


N_CASES = 300


@functools.lru_cache(maxsize=None)
def cases():
    """300 seeded multigraphs (n <= 60, self-loops, repeats, isolated slots, unsequenced ends)
    that the map accepts, each with one mutation, plus the graphs it rejects with a range
    error.  (kind, tail, head, seq, parent, pst, want_ok) and (tail, head, seq)."""
    rng = np.random.default_rng(2024)
    good, ranged = [], []
    while len(good) < N_CASES:
        tail, head, seq = wm.random_multigraph(rng)
        tree = oracle_tree(tail, head, seq)
        if tree is None:
            ranged.append((tail, head, seq))
            continue
        m, k = None, len(good)
        while m is None:              # the next kind this graph has a place for ("none" always has)
            kind = KINDS[k % len(KINDS)]
            m = mutate(kind, rng, tail, head, seq, *tree)
            k += 1
        mt, mh, parent, pst = m
        after = oracle_tree(mt, mh, seq)
        assert after is not None
        want = np.array_equal(parent, after[0]) and np.array_equal(pst, after[1])
        good.append((kind, mt, mh, seq, parent, pst, bool(want)))
    return good, ranged


# ---- CPU: the certificate -----------------------------------------------------------------
def test_certificate_is_the_oracles_tree_on_mutated_random_multigraphs():
    """ok == "the (mutated) tree is the oracle's tree of the (changed) records", both ways."""
    good, ranged = cases()
    seen = {k: 0 for k in KINDS}
    rejected = {k: 0 for k in KINDS}
    for kind, tail, head, seq, parent, pst, want in good:
        v = vm.verify(tail, head, seq, parent, pst)
        assert v == vm.verify_literal(tail, head, seq, parent, pst), kind
        assert v["ok"] == want, (kind, v)
        seen[kind] += 1
        rejected[kind] += not v["ok"]
    assert all(seen[k] >= 15 for k in KINDS), seen
    assert all(rejected[k] >= 1 for k in KINDS if k != "none"), rejected
    assert rejected["none"] == 0
    assert ranged   # the generator reaches the range error too
    for tail, head, seq in ranged:
        roots = np.full(len(seq), INVALID, dtype=np.uint32)
        for f in (vm.verify, vm.verify_literal):
            with pytest.raises(IndexError):
                f(tail, head, seq, roots, np.zeros(len(seq), dtype=np.uint32))


def test_structure_failure_is_final():
    """With a bad parent the other classes read 0, whatever the records say."""
    tail, head = np.array([0, 1, 2], np.uint32), np.array([1, 2, 3], np.uint32)
    v = vm.verify(tail, head, np.arange(4), [1, 1, 9, INVALID], [5, 5, 5, 5])
    assert v == dict(ok=False, bad_parent=2, not_descendant=0, unsupported=0, pst_mismatch=0, first_bad_parent=1,
                     first_not_descendant=vm.NO_ID, first_unsupported=vm.NO_ID, first_pst_mismatch=vm.NO_ID)


@pytest.mark.parametrize("name", ["hep", "edge", "rmat10", "rmat12", "rmat14"])
def test_golden_trees_are_valid(name):
    r = golden_records(name)
    v = vm.verify(r["tail"], r["head"], golden_seq(name), *golden_tree(name))
    assert v["ok"], v


@pytest.mark.parametrize("name", ["hep", "rmat10"])
def test_golden_half_tree_is_valid_for_its_half_only(name):
    r, seq = golden_records(name), golden_seq(name)
    R = len(r)
    for part, which in ((1, "h1.tre"), (2, "h2.tre")):
        half = r[(part - 1) * R // 2: part * R // 2]
        parent, pst = golden_tree(name, which)
        assert vm.verify(half["tail"], half["head"], seq, parent, pst)["ok"], which
        v = vm.verify(r["tail"], r["head"], seq, parent, pst)
        assert not v["ok"] and v["bad_parent"] == 0 and v["pst_mismatch"] > 0, (which, v)
    merged = golden_tree(name, "merge.tre")
    assert vm.verify(r["tail"], r["head"], seq, *merged)["ok"]


def run_verify_tree(*args):
    exe = os.path.join(BIN, "verify_tree")
    assert os.path.exists(exe), "verify_tree is not built (make cli)"
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)


def test_verify_tree_argument_errors(tmp_path):
    """Usage, unreadable files and a malformed -l end with status 1 before any device is opened."""
    usage = "USAGE: verify_tree input_graph input_sequence input_tree [-l n/k] [-v]\n"
    g = lambda ext: os.path.join(GOLDEN, f"hep.{ext}")
    for args in ((), (g("dat"),), (g("dat"), g("seq")), (g("dat"), g("seq"), g("tre"), "extra")):
        p = run_verify_tree(*args)
        assert p.returncode == 1 and p.stdout == usage, args
    missing = tmp_path / "missing"
    for i in range(3):
        args = [g("dat"), g("seq"), g("tre")]
        args[i] = missing
        p = run_verify_tree(*args)
        assert p.returncode == 1 and p.stdout == f"verify_tree: cannot read {missing}\n", i
    for bad in ("3/2", "0/2", "1", "1/", "/2", "1/2x", "a/b", "-1/2"):
        p = run_verify_tree(g("dat"), g("seq"), g("tre"), "-l", bad)
        assert p.returncode == 1 and p.stdout == "Option -l requires n/k with 1 <= n <= k.\n", bad
    p = run_verify_tree(g("dat"), g("seq"), g("tre"), "-q")
    assert p.returncode == 1 and p.stdout.startswith("Unknown option character")


# ---- GPU ------------------------------------------------------------------------------------
def as_dict(res):
    return {f: (bool(getattr(res, f)) if f == "ok" else int(getattr(res, f))) for f in vm.FIELDS}


def gpu_verdict(tail, head, seq, parent, pst):
    import sheep_amd
    d = sheep_amd.records_to_device(np.asarray(tail, np.uint32), np.asarray(head, np.uint32))
    s = sheep_amd.sequence_from_host(np.asarray(seq, np.uint32))
    t = sheep_amd.tree_to_device(np.asarray(parent, np.uint32), np.asarray(pst, np.uint32))
    return as_dict(sheep_amd.verify_tree(d, s, t))


@pytest.mark.gpu
def test_random_graphs_match_the_model(gpu_ctx):
    good, ranged = cases()
    for kind, tail, head, seq, parent, pst, want in good:
        assert gpu_verdict(tail, head, seq, parent, pst) == vm.verify(tail, head, seq, parent, pst), kind
    for tail, head, seq in ranged[:20]:
        with pytest.raises(IndexError):
            gpu_verdict(tail, head, seq, np.full(len(seq), INVALID), np.zeros(len(seq)))


def path(n):
    i = np.arange(n - 1)
    parent = np.append(i + 1, INVALID)
    return i, i + 1, parent, np.append(np.ones(n - 1, np.int64), 0)


def star(k):   # the hub is last: one kid segment of k entries
    parent = np.append(np.full(k, k), INVALID)
    return np.arange(k), np.full(k, k), parent, np.append(np.ones(k, np.int64), 0)


def disjoint_edges(k):
    i = 2 * np.arange(k)
    parent = np.full(2 * k, INVALID, dtype=np.int64)
    parent[i] = i + 1
    pst = np.zeros(2 * k, np.int64)
    pst[i] = 1
    return i, i + 1, parent, pst


def caterpillar(spine, legs):   # legs first, then the spine as a path: segments of legs (+ 1) kids, depth = spine
    k = spine * legs
    leg, s = np.arange(k), k + np.arange(spine)
    tail = np.concatenate([leg, s[:-1]])
    head = np.concatenate([k + leg // legs, s[1:]])
    parent = np.concatenate([k + leg // legs, s[1:], [INVALID]])
    pst = np.append(np.ones(k + spine - 1, np.int64), 0)
    return tail, head, parent, pst


CLOSED = {"path": lambda: path(100_000), "star": lambda: star(100_000), "disjoint": lambda: disjoint_edges(50_000),
          "caterpillar": lambda: caterpillar(1000, 100)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(CLOSED))
def test_closed_forms(gpu_ctx, shape):
    """Valid as built (by hand, not by the builder); then one seeded mutation of every kind
    the shape has a place for, against the model's counts."""
    tail, head, parent, pst = CLOSED[shape]()
    n = len(parent)
    seq = np.arange(n)
    valid = dict(ok=True, bad_parent=0, not_descendant=0, unsupported=0, pst_mismatch=0, first_bad_parent=vm.NO_ID,
                 first_not_descendant=vm.NO_ID, first_unsupported=vm.NO_ID, first_pst_mismatch=vm.NO_ID)
    assert gpu_verdict(tail, head, seq, parent, pst) == valid
    rng = np.random.default_rng(n)
    tried = []
    for kind in KINDS[1:]:
        m = mutate(kind, rng, tail, head, seq, parent, pst)
        if m is None:
            continue
        mt, mh, mp, mw = m
        want = vm.verify(mt, mh, seq, mp, mw)
        assert not want["ok"], kind
        assert gpu_verdict(mt, mh, seq, mp, mw) == want, kind
        tried.append(kind)
    # (one root, the last node: no root to attach; a path has only ancestors above a node; depth 1 has no grandparent)
    nowhere = {"path": {"to_non_ancestor", "attach_root"}, "star": {"to_ancestor", "attach_root"},
               "disjoint": {"to_ancestor"}, "caterpillar": {"attach_root"}}
    assert set(tried) == set(KINDS[1:]) - nowhere[shape]
    if shape == "star":   # the counts by the closed form itself: every leaf loses its hub
        mp = parent.copy()
        mp[:] = INVALID
        v = gpu_verdict(tail, head, seq, mp, pst)
        assert (v["not_descendant"], v["first_not_descendant"], v["unsupported"], v["pst_mismatch"]) == (n - 1, 0, 0, 0)
    if shape == "path":   # cut in the middle: one record leaves its subtree, nothing else changes
        mp = parent.copy()
        mp[n // 2] = INVALID
        v = gpu_verdict(tail, head, seq, mp, pst)
        assert (v["not_descendant"], v["first_not_descendant"], v["unsupported"], v["pst_mismatch"]) == (1, n // 2, 0, 0)


@pytest.mark.gpu
def test_empty_inputs(gpu_ctx):
    none = np.zeros(0, dtype=np.uint32)
    roots, zeros = np.full(5, INVALID), np.zeros(5)
    assert gpu_verdict(none, none, none, none, none)["ok"]                      # n == 0
    assert gpu_verdict(np.arange(3), np.arange(3) + 1, none, none, none)["ok"]  # n == 0, records of no sequenced vertex
    assert gpu_verdict(none, none, np.arange(5), roots, zeros)["ok"]            # nrec == 0
    loops = np.arange(5)
    assert gpu_verdict(loops, loops, np.arange(5), roots, zeros)["ok"]          # self-loops only
    for tail, head in ((none, none), (loops, loops)):
        v = gpu_verdict(tail, head, np.arange(5), [1, INVALID, INVALID, 4, INVALID], [0, 0, 2, 0, 0])
        assert v == vm.verify(tail, head, np.arange(5), [1, INVALID, INVALID, 4, INVALID], [0, 0, 2, 0, 0])
        assert (v["unsupported"], v["first_unsupported"], v["pst_mismatch"], v["first_pst_mismatch"]) == (2, 0, 1, 2)


@pytest.mark.gpu
def test_device_built_tree_and_the_case_the_old_check_missed(gpu_ctx):
    """An RMAT-18 tree from the builder is valid.  One root component hung under a later,
    unrelated node keeps every edge's earlier end below its later end — sheep_tree_widths
    accepts that input, and the structural check of the old graph2tree -c did — but the
    component has no edge to its new parent: unsupported == 1 and nothing else."""
    import sheep_amd
    d = sheep_amd.rmat(18, 16, 18)
    s = sheep_amd.degree_sequence(d)
    tree = sheep_amd.build_tree(d, s)
    v = as_dict(sheep_amd.verify_tree(d, s, tree))
    assert v["ok"] and sum(v[f] for f in vm.FIELDS[1:5]) == 0, v
    parent, pst = sheep_amd.tree_to_numpy(tree)
    n = len(parent)
    roots = np.flatnonzero(parent[: n - 1] == INVALID)
    assert len(roots), "the graph has one component only: pick another seed"
    r = int(roots[0])
    parent[r] = n - 1
    hung = sheep_amd.tree_to_device(parent, pst)
    v = as_dict(sheep_amd.verify_tree(d, s, hung))
    assert v == dict(ok=False, bad_parent=0, not_descendant=0, unsupported=1, pst_mismatch=0,
                     first_bad_parent=vm.NO_ID, first_not_descendant=vm.NO_ID, first_unsupported=r,
                     first_pst_mismatch=vm.NO_ID)
    sheep_amd.tree_widths(d, s, hung)   # no error: the descent test alone cannot see it


@pytest.mark.gpu
def test_shards(gpu_ctx):
    import sheep_amd
    import torch
    d = sheep_amd.rmat(16, 16, 16)
    s = sheep_amd.degree_sequence(d)
    R = d.shape[0]
    shards = [d[j * R // 4: (j + 1) * R // 4].contiguous() for j in range(4)]
    trees = [sheep_amd.build_tree(x, s).clone() for x in shards]
    for x, t in zip(shards, trees):
        assert sheep_amd.verify_tree(x, s, t).ok
    assert not sheep_amd.verify_tree(d, s, trees[0]).ok          # a shard's tree is not the whole graph's
    merged = sheep_amd.merge_trees_many(torch.stack(trees))
    whole = sheep_amd.verify_tree(d, s, merged)
    assert whole.ok
    tv = sheep_amd.TreeVerifier(s, merged)
    for j in (2, 0, 3, 1):
        tv.add(shards[j])
    assert tv.finish() == whole
    tv.close()
    tv = sheep_amd.TreeVerifier(s, merged)
    for j in (3, 1, 0):
        tv.add(shards[j])
    part = tv.finish()
    assert not part.ok and part.bad_parent == 0 and part.pst_mismatch > 0
    tv.add(shards[2])                                            # the missing shard, after a finish
    assert tv.finish() == whole
    tv.close()


@pytest.mark.gpu
def test_errors_and_handle_lifetime(gpu_ctx):
    import sheep_amd
    tail, head = np.array([0, 1, 2], np.uint32), np.array([1, 2, 7], np.uint32)   # 7 >= pos_size = 4
    seq = np.arange(4, dtype=np.uint32)
    d, s = sheep_amd.records_to_device(tail, head), sheep_amd.sequence_from_host(seq)
    good = sheep_amd.records_to_device(tail[:2], head[:2])
    t = sheep_amd.tree_to_device([1, 2, INVALID, INVALID], [1, 1, 0, 0])
    with pytest.raises(IndexError):
        sheep_amd.verify_tree(d, s, t)
    tv = sheep_amd.TreeVerifier(s, t)
    with pytest.raises(IndexError):
        tv.add(d)
    with pytest.raises(IndexError):     # no verdict after a failed add
        tv.finish()
    tv.close()
    tv = sheep_amd.TreeVerifier(s, t)   # destroyed before finish
    tv.add(good)
    tv.close()
    tv.close()
    # two handles live on one context, their adds interleaved
    other = sheep_amd.tree_to_device([1, 3, INVALID, INVALID], [1, 1, 0, 0])
    a, b = sheep_amd.TreeVerifier(s, t), sheep_amd.TreeVerifier(s, other)
    a.add(good[:1].contiguous())
    b.add(good)
    a.add(good[1:].contiguous())
    assert as_dict(a.finish()) == vm.verify(tail[:2], head[:2], seq, [1, 2, INVALID, INVALID], [1, 1, 0, 0])
    assert as_dict(b.finish()) == vm.verify(tail[:2], head[:2], seq, [1, 3, INVALID, INVALID], [1, 1, 0, 0])
    assert a.finish().ok and not b.finish().ok
    a.close()
    b.close()
    assert sheep_amd.verify_tree(good, s, t).ok   # the context is usable afterwards


@pytest.mark.gpu
def test_timers_are_named(gpu_ctx):
    import sheep_amd
    r = golden_records("rmat10")
    d = sheep_amd.records_to_device(r["tail"], r["head"])
    s = sheep_amd.sequence_from_host(golden_seq("rmat10"))
    t = sheep_amd.tree_to_device(*golden_tree("rmat10"))
    gpu_ctx.timing(True)
    try:
        gpu_ctx.timer_reset()
        assert sheep_amd.verify_tree(d, s, t).ok
        names = set(gpu_ctx.timer_names())
    finally:
        gpu_ctx.timing(False)
    assert {"verify", "verify_structure", "verify_tour", "verify_records", "verify_finish"} <= names


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hep", "edge", "rmat10", "rmat12", "rmat14"])
def test_golden_trees_on_the_gpu(gpu_ctx, name):
    r, seq = golden_records(name), golden_seq(name)
    parent, pst = golden_tree(name)
    assert gpu_verdict(r["tail"], r["head"], seq, parent, pst)["ok"]
    R = len(r)
    hp, hw = golden_tree(name, "h1.tre")
    assert gpu_verdict(r["tail"][: R // 2], r["head"][: R // 2], seq, hp, hw)["ok"]
    assert gpu_verdict(r["tail"], r["head"], seq, hp, hw) == vm.verify(r["tail"], r["head"], seq, hp, hw)


# ---- GPU: the CLIs --------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_verify_tree(gpu_ctx, tmp_path):
    g = lambda ext: os.path.join(GOLDEN, f"hep.{ext}")
    for seq in (g("seq"), "-"):
        p = run_verify_tree(g("dat"), seq, g("tre"))
        assert (p.returncode, p.stdout) == (0, "Tree is valid.\n"), p.stdout + p.stderr
    p = run_verify_tree(g("dat"), g("seq"), g("h1.tre"), "-l", "1/2")
    assert (p.returncode, p.stdout) == (0, "Tree is valid.\n"), p.stdout + p.stderr
    # one parent word rewritten: node 0 hung under the last node
    parent, pst = golden_tree("hep")
    n = len(parent)
    assert parent[0] != n - 1
    parent[0] = n - 1
    raw = np.empty(1 + 2 * n, dtype=np.uint32)
    raw[0], raw[1::2], raw[2::2] = n, parent, pst
    bad = tmp_path / "bad.tre"
    raw.tofile(bad)
    r = golden_records("hep")
    want = vm.verify(r["tail"], r["head"], golden_seq("hep"), parent, pst)
    assert not want["ok"]
    p = run_verify_tree(g("dat"), g("seq"), bad)
    assert (p.returncode, p.stdout) == (2, "ERROR: Tree is not valid.\n" + vm.counts_line(want)), p.stdout + p.stderr
    p = run_verify_tree(g("dat"), g("seq"), g("h1.tre"))   # a half tree against the whole file
    half = vm.verify(r["tail"], r["head"], golden_seq("hep"), *golden_tree("hep", "h1.tre"))
    assert (p.returncode, p.stdout) == (2, "ERROR: Tree is not valid.\n" + vm.counts_line(half))


@pytest.mark.gpu
def test_cli_graph2tree_c(gpu_ctx):
    exe = os.path.join(BIN, "graph2tree")
    dat = os.path.join(GOLDEN, "hep.dat")
    for flags in ((), ("-s", os.path.join(GOLDEN, "hep.seq")), ("-l", "1/2", "-s", os.path.join(GOLDEN, "hep.seq"))):
        p = subprocess.run([exe, dat, "-c", *flags], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.splitlines()[-1] == "Tree is valid.", p.stdout
