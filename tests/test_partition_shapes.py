"""sheep_partition / sheep_partition_pos, the kid table, sheep_facts and the tree merges on
hand-built trees (tests/partition_shapes.py) under every weight mode, balance and k class,
against the CPU oracle (forwardPartition, partition.cpp:50-157; Facts and merge,
jnode.cpp:174-201,256-290).  Integers throughout: every comparison is exact.

The shapes force the branches that elimination trees of power-law graphs never take: deep
cores (path, caterpillar, narrow, broom), an empty core (two_level), forests with packed
and childless roots, kid lists past the staging area (star), event tables past the
kernel-argument, LDS and k_event_loop sizes (k = 8192 on a path), 64-bit rake words and
no raking at all (wide weights), a zero total, and long runs of equal sort keys."""
import numpy as np
import pytest

import oracle
import partition_shapes as ps
from partition_shapes import INVALID

gpu = pytest.mark.gpu


def _unpackable_pst():
    pst = np.ones(ps.WIDE_N, np.uint32)
    pst[ps.WIDE_N // 2] = 10 ** 6   # alone above max_component = (total / 64) * 1.03 = 16,159
    return pst


# ------------------------------------------------------------------------------------
# CPU: the case lists are well formed and reach what they exist for
# ------------------------------------------------------------------------------------
def _packed_root(parent, parts):
    """A kid that kept a part of its own under a root was packed there (the descending
    pass gives every other kid its parent's part, partition.cpp:141-142)."""
    kid = np.flatnonzero(parent != INVALID)
    under_root = kid[parent[parent[kid]] == INVALID]
    return bool(np.any(parts[under_root] != parts[parent[under_root]]))


def test_partition_shape_cases_are_well_formed():
    """CPU: every generator gives parent[i] > i or INVALID; the oracle partitions every
    listed case without raising, below MAX_PARTS parts; and each threshold a case exists
    for really holds (so no case can silently stop reaching its branch)."""
    for name in ps.GENERATORS:
        p = ps.shape(name)
        assert p.dtype == np.uint32 and len(p) >= 1
        assert np.all((p == INVALID) | ((p > np.arange(len(p))) & (p < len(p)))), name
    assert [len(ps.shape(s)) for s in ps.TINY_SHAPES] == [1, 2, 3]
    assert np.all(ps.shape("tiny3") == INVALID)
    for name in ps.MERGE_SHAPES:
        p = ps.shape(name, 100_000)
        assert len(p) == 100_000 and np.all((p == INVALID) | ((p > np.arange(len(p))) & (p < len(p)))), name

    packed_roots = set()
    for sparse, cases in ((False, ps.ALL_CASES + ps.EVENT_LOOP_CASES), (True, ps.SPARSE_CASES)):
        for name, mode, balance, ks in cases:
            parent = ps.shape(name)
            total = int(ps.weights(name, mode)[3].sum())
            runs = ps.oracle_run(name, mode, balance, ks, sparse)   # raises if a case cannot be packed
            for k, (parts, info) in zip(ks, runs):
                tag = f"{name} {mode} b={balance} k={k}"
                assert info["created"] < ps.MAX_PARTS, tag
                assert info["max_component"] == ps.max_component_of(total, k, balance), tag
                assert len(parts) == (int(ps.sparse_seq(len(parent)).max()) + 1 if sparse else len(parent)), tag
                assert total < ps.RAKE_TOTAL_LIMIT and info["max_component"] < ps.LW32_LIMIT, tag
                if k == ps.K_EVENTS:   # past EV_ARG, EV_LDS and k_event_loop's table in one run
                    assert info["packing_nodes"] > max(ps.EV_ARG, ps.EV_LDS, ps.EVENT_LOOP_CAP), tag
                if mode == "pst_zero":
                    assert total == 0 and info == {"created": 1, "max_component": 0, "packing_nodes": 0}, tag
                if name == "two_level" and total and k <= 64:   # two rake rounds finish all but the root
                    assert np.all(ps.subtree_sums(name, mode)[:-1] <= info["max_component"]), tag
                if not sparse and _packed_root(parent, parts):
                    packed_roots.add(name)
    # kid lists past the staging area and past the LDS event table
    assert len(ps.shape("star")) - 1 > ps.EV_STAGE
    assert len(ps.shape("broom")) // 2 > ps.EV_LDS
    # forests: many roots, roots without kids, and packings at roots
    fp = ps.shape("forest")
    assert np.count_nonzero(fp == INVALID) > 3000 and np.count_nonzero(ps.shape("narrow") == INVALID) > 1
    assert np.any(np.bincount(fp[fp != INVALID], minlength=len(fp))[fp == INVALID] == 0)
    assert {"forest", "star", "two_level", "path"} <= packed_roots, packed_roots

    # wide weights: which side of each switch every k is on
    parent = ps.shape_wide()
    for wname, (kind, balance, ks, norake) in ps.WIDE_CASES.items():
        pst = ps.wide_pst(kind)
        for vtx, pstw in ps.WIDE_FLAGS:
            w = vtx + pst.astype(np.uint64)
            assert (int(w.sum()) >= ps.RAKE_TOTAL_LIMIT) == norake, wname
            for k, wide in ks.items():
                parts, info = oracle.partition(parent, pst, ps.identity_seq(ps.WIDE_N), k, balance, vtx, pstw)
                assert info["created"] < ps.MAX_PARTS
                assert (info["max_component"] >= ps.LW32_LIMIT) == wide, (wname, k, info)
                assert info["max_component"] >= int(w.max()) + (kind == "mixed"), (wname, k)
    assert int(ps.wide_pst("p28").astype(np.uint64).sum()) == ps.RAKE_TOTAL_LIMIT

    # the one case that cannot be packed
    with pytest.raises(RuntimeError):
        oracle.partition(parent, _unpackable_pst(), ps.identity_seq(ps.WIDE_N), 64)


# ------------------------------------------------------------------------------------
# GPU: partition parity
# ------------------------------------------------------------------------------------
def _check(res, parts, info, total, tag):
    assert np.array_equal(res.numpy(), parts), tag
    assert res.created == info["created"], tag
    assert res.packing_nodes == info["packing_nodes"], tag
    assert res.max_component == info["max_component"], tag
    assert res.total_weight == total, tag
    assert res.first_size == np.count_nonzero(parts == 0), tag
    assert res.second_size == np.count_nonzero(parts == 1), tag


def _run_case(case, sparse=False):
    """One case on the GPU: every k in order on one KidTable per use_pos variant (each keeps
    the kid order its earlier k left, as the oracle's Kids does), every result compared
    with the oracle's.  Returns sheep_partition_pos's result for every k."""
    import sheep_amd
    name, mode, balance, ks = case
    parent = ps.shape(name)
    vtx, pstw, pst, w = ps.weights(name, mode)
    total = int(w.sum())
    s = sheep_amd.sequence_from_host(ps.sparse_seq(len(parent)) if sparse else ps.identity_seq(len(parent)))
    tree = sheep_amd.tree_to_device(parent, pst)
    tables = {True: sheep_amd.KidTable(tree), False: sheep_amd.KidTable(tree)}
    out = []
    for k, (parts, info) in zip(ks, ps.oracle_run(name, mode, balance, ks, sparse)):
        for use_pos, kt in tables.items():
            res = sheep_amd.partition(s, tree, k, balance, bool(vtx), bool(pstw), kids=kt, use_pos=use_pos)
            _check(res, parts, info, total, f"{ps.case_id(case)} k={k} use_pos={use_pos} sparse={sparse}")
            if use_pos:
                out.append(res)
    return out


def _heavy(name, mode, res):
    """|{v : S(v) > max_component}|, the partitioner's heavy_nodes."""
    return int(np.count_nonzero(ps.subtree_sums(name, mode) > res.max_component))


@gpu
@pytest.mark.parametrize("case", ps.SHAPE_CASES, ids=ps.case_id)
def test_partition_shapes(gpu_ctx, case):
    """Every shape under every weight mode at balance 1.03 over its k list, both scatter
    variants, plus what proves that the shape's branch ran."""
    name, mode, _, ks = case
    n = len(ps.shape(name))
    for k, res in zip(ks, _run_case(case)):
        tag = f"{ps.case_id(case)} k={k}"
        if mode == "pst_zero":   # total == 0: max_component 0, nothing packs, one part
            assert (res.total_weight, res.max_component, res.packing_nodes, res.heavy_nodes, res.created) == \
                (0, 0, 0, 0, 1), tag
            continue
        if name in ("path", "caterpillar", "star", "two_level", "three_level"):
            assert res.heavy_nodes == _heavy(name, mode, res), tag
        if name == "two_level" and k <= 64:   # the rake finishes all but the root: a core without arcs
            assert res.heavy_nodes == (0 if k == 1 else 1), tag
        if name == "three_level" and k <= 64:   # the core is the path of 4 on top
            assert res.heavy_nodes <= 4, tag
        if name == "path" and mode == "unit" and k >= 2:   # one long tour, most of it heavy
            assert res.heavy_nodes == n - res.max_component >= n // 3, tag
        if name == "star" and k >= 2:
            # the root is the only packing node, and its 70,000 kids need k_event_kids twice
            # (EV_STAGE = 65,536 per launch) between two k_event_loop launches
            assert (res.packing_nodes, res.heavy_nodes) == (1, 1) and n - 1 > ps.EV_STAGE, tag
            assert res.event_launches >= 4, tag


@gpu
@pytest.mark.parametrize("case", ps.BALANCE_CASES, ids=ps.case_id)
def test_partition_balances(gpu_ctx, case):
    """balance 1.0 and 2.0 (partition_tree -b) on the deep, the forest and the shallow shape."""
    _run_case(case)


@gpu
@pytest.mark.parametrize("case", ps.EVENT_CASES, ids=ps.case_id)
def test_partition_event_table_sizes(gpu_ctx, case):
    """k = 8192 with unit weights: max_component is 12, so about every 12th spine node packs.
    The event table passes the kernel argument (EV_ARG), the LDS copy (EV_LDS) and the
    default k_event_loop capacity, after which every event is a k_event launch."""
    (res,) = _run_case(case)
    assert res.max_component == 12
    assert res.packing_nodes > 4096 == ps.EVENT_LOOP_CAP == ps.EV_LDS > ps.EV_ARG
    assert res.event_launches >= res.packing_nodes - ps.EVENT_LOOP_CAP   # the hand-over happened


@gpu
@pytest.mark.parametrize("case", ps.TIE_CASES, ids=ps.case_id)
def test_partition_kid_order_under_ties(gpu_ctx, case):
    """Unit weights: the host std::sort permutes long runs of equal keys, and the order it
    uploads into the kid table decides every later k on that table.  One KidTable and one
    oracle.Kids through k = 64, 1000, 7, 256, 2, compared after every k."""
    assert case[3] == (64, 1000, 7, 256, 2)
    res = _run_case(case)
    assert all(r.packing_nodes > 0 for r in res)


@gpu
@pytest.mark.parametrize("case", ps.SPARSE_CASES, ids=ps.case_id)
def test_partition_sparse_sequence(gpu_ctx, case):
    """vid = 3 * perm[j] + 5: both scatter variants fill a parts vector of about 3n slots,
    the unsequenced ones with INVALID_PART."""
    n = len(ps.shape(case[0]))
    for res in _run_case(case, sparse=True):
        parts = res.numpy()
        assert len(parts) == int(ps.sparse_seq(n).max()) + 1 > 2 * n
        assert np.count_nonzero(parts == -1) == len(parts) - n


@gpu
@pytest.mark.parametrize("event_loop", [0, 3, None])
@pytest.mark.parametrize("case", ps.EVENT_LOOP_CASES, ids=ps.case_id)
def test_partition_shapes_event_loop_variants(gpu_ctx, case, event_loop):
    """sheep_tuning event_loop 0 (a k_event launch per event), 3 (k_event_loop hands over
    after three table entries) and the default, on the 8192-part path and on a forest."""
    gpu_ctx.set_tuning(**({} if event_loop is None else {"event_loop": event_loop}))
    try:
        for res in _run_case(case):
            if event_loop == 0:   # one launch per event and one for the empty search
                assert res.event_launches >= res.packing_nodes + 1
    finally:
        gpu_ctx.set_tuning()


# ------------------------------------------------------------------------------------
# GPU: wide weights
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", ps.WIDE_FLAGS, ids=["pst", "both"])
@pytest.mark.parametrize("wname", list(ps.WIDE_CASES))
def test_partition_wide_weights(gpu_ctx, wname, flags):
    """Constant weights of 2^26, 2^28 and 2^31 and random 32-bit ones on a 4096-node tree:
    max_component on both sides of 2^32 - 1 (k_rake_init / k_rake_pull1 on u64 or u32
    words) and totals from 2^40 on (no raking, k_core_flags)."""
    import sheep_amd
    kind, balance, ks, norake = ps.WIDE_CASES[wname]
    vtx, pstw = flags
    parent, pst = ps.shape_wide(), ps.wide_pst(kind)
    total = int((vtx + pst.astype(np.uint64)).sum())
    s = sheep_amd.sequence_from_host(ps.identity_seq(ps.WIDE_N))
    tree = sheep_amd.tree_to_device(parent, pst)
    okids = oracle.Kids(parent)
    tables = {True: sheep_amd.KidTable(tree), False: sheep_amd.KidTable(tree)}
    for k, wide in ks.items():
        parts, info = oracle.partition(parent, pst, ps.identity_seq(ps.WIDE_N), k, balance, vtx, pstw, okids)
        for use_pos, kt in tables.items():
            res = sheep_amd.partition(s, tree, k, balance, bool(vtx), bool(pstw), kids=kt, use_pos=use_pos)
            tag = f"{wname} k={k} use_pos={use_pos}"
            _check(res, parts, info, total, tag)
            if wide:
                assert res.max_component >= 2 ** 32 - 1, tag
            else:
                assert res.max_component < 2 ** 32 - 1, tag
            if norake:
                assert res.total_weight >= 2 ** 40, tag
            else:
                assert res.total_weight < 2 ** 40, tag
            assert res.packing_nodes > 0, tag


# ------------------------------------------------------------------------------------
# GPU: the "cannot pack" return
# ------------------------------------------------------------------------------------
@gpu
def test_partition_cannot_pack_then_recovers(gpu_ctx):
    """One node heavier than max_component: the oracle throws, sheep_partition returns
    SHEEP_ERR_PACK (-4), and its catch released k_event_loop: the next partition on the same
    context, with fresh kid tables on both sides, matches the oracle again."""
    import sheep_amd
    parent, pst = ps.shape_wide(), _unpackable_pst()
    s = sheep_amd.sequence_from_host(ps.identity_seq(ps.WIDE_N))
    tree = sheep_amd.tree_to_device(parent, pst)
    with pytest.raises(RuntimeError, match="oracle"):
        oracle.partition(parent, pst, ps.identity_seq(ps.WIDE_N), 64)
    for use_pos in (True, False):
        with pytest.raises(RuntimeError, match="sheep_hip error -4"):
            sheep_amd.partition(s, tree, 64, use_pos=use_pos)
        _run_case(("forest", "both_uniform", 1.03, (64,)))
    # and the same tree is packable at a k whose max_component exceeds the heavy node
    parts, info = oracle.partition(parent, pst, ps.identity_seq(ps.WIDE_N), 1)
    res = sheep_amd.partition(s, tree, 1)
    _check(res, parts, info, int(pst.sum()), "k=1 after the error")


# ------------------------------------------------------------------------------------
# GPU: facts and merges on the same shapes
# ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["zero", "uniform", "wide"])
@pytest.mark.parametrize("name", list(ps.GENERATORS))
def test_facts_shapes(gpu_ctx, name, kind):
    import sheep_amd
    parent = ps.shape(name)
    n = len(parent)
    pst = ps.pst_of(kind, n)
    f = sheep_amd.facts(sheep_amd.tree_to_device(parent, pst)).__dict__
    assert f == oracle.facts(parent, pst)
    assert f["vert_cnt"] == n and f["root_cnt"] == np.count_nonzero(parent == INVALID)
    if name == "path":
        assert f["vert_height"] == n
    if kind == "wide" and name in ps.BIG_SHAPES:   # 64-bit sums
        assert f["edge_cnt"] == n << 26 > 2 ** 32
        if name in ("path", "caterpillar", "broom", "narrow", "forest"):
            assert f["edge_height"] > 2 ** 32


@gpu
def test_facts_root_without_kids(gpu_ctx):
    """A root without kids is on no tour: its own pst is its edge height, and the tree's
    when no path under another root is heavier (regression: it was left out, so a single
    node, or a forest whose heaviest root had no kids, reported too small an edge height)."""
    import sheep_amd
    parent = np.array([INVALID, 2, INVALID, 4, INVALID], np.uint32)
    for pst in ([7, 1, 2, 0, 0], [2, 1, 2, 9, 1], [0, 0, 0, 0, 11]):
        pst = np.array(pst, np.uint32)
        f = sheep_amd.facts(sheep_amd.tree_to_device(parent, pst)).__dict__
        assert f == oracle.facts(parent, pst)
        assert f["edge_height"] == max(pst[0], pst[1] + pst[2], pst[3] + pst[4])


@gpu
@pytest.mark.parametrize("a,b", [("path", "star"), ("caterpillar", "recursive"), ("forest", "narrow")])
def test_merge_shapes(gpu_ctx, a, b):
    """sheep_merge_trees on trees that are no shards of one graph, at a common n = 100,000."""
    import sheep_amd
    ta, tb = ps.merge_tree(a), ps.merge_tree(b)
    p, w = sheep_amd.tree_to_numpy(sheep_amd.merge_trees(sheep_amd.tree_to_device(*ta), sheep_amd.tree_to_device(*tb)))
    op, ow = oracle.merge(*ta, *tb)
    assert np.array_equal(p, op) and np.array_equal(w, ow)


@gpu
def test_merge_many_shapes(gpu_ctx):
    """sheep_merge_trees_many over all the merge shapes == the left fold of the oracle's merge."""
    import sheep_amd
    import torch
    trees = [ps.merge_tree(name) for name in ps.MERGE_SHAPES]
    p, w = sheep_amd.tree_to_numpy(sheep_amd.merge_trees_many(torch.stack([sheep_amd.tree_to_device(*t) for t in trees])))
    op, ow = trees[0]
    for t in trees[1:]:
        op, ow = oracle.merge(op, ow, *t)
    assert np.array_equal(p, op) and np.array_equal(w, ow)
