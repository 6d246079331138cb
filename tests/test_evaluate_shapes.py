"""The evaluator (sheep_amd/csrc/evaluate.hip: sheep_evaluate, sheep_evaluate_step, the
sharded sheep_eval_shard / _combine / _finish, sheep_edge_parts) under arbitrary int16 part
vectors, bit-exact against a plain model of the definition (tests/evaluate_model.py).

The other evaluator tests feed it what sheep_partition produced: a few hundred parts at the
most, neighbouring records mostly in one part.  The cases of tests/evaluate_shapes.py go up
to 32,768 parts (the int16 ceiling) on graphs of at most 2^12 vertex slots and pin both sides
of every switch in the kernels: 64 -> 65 and 128 -> 129 parts (the bitset word count, the
16-byte row kernel, the wave-combined tail runs), 2048 -> 2049 (balance histograms in LDS or
by global atomics), part ids with gaps, a vertex whose neighbours cover every part, vertices
whose only record is a self-loop, and waves of 64 different parts (wave_count's per-lane
fallback).

CPU: the model against the reference's printed numbers (golden), against the oracle, the
coverage the case list claims, and the edge owners.  GPU: every case, every metric mask,
the record and the step-edge form, the sharded form, the edge owners, the errors."""
import time

import numpy as np
import pytest

import evaluate_model as model
import evaluate_shapes as es
import oracle
from conftest import golden_part_text, golden_parts, golden_records, golden_seq, ks
from test_partition_files import restate, write_cases

ORACLE_K_CAP = 1 << 15   # (no cap below the largest k: see test_model_matches_oracle)


# ------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hep", "edge", "rmat10"])
def test_model_reproduces_golden_text(name):
    """The model's counts, rendered by EvalResult.text, are the lines the reference printed
    (partition_tree -f -g) for the reference's own parts at every golden k."""
    import sheep_amd
    rec, seq = golden_records(name), golden_seq(name)
    _, blocks = golden_part_text(name)
    assert len(blocks) == len(ks(name))
    for k, block in zip(ks(name), blocks):
        got = model.evaluate(rec["tail"], rec["head"], seq, golden_parts(name, k))
        want = "".join(block.splitlines(keepends=True)[2:])   # (after the two Partition::print lines)
        assert want.startswith("edges cut: ")
        assert sheep_amd.EvalResult(**got).text(k) == want, f"k={k}"
        assert oracle.eval_text(got, k) == want, f"k={k}"


@pytest.mark.parametrize("case", es.CASES, ids=es.case_id)
def test_model_matches_oracle(case):
    """Field for field on every case, the largest k included: the oracle's per-node sets are
    sized by the part count but cleared through a list of the words touched, so its time does
    hardly grows with k: rmat12_mixed/random at 32,768 parts took 0.36 s at worst (a first
    call) and 0.008 s repeated, against 0.43 s and 0.008 s at 2 parts; the stars under 0.01 s
    (one thread).  The comparison is not capped."""
    name, gen, k = case
    assert k <= ORACLE_K_CAP
    t, h, seq, _ = es.graph(name)
    t0 = time.perf_counter()
    got = oracle.evaluate(t, h, seq, es.parts(name, gen, k))
    print(f"oracle.evaluate {es.case_id(case)}: {time.perf_counter() - t0:.3f} s")
    assert es.expected(name, gen, k)[0] == got


def test_masked():
    full = {f: i + 1 for i, f in enumerate(oracle.EVAL_FIELDS)}
    assert tuple(full) == model.FIELDS
    assert model.masked(full, 0) == full == model.masked(full, 7)
    for what, zero in [(1, ("ecv_down", "max_down_bal", "ecv_up", "max_up_bal")),
                       (2, ("edges_cut", "vcom_vol", "max_vertex_bal", "ecv_hash", "max_hash_bal", "ecv_up", "max_up_bal")),
                       (6, ("edges_cut", "vcom_vol", "max_vertex_bal", "ecv_hash", "max_hash_bal")),
                       (5, ("ecv_down", "max_down_bal"))]:
        assert model.masked(full, what) == {f: (0 if f in zero else v) for f, v in full.items()}


def test_graphs_and_part_vectors():
    """The graphs and generators are what the case list takes them for."""
    for name in es.GRAPHS:
        t, h, seq, pos_size = es.graph(name)
        assert pos_size <= es.MAX_SLOTS and len(np.unique(seq)) == len(seq)
        assert set(seq.tolist()) == set(np.concatenate([t, h]).tolist())
    t, h, _, _ = es.graph("rmat12")
    assert (np.diff(t.astype(np.int64)) >= 0).all() and not (t == h).any()
    tm, hm, _, _ = es.graph("rmat12_mixed")
    assert len(tm) == len(t) + 1500 and np.count_nonzero(tm == hm) == 500
    assert np.count_nonzero(tm[1:] == tm[:-1]) < len(tm) // 100          # no tail runs to speak of
    assert len(es.loop_only_nodes("rmat12_mixed")) == 0
    pair = lambda a, b: np.minimum(a, b).astype(np.int64) << 32 | np.maximum(a, b)
    assert len(np.unique(pair(tm, hm))) <= len(np.unique(pair(t, h))) + 500   # the 1,000 repeats add no pair
    assert np.count_nonzero(tm > hm) > len(tm) // 4 and np.count_nonzero(tm < hm) > len(tm) // 4
    for name, hub_major in (("star_leaf", False), ("star_hub", True)):
        st, sh, seq, pos_size = es.graph(name)
        assert pos_size == es.STAR_LEAVES + 1 and len(st) == es.STAR_LEAVES
        assert ((st if hub_major else sh) == es.STAR_HUB_VID).all()
        assert seq[-1] == es.STAR_HUB_VID     # the hub is every edge's later end
    lt, lh, lseq, _ = es.graph("loops_only")
    lo = es.loop_only_nodes("loops_only")
    assert len(lo) == 300 and len(lseq) == 350 and np.count_nonzero(lt != lh) == 49
    assert np.count_nonzero(lt != lh) != len(lt)                          # m_pairs != nrec
    _, _, eseq, epos = es.graph("edge")
    assert len(eseq) < epos                                               # isolated slots
    for case in es.CASES + [es.ERROR_CASE]:
        name, gen, k = case
        t, h, _, pos_size = es.graph(name)
        p = es.parts(name, gen, k)
        assert p.dtype == np.int16 and len(p) == pos_size and p.min() >= 0
        ends = p[np.concatenate([t, h])]
        assert int(p.max()) + 1 == k == int(ends.max()) + 1, case         # nparts == k, from an edge endpoint
        if gen == "sparse":
            assert set(np.unique(p).tolist()) == ({0, k - 1})
        if gen == "one":
            assert (p == k - 1).all()
    assert max(c[2] for c in es.CASES) == 32768 == np.iinfo(np.int16).max + 1
    assert {c[0] for c in es.CASES if c[2] > 4096} == {"star_leaf", "star_hub", "rmat12_mixed"}


def test_case_table_covers_what_it_claims():
    rows = es.coverage_table()
    assert len(rows) == len(es.CASES) * len(es.MASKS) * len(es.FORMS)

    def some(**kw):
        return any(all(r[f] == v for f, v in kw.items()) for r in rows)

    for form in es.FORMS:
        for M in (1, 2, 3, 4):          # every array count with LDS and with global balances
            for bal in ("LDS", "global"):
                assert some(form=form, M=M, balances=bal), (form, M, bal)
        # bitset words: 64 | 65, 128 | 129, 2048 | 2049, the int16 ceiling
        assert {1, 2, 3, 32, 33, 64, 512} <= {r["W64"] for r in rows if r["form"] == form}
        for one_word in (True, False):
            assert some(form=form, one_word=one_word, M=1) and some(form=form, one_word=one_word, M=4)
        for lo in (True, False):
            assert some(form=form, loop_only_nodes=lo, balances="LDS")
            assert some(form=form, loop_only_nodes=lo, balances="global")
        assert some(form=form, loop_only_nodes=True, what=4)    # own[1] comes from up_own: the loop's bit carries it
        assert some(form=form, full_vcom=True, one_word=True)
        assert some(form=form, full_vcom=True, one_word=False, balances="LDS")
        assert some(form=form, full_vcom=True, balances="global")
        assert some(form=form, full_vcom=False, what=0)
    assert some(ROW16=True) and some(ROW16=False, M=1, form="records") and some(ROW16=False, one_word=True, M=2)
    assert not some(ROW16=True, form="step")
    for k, side in ((64, True), (65, False)):                    # the ROW16 switch at one metric
        for what in (2, 4):
            assert some(case=es.case_id(("rmat12_mixed", "random", k)), what=what, form="records", ROW16=side)
    ks_ = {c[2] for c in es.CASES}
    assert set(es.ALL_K) <= ks_
    for name in ("rmat12_mixed", "star_leaf"):
        assert {c[2] for c in es.CASES if c[0] == name} >= set(es.ALL_K)
    # nparts exactly LDS_PARTS (the x / nparts flush of all three LDS histograms) and its neighbours
    for k in (es.LDS_PARTS - 1, es.LDS_PARTS, es.LDS_PARTS + 1):
        assert some(case=es.case_id(("rmat12_mixed", "random", k)), what=0)
    # gaps: two parts in use, nparts from the maximum
    assert any(c[1] == "sparse" and c[2] > es.LDS_PARTS for c in es.CASES)
    assert set(es.K_SHARDS) == {c[2] for c in es.SHARD_CASES} and es.ERROR_CASE[2] > es.LDS_PARTS


def test_star_hub_sees_every_part():
    """distinct_leaves: the hub's Vcom set holds all k parts while k <= the leaf count (a
    popcount over every word, the own-part bit in the last one), and beyond that is at least
    4,000 wide over every word the leaves reach.  With k >= 4096 every 64 star edges have 64
    different leaf parts and one hub part in whatever order the map leaves them: ECV(down)'s
    balance takes wave_count's per-lane path, ECV(up)'s its leader path, in one launch."""
    seen_big = False
    for name, gen, k in es.CASES:
        if gen != "distinct_leaves":
            continue
        width, who = es.vcom_width(name, gen, k)
        p = es.parts(name, gen, k).astype(np.int64)
        assert who == es.STAR_HUB_VID or k == 1
        if k <= es.STAR_LEAVES:
            assert width == k
        else:
            assert width >= es.STAR_LEAVES
            words = np.unique(np.append(p[1:], p[es.STAR_HUB_VID]) >> 6)
            assert set(range((es.STAR_LEAVES + 63) // 64)) <= set(words.tolist())
        if k >= 4096:
            seen_big = True
            leaves = p[1:]
            assert len(np.unique(leaves)) == len(leaves)         # any 64 edges: 64 lo parts (< WAVE_COUNT_RARE equal)
            assert 1 < es.WAVE_COUNT_RARE <= es.WAVE
            assert es.positions(name)[es.STAR_HUB_VID] == es.STAR_LEAVES   # hi = the hub, part k - 1, in every lane
    assert seen_big
    assert all(("star_leaf", "distinct_leaves", k) in es.CASES for k in (4096, 32767, 32768))


@pytest.mark.parametrize("name,k", write_cases())
def test_edge_owner_reproduces_partition_files(name, k):
    """edge_owner's parts put every record where restate() of tests/test_partition_files.py
    (and so the reference's writer) put it, in graph order and in input-file order."""
    rec, seq = golden_records(name), golden_seq(name)
    t, h = rec["tail"].astype(np.int64), rec["head"].astype(np.int64)
    owner = model.edge_owner(t, h, seq, golden_parts(name, k))
    assert owner.dtype == np.int16 and len(owner) == len(t)
    files = [""] * (int(owner.max()) + 1)
    for i in list(range(len(t))) + [len(t) - 1]:                 # XS1Reader reads the last record twice
        files[owner[i]] += f"{t[i]} {h[i]}\n"
    assert files == restate(name, k, True)
    keep = np.nonzero(t != h)[0]
    lo, hi = np.minimum(t, h)[keep], np.maximum(t, h)[keep]
    graph_files = [""] * (int(owner.max()) + 1)
    for i in np.argsort(lo, kind="stable"):
        graph_files[owner[keep[i]]] += f"{lo[i]} {hi[i]}\n"
    assert graph_files == restate(name, k, False)


def test_model_raises_on_unassigned_endpoint():
    t, h, seq, _ = es.graph("edge")
    p = es.parts("edge", "mod", 3).copy()
    p[t[0]] = -1
    with pytest.raises(IndexError):
        model.evaluate(t, h, seq, p)
    with pytest.raises(IndexError):
        model.edge_owner(t, h, seq, p)


# ------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------
_DEVICE = {}


def device_graph(name):
    """The records and their degree sequence on the device, once per graph."""
    import sheep_amd
    if name not in _DEVICE:
        t, h, seq, pos_size = es.graph(name)
        d = sheep_amd.records_to_device(t, h)
        s = sheep_amd.degree_sequence(d)
        assert np.array_equal(s.numpy(), seq) and s.pos_size == pos_size
        _DEVICE[name] = (d, s)
    return _DEVICE[name]


def device_parts(p):
    import torch
    return torch.from_numpy(np.array(p, dtype=np.int16)).to("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("case", es.CASES, ids=es.case_id)
def test_evaluate_matches_model(gpu_ctx, case):
    """sheep_evaluate and sheep_evaluate_step under every metric mask, and sheep_edge_parts:
    all eleven fields equal the model's (the metrics outside the mask 0)."""
    import sheep_amd
    name, gen, k = case
    want, owners = es.expected(name, gen, k)
    d, s = device_graph(name)
    parts = device_parts(es.parts(name, gen, k))
    assert sheep_amd.ShardedEvaluator.num_parts(parts, s) == k
    for what in es.MASKS:
        assert sheep_amd.evaluate(d, s, parts, what=what).__dict__ == model.masked(want, what), f"records what={what}"
    sheep_amd.build_tree(d, s)    # the step edges are the context's last map's
    for what in es.MASKS:
        got = sheep_amd.evaluate(d, s, parts, what=what, from_step=True)
        assert got.__dict__ == model.masked(want, what), f"step what={what}"
    assert np.array_equal(sheep_amd.edge_parts(d, s, parts).cpu().numpy(), owners)


@pytest.mark.gpu
@pytest.mark.parametrize("case", es.SHARD_CASES, ids=es.case_id)
def test_sharded_evaluator_matches_model(gpu_ctx, case):
    """Three uneven shards (1 record, 64, the rest) added alternately to two states, an empty
    shard added to one of them, the states combined: finish() equals the model."""
    import sheep_amd
    name, gen, k = case
    want, _ = es.expected(name, gen, k)
    d, s = device_graph(name)
    parts = device_parts(es.parts(name, gen, k))
    R = d.shape[0]
    assert R > 65
    shards = [d[:1], d[1:65], d[65:]]
    for what in es.SHARD_MASKS:
        a = sheep_amd.ShardedEvaluator(s, parts, what)
        assert a.nparts == k
        b = sheep_amd.ShardedEvaluator(s, parts, what, nparts=a.nparts)
        for i, shard in enumerate(shards):
            (b if i % 2 else a).add(shard)
        b.add(d[:0])
        a.combine(b.bits, b.acc)
        assert a.finish().__dict__ == model.masked(want, what), f"what={what}"


@pytest.mark.gpu
@pytest.mark.parametrize("what", es.ERROR_MASKS)
def test_unassigned_endpoint_at_many_parts(gpu_ctx, what):
    """Above LDS_PARTS parts: a part of -1 on an edge endpoint raises in both evaluator forms
    and in edge_parts; on a sequenced vertex that is no endpoint it changes nothing; and the
    next call with the intact vector gives the model's counts again on the same context."""
    import sheep_amd
    name, gen, k = es.ERROR_CASE
    t, h, seq, pos_size = es.graph(name)
    want, owners = es.expected(name, gen, k)
    d, _ = device_graph(name)
    extra = es.isolated_slot(name)     # sequenced by hand, never an endpoint
    assert extra < pos_size and extra not in seq
    s = sheep_amd.sequence_from_host(np.append(seq, np.uint32(extra)))
    assert s.pos_size == pos_size
    seq_x = np.append(seq, np.uint32(extra))
    assert model.evaluate(t, h, seq_x, es.parts(name, gen, k)) == want
    good = device_parts(es.parts(name, gen, k))
    sheep_amd.build_tree(d, s)
    forced = es.forced_endpoint(name)
    victims = [v for v in (int(t[0]), int(h[0]), int(h[-1])) if v != forced]
    assert victims
    for victim in victims:
        bad = good.clone()
        bad[victim] = -1
        with pytest.raises(IndexError):
            sheep_amd.evaluate(d, s, bad, what=what)
        with pytest.raises(IndexError):
            sheep_amd.evaluate(d, s, bad, what=what, from_step=True)
        with pytest.raises(IndexError):
            sheep_amd.edge_parts(d, s, bad)
        # the very next calls, intact vector, same context
        assert sheep_amd.evaluate(d, s, good, what=what).__dict__ == model.masked(want, what)
        assert sheep_amd.evaluate(d, s, good, what=what, from_step=True).__dict__ == model.masked(want, what)
        assert np.array_equal(sheep_amd.edge_parts(d, s, good).cpu().numpy(), owners)
    idle = good.clone()
    idle[extra] = -1
    assert sheep_amd.evaluate(d, s, idle, what=what).__dict__ == model.masked(want, what)
    assert sheep_amd.evaluate(d, s, idle, what=what, from_step=True).__dict__ == model.masked(want, what)
    assert np.array_equal(sheep_amd.edge_parts(d, s, idle).cpu().numpy(), owners)
