"""True tree widths (graph2tree -k -e -j; sheep_tree_widths / sheep_facts_widths):
width(id) = 1 + |jxn(id)|, jxn(id) = the later vertices adjacent to id's subtree
(jtree.cpp:97, jnode.h:230-260).  All results are integers; the bar is equality.

CPU: the row-subtree rule of sheep_amd/csrc/widths.hip (widths_model.row_subtree) against
the elimination game.  GPU: the kernels against the game, closed forms past one tile of
every pass, argument errors, and the CLI.  Reference pin: tests/golden/widths/*.json.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import widths_model as wm
from conftest import GOLDEN, ROOT, check_print, golden_records, golden_seq, golden_tree

BIN = os.environ.get("SHEEP_BIN_DIR") or os.path.join(ROOT, "sheep_amd", "bin")
TIMING = ("Loaded graph in:", "Sorted in:", "Mapped in:", "Reduced in:", "Finished in:", "Built in:")
FACT_FIELDS = ("width", "root_cnt", "vert_height", "edge_height", "vert_cnt", "edge_cnt", "halo_id", "core_id", "fill")
INVALID = wm.INVALID


def strip_timing(text):
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(TIMING))


# ---- CPU: the identity the kernels rest on ------------------------------------------------
def test_game_forms_agree_on_random_multigraphs():
    """The merge-into-the-parent game (used on the larger graphs below) is the literal one."""
    rng = np.random.default_rng(20)
    for _ in range(200):
        tail, head, seq = wm.random_multigraph(rng)
        lo, hi = wm.position_edges(tail, head, seq)
        assert np.array_equal(wm.game(len(seq), lo, hi), wm.game_literal(len(seq), lo, hi))


def test_row_subtree_rule_is_the_elimination_game_on_random_multigraphs():
    """200 seeded multigraphs, n <= 60, with self-loops, repeats and isolated slots; both
    forms of the lowest common ancestor (depth minimum, id maximum) give the game's widths."""
    rng = np.random.default_rng(7)
    nonempty = 0
    for _ in range(200):
        tail, head, seq = wm.random_multigraph(rng)
        n = len(seq)
        lo, hi = wm.position_edges(tail, head, seq)
        parent, pst = wm.etree(n, lo, hi)
        want = wm.game_literal(n, lo, hi)
        assert np.array_equal(wm.row_subtree(n, parent, lo, hi, "max_id"), want)
        assert np.array_equal(wm.row_subtree(n, parent, lo, hi, "min_depth"), want)
        assert np.all(want[parent == INVALID] == 1)
        nonempty += len(lo) > 0
    assert nonempty > 150


def test_row_subtree_rule_on_hep_with_its_golden_tree():
    r = golden_records("hep")
    seq = golden_seq("hep")
    parent, pst = golden_tree("hep")
    lo, hi = wm.position_edges(r["tail"], r["head"], seq)
    want = wm.game(len(seq), lo, hi)
    got = wm.row_subtree(len(seq), parent.astype(np.int64), lo, hi)
    assert np.array_equal(got, want)
    assert want.max() > 1 + pst.max()   # the placeholder width understates the real one here


def test_facts_rule_without_widths_is_the_golden_facts():
    """widths_model.facts is JNodeTable::Facts: with the placeholder widths it prints the
    reference's TREEFAQS."""
    for name in ("hep", "edge"):
        parent, pst = golden_tree(name)
        assert wm.facts_text(wm.facts(parent, pst)) == open(os.path.join(GOLDEN, f"{name}.facts")).read()


def test_cli_rejects_j_without_k_and_e():
    exe = os.path.join(BIN, "graph2tree")
    if not os.path.exists(exe):
        pytest.skip("CLIs not built (make cli)")
    for flags in (["-j"], ["-j", "-k"], ["-e", "-j"]):
        p = subprocess.run([exe, "x.dat", *flags, "-f"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout == "Option -j (junction sets) needs both -k and -e.\n", flags
    for flag in ("-x", "-m", "-w"):   # the width-limit experiments stay rejected
        p = subprocess.run([exe, "x.dat", flag, "1"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "is not supported by this build" in p.stdout, flag


def test_cli_rejects_j_in_a_world_of_two_ranks_and_with_partial_loads():
    exe = os.path.join(BIN, "graph2tree")
    if not os.path.exists(exe):
        pytest.skip("CLIs not built (make cli)")
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PMI_RANK", "PMI_SIZE", "OMPI_COMM_WORLD_SIZE")}
    env["SHEEP_DEVICES"] = "0,0"
    for flags in (["-r"], ["-i"], ["-i", "-r"]):
        p = subprocess.run([exe, "x.dat", "-k", "-e", "-j", *flags, "-f"], capture_output=True, text=True, timeout=60,
                           env=env)
        assert p.returncode == 1, flags
        assert p.stdout == ("Option -j (junction sets) is not supported together with -i / -r over more than one "
                            "rank by this build.\n"), flags
    p = subprocess.run([exe, "x.dat", "-k", "-e", "-j", "-l", "1/2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    assert p.stdout == "Option -j (junction sets) is not supported together with -l by this build.\n"


# ---- GPU ------------------------------------------------------------------------------------
def gpu_run(tail, head, seq, tree=None):
    """(parent, pst, widths, Facts) of the records under the explicit sequence `seq`."""
    import sheep_amd
    d = sheep_amd.records_to_device(np.asarray(tail, np.uint32), np.asarray(head, np.uint32))
    s = sheep_amd.sequence_from_host(np.asarray(seq, np.uint32))
    t = sheep_amd.build_tree(d, s) if tree is None else tree
    w = sheep_amd.tree_widths(d, s, t)
    f = sheep_amd.facts(t, w)
    parent, pst = sheep_amd.tree_to_numpy(t)
    return parent, pst, sheep_amd.to_numpy_u32(w).astype(np.int64), f


def check_facts(f, parent, pst, width):
    want = wm.facts(parent, pst, width)
    assert {k: getattr(f, k) for k in FACT_FIELDS} == want


def edges(pairs):
    a = np.array(pairs, dtype=np.uint32).reshape(-1, 2)
    return a[:, 0], a[:, 1]


K6 = [(i, j) for i in range(6) for j in range(i + 1, 6)]
HAND = {
    # name: (pairs, sequence, widths, fill)
    "path5": ([(0, 1), (1, 2), (2, 3), (3, 4)], range(5), [2, 2, 2, 2, 1], 0),
    "star_hub_last": ([(i, 5) for i in range(5)], range(6), [2, 2, 2, 2, 2, 1], 0),
    "star_hub_first": ([(0, i) for i in range(1, 6)], range(6), [6, 5, 4, 3, 2, 1], 10),
    "k6": (K6, range(6), [6, 5, 4, 3, 2, 1], 0),
    "cycle4": ([(0, 1), (1, 2), (2, 3), (3, 0)], range(4), [3, 3, 2, 1], 1),
    # components {0,1,2} and {3,4}, vertex 5 isolated but sequenced: the roots 2, 4, 5 have width 1
    "components": ([(0, 1), (1, 2), (3, 4)], range(6), [2, 2, 1, 2, 1, 1], 0),
    # vertex 3's lower neighbours 0 and 2: 0 is a descendant of 2
    "nested_neighbours": ([(0, 1), (1, 2), (0, 3), (2, 3)], range(4), [3, 3, 2, 1], 1),
    # the same through a sequence that is no identity (vids 7, 3, 9, 1 at positions 0..3), a repeat and a self-loop
    "relabelled": ([(7, 3), (3, 9), (1, 7), (9, 1), (9, 1), (3, 3)], [7, 3, 9, 1], [3, 3, 2, 1], 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_shapes(gpu_ctx, name):
    pairs, seq, widths, fill = HAND[name]
    tail, head = edges(pairs)
    seq = np.array(list(seq), dtype=np.uint32)
    parent, pst, w, f = gpu_run(tail, head, seq)
    assert w.tolist() == widths
    lo, hi = wm.position_edges(tail, head, seq)
    assert wm.game_literal(len(seq), lo, hi).tolist() == widths   # the table above is the game's
    assert np.all(w[parent == INVALID] == 1)
    assert f.fill == fill and f.width == max(widths)
    check_facts(f, parent, pst, w)


@pytest.mark.gpu
def test_edge_golden_multigraph_fill_wraps(gpu_ctx):
    """Repeats raise pst above the number of distinct later neighbours, so single fill terms
    are negative: the sum is taken in wrapping 64-bit arithmetic, as the reference's size_t."""
    r = golden_records("edge")
    seq = golden_seq("edge")
    parent, pst, w, f = gpu_run(r["tail"], r["head"], seq)
    gp, gw = golden_tree("edge")
    assert np.array_equal(parent, gp) and np.array_equal(pst, gw)
    lo, hi = wm.position_edges(r["tail"], r["head"], seq)
    assert np.array_equal(w, wm.game_literal(len(seq), lo, hi))
    assert np.any(w - pst.astype(np.int64) - 1 < 0)
    check_facts(f, parent, pst, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1000, 2000])
def test_random_graphs(gpu_ctx, n):
    """About 3n records over n slots, with repeats and self-loops, a random sequence that
    leaves a few slots out; per-node widths and all Facts fields against the game."""
    rng = np.random.default_rng(n)
    tail, head = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    seq = rng.permutation(n)[: n - n // 16]
    parent, pst, w, f = gpu_run(tail, head, seq)
    lo, hi = wm.position_edges(tail, head, seq)
    assert np.array_equal(w, wm.game(len(seq), lo, hi))
    check_facts(f, parent, pst, w)


@pytest.mark.gpu
def test_band_graph_closed_form(gpu_ctx):
    """n = 100,000, edges (i, i+1..i+8), identity sequence: every pass runs past one tile."""
    n, b = 100_000, 8
    i = np.repeat(np.arange(n, dtype=np.int64), b)
    j = i + np.tile(np.arange(1, b + 1), n)
    keep = j < n
    parent, pst, w, f = gpu_run(i[keep], j[keep], np.arange(n))
    assert np.array_equal(w, 1 + np.minimum(b, n - 1 - np.arange(n)))
    assert f.fill == 0 and f.width == b + 1 and f.halo_id == 0 and f.core_id == 0
    check_facts(f, parent, pst, w)


@pytest.mark.gpu
def test_path_is_the_deepest_tree(gpu_ctx):
    """n = 300,000 in a path: depth n, so the tour, the ancestor table and the subtree sums
    run on the deepest possible tree."""
    n = 300_000
    i = np.arange(n - 1)
    parent, pst, w, f = gpu_run(i, i + 1, np.arange(n))
    assert np.all(w[:-1] == 2) and w[-1] == 1
    assert f.vert_height == n and f.fill == 0 and f.width == 2 and f.halo_id == INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("tail_vertex", [False, True])
def test_hub(gpu_ctx, tail_vertex):
    """One vertex adjacent to 200,000 leaves, hub last: every pair of neighbours in the hub's
    run meets at the hub.  With one more vertex after the hub the hub is no root, and all
    those -1 land on one address (combined within the wave)."""
    k = 200_000
    tail, head = np.arange(k), np.full(k, k)
    want = np.full(k + 1, 2)
    want[k] = 1
    if tail_vertex:
        tail, head = np.append(tail, k), np.append(head, k + 1)
        want = np.append(want, 1)
        want[k] = 2
    parent, pst, w, f = gpu_run(tail, head, np.arange(len(want)))
    assert np.array_equal(w, want)
    assert f.fill == 0 and f.width == 2


@functools.lru_cache(maxsize=None)
def golden_expected(name):
    r = golden_records(name)
    seq = golden_seq(name)
    lo, hi = wm.position_edges(r["tail"], r["head"], seq)
    return r, seq, wm.game(len(seq), lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hep", "rmat10", "rmat12", "rmat14"])
def test_golden_graphs(gpu_ctx, name):
    r, seq, want = golden_expected(name)
    parent, pst, w, f = gpu_run(r["tail"], r["head"], seq)
    gp, gw = golden_tree(name)
    assert np.array_equal(parent, gp) and np.array_equal(pst, gw)
    assert np.array_equal(w, want)
    check_facts(f, parent, pst, w)


@pytest.mark.gpu
def test_shuffled_records_give_the_same_widths(gpu_ctx):
    r, seq, want = golden_expected("rmat10")
    order = np.random.default_rng(3).permutation(len(r))
    flip = np.random.default_rng(4).integers(0, 2, len(r)).astype(bool)
    tail = np.where(flip, r["head"], r["tail"])[order]
    head = np.where(flip, r["tail"], r["head"])[order]
    _, _, w, _ = gpu_run(tail, head, seq)
    assert np.array_equal(w, want)


@pytest.mark.gpu
def test_facts_without_widths_is_sheep_facts(gpu_ctx):
    import ctypes
    import sheep_amd
    parent, pst = golden_tree("hep")
    t = sheep_amd.tree_to_device(parent, pst)
    out = sheep_amd._Facts()
    sheep_amd._check(sheep_amd.lib().sheep_facts_widths(gpu_ctx.handle, t.data_ptr(), t.shape[0], None,
                                                        ctypes.byref(out)))
    assert sheep_amd.Facts(*[getattr(out, k) for k in FACT_FIELDS]) == sheep_amd.facts(t)
    assert sheep_amd.facts(t).text() == open(os.path.join(GOLDEN, "hep.facts")).read()


# a tree of part of the records, widths asked for all of them: (records of the tree, the
# extra record, which check sees it)
FOREIGN = {
    "lo_is_a_root": ([(0, 1), (1, 2)], (2, 3)),                       # 2 is a root of the half tree
    "under_another_root": ([(0, 1), (2, 3)], (0, 3)),                 # 0 is below root 1, not below root 3
    "under_another_node": ([(0, 1), (1, 4), (2, 3), (3, 4)], (0, 3)),  # 0 and 3 are cousins below 4
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FOREIGN))
def test_foreign_tree_is_an_argument_error(gpu_ctx, name):
    import sheep_amd
    part, extra = FOREIGN[name]
    s = sheep_amd.sequence_from_host(np.arange(5, dtype=np.uint32))
    tree = sheep_amd.build_tree(sheep_amd.records_to_device(*edges(part)), s)
    everything = sheep_amd.records_to_device(*edges(part + [extra]))
    with pytest.raises(ValueError, match="not the tree of these records"):
        sheep_amd.tree_widths(everything, s, tree)
    # the context is usable afterwards
    w = sheep_amd.tree_widths(sheep_amd.records_to_device(*edges(part)), s, tree)
    lo, hi = wm.position_edges(*edges(part), np.arange(5))
    assert np.array_equal(sheep_amd.to_numpy_u32(w), wm.game_literal(5, lo, hi))


@pytest.mark.gpu
def test_half_the_records_tree_is_an_argument_error(gpu_ctx):
    import sheep_amd
    r, seq, want = golden_expected("rmat10")
    d = sheep_amd.records_to_device(r["tail"], r["head"])
    s = sheep_amd.sequence_from_host(seq)
    half = sheep_amd.build_tree(d[: len(r) // 2].contiguous(), s)
    with pytest.raises(ValueError, match="not the tree of these records"):
        sheep_amd.tree_widths(d, s, half)
    w = sheep_amd.tree_widths(d, s, sheep_amd.build_tree(d, s))
    assert np.array_equal(sheep_amd.to_numpy_u32(w), want)


@pytest.mark.gpu
def test_empty_inputs(gpu_ctx):
    import sheep_amd
    none = np.zeros(0, dtype=np.uint32)
    parent, pst, w, f = gpu_run(none, none, none)                      # n == 0
    assert len(w) == 0 and f.vert_cnt == 0
    parent, pst, w, f = gpu_run(none, none, np.arange(5))              # nrec == 0
    assert w.tolist() == [1] * 5 and f.width == 1 and f.fill == 0 and f.root_cnt == 5
    loops = np.arange(5, dtype=np.uint32)
    parent, pst, w, f = gpu_run(loops, loops, np.arange(5))            # self-loops only
    assert w.tolist() == [1] * 5 and f.width == 1 and f.fill == 0


@pytest.mark.gpu
def test_workspaces_and_timers_are_named(gpu_ctx):
    import sheep_amd
    r, seq, want = golden_expected("rmat10")
    d = sheep_amd.records_to_device(r["tail"], r["head"])
    s = sheep_amd.sequence_from_host(seq)
    t = sheep_amd.build_tree(d, s)
    gpu_ctx.timing(True)
    try:
        gpu_ctx.timer_reset()
        sheep_amd.tree_widths(d, s, t)
        names = set(gpu_ctx.timer_names())
    finally:
        gpu_ctx.timing(False)
    assert {"widths", "widths_tour", "widths_sort", "widths_lca", "widths_weights", "widths_sums"} <= names
    ws = gpu_ctx.workspace()
    arcs = 2 * int(np.count_nonzero(golden_tree("rmat10")[0] != INVALID))
    assert ws["wd_lca"] >= 4 * arcs * arcs.bit_length() and ws["wd_keys"] >= 8 * len(r)


# ---- GPU: the CLI ---------------------------------------------------------------------------
def run_cli(*args):
    p = subprocess.run([os.path.join(BIN, "graph2tree"), *[str(a) for a in args]], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return strip_timing(p.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hep", "edge"])
def test_cli_kej_prints_the_true_widths(gpu_ctx, tmp_path, name):
    """graph2tree G -k -e -j -f -t: TREEFAQS and JTree::print with the real widths; the saved
    tree is the golden one (the reference does not store jxn either)."""
    r = golden_records(name)
    seq = golden_seq(name)
    parent, pst = golden_tree(name)
    lo, hi = wm.position_edges(r["tail"], r["head"], seq)
    width = wm.game(len(seq), lo, hi)
    want = wm.facts_text(wm.facts(parent, pst, width)) + wm.print_text(seq, parent, pst, width)
    out = tmp_path / "t.tre"
    dat = os.path.join(GOLDEN, f"{name}.dat")
    assert run_cli(dat, "-k", "-e", "-j", "-f", "-t", "-o", out) == want
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, f"{name}.tre"), "rb").read()
    # an explicit sequence file and -c
    text = run_cli(dat, "-k", "-e", "-j", "-f", "-c", "-s", os.path.join(GOLDEN, f"{name}.seq"))
    assert text == wm.facts_text(wm.facts(parent, pst, width)) + "Tree is valid.\n"


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(), ("-k",), ("-e",), ("-k", "-e")])
def test_cli_without_j_is_unchanged(gpu_ctx, flags):
    dat = os.path.join(GOLDEN, "hep.dat")
    facts = open(os.path.join(GOLDEN, "hep.facts")).read()
    text = run_cli(dat, *flags, "-f", "-t")
    assert text.startswith(facts)
    check_print(text[len(facts):], "hep", "print")


# ---- the reference's own answer -------------------------------------------------------------
PINS = os.path.join(GOLDEN, "widths")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hep", "edge", "rmat10"])
def test_reference_pin(gpu_ctx, name):
    """Per-node widths and TREEFAQS of the reference's own JTree with make_kids, make_pst and
    make_jxn (tests/golden/widths/README.md)."""
    pin = json.load(open(os.path.join(PINS, f"{name}.json")))
    r = golden_records(name)
    parent, pst, w, f = gpu_run(r["tail"], r["head"], golden_seq(name))
    assert w.tolist() == pin["widths"]
    assert f.text() == pin["treefaqs"]
