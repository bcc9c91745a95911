"""The layout of the counter arrays nc / ec as include/legion_batch_layout.h and legion1_amd/layout.py state it, against batches of
tests/pyref.py.  No GPU.

Every expected value is read off the reference batch's ARRAYS, never off its counters: the seeds are the labels, a node behind the
seeds has its batch position in src_off (a node is only ever found as the source end of an edge), and the batch of the first h hops
is the batch with fan-outs fanout[:h] -- the draws of a hop depend on nothing behind it -- so the lengths of those shorter batches are
the per-level and per-hop counts in the order pyref appended them.  The header is compiled as plain C by the host compiler into
tests/layout_probe.c; the C value, the Python value and the reference's must agree."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pyref
from conftest import ROOT
from legion1_amd import layout

FANOUTS = [[3], [3, 2], [4, 3, 2], [2, 2, 2, 2], [2, 2, 2, 2, 2]]
BATCH = 16


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    exe = str(tmp_path_factory.mktemp("layout_probe") / "layout_probe")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "layout_probe.c"), "-o", exe])

    def run(H, nc, ec):
        text = " ".join(str(int(v)) for v in [H, *nc, *ec])
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        vals = {}
        for line in out.splitlines():
            name, *arg, value = line.split()
            vals[(name, *map(int, arg))] = int(value)
        return vals
    return run


@pytest.fixture(scope="module")
def graph():
    rs = np.random.RandomState(20)
    V = 300
    deg = rs.randint(0, 7, size=V)
    deg[rs.randint(0, V, 30)] = 0
    assert (deg == 0).sum() >= 30
    indptr = np.zeros(V + 1, np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rs.randint(0, V, size=int(indptr[-1])).astype(np.int32)
    feats = rs.standard_normal((V, 2)).astype(np.float32)
    labels = rs.randint(0, 5, size=V).astype(np.int32)
    seeds = rs.permutation(V)[:4 * BATCH + 5].astype(np.int32)
    return indptr, indices, feats, labels, seeds


def counts_off_the_arrays(batch):
    """(nodes, edges) of a batch from its arrays alone."""
    seeds, src = len(batch["labels"]), batch["src_off"]
    nodes = max(seeds, int(src.max()) + 1 if len(src) else 0)
    assert nodes == len(batch["ids"]) == len(batch["features"]) and len(batch["dst_off"]) == len(src)
    return nodes, len(src)


@pytest.mark.parametrize("counter", [0, 3])
@pytest.mark.parametrize("fan", FANOUTS, ids=lambda f: "x".join(map(str, f)))
def test_header_python_and_reference_agree(probe, graph, fan, counter):
    indptr, indices, feats, labels, seeds = graph
    H = len(fan)
    run = lambda f: pyref.run_batch(indptr, indices, feats, seeds, labels[seeds], BATCH, counter, f)
    full = run(fan)
    nc, ec = full["nc"], full["ec"]
    # through[h] = (nodes through level h, edges through hop h), h = 0..H, from the batches of the first h hops
    through = [(len(full["labels"]), 0)]
    for h in range(1, H + 1):
        part = full if h == H else run(fan[:h])
        n, e = counts_off_the_arrays(part)
        assert np.array_equal(part["ids"], full["ids"][:n]) and np.array_equal(part["src_off"], full["src_off"][:e])
        through.append((n, e))
    assert through[0][0] == BATCH and through[H][0] > BATCH and through[H][1] > 0      # the case is not empty

    c = probe(H, nc, ec)
    for name in ("MAX_HOPS", "COUNTER_WORDS", "LEVEL_WORDS", "NC_TOTAL", "NC_HOP_NEW", "NC_NEXT_INPUTS", "EC_TOTAL", "EC_HOP", "EC_INPUT_OFF"):
        assert c[(name,)] == getattr(layout, name), name
    assert layout.COUNTER_WORDS == len(nc) == len(ec) and layout.COUNTER_BYTES == nc.nbytes

    def agree(expected, name, *arg):
        """C value == Python value == the quantity read off the reference batch."""
        fn = getattr(layout, name)
        py = fn(*[{"nc": nc, "ec": ec}.get(a, a) for a in arg])
        key = (name, *[a for a in arg if not isinstance(a, str)])
        assert c[key] == py == expected, (name, arg, c[key], py, expected)

    for l in range(H + 1):
        before = through[l - 1][0] if l else 0
        agree(before, "level_offset", "nc", l)
        agree(through[l][0] - before, "level_size", "nc", l)                     # ids per level
        agree(through[l][0], "nodes_through", "nc", l)
        agree(through[l][1], "edges_through", "ec", l)
        for name in ("idx_level_offset", "idx_level_size", "idx_nodes_through"):
            assert c[(name, l)] == getattr(layout, name)(l)
        assert c[("idx_level", layout.idx_level_offset(l))] == layout.idx_level(layout.idx_level_offset(l)) == l
        assert layout.idx_nodes_through(l) == layout.idx_level_offset(l + 1) < layout.COUNTER_WORDS
    for h in range(1, H + 1):
        assert c[("idx_edges_through", h)] == layout.idx_edges_through(h) < layout.COUNTER_WORDS
        agree(through[h - 1][1], "hop_edges_begin", "ec", h)
        agree(through[h][1], "hop_edges_end", "ec", h)                           # edges per hop = end - begin
        # input slots of hop h: the seeds, else the edges of hop h - 1
        agree(len(full["labels"]) if h == 1 else through[h - 1][1] - through[h - 2][1], "hop_inputs", "nc", "ec", h)
    agree(len(full["ids"]), "batch_nodes", "nc", H)
    agree(len(full["src_off"]), "batch_edges", "ec", H)
    agree(through[H - 1][0], "first_block_dst", "nc", H)
    last_inputs = len(full["labels"]) if H == 1 else through[H - 1][1] - through[H - 2][1]
    agree(through[H - 1][0] + last_inputs, "agg_rows", "nc", "ec", H)
    # the running totals end at the batch's totals
    assert int(nc[layout.NC_TOTAL]) == len(full["ids"]) and int(ec[layout.EC_TOTAL]) == len(full["src_off"])
