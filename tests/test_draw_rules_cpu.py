"""The draw rules (DrawRule, csrc/internal.h), the parts that need no GPU: the cap on near-tied rows that tests/test_gpu_draw_rules.py
relies on, and each rule's fan-out bound through the `legion` binary's boot."""
import os
import re
import subprocess

import pytest

import drawrulecases as D
import wdistinctref
from conftest import ROOT

SERVER = os.path.join(ROOT, "legion-1_amd", "csrc", "legion")
MODE_VARS = ("LEGION_AGG_LAST_HOP", "LEGION_AGG_NORM", "LEGION_SAMPLING", "LEGION_SAMPLING_SEED", "LEGION_LP_DRAW", "LEGION_WEIGHTED_DISTINCT")
# the boot went past the modes: the meta line names a synth: workload that does not exist, which Server_Initialize refuses right behind
# them and before any device is touched (tests/test_serve_modes_cpu.py)
ACCEPTED = "Server_Initialize: the synth: dataset path names no known workload / scale"


def test_no_row_of_the_gpu_tests_batches_is_a_near_tie():
    """Weighted sampling without replacement is compared bit for bit except on rows whose f-th and (f + 1)-th key lie within 2^-40
    (wdistinctref.near_ties).  The cap on such rows is zero: drawrulecases.GRAPH_SEED is chosen so that the graph, seed lists and counters
    of the GPU test have none, and the GPU test then leaves out no row."""
    g = D.graph()
    weights = wdistinctref.Weights(g["indptr"], g["indices"], g["w"])
    for tile, (B, fan) in D.SHAPES.items():
        assert wdistinctref.near_ties(weights, D.seed_list(tile), B, D.COUNTERS, fan) == [], tile


RULE_ENV = dict(stream=dict(LEGION_SAMPLING="replace"), distinct=dict(LEGION_SAMPLING="distinct"), weighted=dict(LEGION_SAMPLING="weighted"),
                wdistinct=dict(LEGION_SAMPLING="weighted", LEGION_WEIGHTED_DISTINCT="1"))
REFUSAL = dict(distinct="Server_Initialize: LEGION_SAMPLING=distinct takes fan-outs of at most 64, hop 2 has 65: k_sample stages the picks of a tile's rows in static LDS",
               wdistinct="Server_Initialize: LEGION_WEIGHTED_DISTINCT=1 takes fan-outs of at most 64, hop 2 has 65: k_sample keeps a row's best picks one per lane and "
                         "stages them in static LDS")


@pytest.mark.parametrize("fan", ["5,64", "5,65"])
@pytest.mark.parametrize("rule", D.RULES)
def test_boot_applies_each_rules_fan_out_bound(tmp_path, rule, fan):
    """A fan-out of 64 boots past the modes under every rule; 65 is refused under the two rules without replacement, each by its own
    text (the whole message), and boots on under `replace` and `weighted`."""
    meta = str(tmp_path / "meta_config")
    with open(meta, "w") as f:
        f.write("synth:nosuchworkload 512 1000 0 16 100 0 0 %d 1 0\n" % (1 << 30))
    env = {k: v for k, v in os.environ.items() if k not in MODE_VARS}
    env.update(RULE_ENV[rule], LEGION_IPC_NAMESPACE="cpurules%d_" % os.getpid())
    r = subprocess.run([SERVER, "1", "0", fan, meta], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    said = r.stdout + r.stderr
    want = REFUSAL.get(rule, ACCEPTED) if fan.endswith("65") else ACCEPTED
    assert r.returncode == 1 and want in said, said[-2000:]
    assert len(set(re.findall(r"Server_Initialize: .*", said))) == 1, said[-2000:]
