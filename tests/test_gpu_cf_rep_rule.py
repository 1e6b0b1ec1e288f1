"""GPU twin of tests/test_cf_rep_rule_emulated.py: the one-workgroup form of mprg_cluster_further admits a view by its representatives.
The same hand-built tables on the MI355X, the library's switches in child processes, and 300 config-C alignments through the per-step
host and mprg_forest_level with the rule on (this process) and off (a child), four of them against the oracle.  Run with `-m gpu`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cf_classes_cases as cc
from tests import cf_rep_rule_cases as rr
from tests import parity_common as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 300


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


def child(code, **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import cf_rep_rule_cases as rr; "
                          "from make_prg_amd.backend import HipRuntimeBackend; be = HipRuntimeBackend(0); " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.mark.parametrize("k", [1, 2, 10])
def test_each_view_has_one_side(rt, k):
    named = rr.cases(k)
    rr.check_split(rt, named, k, "bounded")
    rr.check_split(rt, named, k, "classes")


def test_both_entry_points_on_the_same_tables(rt):
    for k in (1, 2, 10):
        rng = np.random.default_rng(k)
        cc.check(rt, [cc.with_labels(p, k, rng) if k > 1 else p for _, p in rr.cases(k)], k)


def test_rep_g_without_gcodes_is_refused(rt):
    """The forest's work lists leave out the problems of the one-workgroup form, which needs the dense copies: a call with rep_g and
    without them would leave those problems to nobody, and fails instead (without rep_g it runs the tiled kernels, as before)."""
    named = rr.cases(1)[:2]
    with pytest.raises(Exception):
        rr.run(rt, [p for _, p in named], 1, "classes", {0, 1}, gcodes=False)
    rt.synchronize()


def test_the_switches_restore_the_split_by_rows():
    child("rr.check_all(be, by_reps=False)", MPRG_CF_REP_RULE="0")
    child("rr.check_all(be, classes=False)", MPRG_CF_CLASSES="0")


def test_batch_equal_with_the_rule_off(rt):
    on = rr.batch_digest(rt, range(BATCH))
    assert on["rounds"] == on["per_step"] == on["level"]
    off = json.loads(child(f"import json; print(json.dumps(rr.batch_digest(be, range({BATCH}))))", MPRG_CF_REP_RULE="0", MPRG_CF_LISTS="0").strip().splitlines()[-1])
    assert off == on


def test_four_alignments_vs_oracle(rt, monkeypatch):
    from make_prg_amd import forest
    from make_prg_amd.utils.synthetic import synth_config_fasta
    monkeypatch.setattr(pc, "ENGINE", "forest")
    monkeypatch.setattr(forest, "KLOOP", "rounds")
    pc.check_vs_oracle(rt, [synth_config_fasta("C", s) for s in (1, 5, 17, 23)])
