"""GPU twin of tests/test_cf_classes_emulated.py: the same hand-built tables through mprg_cluster_further_bounded and
mprg_cluster_further_classes on the MI355X (LDS atomics of many wavefronts, many workgroups at once), and one batch of pan-genome
alignments with MPRG_CF_CLASSES on (this process) and off (a child: the switch is read once when the library loads).  Run with `-m gpu`."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cf_classes_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = cc.families()
BATCH = 300


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_k1_null_labels(rt, family):
    cc.check(rt, FAMILIES[family], 1)


@pytest.mark.parametrize("k", [2, 10])
@pytest.mark.parametrize("family", ["gapped_twins", "shorts", "small_random", "ties", "widths"])
def test_clusters(rt, family, k):
    rng = np.random.default_rng(k)
    cc.check(rt, [cc.with_labels(p, k, rng) for p in FAMILIES[family]], k)


@pytest.mark.parametrize("k", [2, 10])
def test_sat_out_and_not_accepted(rt, k):
    rng = np.random.default_rng(10 + k)
    probs = [cc.with_labels(p, k, rng) for p in FAMILIES["small_random"][:40] + FAMILIES["shorts"] + FAMILIES["gapped_twins"]]
    n = len(probs)
    cc.check(rt, probs, k, sat_out=set(range(0, n, 3)), not_accepted=set(range(1, n, 3)), use_info=True)


def batch_digest(be) -> dict:
    """PRGs and node tables (as the tree dumps made from them: the order of a level's nodes in the raw table is the order in which
    workgroups reserved their places, different from run to run) of BATCH config-C alignments, per-round launches (every call of the loop goes through the entry point)."""
    from make_prg_amd import forest
    from make_prg_amd.msa import load_alignment_text
    from make_prg_amd.utils.synthetic import synth_config_fasta
    msas = [load_alignment_text(synth_config_fasta("C", s), defer_n=True) for s in range(BATCH)]
    eng = forest.ForestEngine(be, 5, 7)
    eng.load(msas)
    kloop, forest.KLOOP = forest.KLOOP, "rounds"
    try:
        eng.run_forest()
    finally:
        forest.KLOOP = kloop          # (the module's setting is every later engine's)
    sha = lambda parts: hashlib.sha256(b"\n".join(parts)).hexdigest()
    out = dict(prgs=sha([(p or "<none>").encode() for p in eng.assemble_prgs()]),
               trees=sha([json.dumps(eng.tree_dump(i, m.ids), sort_keys=True).encode() for i, m in enumerate(msas)]))
    return out


def test_batch_equal_with_the_switch_off(rt):
    on = batch_digest(rt)
    child = subprocess.run([sys.executable, "-c", "import json, sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_cf_classes as t; "
                            "from make_prg_amd.backend import HipRuntimeBackend; print(json.dumps(t.batch_digest(HipRuntimeBackend(0))))", ROOT],
                           env=dict(os.environ, MPRG_CF_CLASSES="0"), capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    off = json.loads(child.stdout.strip().splitlines()[-1])
    assert off == on, sorted(k for k in on if on[k] != off.get(k))
