"""The one-workgroup form of mprg_cluster_further admits a view by its representatives (tests/cf_rep_rule_cases.py) on the emulation
backend: hand-built tables through both entry points with the side that took each view read from the work lists, the library's two
switches in child processes (they are read once, when the library loads), and alignments through both forest hosts against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cf_classes_cases as cc
from tests import cf_rep_rule_cases as rr
from tests import parity_common as pc
from tests.emu.backend import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 5)          # (config-C alignments whose k = 1 checks hold views that only fit by their representatives: asserted below)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def child(code, **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import cf_rep_rule_cases as rr; "
                          "from tests.emu.backend import EmuBackend; be = EmuBackend(); " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.mark.parametrize("k", [1, 2, 10])
def test_each_view_has_one_side(emu, k):
    named = rr.cases(k)
    rr.check_split(emu, named, k, "bounded")
    rr.check_split(emu, named, k, "classes")


def test_both_entry_points_on_the_same_tables(emu):
    """cf_classes_cases.check (both entry points against the restatement and each other) on the shapes of this rule."""
    for k in (1, 2, 10):
        rng = np.random.default_rng(k)
        cc.check(emu, [cc.with_labels(p, k, rng) if k > 1 else p for _, p in rr.cases(k)], k)


def test_rep_g_without_gcodes_is_refused(emu):
    """The forest's work lists leave out the problems of the one-workgroup form, which needs the dense copies: a call with rep_g and
    without them would leave those problems to nobody, and fails instead (without rep_g it runs the tiled kernels, as before)."""
    named = rr.cases(1)[:2]
    with pytest.raises(Exception):
        rr.run(emu, [p for _, p in named], 1, "classes", {0, 1}, gcodes=False)
    emu.synchronize()


def test_the_switches_restore_the_split_by_rows():
    child("rr.check_all(be, by_reps=False)", MPRG_CF_REP_RULE="0")
    child("rr.check_all(be, classes=False)", MPRG_CF_CLASSES="0")


def test_alignments_both_hosts_switch_on_and_off(emu, monkeypatch):
    from make_prg_amd import forest
    from make_prg_amd.utils.synthetic import synth_config_fasta
    seen, listed = [], []
    orig = forest.ForestEngine._cluster_further

    def spy(self, d_sub, d_prob, n_probs, k, dd, *a, **kw):
        be = self.be
        prob = be.download(d_prob, np.int64, rr.PF * n_probs).reshape(n_probs, rr.PF)
        nv = int(prob[:, 0].max()) + 1
        sub, summ = be.download(d_sub, np.int64, rr.VF * nv).reshape(nv, rr.VF), be.download(dd["summary"], np.int64, 8 * nv).reshape(nv, 8)
        for q in prob[:, 0]:
            S, n, G = int(sub[q, 5]), int(sub[q, 7]), int(summ[q, 1])
            seen.append(rr.one_takes(S, n, k, G, True, True) and not rr.one_takes(S, n, k, G, True, False))
        # the work lists name exactly the problems the one-workgroup form does not take by its rows (k = 1: the check's lists; the rounds'
        # lists serve k = 2 .. 10: what fits at 10) — a problem that is not listed is the one-workgroup form's at this call
        d_wc, n_wc, d_wr, n_wr = a[2:6]
        kk = 1 if k == 1 else rr.KMAX
        want = {b for b, q in enumerate(prob[:, 0]) if not rr.one_takes(int(sub[q, 5]), int(sub[q, 7]), kk, 0, True, False)}
        for d_w, n_w in ((d_wc, n_wc), (d_wr, n_wr)):
            got = set(be.download(d_w, np.int32, 2 * n_w).reshape(-1, 2)[:, 0].tolist()) if n_w else set()
            assert got == want, (k, sorted(got ^ want))
        for b in set(range(n_probs)) - want:
            q = prob[b, 0]
            assert rr.one_takes(int(sub[q, 5]), int(sub[q, 7]), k, int(summ[q, 1]), True, True)
        listed.append((len(want), n_probs))
        return orig(self, d_sub, d_prob, n_probs, k, dd, *a, **kw)
    monkeypatch.setattr(forest.ForestEngine, "_cluster_further", spy)
    on = rr.batch_digest(emu, SEEDS)
    assert sum(seen) >= 2, "the alignments hold views the rule moves"
    assert any(w == 0 for w, _ in listed) and any(0 < w < n for w, n in listed), "an empty list and a partial one"
    assert on["rounds"] == on["per_step"] == on["level"]
    monkeypatch.setattr(forest.ForestEngine, "_cluster_further", orig)
    off = json.loads(child(f"import json; print(json.dumps(rr.batch_digest(be, {SEEDS!r})))", MPRG_CF_REP_RULE="0", MPRG_CF_LISTS="0").strip().splitlines()[-1])
    assert off == on
    monkeypatch.setattr(pc, "ENGINE", "forest")
    monkeypatch.setattr(forest, "KLOOP", "rounds")
    pc.check_vs_oracle(emu, [synth_config_fasta("C", s) for s in SEEDS])
