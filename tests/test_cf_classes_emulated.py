"""mprg_cluster_further_classes (a class of identical gapped rows walked once, counted by its size) on the emulation backend: the old
and the new entry point on the same hand-built tables against the restated reference (tests/cf_classes_cases.py) — through the
one-workgroup form and the tiled kernels —, and alignments through the forest host, which calls the new entry point, against the oracle."""
import numpy as np
import pytest

from tests import cf_classes_cases as cc
from tests import parity_common as pc
from tests.emu.backend import EmuBackend

FAMILIES = cc.families()


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_k1_null_labels(emu, family):
    cc.check(emu, FAMILIES[family], 1)


@pytest.mark.parametrize("k", [2, 10])
@pytest.mark.parametrize("family", ["gapped_twins", "shorts", "small_random", "ties", "widths"])
def test_clusters(emu, family, k):
    rng = np.random.default_rng(k)
    cc.check(emu, [cc.with_labels(p, k, rng) for p in FAMILIES[family]], k)


def test_forms_are_both_reached():
    """Every family but the smallest ones holds views of the one-workgroup form and views of the tiled kernels, under either bound."""
    for name in ("all_identical", "widths", "thresholds", "shorts", "ties", "gapped_twins"):
        fits = [cc.one_fits(*p["rows"].shape, 1, True) for p in FAMILIES[name]]
        assert any(fits) and not all(fits), name
    S = [p["rows"].shape[0] for p in FAMILIES["all_identical"]]
    assert cc.one_fits(302, 20, 1, True) and not cc.one_fits(303, 20, 1, True) and cc.one_fits(355, 20, 1, False) and not cc.one_fits(356, 20, 1, False)
    assert {302, 303, 355, 356, 1025} <= set(S)


@pytest.mark.parametrize("k", [2, 10])
def test_sat_out_and_not_accepted(emu, k):
    """A round where kinfo says a problem sat out (nothing written for it) and a fit with fewer than k distinct labels (assign untouched)."""
    rng = np.random.default_rng(10 + k)
    probs = [cc.with_labels(p, k, rng) for p in FAMILIES["small_random"][:40] + FAMILIES["shorts"] + FAMILIES["gapped_twins"]]
    n = len(probs)
    cc.check(emu, probs, k, sat_out=set(range(0, n, 3)), not_accepted=set(range(1, n, 3)), use_info=True)


def test_alignments_vs_oracle(emu, monkeypatch):
    """The forest host (per-round launches: every call of the loop is the new entry point's) on pan-genome-like alignments."""
    from make_prg_amd import forest
    from make_prg_amd.utils.synthetic import synth_config_fasta
    monkeypatch.setattr(pc, "ENGINE", "forest")
    monkeypatch.setattr(forest, "KLOOP", "rounds")
    calls = []
    orig = forest.ForestEngine._cluster_further
    monkeypatch.setattr(forest.ForestEngine, "_cluster_further", lambda self, *a, **kw: (calls.append(a[3]), orig(self, *a, **kw))[1])
    pc.check_vs_oracle(emu, [synth_config_fasta("C", s) for s in (3, 11)])
    assert 1 in calls and max(calls) >= 2
