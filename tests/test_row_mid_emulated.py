"""mprg_ungap_dedupe's mid-width views (k_rows_mid: 65 .. 1 024 columns, at most 128 rows; tests/row_mid_cases.py) on the emulation
backend.  Every batch: the entry point on hand-built tables — all output arrays against the same library with MPRG_ROW_MID=0 (a child
process) and against the plain restatement — and two of its alignments through the forest host against the oracle.  The contents cases
again in the MPRG_TEST_WEAK_HASH build, where the exact comparisons decide alone.  Two config-C alignments through the per-step host and
mprg_forest_level, the switch on and off."""
import json
import os
import subprocess
import sys

import pytest

from tests import parity_common as pc
from tests import row_mid_cases as rm
from tests.emu.backend import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEAK = dict(defines=("MPRG_TEST_WEAK_HASH",), tag="_weakhash")


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(autouse=True)
def forest_host(monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")


def child(code, backend="EmuBackend()", **env):
    run = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from tests import row_mid_cases as rm; "
                          f"from tests.emu.backend import EmuBackend; be = {backend}; " + code, ROOT],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    return run.stdout


@pytest.mark.parametrize("batch", rm.BATCHES)
def test_every_output_equals_the_switch_off(emu, batch, tmp_path):
    off = str(tmp_path / "off.npz")
    child(f"rm.dump(be, {batch!r}, {off!r})", MPRG_ROW_MID="0")
    assert rm.check_views(emu, batch, off) >= 3          # (mid-width views in the batch, by the restated rule)


@pytest.mark.parametrize("batch", rm.BATCHES)
def test_two_alignments_vs_oracle(emu, batch):
    pc.check_vs_oracle(emu, *rm.oracle_texts(batch))


@pytest.mark.parametrize("batch", ["row_content()", "identical_rows()"])
def test_when_every_hash_collides(batch, tmp_path):
    """MPRG_TEST_WEAK_HASH: a row's hash only counts its words — the counts must agree with the launches', and inside k_rows_mid the
    nominee check refutes, the exact search decides."""
    off = str(tmp_path / "off.npz")
    child(f"rm.dump(be, {batch!r}, {off!r})", backend=f"EmuBackend(**{WEAK!r})", MPRG_ROW_MID="0")
    weak = EmuBackend(**WEAK)
    rm.check_views(weak, batch, off)
    pc.check_vs_oracle(weak, *rm.oracle_texts(batch))


def test_forest_equal_with_the_switch_off(emu):
    from make_prg_amd.utils.synthetic import synth_config_fasta
    seeds = (3, 11)
    on = rm.forest_digest(emu, seeds)
    assert on["per_step"] == on["level"]
    off = json.loads(child(f"import json; print(json.dumps(rm.forest_digest(be, {seeds!r})))", MPRG_ROW_MID="0").strip().splitlines()[-1])
    assert off == on
    pc.check_vs_oracle(emu, [synth_config_fasta("C", s) for s in seeds])
