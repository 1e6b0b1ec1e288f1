"""mprg_ungap_dedupe's narrow views (k_rows_narrow: one workgroup per view, a lane per row) on the emulation backend against the
oracle: every width and height around the rule that selects them, the row contents that exercise the 8-byte compaction, identical
rows, the k-mer boundary, the exact comparison path and a batch that mixes narrow, small and wide views (tests/row_view_cases.py)."""
import pytest

from tests import parity_common as pc
from tests import row_view_cases as rv
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.fixture(autouse=True)
def forest_host(monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")


@pytest.mark.parametrize("col0_mod", [0, 1, 2, 3])
def test_widths(emu, col0_mod):
    pc.check_vs_oracle(emu, *rv.widths(col0_mod))


def test_heights(emu):
    pc.check_vs_oracle(emu, *rv.heights())


@pytest.mark.parametrize("L", [7, 3])
def test_row_content(emu, L):
    pc.check_vs_oracle(emu, *rv.row_content(L))


def test_identical_rows(emu):
    pc.check_vs_oracle(emu, *rv.identical_rows())


@pytest.mark.parametrize("L", [3, 7])
def test_kmer_boundary(emu, L):
    pc.check_vs_oracle(emu, *rv.kmer_boundary(L))


def test_exact_comparison_decides_when_every_hash_collides():
    """Test-only build whose row hash only counts words: inside k_rows_narrow the nominee check refutes, the exact search decides."""
    weak = EmuBackend(defines=("MPRG_TEST_WEAK_HASH",), tag="_weakhash")
    pc.check_vs_oracle(weak, *rv.identical_rows())
    pc.check_vs_oracle(weak, *rv.row_content(7))


def test_mixed_batch(emu):
    pc.check_vs_oracle(emu, *rv.mixed_batch())
