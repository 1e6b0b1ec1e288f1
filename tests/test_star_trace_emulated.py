"""star_align.star_msas asks of the backend exactly what it asked before the host side was restructured: per scenario of
tests/star_trace.py the launches (entry point, arguments, work), uploads (bytes) and downloads, in order, and the MSAs' text,
against the digests recorded at the parent commit (tests/golden/star_trace.json), on the CPU emulation build."""
import pytest

from tests import star_trace as tr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("name", list(tr.scenarios()))
def test_trace_equals_the_golden(emu, name):
    assert tr.run(emu, name)[1] == tr.golden()[name]
