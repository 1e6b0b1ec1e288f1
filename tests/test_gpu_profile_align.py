"""The built-in profile aligner of `update --aligner builtin` on the MI355X, through both backends: bit-parity with the spec's
statement (tests/align_ref.py) including large pairs, invariants on a leaf-shaped batch of ~10 000 pairs, the reference's ten
update cases, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from make_prg_amd.update import profile_align as pa
from tests import align_ref as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ASCII = np.frombuffer(b"ACGT-RYKMSWN", np.uint8)


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def text(codes):
    return _ASCII[codes].tobytes().decode()


def test_bit_parity_with_the_spec_including_large_pairs(backend):
    probs = ar.random_pairs(21)
    rng = np.random.default_rng(5)
    big = []
    for C, n in ((3000, 3100), (3200, 3000), (4000, 3500)):
        rows = ["".join(rng.choice(list("ACGT-"), C, p=[0.24, 0.24, 0.24, 0.24, 0.04])) for _ in range(3)]
        s = list(rows[0].replace("-", ""))
        s = "".join(s)[:n] + "".join(rng.choice(list("ACGT"), max(0, n - len(s))))
        big.append((rows, [s, "".join(rng.choice(list("ACGT"), n))]))
    leaves = [ar_leaf for ar_leaf in (np.frombuffer("".join(r).encode(), np.uint8).reshape(len(r), -1) for r, _ in probs + big)]
    from make_prg_amd.msa import encode
    res = pa.align_batch(backend, [encode(m) for m in leaves], [[pa._codes(s, "t") for s in ss] for _, ss in probs + big])
    for k, ((rows, ss), got) in enumerate(zip(probs + big, res)):
        for s, (ops, score) in zip(ss, got):
            want = ar.align_pair(rows, s) if k < len(probs) else ar.align_pair_np(rows, s)
            assert (ops.decode(), score) == want, (k, len(s))


def test_synthetic_leaf_batch_invariants(backend):
    leaves, seqs = ar.synth_leaf_batch(1, 10_000)
    res = pa.align_batch(backend, leaves, seqs)
    n = 0
    for rows, ss, got in zip(leaves, seqs, res):
        merged = pa.merge(_ASCII[rows], ss, [ops for ops, _ in got])
        R = rows.shape[0]
        # every row ungaps to its input
        for r in range(R):
            assert merged[r][merged[r] != ord("-")].tobytes() == _ASCII[rows[r]][rows[r] != 4].tobytes()
        for k, s in enumerate(ss):
            assert merged[R + k][merged[R + k] != ord("-")].tobytes() == _ASCII[s].tobytes()
        # the original rows keep their relative columns
        keep_new = ~(merged[:R] == ord("-")).all(0)
        keep_old = ~(rows == 4).all(0)
        assert np.array_equal(merged[:R][:, keep_new], _ASCII[rows][:, keep_old])
        # the reported score is the score of the reported ops
        for s, (ops, score) in zip(ss, got):
            assert ar.score_of_ops_np(rows, s, ops) == score
            n += 1
    assert n >= 10_000


def test_reference_update_cases_on_gpu_with_builtin_aligner(backend, tmp_path):
    from make_prg_amd import device
    from tests import update_common as uc
    from tests.test_profile_align_emulated import run_case_builtin
    device.set_backend(backend)
    try:
        n = 0
        for case in uc.load_cases()["cases"]:
            n += uc.check_outputs(case, run_case_builtin(case, tmp_path, backend))
        assert n >= 20
    finally:
        device.set_backend(None)


def test_command_line_update_aligner_builtin(tmp_path):
    """from_msa then `update --aligner builtin` on sample_example as a user runs them (child processes): the three output files
    equal the reference's (the built-in reproduces this case's MAFFT calls)."""
    from tests import update_common as uc
    case = next(c for c in uc.load_cases()["cases"] if c["case"] == "sample_example_update")
    src = tmp_path / "msas"
    src.mkdir()
    for f in case["inputs"]:
        (src / f["name"]).write_text(f["fasta"])
    (tmp_path / "denovo_paths.txt").write_text(case["denovo_paths"])
    env = dict(os.environ, PYTHONPATH=ROOT)
    base, out = str(tmp_path / "base" / "sample"), str(tmp_path / "out" / "sample_example_update")
    for args in (["from_msa", "-i", str(src), "-o", base],
                 ["update", "-u", base + ".update_DS.zip", "-d", str(tmp_path / "denovo_paths.txt"), "-o", out,
                  "-D", str(case["long_deletion_threshold"]), "--aligner", "builtin"]):
        res = subprocess.run([sys.executable, "-m", "make_prg_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
    assert uc.check_outputs(case, out) == 3
