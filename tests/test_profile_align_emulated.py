"""The built-in profile aligner of `update --aligner builtin` (make_prg_amd/update/profile_align.py, csrc/k_align.inc) on the CPU
emulation build: ops and scores bit-equal to the spec's plain-Python statement (tests/align_ref.py), the recorded MAFFT calls of
the reference's update cases reproduced, and `update` end to end with it."""
import gzip
import json
import os
from argparse import Namespace
from pathlib import Path

import numpy as np
import pytest

from make_prg_amd import device
from make_prg_amd.msa import MSA, encode, read_fasta_alignment
from make_prg_amd.update import profile_align as pa
from make_prg_amd.utils.msa_aligner import BuiltinAligner
from tests import align_ref as ar
from tests.emu.backend import EmuBackend

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    be = EmuBackend()
    device.set_backend(be)
    yield be
    device.set_backend(None)


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "update.json.gz"), "rt") as fh:
        return json.load(fh)


def leaf_codes(rows):
    return encode(np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), -1))


def seq_codes(s):
    return pa._codes(s, "test")


def test_pairs_bit_equal_to_the_spec(emu):
    probs = ar.random_pairs(7)
    res = pa.align_batch(emu, [leaf_codes(r) for r, _ in probs], [[seq_codes(s) for s in ss] for _, ss in probs])
    n = 0
    for (rows, ss), got in zip(probs, res):
        for s, (ops, score) in zip(ss, got):
            want = ar.align_pair(rows, s)
            assert (ops.decode(), score) == want, (rows, s)
            assert ar.score_of_ops_np(leaf_codes(rows), seq_codes(s), ops) == score
            n += 1
    assert n >= 250


def test_row_form_of_the_spec_matches_the_cell_form():
    """tests/align_ref.align_pair_np (the GPU tests' reference for large pairs) is align_pair."""
    for rows, ss in ar.random_pairs(11)[:40]:
        for s in ss:
            assert ar.align_pair_np(rows, s) == ar.align_pair(rows, s)


def test_chunked_launches_give_the_same_answers(emu):
    """A workspace budget of a few pairs per launch: several chunks, the same ops; a pair larger than the budget is an error."""
    probs = ar.random_pairs(3)[:25]
    leaves, seqs = [leaf_codes(r) for r, _ in probs], [[seq_codes(s) for s in ss] for _, ss in probs]
    whole = pa.align_batch(emu, leaves, seqs)
    assert pa.align_batch(emu, leaves, seqs, budget_bytes=4 * pa.workspace_words(192, 128)) == whole
    with pytest.raises(pa.ProfileAlignError, match="budget"):
        pa.align_batch(emu, leaves, seqs, budget_bytes=4 * 64)


def test_pair_too_long_is_refused(emu):
    with pytest.raises(pa.ProfileAlignError, match="10"):
        pa.align_batch(emu, [leaf_codes(["A" * 10])], [[np.zeros(pa.MAX_LEN - 10, np.uint8)]])


def test_kernel_refuses_out_of_range_pairs(emu):
    """The entry point's own checks: a pair with n + C >= 10^6, and one whose workspace lies outside the buffer, get a status and
    no write."""
    be = emu
    leaf = np.array([0, 1, 4, 0], np.int64)
    d_leaves, d_cells = be.upload(leaf), be.upload(np.zeros(4, np.uint8))
    d_work = be.upload(np.array([0, 0], np.int32))
    d_prof = be.empty(4 * 24)
    be.call("mprg_align_profiles", be.ptr(d_cells), be.ptr(d_leaves), be.ptr(d_work), 1, be.ptr(d_prof), be.stream)
    pairs = np.array([[0, 0, pa.MAX_LEN, 0, 0], [0, 0, 3, 1 << 20, 0], [5, 0, 3, 0, 0]], np.int64)
    d_out = be.empty(36)
    be.call("mprg_align_pairs", be.ptr(d_prof), be.ptr(d_leaves), 1, be.ptr(be.upload(np.zeros(8, np.uint8))), be.ptr(be.upload(pairs)),
            3, be.ptr(be.empty(4 * 4096)), 4096, be.ptr(be.empty(64)), 64, be.ptr(d_out), be.stream)
    assert be.download(d_out, np.int32, 9).reshape(3, 3)[:, 0].tolist() == [1, 2, 3]


def test_recorded_mafft_calls_reproduced(emu, golden):
    """All 13 aligner calls of the reference's ten update cases: rows (ids, descriptions, order, sequences) as recorded."""
    reqs, wants = [], []
    for case in golden["cases"]:
        for rec in case["aligner_replay"]:
            reqs.append((read_fasta_alignment(rec["previous_msa"]), set(rec["new_sequences"])))
            wants.append(rec["updated_rows"])
    assert len(reqs) == 13
    aligner = BuiltinAligner(emu)
    for got, want in zip(aligner.get_updated_alignments(reqs), wants):
        assert [[i, d, s] for i, d, s in zip(got.ids, got.descriptions, got.rows_as_strings())] == want
    one = aligner.get_updated_alignment(*reqs[0])
    assert one.rows_as_strings() == [s for _, _, s in wants[0]]


def run_case_builtin(case, tmp: Path, backend):
    """tests/update_common.run_case with the built-in aligner in place of the recorded answers."""
    from make_prg_amd.subcommands import from_msa, update
    from make_prg_amd.subcommands.output_type import OutputType
    src = tmp / case["case"] / "msas"
    src.mkdir(parents=True)
    for f in case["inputs"]:
        (src / f["name"]).write_text(f["fasta"])
    single = len(case["inputs"]) == 1
    base_prefix = str(tmp / case["case"] / "base" / "base")
    from_msa.run(Namespace(input=str(src / case["inputs"][0]["name"]) if single else str(src), suffix="",
                           output_prefix=base_prefix, alignment_format="fasta", max_nesting=case["N"],
                           min_match_length=case["L"], output_type=OutputType("a"), force=False, threads=1), backend)
    denovo = tmp / case["case"] / "denovo_paths.txt"
    denovo.write_text(case["denovo_paths"])
    prefix = str(tmp / case["case"] / "out" / case["case"])
    aligner = BuiltinAligner(backend)
    update.run(Namespace(update_DS=Path(base_prefix + ".update_DS.zip"), denovo_paths=str(denovo), output_prefix=prefix,
                         long_deletion_threshold=case["long_deletion_threshold"], output_type=OutputType(case["output_type"]),
                         force=False, threads=1), aligner=aligner)
    assert aligner.calls == len(case["aligner_replay"])
    return prefix


def test_reference_update_cases_with_builtin_aligner(emu, golden, tmp_path):
    """Byte-equal to the reference's outputs because the built-in reproduces these calls (not a claim of MAFFT equivalence)."""
    from tests import update_common as uc
    n = 0
    for case in golden["cases"]:
        n += uc.check_outputs(case, run_case_builtin(case, tmp_path, emu))
    assert n >= 20


def test_update_aligner_builtin_rebuilds_leaves_that_spell_their_rows(emu, golden, tmp_path, monkeypatch):
    """`--aligner builtin` through update.run's own option handling on sample_example: every touched leaf's rebuilt sub-tree
    spells all its old rows and all its new sequences."""
    from make_prg_amd.recursion_tree import LeafNode
    from make_prg_amd.subcommands import from_msa, update
    from make_prg_amd.subcommands.output_type import OutputType
    from tests.prg_walk import _prepare, parse_prg, spellings
    case = next(c for c in golden["cases"] if c["case"] == "sample_example_update")
    src = tmp_path / "msas"
    src.mkdir()
    for f in case["inputs"]:
        (src / f["name"]).write_text(f["fasta"])
    base = str(tmp_path / "base" / "base")
    from_msa.run(Namespace(input=str(src), suffix="", output_prefix=base, alignment_format="fasta", max_nesting=case["N"],
                           min_match_length=case["L"], output_type=OutputType("a"), force=False, threads=1), emu)
    (tmp_path / "denovo_paths.txt").write_text(case["denovo_paths"])
    replaced = []
    original = LeafNode.replace_by

    def record(self, new_node):
        replaced.append((self.alignment.rows_as_strings(), sorted(self.new_sequences), new_node))
        original(self, new_node)
    monkeypatch.setattr(LeafNode, "replace_by", record)
    n_ok, _ = update.run(Namespace(update_DS=Path(base + ".update_DS.zip"), denovo_paths=str(tmp_path / "denovo_paths.txt"),
                                   output_prefix=str(tmp_path / "out" / "u"), long_deletion_threshold=case["long_deletion_threshold"],
                                   output_type=OutputType("a"), force=False, threads=1, aligner="builtin", aligner_replay=None))
    assert n_ok > 0 and len(replaced) == 3
    for rows, new, sub in replaced:
        sub.prg_builder.site_num = 5
        parts = []
        sub.preorder_traversal_to_build_prg(parts)
        tree = parse_prg("".join(parts))
        _prepare(tree)
        for r in rows + new:
            assert spellings(tree, r.replace("-", "")) >= 1, r
    assert os.path.exists(str(tmp_path / "out" / "u") + ".prg.fa")


def test_aligner_flags_are_mutually_exclusive(capsys):
    from make_prg_amd.__main__ import main
    with pytest.raises(SystemExit) as exc:
        main(["update", "-u", "x.update_DS.zip", "-d", "d.txt", "-o", "o", "--aligner", "builtin", "--aligner-replay", "x"])
    assert exc.value.code == 2
    assert "not allowed with argument" in capsys.readouterr().err


def test_merge_left_justifies_insertions():
    rows = ["AAAA", "AAAA"]
    seqs = ["CAAAAC", "GGAAAAG", "TAAAAT"]
    got = ar.update_alignment(rows, seqs)
    assert got == ["--AAAA-", "--AAAA-", "C-AAAAC", "GGAAAAG", "T-AAAAT"]
    ops = [ar.align_pair(rows, s)[0].encode() for s in sorted(seqs)]
    merged = pa.merge(np.frombuffer("".join(rows).encode(), np.uint8).reshape(2, -1), [seq_codes(s) for s in sorted(seqs)], ops)
    assert [r.tobytes().decode() for r in merged] == got
    assert MSA.from_strings(got).get_alignment_length() == 7
