"""TEST INFRASTRUCTURE: the oracle's answer for the rare-path alignment with ambiguity codes that takes it 15 s
(tests/view_edges.py: wide_and_tall_view with sprinkle(.., SEED_AMB, P_AMB) — 530 x 4 200 cells whose ~1 800 codes make a tree of
1 568 nodes), so that its GPU test compares with a record instead of waiting for the oracle.  tests/test_oracle_golden.py holds the
record against the oracle itself.  `--reference` additionally runs the unmodified reference on the same text (container only) and
records whether PRG and node count are identical.
Writes tests/golden/rare_paths_codes.json: hashes of the text, the PRG / .bin / .gfa / recursion tree / prg_index.

    python -m oracle.tools.gen_rare_paths_golden [--reference]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = ("wide_and_tall_view",)


def main():
    want_reference = "--reference" in sys.argv
    if want_reference:
        import oracle.refshim.bootstrap as rb
        rb.preset_env()
        rb.install()
    import oracle.from_msa_oracle as orc
    from oracle.tools.gen_ddeep_golden import sha
    from tests import view_edges as ve
    out = {}
    for name in CASES:
        texts, N, L = ve.sprinkled(getattr(ve, name)(), ve.SEED_AMB, ve.P_AMB)
        t0 = time.time()
        prg, b, root = orc.build_locus_from_text(texts[0], N, L)
        tree = orc.tree_dump(root)
        rec = dict(builder=name, seed=ve.SEED_AMB, p=ve.P_AMB, N=N, L=L, fasta_sha256=sha(texts[0]), oracle_seconds=round(time.time() - t0, 1),
                   expect=dict(prg_sha256=sha(prg), prg_len=len(prg), bin_sha256=sha(orc.encode_prg_bytes(prg)), gfa_sha256=sha(orc.gfa_text(prg)),
                               tree_sha256=sha(tree), next_node_id=b.next_node_id, site_num=b.site_num,
                               prg_index_sha256=sha(sorted([s, e, n] for (s, e), n in b.prg_index.items()))))
        if want_reference:
            import tempfile
            from pathlib import Path
            from make_prg.prg_builder import PrgBuilder
            p = Path(tempfile.mkdtemp()) / f"{name}.fa"
            p.write_text(texts[0])
            t0 = time.time()
            rb_ = PrgBuilder(name, p, "fasta", N, L)
            ref_prg = rb_.build_prg()
            rec["reference"] = dict(seconds=round(time.time() - t0, 1), prg_identical=ref_prg == prg,
                                    next_node_id_identical=rb_.next_node_id == b.next_node_id)
            assert ref_prg == prg, "the real reference disagrees with the oracle on " + name
        out[name] = rec
    with open(os.path.join(ROOT, "tests", "golden", "rare_paths_codes.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
