"""Records tests/golden/stage_names.json: the profile stage names of the calls test_stage_sequence_is_unchanged makes (one call of a
fresh Mapper per case, on the genome of the GPU suite's `env` fixture).  Run on the GPU with the library whose launch sequence is the
reference -- the committed file was written by the library of the commit before the launch path was split into stage functions:

    python tests/golden/make_stage_names.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from bitmapperbs_amd import synth, mapper
    from common import plant_repeats
    import test_gpu_parity as T
    wd = tempfile.mkdtemp(prefix="bmbs_stage_names_")
    names, chroms = synth.make_genome(1_500_000, 3, seed=77)            # as the `env` fixture
    plant_repeats(chroms, seed=78)
    fa = os.path.join(wd, "g.fa")
    synth.write_fasta(fa, names, chroms)
    mapper.Index.build(fa, fa, threads=8)
    ix = mapper.Index(fa)
    out = {case: T.stage_names(chroms, ix, case) for case in sorted(T.STAGE_CASES)}
    assert "k_vote_mid" in out["se_L250"], out["se_L250"]
    sens = out["pe_sensitive_L100"]
    assert "k_pes_vote" in sens and "k_filter_pe_r3" in sens, "raise the error rate of the sensitive case: %r" % (sens,)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "stage_names.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for case, v in out.items():
        print(case, len(v), " ".join(v))


if __name__ == "__main__":
    main()
