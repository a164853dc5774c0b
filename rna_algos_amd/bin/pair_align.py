"""What the callers of the reference binary `durbin_algo` keep of all pairs of a FASTA: the match
probabilities above a threshold and an alignment of each pair, made on the GPU while the matrices
are there:

    python -m rna_algos_amd.bin.pair_align -i FASTA -o OUT_DIR [-g GAMMA ...] [--min-prob P]

All pairs in ascending (id1, id2).  `OUT_DIR/match.dat` has `durbin_algo`'s text format (with
`--min-prob 0` the text is identical to `durbin_algo`'s); per gamma `OUT_DIR/gamma={g}.aln` holds per
pair a header `>{id1},{id2} {expect_accuracy}` and the two gapped rows."""
import argparse
import os
import sys

from ..durbin_algo import AlignScores, with_pseudo_bases
from ..pair_align import pair_align_batch
from ..utils import read_fasta
from .durbin_algo import HEADER
from .mccaskill_algo import fmt_f32


def main(argv=None):
    ap = argparse.ArgumentParser(prog="pair_align")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_dir_path", required=True)
    ap.add_argument("-g", "--gamma", type=float, action="append", default=None,
                    help="a gamma of the centroid alignment (repeatable; default 2)")
    ap.add_argument("--min-prob", type=float, default=0.01)
    args = ap.parse_args(argv)
    gammas = args.gamma or [2.0]
    seqs = [with_pseudo_bases(s) for _, s in read_fasta(args.input_file_path)]
    align_scores = AlignScores.new(0.0)
    align_scores.transfer()
    pairs = [(a, b) for a in range(len(seqs)) for b in range(a + 1, len(seqs))]
    res = pair_align_batch(seqs, pairs, align_scores, gammas=gammas, min_prob=args.min_prob)
    os.makedirs(args.output_dir_path, exist_ok=True)
    buf = [HEADER]
    for (a, b), r in zip(pairs, res):
        buf.append(f"\n\n>{a},{b}\n")
        buf.append("".join(f"{int(i) - 1},{int(j) - 1},{fmt_f32(p)} " for i, j, p in zip(r.i, r.j, r.p)))
    with open(os.path.join(args.output_dir_path, "match.dat"), "w") as fh:
        fh.write("".join(buf))
    blocks = [[] for _ in gammas]
    for (a, b), r in zip(pairs, res):
        for block, (row_a, row_b, acc) in zip(blocks, r.alignments):
            block.append(f">{a},{b} {fmt_f32(acc)}\n{row_a}\n{row_b}\n")
    for gamma, block in zip(gammas, blocks):
        with open(os.path.join(args.output_dir_path, f"gamma={fmt_f32(gamma)}.aln"), "w") as fh:
            fh.write("".join(block))
    return 0


if __name__ == "__main__":
    sys.exit(main())
