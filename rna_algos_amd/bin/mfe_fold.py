"""Maximum-score structure prediction (no binary of the reference does this): the MFE structure
under Turner, the Viterbi parse under CONTRAfold.

    python -m rna_algos_amd.bin.mfe_fold -i FASTA -o OUT [-c] [-s] [--synthetic-tables SEED]

The whole FASTA goes to the GPU as one batch (rnamc_mfe_batch).  Per record the output holds
`>{index}`, then one line `dot_bracket<TAB>score`, score being the sum of the structure's loop
scores.  Tables as for the other folding CLIs ($RNAMC_TABLES, or --synthetic-tables)."""
import argparse
import sys

from ..mccaskill_algo import mfe_fold_batch
from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="mfe_fold")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true",
                    help="CONTRAfold only: hairpins of fewer than 3 unpaired bases")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic_tables is not None:
        set_default_tables(FoldScoreSets.synthetic(args.synthetic_tables))
        print(f"warning: SYNTHETIC scoring tables (seed {args.synthetic_tables}): the output is "
              "not comparable with the reference's", file=sys.stderr)
    recs = read_fasta(args.input_file_path)
    fold_score_sets = FoldScoreSets.new(0.0)
    try:
        fold_score_sets.transfer()
    except NoTablesError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    folds = mfe_fold_batch([s for _, s in recs], args.uses_contra_model,
                           args.allows_short_hairpins, fold_score_sets)
    buf = []
    for rna_id, (db, score) in enumerate(folds):
        buf.append(f">{rna_id}\n{db}\t{score:.6f}\n")
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
