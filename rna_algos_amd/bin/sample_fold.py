"""Boltzmann sampling of secondary structures (no binary of the reference does this):

    python -m rna_algos_amd.bin.sample_fold -i FASTA -o OUT -n N [-c] [-s SEED] [--synthetic-tables SEED]
                                            [--constraints FILE] [--max-bp-span L]

The whole FASTA goes to the GPU as one batch (rnamc_sample_batch).  Per record the output holds
`>{index}`, then N lines `dot_bracket<TAB>log_prob` with log_prob = log_weight - ln Z, the
natural logarithm of the structure's probability.  Tables as for the other folding CLIs
($RNAMC_TABLES, or --synthetic-tables).  --constraints / --max-bp-span sample the restricted structure
space (bin/_constraints.py); log_prob is then relative to Z_c."""
import argparse
import sys

from ..mccaskill_algo import sample_structures_batch
from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables
from . import _constraints


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="sample_fold")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-n", "--num_samples", type=int, required=True)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--seed", type=int, default=0)
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    _constraints.add_args(ap)
    args = ap.parse_args(argv)
    if args.num_samples < 0:
        ap.error("-n must be >= 0")
    _constraints.check_span(ap, args)
    return args


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
    cons = None
    if args.constraints is not None:
        try:
            cons = _constraints.load(args.constraints, recs)
        except (_constraints.ConstraintFileError, OSError) as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
    samples, logz = sample_structures_batch([s for _, s in recs], args.num_samples,
                                            args.uses_contra_model, False, fold_score_sets,
                                            args.seed, cons, args.max_bp_span)
    buf = []
    for rna_id, (rows, lz) in enumerate(zip(samples, logz)):
        buf.append(f">{rna_id}\n")
        buf.extend(f"{db}\t{w - float(lz):.6f}\n" for db, w in rows)
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
