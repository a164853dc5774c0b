"""Accessibility of every window of W bases (no binary of the reference does this): the
probability that all W bases are unpaired, P = Z_c / Z with 'x' over the window.

    python -m rna_algos_amd.bin.accessibility -i FASTA -o OUT -w W [-c] [-s] [--synthetic-tables SEED]

Per record one batch of the inside-only sweep (rnamc_log_partition_batch): the unconstrained record
and one constrained record per window.  The output holds `>{index}`, then one line
`start<TAB>P(unpaired)` per window (start 0-based, windows start .. start + W - 1; none when the
record is shorter than W).  Tables as for the other folding CLIs ($RNAMC_TABLES, or
--synthetic-tables)."""
import argparse
import sys

from ..mccaskill_algo import unpaired_probability
from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="accessibility")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-w", "--window", type=int, required=True, help="window length W (bases)")
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true",
                    help="CONTRAfold only: hairpins of fewer than 3 unpaired bases")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    args = ap.parse_args(argv)
    if args.window < 1:
        ap.error("-w must be >= 1")
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
    w = args.window
    buf = []
    for rna_id, (_, seq) in enumerate(recs):
        buf.append(f">{rna_id}\n")
        starts = range(len(seq) - w + 1)
        if len(starts) == 0:
            continue
        p = unpaired_probability(seq, [(a, a + w - 1) for a in starts], args.uses_contra_model,
                                 args.allows_short_hairpins, fold_score_sets)
        buf.extend(f"{a}\t{float(x):.6f}\n" for a, x in zip(starts, p))
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
