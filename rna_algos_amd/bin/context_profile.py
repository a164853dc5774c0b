"""Structural context profiles (what CapR computes; the reference's consprob and consalifold call
them context profiles): for every base the probability of being unpaired in a bulge, the exterior
loop, a hairpin, an internal loop or a multibranch loop, or of being paired.

    python -m rna_algos_amd.bin.context_profile -i FASTA -o OUT [-c] [-s] [--synthetic-tables SEED]
                                                [--constraints FILE] [--max-bp-span L]

The whole FASTA goes to the GPU as one batch (rnamc_context_profile_batch).  The output is CapR's
text format: per record `>{index}`, then six lines `Bulge`, `Exterior`, `Hairpin`, `Internal`,
`Multibranch`, `Stem`, each followed by the record's n values, space-separated, then a blank line.
Tables as for the other folding CLIs ($RNAMC_TABLES, or --synthetic-tables).
--constraints / --max-bp-span fold over a restricted structure space (bin/_constraints.py)."""
import argparse
import sys

from ..mccaskill_algo import CONTEXTS, context_profile_batch
from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables
from . import _constraints


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="context_profile")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true",
                    help="CONTRAfold only: hairpins of fewer than 3 unpaired bases")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    _constraints.add_args(ap)
    args = ap.parse_args(argv)
    _constraints.check_span(ap, args)
    return args


def format_profiles(profiles):
    """CapR's text format of a list of (6, n) arrays"""
    buf = []
    for rna_id, prof in enumerate(profiles):
        buf.append(f">{rna_id}\n")
        for name, row in zip(CONTEXTS, prof):
            buf.append(name.capitalize() + " " + " ".join(f"{float(v):.9g}" for v in row) + "\n")
        buf.append("\n")
    return "".join(buf)


def parse_profiles(text):
    """format_profiles backwards -> list of (6, n) f32 arrays"""
    import numpy as np
    out, rows = [], []
    for line in text.splitlines():
        if line.startswith(">"):
            rows = []
        elif line.strip():
            name, *vals = line.split()
            if name.lower() != CONTEXTS[len(rows)]:
                raise ValueError(f"row {len(rows)} of record {len(out)} is {name!r}")
            rows.append([float(v) for v in vals])
            if len(rows) == len(CONTEXTS):
                out.append(np.array(rows, np.float32))
    return out


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
    profiles, _ = context_profile_batch([s for _, s in recs], args.uses_contra_model,
                                        args.allows_short_hairpins, fold_score_sets, cons, args.max_bp_span)
    with open(args.output_file_path, "w") as fh:
        fh.write(format_profiles(profiles))
    return 0


if __name__ == "__main__":
    sys.exit(main())
