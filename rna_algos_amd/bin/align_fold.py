"""Alignment folding (not a binary of the reference; what CentroidAlifold, PETfold and RNAalifold -p
compute from the model's alignment readers and its `mccaskill_algo`):

    python -m rna_algos_amd.bin.align_fold -i in.{aln,fa,sto} -o OUT_DIR [-c] [-s] [-g GAMMA ...]
                                           [--min-bpp P] [--max-bp-span L] [--synthetic-tables SEED]

The alignment is read by its extension (.aln Clustal, .fa / .fasta FASTA, .sto / .stk Stockholm);
every row is folded without its gaps, the pair probabilities are mapped onto alignment columns and
averaged over all rows on the GPU (rnamc_bpp_alignment: the rows' triangles stay on the device).
OUT_DIR receives `bpp.dat` in the format of `mccaskill_algo --min-bpp` over COLUMNS (the header, one
record `>0`, the triples `ci,cj,p ` with p >= P, default 0.01, ordered by span, then ci) and per
gamma one `centroid_threshold={gamma}.fa` as `centroid_fold` names its files, holding `>0` and the
consensus dot-bracket string over the columns.  Without -g the gammas are 2^-7 .. 2^10.  `-c`
CONTRAfold model, `-s` with it short hairpins, `--max-bp-span L` counted in each row's own bases."""
import argparse
import math
import os
import sys

from ..centroid_fold import MAX_POW_2, MIN_POW_2
from ..mccaskill_algo import alignment_fold
from ..utils import FoldScoreSets, NoTablesError, read_align, set_default_tables
from . import _constraints
from .mccaskill_algo import HEADER, fmt_f32


def pairs2str(res, min_prob):
    """the triples of an AlignmentBpp with p >= min_prob, in `pairs` order"""
    i, j, p = res.pairs(min_prob)
    return "".join(f"{int(a)},{int(b)},{fmt_f32(q)} " for a, b, q in zip(i, j, p))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="align_fold")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_dir_path", required=True)
    ap.add_argument("-g", "--centroid_threshold", type=float, nargs="+", default=None, metavar="GAMMA")
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true")
    ap.add_argument("--min-bpp", type=float, default=0.01, metavar="P",
                    help="write only the column pairs with averaged probability >= P (default 0.01)")
    ap.add_argument("--max-bp-span", type=int, default=0, metavar="L",
                    help="longest admitted base-pair span j - i + 1 in a row's own bases (0: no limit)")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    args = ap.parse_args(argv)
    _constraints.check_span(ap, args)
    if not (math.isfinite(args.min_bpp) and args.min_bpp >= 0):
        ap.error("--min-bpp must be finite and >= 0")
    if args.centroid_threshold is not None and any(math.isnan(g) for g in args.centroid_threshold):
        ap.error("-g must not be NaN")
    return args


def gammas_of(args):
    if args.centroid_threshold is not None:
        return list(args.centroid_threshold)
    return [2.0 ** k for k in range(MIN_POW_2, MAX_POW_2 + 1)]


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic_tables is not None:
        set_default_tables(FoldScoreSets.synthetic(args.synthetic_tables))
        print(f"warning: SYNTHETIC scoring tables (seed {args.synthetic_tables}): the output is "
              "not comparable with the reference's", file=sys.stderr)
    try:
        rows, _ = read_align(args.input_file_path)
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    fold_score_sets = FoldScoreSets.new(0.0)
    try:
        fold_score_sets.transfer()
    except NoTablesError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    gammas = gammas_of(args)
    res = alignment_fold(rows, args.uses_contra_model, args.allows_short_hairpins, fold_score_sets, gammas,
                         args.max_bp_span)
    os.makedirs(args.output_dir_path, exist_ok=True)
    with open(os.path.join(args.output_dir_path, "bpp.dat"), "w") as fh:
        fh.write(HEADER + "\n\n>0\n" + pairs2str(res, args.min_bpp))
    for g, (fold, _) in zip(gammas, res.folds):
        with open(os.path.join(args.output_dir_path, f"centroid_threshold={fmt_f32(g)}.fa"), "w") as fh:
            fh.write(">0\n" + fold)
    return 0


if __name__ == "__main__":
    sys.exit(main())
