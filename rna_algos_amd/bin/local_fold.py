"""Windowed local folding of long RNAs (not in the reference; what RNAplfold / LocalFold compute):

    python -m rna_algos_amd.bin.local_fold -i FASTA -o OUT -w W [-l L] [--stride S] [--min-bpp P]
                                           [-c] [-s] [--constraints FILE] [--synthetic-tables SEED]

Every window of W bases of a record (starts 0, S, 2S, ..., and a last window ending at the record's
end) is folded with the pair-span limit L (default: W), and each pair gets the average of its
probability over the windows that contain it (rnamc_bpp_windowed: the windows' triangles stay on
the GPU, a record may be longer than 65 535 nt).  The output has the format of the `mccaskill_algo`
CLI: the `# Format = ...` header, then per record `\\n\\n>{index}\\n` and `i,j,p ` triples, here the
pairs with p >= P (default 0.01) ordered by span, then i.  `-c` CONTRAfold model, `-s` with it
short hairpins.  `--constraints FILE`: one string per record over `. x < >` only (brackets cannot
be cut at window edges)."""
import argparse
import math
import sys

from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables
from ..mccaskill_algo import mccaskill_algo_windowed
from . import _constraints
from .mccaskill_algo import HEADER, fmt_f32


def pairs2str(res, min_prob):
    """the triples of a WindowedBpp with p >= min_prob, in `pairs` order"""
    i, j, p = res.pairs(min_prob)
    return "".join(f"{int(a)},{int(b)},{fmt_f32(q)} " for a, b, q in zip(i, j, p))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="local_fold")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-w", "--window", type=int, required=True, metavar="W", help="window length, 1 .. 65535")
    ap.add_argument("-l", "--max-bp-span", type=int, default=0, metavar="L",
                    help="longest admitted base-pair span j - i + 1 (0: the window length)")
    ap.add_argument("--stride", type=int, default=1, metavar="S", help="distance of window starts (default 1)")
    ap.add_argument("--min-bpp", type=float, default=0.01, metavar="P",
                    help="write only the pairs with averaged probability >= P (default 0.01)")
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true")
    ap.add_argument("--constraints", default=None, metavar="FILE",
                    help="FASTA file of constraint strings over . x < > (no brackets), one per input record")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    args = ap.parse_args(argv)
    _constraints.check_span(ap, args)
    if not 1 <= args.window <= 65535:
        ap.error("-w must lie in 1 .. 65535")
    if not 1 <= args.stride < 2 ** 32:
        ap.error("--stride must lie in 1 .. 2^32 - 1")
    if not (math.isfinite(args.min_bpp) and args.min_bpp >= 0):
        ap.error("--min-bpp must be finite and >= 0")
    return args


def check_no_brackets(cons):
    """ConstraintFileError for a record whose string holds a bracket: a pair cannot be cut at a window edge"""
    for k, c in enumerate(cons):
        for ch in "()":
            if ch in c:
                raise _constraints.ConstraintFileError(
                    f"constraint record {k}, position {c.index(ch)}: '{ch}' — windowed folding takes "
                    "only . x < > (a bracket pair cannot be cut at window edges)")


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
    cons = [None] * len(recs)
    if args.constraints is not None:
        try:
            cons = _constraints.load(args.constraints, recs)
            check_no_brackets(cons)
        except (_constraints.ConstraintFileError, OSError) as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
    buf = [HEADER]
    for rna_id, ((_, seq), c) in enumerate(zip(recs, cons)):
        res = mccaskill_algo_windowed(seq, args.window, args.uses_contra_model, args.allows_short_hairpins,
                                      fold_score_sets, args.stride, args.max_bp_span, c)
        buf.append(f"\n\n>{rna_id}\n")
        buf.append(pairs2str(res, args.min_bpp))
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
