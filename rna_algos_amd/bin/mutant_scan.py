"""Point-mutation scan (not in the reference; the riboSNitch / SNPfold / RNAsnp / RNAmute question):

    python -m rna_algos_amd.bin.mutant_scan -i FASTA -o OUT.tsv [-c] [-s] [--positions a-b,c]
                                            [--constraints FILE] [--max-bp-span L] [--synthetic-tables SEED]

Every single-base mutant of every record (or of the 0-based positions listed: single positions and
inclusive ranges a-b, in the order given) is folded and its pair-probability matrix compared with
the record's wild type on the GPU (rnamc_mutant_scan: no triangle reaches the host).  Per record the
output holds `>{index}` and one tab-separated line per mutant:

    pos  wt  mut  lnZ  dlnZ  dist2  max_dp  i  j  corr

`pos` 0-based, `wt` / `mut` the bases, `lnZ` the mutant's log partition function, `dlnZ` its
difference from the wild type's, `dist2` the squared Euclidean distance of the two pair-probability
matrices, `max_dp` the largest change of one pair's probability and `i j` that pair (`-1 -1` when
nothing moved), `corr` SNPfold's Pearson correlation of the two paired-probability profiles (`nan`
for a constant profile).  `-c` CONTRAfold model, `-s` with it short hairpins.  `--constraints FILE`:
one string per record over `. x ( ) < >`, applied to the wild type and to every mutant."""
import argparse
import sys

from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables
from ..mccaskill_algo import mutant_scan
from .. import _lib
from . import _constraints
from .mccaskill_algo import fmt_f32

BASES = "ACGU"


def parse_positions(text):
    """'a-b,c' -> [a, ..., b, c]: 0-based single positions and inclusive ranges, in the order given"""
    out = []
    for part in text.split(","):
        part = part.strip()
        lo, dash, hi = part.partition("-")
        if not lo.isdigit() or (dash and not hi.isdigit()):
            raise ValueError(f"bad position or range {part!r}")
        a, b = int(lo), int(hi) if dash else int(lo)
        if b < a or b >= 2 ** 32:
            raise ValueError(f"bad range {part!r}")
        out.extend(range(a, b + 1))
    return out


def lines_of(res, seq):
    """the lines of one record's MutantScan (seq: the wild type's base codes)"""
    corr = res.profile_correlation()
    dz, d2 = res.delta_log_z, res.dist2
    out = []
    for m in range(len(res)):
        p = int(res.pos[m])
        out.append("\t".join((str(p), BASES[int(seq[p])], BASES[int(res.base[m])], fmt_f32(res.log_z[m]),
                              repr(float(dz[m])), repr(float(d2[m])), fmt_f32(res.max_dp[m]),
                              str(int(res.max_pair[m, 0])), str(int(res.max_pair[m, 1])), repr(float(corr[m])))))
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="mutant_scan")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("-s", "--allows_short_hairpins", action="store_true")
    ap.add_argument("--positions", default=None, metavar="LIST",
                    help="0-based positions to mutate: single positions and inclusive ranges a-b, comma-separated "
                         "(default: every base)")
    _constraints.add_args(ap)
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    args = ap.parse_args(argv)
    _constraints.check_span(ap, args)
    if args.positions is not None:
        try:
            args.positions = parse_positions(args.positions)
        except ValueError as e:
            ap.error(f"--positions: {e}")
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
    cons = [None] * len(recs)
    if args.constraints is not None:
        try:
            cons = _constraints.load(args.constraints, recs)
        except (_constraints.ConstraintFileError, OSError) as e:
            print(f"error: {e}", file=sys.stderr)
            return 2
    buf = []
    for rna_id, ((_, seq), c) in enumerate(zip(recs, cons)):
        try:
            res = mutant_scan(seq, args.uses_contra_model, args.allows_short_hairpins, fold_score_sets,
                              args.positions, c, args.max_bp_span)
        except _lib.RnamcError as e:
            print(f"error: record {rna_id}: {e}", file=sys.stderr)
            return 2
        buf.append(f">{rna_id}\n")
        buf.extend(line + "\n" for line in lines_of(res, seq))
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
