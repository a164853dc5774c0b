"""Mirror of the reference binary `mccaskill_algo` (src/bin/mccaskill_algo.rs:6-113):

    python -m rna_algos_amd.bin.mccaskill_algo -i FASTA -o OUT [-c] [-t N]

Same flags, same output text: a `# Format = ...` header, then per record
`\\n\\n>{index}\\n` followed by `i,j,p ` triples (Rust `{}` formatting of the f32).  The
reference iterates a hash map, so the order of the triples inside a record is
unspecified there; here it is ascending (i, j).  The whole FASTA goes to the GPU as one
batch instead of one thread-pool task per record; `-t` is accepted and ignored.
`--constraints FILE` / `--max-bp-span L` (not in the reference) give the pair probabilities over a
restricted structure space (bin/_constraints.py).  `--min-bpp P` (not in the reference) writes only
the triples with p >= P, taken from the device-compacted lists (rnamc_bpp_batch_sparse): the dense
triangles never reach the host.  Without the flag nothing changes."""
import argparse
import math
import sys

import numpy as np

from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables
from ..mccaskill_algo import mccaskill_algo_batch, mccaskill_algo_batch_sparse
from . import _constraints

HEADER = ("# Format = >{RNA sequence id} {line break} {basepairing left nucleotide}, "
          "{basepairing right nucleotide}, {basepairing probability} ...")


def fmt_f32(x):
    """Rust's `{}` for f32: shortest decimal that round-trips, never scientific."""
    return np.format_float_positional(np.float32(x), unique=True, trim="-")


def probs2str(mat):
    """src/bin/mccaskill_algo.rs:104-113 over a BppMatrix."""
    out = []
    n = mat.n
    idx = np.nonzero(mat.packed >= -0.5)[0]
    # packed index -> (i, j); emit ascending (i, j)
    d = np.zeros(idx.shape[0], dtype=np.int64)
    starts = np.array([dd * n - dd * (dd - 1) // 2 for dd in range(n + 1)], dtype=np.int64)
    d = np.searchsorted(starts, idx, side="right") - 1
    i = idx - starts[d]
    j = i + d
    order = np.lexsort((j, i))
    for k in order:
        out.append(f"{int(i[k])},{int(j[k])},{fmt_f32(mat.packed[idx[k]])} ")
    return "".join(out)


def sparse2str(sp):
    """probs2str over a SparseBpp: its triples in ascending (i, j) order."""
    order = np.lexsort((sp.j, sp.i))
    return "".join(f"{int(sp.i[k])},{int(sp.j[k])},{fmt_f32(sp.p[k])} " for k in order)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="mccaskill_algo")
    ap.add_argument("-i", "--input_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-t", "--num_threads", type=int, default=0)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    ap.add_argument("--min-bpp", type=float, default=None, metavar="P",
                    help="write only the pairs with probability >= P (finite, >= 0)")
    _constraints.add_args(ap)
    args = ap.parse_args(argv)
    _constraints.check_span(ap, args)
    if args.min_bpp is not None and not (math.isfinite(args.min_bpp) and args.min_bpp >= 0):
        ap.error("--min-bpp must be finite and >= 0")
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
    buf = [HEADER]
    if args.min_bpp is not None:
        lists, _ = mccaskill_algo_batch_sparse([s for _, s in recs], args.uses_contra_model, False,
                                               fold_score_sets, args.min_bpp, cons, args.max_bp_span)
        for rna_id, sp in enumerate(lists):
            buf.append(f"\n\n>{rna_id}\n")
            buf.append(sparse2str(sp))
    else:
        mats, _ = mccaskill_algo_batch([s for _, s in recs], args.uses_contra_model, False,
                                       fold_score_sets, cons, args.max_bp_span)
        for rna_id, m in enumerate(mats):
            buf.append(f"\n\n>{rna_id}\n")
            buf.append(probs2str(m))
    with open(args.output_file_path, "w") as fh:
        fh.write("".join(buf))
    return 0


if __name__ == "__main__":
    sys.exit(main())
