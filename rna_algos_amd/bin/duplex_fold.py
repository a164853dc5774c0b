"""RNA-RNA duplex folding (the RNAduplex / RNAhybrid / RNAplex question): every query scanned against
every target on the GPU.

    python -m rna_algos_amd.bin.duplex_fold -q QUERIES.fa -t TARGETS.fa -o OUT.tsv [-c] [--probs DIR]
                                            [--synthetic-tables SEED]

Every (query, target) pair is one call item of rnamc_duplex_batch: the query is strand A, the target
strand B, both 5'->3'.  One line per pair, tab-separated, queries outermost:

    query  target  lnZ  best_score  i_first  j_first  structure

lnZ: the log partition function over all duplexes of the pair (no initiation term); best_score: the
log weight of the best duplex; i_first / j_first: its outer-end pair, 0-based positions in query
and target (-1 -1: the strands have no canonical pair); structure: the query's bases as '(' / '.',
'&', the target's bases as ')' / '.'.  --probs DIR also writes every pair's nA x nB matrix of pair
probabilities as DIR/{query index}_{target index}.npy; without it no matrix leaves the device.
Tables as for the other folding CLIs ($RNAMC_TABLES, or --synthetic-tables)."""
import argparse
import os
import sys

from ..duplex import duplex_fold_batch
from ..utils import FoldScoreSets, NoTablesError, read_fasta, set_default_tables


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="duplex_fold")
    ap.add_argument("-q", "--query_file_path", required=True)
    ap.add_argument("-t", "--target_file_path", required=True)
    ap.add_argument("-o", "--output_file_path", required=True)
    ap.add_argument("-c", "--uses_contra_model", action="store_true")
    ap.add_argument("--probs", default=None, metavar="DIR",
                    help="write every pair's matrix of pair probabilities to DIR as .npy")
    ap.add_argument("--synthetic-tables", type=int, default=None, metavar="SEED",
                    help="NOT the reference's parameters: seeded synthetic tables (testing only). "
                         "Without it $RNAMC_TABLES must name a table file dumped from the "
                         "rna-ss-params crate")
    return ap.parse_args(argv)


def format_line(query, target, fold):
    chain = fold.pairs()
    i_first, j_first = chain[0] if chain else (-1, -1)
    return (f"{query}\t{target}\t{fold.log_z:.9g}\t{fold.best_score:.9g}\t{i_first}\t{j_first}\t"
            f"{fold.structure}\n")


def parse_line(line):
    """format_line backwards -> (query, target, lnZ, best_score, i_first, j_first, structure)"""
    q, t, log_z, best, i_first, j_first, structure = line.rstrip("\n").split("\t")
    return q, t, float(log_z), float(best), int(i_first), int(j_first), structure


def main(argv=None):
    args = parse_args(argv)
    if args.synthetic_tables is not None:
        set_default_tables(FoldScoreSets.synthetic(args.synthetic_tables))
        print(f"warning: SYNTHETIC scoring tables (seed {args.synthetic_tables}): the output is "
              "not comparable with the reference's", file=sys.stderr)
    queries = read_fasta(args.query_file_path)
    targets = read_fasta(args.target_file_path)
    fold_score_sets = FoldScoreSets.new(0.0)
    try:
        fold_score_sets.transfer()
    except NoTablesError as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    seqs = [s for _, s in queries] + [s for _, s in targets]
    pairs = [(q, len(queries) + t) for q in range(len(queries)) for t in range(len(targets))]
    folds = duplex_fold_batch(seqs, pairs, args.uses_contra_model, fold_score_sets,
                              want_probs=args.probs is not None, want_best=True)
    if args.probs is not None:
        import numpy as np
        os.makedirs(args.probs, exist_ok=True)
    with open(args.output_file_path, "w") as fh:
        for (q, t), fold in zip(pairs, folds):
            t -= len(queries)
            fh.write(format_line(queries[q][0], targets[t][0], fold))
            if args.probs is not None:
                np.save(os.path.join(args.probs, f"{q}_{t}.npy"), fold.probs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
