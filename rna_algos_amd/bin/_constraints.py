"""The hard-constraint flags of the folding CLIs (include/rnamc.h):

    --constraints FILE   FASTA-format, one constraint string over ". x ( ) < >" per record, in the
                         input's record order and of its record's length
    --max-bp-span L      longest admitted pair span j - i + 1 (0: no limit)

Without them a CLI's output is what it was without constraints."""
from ..mccaskill_algo import check_constraint
from .. import _lib
from ..utils import read_fasta_raw


class ConstraintFileError(ValueError):
    pass


def add_args(ap):
    ap.add_argument("--constraints", default=None, metavar="FILE",
                    help="FASTA file of constraint strings (. x ( ) < >), one per input record")
    ap.add_argument("--max-bp-span", type=int, default=0, metavar="L",
                    help="longest admitted base-pair span j - i + 1 (0: no limit)")


def check_span(ap, args):
    if args.max_bp_span < 0 or args.max_bp_span >= 2 ** 32:
        ap.error("--max-bp-span must lie in 0 .. 2^32 - 1")


def load(path, recs):
    """The constraint strings of `path` for the records `recs` ((id, codes) pairs) -> list of str;
    ConstraintFileError when the count, a length or a string is wrong."""
    cons = read_fasta_raw(path)
    if len(cons) != len(recs):
        raise ConstraintFileError(f"{path} holds {len(cons)} constraint records, the input {len(recs)}")
    out = []
    for k, ((_, c), (_, seq)) in enumerate(zip(cons, recs)):
        if len(c) != len(seq):
            raise ConstraintFileError(f"constraint record {k} has length {len(c)}, its sequence {len(seq)}")
        try:
            check_constraint(c, len(seq))
        except _lib.RnamcError as e:
            raise ConstraintFileError(f"constraint record {k}: {e}") from None
        out.append(c)
    return out
