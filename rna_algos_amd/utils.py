"""Host-side mirror of the reference's `utils` items that the McCaskill path uses
(reference: src/utils.rs): `bytes2seq` (562-577), the `FoldScoreSets` struct
(91-119) with its constructor / accumulate / transfer (src/mccaskill_algo.rs:24-211),
probability bounds (127-129) and the example FASTA path (126).

`FoldScoreSets` here wraps one `rnamc_params` block of the C ABI: the CONTRAfold
set proper (fields named exactly as in the reference) plus the Turner-2004
constants the reference reads straight from the `rna-ss-params` crate.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

EPSILON = 0.001
PROB_BOUND_LOWER = -EPSILON
PROB_BOUND_UPPER = 1.0 + EPSILON
EXAMPLE_FASTA_FILE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                       "tests", "golden", "sampled_trnas.fa")
A, C_, G, U = 0, 1, 2, 3
PSEUDO_BASE = U + 1
MAX_SEQ_LEN = 65535

_SHAPES = {
    "stack_scores": (4, 4, 4, 4), "terminal_mismatch_scores": (4, 4, 4, 4),
    "dangling_scores_left": (4, 4, 4), "dangling_scores_right": (4, 4, 4),
    "helix_close_scores": (4, 4), "basepair_scores": (4, 4),
    "interior_scores_explicit": (4, 4), "interior_scores_1x1": (4, 4),
    "terminal_mismatch_scores_hairpin": (4, 4, 4, 4),
    "terminal_mismatch_scores_1xmany": (4, 4, 4, 4), "terminal_mismatch_scores_2x3": (4, 4, 4, 4),
    "terminal_mismatch_scores_interior": (4, 4, 4, 4),
    "terminal_mismatch_scores_multibranch": (4, 4, 4, 4),
    "dangling_scores_5prime": (4, 4, 4), "dangling_scores_3prime": (4, 4, 4),
}
_TURNER_SHAPES = {"interior_scores_1x1": (4,) * 6, "interior_scores_1x2": (4,) * 7,
                  "interior_scores_2x2": (4,) * 8}


def bytes2seq(x):
    """ASCII ACGUacgu -> base codes 0..3 (np.uint8).  Any other byte raises
    (the reference panics, src/utils.rs:570-572)."""
    if isinstance(x, str):
        x = x.encode("ascii")
    raw = np.frombuffer(bytes(x), dtype=np.uint8)
    out = np.empty(raw.shape[0], dtype=np.uint8)
    _lib.check(_lib.lib().rnamc_bytes2seq(raw.ctypes.data, raw.shape[0], out.ctypes.data))
    return out


def read_fasta(path):
    """Minimal FASTA reader standing in for bio::io::fasta::Reader: list of
    (id, seq codes)."""
    recs, cur_id, cur = [], None, []
    with open(path, "rb") as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line.startswith(b">"):
                if cur_id is not None:
                    recs.append((cur_id, bytes2seq(b"".join(cur))))
                cur_id = line[1:].split()[0].decode() if len(line) > 1 else ""
                cur = []
            else:
                cur.append(line)
    if cur_id is not None:
        recs.append((cur_id, bytes2seq(b"".join(cur))))
    return recs


def read_fasta_raw(path):
    """FASTA records as they are written: list of (id, str), lines of a record joined, nothing
    decoded (constraint files: their characters are not bases)."""
    recs, cur_id, cur = [], None, []
    with open(path, "rb") as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line.startswith(b">"):
                if cur_id is not None:
                    recs.append((cur_id, b"".join(cur).decode("ascii", errors="replace")))
                cur_id = line[1:].split()[0].decode() if len(line) > 1 else ""
                cur = []
            else:
                cur.append(line)
    if cur_id is not None:
        recs.append((cur_id, b"".join(cur).decode("ascii", errors="replace")))
    return recs


# ---- alignment readers (src/utils.rs:657-754) ----
# The reference returns (Cols, SeqIds), the alignment column by column; here `rows` is the u8 array
# (n_rows, n_cols) of the same codes and `rows.T` its Cols.  Lines are cut as BufRead::lines cuts
# them ('\n', a trailing '\r' dropped), fields as split_whitespace does.

_ALIGN_CODES = np.full(256, PSEUDO_BASE, dtype=np.uint8)
for _ch, _code in (("A", A), ("C", C_), ("G", G), ("U", U)):
    _ALIGN_CODES[ord(_ch)] = _ALIGN_CODES[ord(_ch.lower())] = _code


def align_char2base(x):
    """One alignment character (str, bytes of length 1, or its code) -> 0..3 for ACGUacgu, PSEUDO_BASE
    (4, the gap) for everything else: '-', '.', 'T', 'N', ... (src/utils.rs:746-754)."""
    if isinstance(x, (str, bytes)):
        if len(x) != 1:
            raise ValueError("align_char2base takes one character")
        x = ord(x)
    x = int(x)
    return int(_ALIGN_CODES[x]) if 0 <= x < 256 else PSEUDO_BASE


def _align_lines(path):
    with open(path, "rb") as fh:
        data = fh.read().decode("utf-8")
    lines = data.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return [ln[:-1] if ln.endswith("\r") else ln for ln in lines]


def _align_rows(seqs, what):
    """equal-length strings -> u8 (n_rows, n_cols); ValueError for ragged rows or none"""
    if not seqs:
        raise ValueError(f"{what}: no sequence")
    n = len(seqs[0])
    for s, x in enumerate(seqs):
        if len(x) != n:
            raise ValueError(f"{what}: row {s} has {len(x)} columns, row 0 has {n}")
    rows = np.empty((len(seqs), n), dtype=np.uint8)
    for s, x in enumerate(seqs):
        codes = np.array([ord(ch) for ch in x], dtype=np.int64)
        rows[s] = np.where(codes < 256, _ALIGN_CODES[np.minimum(codes, 255)], PSEUDO_BASE)
    return rows


def read_align_clustal(path):
    """src/utils.rs:657-692: the first line (the CLUSTAL header), empty lines and lines that start with
    a blank (the conservation line) separate blocks; every other line is `id sequence`, the ids are
    taken from the first block, later blocks extend the rows in order -> (rows, seq_ids)."""
    seqs, seq_ids = [], []
    seq_pointer, has_read_seq_ids = 0, False
    for i, line in enumerate(_align_lines(path)):
        if i == 0 or line == "" or line.startswith(" "):
            if seqs:
                seq_pointer = 0
                has_read_seq_ids = True
            continue
        fields = line.split()
        if len(fields) < 2:
            raise ValueError(f"{path}: line {i + 1}: expected `id sequence`")
        if not has_read_seq_ids:
            seq_ids.append(fields[0])
            seqs.append("")
        if seq_pointer >= len(seqs):
            raise ValueError(f"{path}: line {i + 1}: a block with more rows than the first")
        seqs[seq_pointer] += fields[1]
        seq_pointer += 1
    return _align_rows(seqs, path), seq_ids


def read_align_fasta(path):
    """src/utils.rs:694-717: records split at '>', the first whitespace-separated token the id, the
    rest joined to the row -> (rows, seq_ids)."""
    seqs, seq_ids = [], []
    with open(path, "rb") as fh:
        chunks = fh.read().decode("utf-8").split(">")
    for i, chunk in enumerate(chunks):
        if i == 0:
            continue
        fields = chunk.split()
        if not fields:
            raise ValueError(f"{path}: record {i - 1} has no id")
        seq_ids.append(fields[0])
        seqs.append("".join(fields[1:]))
    return _align_rows(seqs, path), seq_ids


def read_align_stockholm(path):
    """src/utils.rs:719-744: empty lines and lines that start with '#' (the header, #=GF, #=GC, ...)
    are skipped, reading stops at the first line that starts with '//'; every other line is
    `id sequence`, one row each (no interleaved blocks) -> (rows, seq_ids)."""
    seqs, seq_ids = [], []
    for i, line in enumerate(_align_lines(path)):
        if line == "" or line.startswith("#"):
            continue
        if line.startswith("//"):
            break
        fields = line.split()
        if len(fields) < 2:
            raise ValueError(f"{path}: line {i + 1}: expected `id sequence`")
        seq_ids.append(fields[0])
        seqs.append(fields[1])
    return _align_rows(seqs, path), seq_ids


_ALIGN_READERS = {".aln": read_align_clustal, ".fa": read_align_fasta, ".fasta": read_align_fasta,
                  ".sto": read_align_stockholm, ".stk": read_align_stockholm}


def read_align(path):
    """The reader of the file's extension: .aln Clustal, .fa / .fasta FASTA, .sto / .stk Stockholm
    -> (rows, seq_ids)."""
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if ext not in _ALIGN_READERS:
        raise ValueError(f"{path}: unknown alignment format (known: {' '.join(sorted(_ALIGN_READERS))})")
    return _ALIGN_READERS[ext](path)


class FoldScoreSets:
    """`FoldScoreSets::new(init_val)` then `.transfer()` as every reference caller
    does (tests/tests.rs:21-22, src/bin/mccaskill_algo.rs:59-60)."""

    def __init__(self, init_val=0.0, _buf=None):
        L = _lib.lib()
        self._buf = _buf if _buf is not None else np.zeros(L.rnamc_params_sizeof(), dtype=np.uint8)
        if _buf is None:
            _lib.check(L.rnamc_params_new(C.c_float(init_val), self._buf.ctypes.data))
        self._fields = {}
        name, off, cnt = C.c_char_p(), C.c_uint64(), C.c_uint64()
        idx = 0
        while L.rnamc_params_field(idx, C.byref(name), C.byref(off), C.byref(cnt)) == _lib.OK:
            self._fields[name.value.decode()] = (off.value, cnt.value)
            idx += 1

    # -- constructors ------------------------------------------------------
    @classmethod
    def new(cls, init_val=0.0):
        return cls(init_val)

    @classmethod
    def synthetic(cls, seed=0):
        """Seeded synthetic tables for both models (the real ones live in the
        absent rna-ss-params crate)."""
        L = _lib.lib()
        buf = np.zeros(L.rnamc_params_sizeof(), dtype=np.uint8)
        _lib.check(L.rnamc_params_synthetic(C.c_uint64(seed), buf.ctypes.data))
        return cls(_buf=buf)

    @classmethod
    def load(cls, path):
        L = _lib.lib()
        buf = np.zeros(L.rnamc_params_sizeof(), dtype=np.uint8)
        _lib.check(L.rnamc_params_load(os.fsencode(path), buf.ctypes.data))
        return cls(_buf=buf)

    def save(self, path):
        _lib.check(_lib.lib().rnamc_params_save(self.ptr, os.fsencode(path)))

    # -- reference methods -------------------------------------------------
    def accumulate(self):
        off, _ = self._fields["contra.hairpin_scores_len"]
        _lib.check(_lib.lib().rnamc_fold_score_sets_accumulate(self._buf.ctypes.data + off))

    def transfer(self, source=None):
        """Copy the compiled tables (of `source`, default: the table set named by
        $RNAMC_TABLES / set_default_tables(); raises NoTablesError when neither is given) the
        way the reference's transfer() copies the crate constants; Turner constants are taken
        over as they are."""
        src = source if source is not None else default_tables()
        off, _ = self._fields["contra.hairpin_scores_len"]
        # Turner block and header come over wholesale; the contra block goes through
        # the canonical-pair mask of transfer().
        mine = self._buf[off:].copy()
        self._buf[:] = src._buf
        self._buf[off:] = mine
        _lib.check(_lib.lib().rnamc_fold_score_sets_transfer(
            self._buf.ctypes.data + off, src._buf.ctypes.data + off))

    # -- plumbing ------------------------------------------------------------
    @property
    def ptr(self):
        return self._buf.ctypes.data

    def content_key(self):
        """Digest of the whole parameter block: host mirrors re-upload the tables of a
        cached device context when this changes (the set is mutable, the reference reads it
        on every call)."""
        import hashlib
        return hashlib.blake2b(self._buf.tobytes(), digest_size=16).digest()

    @property
    def is_synthetic(self):
        """table_id of the header: rnamc_params_synthetic tags it "SYNT" ^ seed."""
        return (int(self._buf[8:16].view(np.uint64)[0]) >> 32) == 0x53594E54

    def field(self, qualified):
        off, cnt = self._fields[qualified]
        arr = self._buf[off:off + 4 * cnt].view(np.float32)
        short = qualified.split(".", 1)[1]
        if qualified.startswith("turner.") and short in _TURNER_SHAPES:
            return arr.reshape(_TURNER_SHAPES[short])
        if short in _SHAPES:
            return arr.reshape(_SHAPES[short])
        return arr

    def __getattr__(self, item):
        fields = self.__dict__.get("_fields", {})
        if "contra." + item in fields:
            v = self.field("contra." + item)
            return v if v.shape[0] > 1 or v.ndim > 1 else v
        raise AttributeError(item)

    def turner(self, item):
        return self.field("turner." + item)


_default = None


class NoTablesError(RuntimeError):
    pass


def set_default_tables(tables):
    """Name the table set `transfer()` draws from (a FoldScoreSets holding the "compiled"
    constants): FoldScoreSets.load(path) of a real dump, or — explicitly — a synthetic set."""
    global _default
    _default = tables


def default_tables():
    """The compiled constants `transfer()` copies.  In the reference they come from the
    rna-ss-params crate, which this tree does not hold: a table file dumped from that crate
    (bindings/rust/dump_tables.rs) must be named by $RNAMC_TABLES, or a set installed with
    set_default_tables().  There is NO silent synthetic fallback: results computed from
    made-up tables must never look like the reference's."""
    global _default
    if _default is None:
        path = os.environ.get("RNAMC_TABLES")
        if not path:
            raise NoTablesError(
                "no scoring tables configured: set $RNAMC_TABLES to a table file dumped from the "
                "rna-ss-params crate (bindings/rust/dump_tables.rs), or choose synthetic tables "
                "explicitly (utils.set_default_tables(FoldScoreSets.synthetic(seed)); the CLIs "
                "take --synthetic-tables SEED)")
        _default = FoldScoreSets.load(path)
    return _default
