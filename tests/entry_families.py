"""Every entry family of a context as (name, honours summation_mode 1, call(context, shape)), shared by the
tests that run all of them on ONE context and compare with fresh contexts (test_gpu_growth.py: buffer sizes;
test_gpu_tables.py: replaced tables).  A shape is (records, bases per record)."""
import numpy as np


def records(shape):
    from rna_algos_amd.workloads import synthetic_seq
    count, n = shape
    return [synthetic_seq(n, seed=1700 + 31 * n + k) for k in range(count)]


def freeze(x):
    """a result of any entry as nested tuples of bytes"""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (np.floating, float)):
        return np.float64(x).tobytes()
    if isinstance(x, (np.integer, int, str, bytes, type(None))):
        return x
    if isinstance(x, dict):
        return tuple((k, freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(freeze(v) for v in x)
    return freeze({k: v for k, v in vars(x).items() if not k.startswith("_")})


def durbin(ctx, shape):
    from rna_algos_amd.durbin_algo import AlignScores, durbin_algo_batch, with_pseudo_bases
    count, _ = shape
    scores = AlignScores.new(0.0)
    scores.transfer()
    seqs = [with_pseudo_bases(r) for r in records(shape)]
    return durbin_algo_batch(seqs, [(k, (k + 1) % count) for k in range(count)], scores, ctx)


def families(contra=False, short=False):
    """the families that take host arrays, under one model"""
    # a sequence whose windows / mutants are `count` records of n bases
    def windowed(ctx, shape):
        count, n = shape
        return ctx.bpp_windowed(records((1, n + count - 1))[0], n, contra, short, stride=1)

    def mutants(ctx, shape):
        count, n = shape
        return ctx.mutant_scan(records((1, n))[0], contra, short, positions=list(range(0, n, 3 * n // count)))

    return [
        ("bpp_batch", True, lambda c, s: c.bpp_batch(records(s), contra, short)),
        ("log_partition_batch", False, lambda c, s: c.log_partition_batch(records(s), contra, short)),
        ("sample_batch", False, lambda c, s: c.sample_batch(records(s), 4, contra, short, seed=7)),
        ("mfe_batch", False, lambda c, s: c.mfe_batch(records(s), contra, short)),
        ("centroid_fold_batch", True, lambda c, s: c.centroid_fold_batch(records(s), [0.5, 2.0, 8.0], contra, short)),
        ("bpp_batch_sparse", True, lambda c, s: c.bpp_batch_sparse(records(s), contra, short, 0.01)),
        ("bpp_windowed", True, windowed),
        ("mutant_scan", True, mutants),
        ("durbin_batch", False, durbin),
    ]


FAMILIES = families()


def table_families(contra=False, short=False):
    """`families` without the one that reads no folding table (durbin_batch), with the two single-sequence
    entries that score on the host (fold_sums: reference order only) and the device-resident entry"""
    def device_resident(ctx, shape):
        import torch
        seqs = records(shape)
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offsets[1:])
        out_offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens * (lens + np.uint64(1)) // np.uint64(2), out=out_offsets[1:])
        dev = torch.device("cuda:0")
        d_bases = torch.from_numpy(np.concatenate(seqs)).to(dev)
        d_out = torch.full((int(out_offsets[-1]),), 7.0, dtype=torch.float32, device=dev)
        d_logz = torch.zeros(len(seqs), dtype=torch.float32, device=dev)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.bpp_batch_device(len(seqs), d_bases.data_ptr(), offsets, contra, short, d_out.data_ptr(),
                                 out_offsets, d_logz.data_ptr(), side.cuda_stream)
        side.synchronize()
        return d_out.cpu().numpy(), d_logz.cpu().numpy()

    return [f for f in families(contra, short) if f[0] != "durbin_batch"] + [
        ("fold_sums", False, lambda c, s: c.fold_sums(records(s)[0], contra, short).dense),
        ("fold_scores_packed", False, lambda c, s: c.fold_scores_packed(records(s)[0], contra, short)),
        ("bpp_batch_device", True, device_resident),
    ]
