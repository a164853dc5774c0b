"""Generates tests/golden/duplex_slots_f64.npz: the f64 reference (tests/duplex_ref.py: Scores and
Recurrences over the CPU oracle's loop scores, seeded synthetic tables) of every record of
tests/duplex_slots.py under both models -- the probabilities of the twelve designed pairs, ln Z, the
optimum, the designed duplex's share exp(w - ln Z) and the largest partial value of the max-plus
chain -- and the (a, b, flanks) of the records it belongs to.  About a minute.  Usage:
    python tests/make_duplex_slots_golden.py
test_duplex_slots_cpu.py evaluates every tenth record again and compares to 1e-12."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import duplex_slots as S  # noqa: E402


def main():
    recs = S.records()
    out = {"keys": S.keys()}
    for contra, model in S.MODELS.items():
        t0 = time.time()
        refs = S.pmap(lambda r: S.Ref(r, *S.evaluate(r, contra)), recs)
        for f in S.FIELDS:
            out[f"{f}_{model}"] = np.array([getattr(x, f) for x in refs], dtype=np.float64)
        print(f"{model}: {len(recs)} records in {time.time() - t0:.1f} s, designed P >= "
              f"{out[f'designed_{model}'].min():.4f}, share >= {out[f'share_{model}'].min():.4f}")
    np.savez(S.GOLDEN, **out)
    print(f"{S.GOLDEN}: {os.path.getsize(S.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
