#!/usr/bin/env python3
"""What every ``compute_*`` entry point of ``tests/score_pass_cases.py`` returns, recorded on an MI355X at the commit BEFORE
``hipvae/inference.py`` took over the encode loops and the image draw of the evaluation modules.  Needs the built library
and a GPU.

Writes ``score_pass_bits.npz``: one array per returned value (scores, features, per-image vectors, the ``indices`` used),
keyed ``<call>.<dataset|table>.<field>``.  Every call runs twice and must repeat its own bytes, so that what
tests/test_hip_score_pass_bits.py compares afterwards is the code and not the order of an atomic.  The counts in
``score_pass_cases.py`` are the smallest the code at that commit accepted (it refuses a covariance of too few rows and
a classifier that does not converge).  The file holds data only.

    python tests/golden/make_golden_score_pass.py [--out FILE]
"""
import argparse
import os
import sys
import time
import traceback

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "intro-tc-vae_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import score_pass_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "score_pass_bits.npz"))
    a = ap.parse_args()
    ctx = C.Context()
    out, failed = {}, []
    for name in C.NAMES:
        for kind in C.SOURCES:
            t0 = time.time()
            try:
                first, second = C.run(ctx, name, kind), C.run(ctx, name, kind)
            except Exception:  # noqa: BLE001  report every call that the code refuses, then fail
                traceback.print_exc()
                failed.append((name, kind, "raised"))
                continue
            unstable = [k for k in first if not C.same_bytes(first[k], second[k])]
            if unstable or set(first) != set(second):
                failed.append((name, kind, unstable))
            out.update(first)
            print(f"{name}.{kind}: {len(first)} arrays, {(time.time() - t0) / 2:.2f} s per call", flush=True)
    for name in C.NAMES:                # a table serves the images a dataset serves: the two kinds agree
        d = {k.split(".", 2)[2]: v for k, v in out.items() if k.startswith(f"{name}.dataset.")}
        t = {k.split(".", 2)[2]: v for k, v in out.items() if k.startswith(f"{name}.table.")}
        print(name, "dataset == table:", set(d) == set(t) and all(C.same_bytes(d[k], t[k]) for k in d))
    if failed:
        print("FAILED:", failed)
        sys.exit(1)
    np.savez_compressed(a.out, **out)
    print(len(out), "arrays,", os.path.getsize(a.out), "bytes ->", a.out)


if __name__ == "__main__":
    main()
