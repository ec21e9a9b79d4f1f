#!/usr/bin/env python3
"""The call log of ``VAESolver.write_disentanglemnt_scores`` for every case of ``tests/score_writer_cases.py``, recorded at
the commit BEFORE the score table (solvers/scores.py) replaced the writer's copied blocks.  Needs the built library and
no GPU: every ``compute_*`` is stubbed.

Writes ``score_writer_calls.json``: ``{case name: log}``, a log being the ``compute`` / ``metrics`` / ``add_scalar`` /
``add_scalars`` / ``raised`` entries in order and the model's training flag afterwards.  tests/test_score_writer_host.py
replays the cases and requires the same logs.  The file holds data only.

    python tests/golden/make_golden_score_writer.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "intro-tc-vae_amd")):
    sys.path.insert(0, p)

import score_writer_cases as C  # noqa: E402


def main():
    out = {c["name"]: C.run_case(c) for c in C.cases()}
    with open(os.path.join(HERE, "score_writer_calls.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "cases,", sum(map(len, out.values())), "entries")


if __name__ == "__main__":
    main()
