"""``VAESolver.write_disentanglemnt_scores`` over the score table (solvers/scores.py) calls what the writer of copied blocks
called: every case of ``score_writer_cases`` is replayed on the CPU with stubbed ``compute_*`` functions and must give the
log recorded before the change (tests/golden/score_writer_calls.json), entry for entry: which function, on the dataset
or the device table, with which keyword arguments and with the model in which mode, then which tag, keys, values and step
reach the writer, in order."""
import json
import os

import pytest

import score_writer_cases as C

CASES = {c["name"]: c for c in C.cases()}


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "score_writer_calls.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert len(recorded["everything at once"]) == 28 + 1              # 14 scores computed and written, then the flag


@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_log_is_the_recorded_one(recorded, name):
    got, want = C.run_case(CASES[name]), recorded[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"entry {i}"
    assert len(got) == len(want)


def test_the_table_is_the_only_list_of_names():
    from solvers import scores
    assert tuple(scores.TABLE) == C.FACTOR + C.NON_FACTOR
    assert tuple(n for n, s in scores.TABLE.items() if s.factors) == C.FACTOR
    assert {n: s.params for n, s in scores.TABLE.items()} == C.PARAMS_OF
    assert scores.KNOWN == C.ALL_EXTRAS                     # the unknown-name message keeps the order it had
    assert list(scores.DEVICE) == ["bvae_score", "mig_score", "mod_expl", "dci"]
    assert scores.DEVICE["dci"].params == "dci_params"


@pytest.mark.parametrize("failing", ["disentangle.compute_sap_score", "disentangle.compute_mod_expl_score",
                                     "disentangle.compute_scores"])
def test_a_score_that_raises_leaves_the_training_flag_as_found(failing):
    """The one intended change of behaviour: the factor block's eval bracket is ``inference.eval_mode``, so an exception
    inside it puts the flag back.  Before, the model stayed in eval mode."""
    c = C.case("raises", factored=True, extras=("sap", "irs"), raises=failing,
               device_scores=True if failing.endswith("compute_scores") else "all")
    log = C.run_case(c)
    assert log[-2] == ["raised", "RuntimeError", f"{failing} failed"]
    assert [e for e in log if e[0] == "compute"][-1][1] == failing      # nothing was computed after it
    assert [e[-1] for e in log if e[0] == "compute"] == [False] * sum(e[0] == "compute" for e in log)   # all in eval mode
    assert log[-1] == ["training", True]
