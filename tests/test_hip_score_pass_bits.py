"""The evaluation passes compute the bytes they computed before ``hipvae/inference.py`` took over their encode loops and
their image draw: every ``compute_*`` entry point of ``score_pass_cases``, once on a dataset and once on a
``DeviceImageTable``, against tests/golden/score_pass_bits.npz, recorded on an MI355X at the commit before.  No tolerance:
the change moves no arithmetic.  ``score_pass_cases.run`` also requires the model's training flag and buffers back as
found."""
import os

import numpy as np
import pytest

import score_pass_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with np.load(os.path.join(golden_dir, "score_pass_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def context():
    return C.Context()


def test_every_call_is_recorded(recorded):
    assert {k.split(".")[0] for k in recorded} == set(C.NAMES)
    assert {k.split(".")[1] for k in recorded} == set(C.SOURCES)
    for name in ("log_likelihood.{}.per_image.indices", "sample_quality_normal.{}.indices", "sample_quality_gmm.{}.indices",
                 "reconstruction_drawn.{}.indices", "reconstruction_all.{}.indices", "latent_density.{}.indices.fit"):
        assert all(name.format(kind) in recorded for kind in C.SOURCES)
    # both arms of the draw: a sorted subset, and everything
    assert len(recorded["reconstruction_drawn.dataset.indices"]) == 50
    assert np.array_equal(recorded["reconstruction_all.dataset.indices"], np.arange(C.N_IMAGES))


@pytest.mark.parametrize("kind", C.SOURCES)
@pytest.mark.parametrize("name", C.NAMES)
def test_same_bytes_as_recorded(recorded, context, name, kind):
    got = C.run(context, name, kind)
    want = {k: v for k, v in recorded.items() if k.startswith(f"{name}.{kind}.") or k == f"{name}.{kind}"}
    assert want and sorted(got) == sorted(want)
    for k in sorted(want):
        assert C.same_bytes(got[k], want[k]), k
