"""The verification kernels and the quantile path of the post-processing kernels give, bit for bit, what the commit before
their helpers were gathered into csrc/verify_common.h gave: every output of every public function of verification.py, and of
special_transforms.sample_extremes, on the cases of tests/util_verify_runs.py, against tests/golden/verify_parent.npz (written
by `python tests/util_verify_runs.py ROOT OUT COMMIT` from a build of that commit, which ran every case twice and found no key
whose two runs differed).  NaNs and the sign of zero are compared by bit pattern."""
import pytest

import util_verify_runs as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return U.load_fixture()


@pytest.fixture(scope="module")
def computed():
    return U.run_all()


def test_fixture_is_complete(recorded, computed):
    want, meta = recorded
    assert meta["commit"] and meta["unstable_keys"] == []
    assert {k for k in want if not k.startswith("ws/")} == set(computed)


def test_every_output_is_bit_equal_to_the_parent(recorded, computed):
    want, _ = recorded
    differing = [k for k, v in computed.items() if not U.same_bits(want[k], v)]
    for k in differing[:5]:
        print(f"{k}:\n  parent {want[k]!r}\n  now    {computed[k]!r}")
    assert differing == []
