"""The engine gives, bit for bit, what the commit before csrc/engine.hip was split into model.hip, forward.hip and sampler_run.hip
gave: plain and measured evaluations, every step sampler kind with its options (graph replay and eager, guided, held, joint, labels,
churn, eta), the RK45 driver with its integer statistics, the kernel names of the measured evaluation and the workspace size after
every case, on the cases of tests/util_engine_runs.py, against tests/golden/engine_parent.npz (written by
`python tests/util_engine_runs.py ROOT OUT COMMIT` from a build of that commit, which ran every case twice in separate interpreters and
found no key whose two runs differed).  NaNs and the sign of zero are compared by bit pattern."""
import pytest

import util_engine_runs as U

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
    assert set(want) == set(computed)
    assert {sp["name"] for sp in U.SPECS} | {sp["name"] + "/ws" for sp in U.SPECS} <= set(want)


def test_every_output_is_bit_equal_to_the_parent(recorded, computed):
    want, _ = recorded
    differing = [k for k, v in computed.items() if not U.same_bits(want[k], v)]
    for k in differing[:5]:
        print(f"{k}:\n  parent {want[k]!r}\n  now    {computed[k]!r}")
    assert differing == []
