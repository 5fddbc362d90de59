"""Time rows of an EM / PC run: the nine time-bias vectors of all N steps are computed once per run and the step's
advance publishes the next row, instead of a time-embedding and a time-projection launch in every evaluation.  The rows come from the
same two kernels at the same fp32 times, so every run must equal the run with SBGM_NO_TIME_ROWS=1 bit for bit; the switch is read once
per process, so both sides run in fresh interpreters (tests/util_step_runs.py), one child each for all the runs below."""
import numpy as np
import pytest

from util_step_runs import run_specs

pytestmark = pytest.mark.gpu

SWITCHED = [
    dict(name="em_n5", kind="em", B=2, N=5),
    dict(name="em_n2", kind="em", B=2, N=2),                       # the last (second) step clamps its row index
    dict(name="pc_n3", kind="pc", B=2, N=3),                       # the corrector's advance must leave the rows alone
    dict(name="em_guided", kind="em", B=2, N=3, guided=True),      # 2B rows are broadcast
    dict(name="em_held", kind="em", B=2, N=3, held=True),
    dict(name="em_b9", kind="em", B=9, N=3),                       # more than one group of 8 samples in the per-step projection
    dict(name="em_labels", kind="em", B=2, N=3, classes=4, labels=True),   # labels: the route is off, both sides take today's path
]
ONE_HANDLE = [                                                     # after em_n5 (N = 5) on the cached model's handle
    dict(name="h_n7", kind="em", B=2, N=7),
    dict(name="h_n7_eps", kind="em", B=2, N=7, eps=5e-3),
    dict(name="f_n5", kind="em", B=2, N=5, fresh=True),
    dict(name="f_n7", kind="em", B=2, N=7, fresh=True),
    dict(name="f_n7_eps", kind="em", B=2, N=7, eps=5e-3, fresh=True),
    dict(name="em_n5_eager", kind="em", B=2, N=5, graph=False),
]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_rows")
    return {"rows": run_specs(SWITCHED + ONE_HANDLE, {}, d / "rows.npz"),
            "parent": run_specs(SWITCHED, {"SBGM_NO_TIME_ROWS": "1"}, d / "parent.npz")}


@pytest.mark.parametrize("name", [s["name"] for s in SWITCHED])
def test_run_equals_the_per_step_launches(runs, name):
    got, want = runs["rows"][name], runs["parent"][name]
    assert np.isfinite(got).all() and got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: max |diff| {np.abs(got - want).max():.3e}"


def test_graph_replay_equals_eager(runs):
    assert np.array_equal(runs["rows"]["em_n5"], runs["rows"]["em_n5_eager"])


@pytest.mark.parametrize("reused,fresh", [("em_n5", "f_n5"), ("h_n7", "f_n7"), ("h_n7_eps", "f_n7_eps")])
def test_calls_on_one_handle_equal_a_fresh_handle(runs, reused, fresh):
    """N = 5, then N = 7, then N = 7 with another eps on one handle: the rows are recomputed on every call"""
    assert np.array_equal(runs["rows"][reused], runs["rows"][fresh])
    assert not np.array_equal(runs["rows"]["h_n7"], runs["rows"]["h_n7_eps"])
