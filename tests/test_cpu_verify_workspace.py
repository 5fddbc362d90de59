"""The workspace queries of the chunked and planned verification scores (neighbourhood, exceedance, object, energy, variogram)
return, over the shape and cap table of tests/util_verify_runs.py, the sizes recorded in tests/golden/verify_parent.npz from the
commit before the two chunk planners became one (csrc/verify_common.h, plan_chunks).  Host arithmetic: no device needed."""
import util_verify_runs as U


def test_workspace_sizes_are_the_parents():
    want, _ = U.load_fixture()
    got = U.workspace_sizes()
    assert set(got) == {k for k in want if k.startswith("ws/")} and len(got) > 100
    assert {k: int(v) for k, v in got.items()} == {k: int(want[k]) for k in got}
    assert any(int(v) == 0 for v in got.values()) and sum(int(v) > 0 for v in got.values()) > 100
