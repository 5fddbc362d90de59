"""Record tests/golden/wgrad_plans_parent.json: what the weight-gradient planner and the flush of the sbgm_danra_amd package on the path
decide, for test_cpu_wgrad_plan.py and test_gpu_conv_wgrad.py to hold later commits to.  Run it against a build of the commit whose
decisions are the reference (that checkout first on PYTHONPATH; its hash goes into the file):

    python tools/record_wgrad_plans.py plans COMMIT     no device: sbgm_conv2d_wgrad_plan of every geometry the tests and bench_wgrad.py use
    python tools/record_wgrad_plans.py flush COMMIT     on the GPU, after `plans`: sbgm_wgrad_flush_plan of the named queues of test_gpu_conv_wgrad.py
"""
import json
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path += [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]
OUT = ROOT / "tests" / "golden" / "wgrad_plans_parent.json"


def record_plans():
    import bench_wgrad
    import conv_wgrad_ref as R
    import test_cpu_wgrad_plan as T
    rows = []

    def add(source, geom, no_lds=False):
        if no_lds:
            os.environ["SBGM_NO_LDS_WGRAD"] = "1"
        rows.append(dict(source=source, geom=list(R.full(geom)), no_lds=no_lds, plan=T.raw_plan(geom)))
        os.environ.pop("SBGM_NO_LDS_WGRAD", None)

    for g, _, _ in R.CASES:
        add("CASES", g)
    for g, _ in R.ONE_HOT_CASES:
        add("ONE_HOT_CASES", g)
    for g in R.REFUSED:
        add("REFUSED", g)
    for g in R.GENERAL4_CASES:
        add("GENERAL4_CASES", g)
        add("GENERAL4_CASES", g, no_lds=True)
    for name in ("CFGS", "GENERAL_CFGS"):
        for B, H, Cin, Cout, k, s in (tuple(c) + (3, 1)[len(c) - 4:] for c in getattr(bench_wgrad, name)):
            add(f"bench_wgrad.{name}", (B, Cin, H, H, Cout, k, s, k // 2 if k != 8 else 3))
    return rows


def record_flush():
    import test_gpu_conv_wgrad as T
    flush = {}
    T.check_against_parent = lambda name, rows, passes, launches: flush.__setitem__(name, T.flush_record(rows, passes, launches))
    for name in sorted(vars(T)):
        if name.startswith("test_flush_splits_") or name.endswith("_ride_in_two_launches"):
            getattr(T, name)()
    return flush


if __name__ == "__main__":
    what, commit = sys.argv[1:]
    doc = json.loads(OUT.read_text()) if OUT.exists() else {}
    assert doc.get("parent", commit) == commit, "both halves come from one commit"
    doc["parent"] = commit
    doc[what] = {"plans": record_plans, "flush": record_flush}[what]()
    one = json.dumps                                            # one plan row / one queue per line
    OUT.write_text('{"parent": %s,\n"plans": [\n%s\n],\n"flush": {\n%s\n}}\n' % (
        one(commit), ",\n".join(one(r) for r in doc.get("plans", [])), ",\n".join(f"{one(k)}: {one(v)}" for k, v in doc.get("flush", {}).items())))
    from sbgm_danra_amd import _native
    print(f"{what}: {len(doc[what])} entries from {_native.LIB_PATH} -> {OUT}")
