"""The engine's routes on the smallest network input (32 x 32, `build_pair` weights, batch 2), as specs for util_step_runs.run_specs:
plain and measured evaluations, the step samplers of every kind with their options, the RK45 driver, and the workspace size after every
case.  The engine promises the same launches in the same order whoever owns the code, so a refactor of csrc/model.hip, forward.hip or
sampler_run.hip must leave every array unchanged: tests/golden/engine_parent.npz holds them as the commit before the engine file was
split computed them, and tests/test_gpu_engine_parent.py compares bit for bit.

`python tests/util_engine_runs.py ROOT OUT [COMMIT]` writes that fixture from the package under ROOT: it runs the list twice, in two
fresh interpreters, and records only the keys whose two runs agree bit for bit (any other is printed with both values and listed under
`unstable_keys`), and COMMIT under `commit`."""
import os
import sys
import tempfile

import numpy as np

import util_step_runs
from util_verify_runs import _pack, load_fixture as _load, same_bits  # noqa: F401

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_parent.npz")
LABELS = dict(classes=4, labels=True)


def _specs():
    s = [
        dict(name="forward", kind="forward", N=0),
        dict(name="forward_no_cond", kind="forward", N=0, n_cond=0),
        dict(name="forward_labels", kind="forward", N=0, **LABELS),
        dict(name="measured", kind="measured", N=0),
        dict(name="em_graph", kind="em", N=4),
        dict(name="em_graph_again", kind="em", N=4),                 # the cached step graph is reused
        dict(name="em_eager", kind="em", N=4, graph=False),
        dict(name="pc_graph", kind="pc", N=4),
        dict(name="pc_eager", kind="pc", N=4, graph=False),
        dict(name="em_guided", kind="em", N=4, guided=True),
        dict(name="em_held", kind="em", N=4, held=True),
        dict(name="em_joint", kind="em", N=4, joint=True),
        dict(name="em_labels", kind="em", N=4, **LABELS),            # labels: no time rows
        dict(name="edm", kind="edm", N=4),
        dict(name="edm_churn", kind="edm", N=4, s_churn=8.0),
        dict(name="edm_held", kind="edm", N=4, held=True),
        dict(name="dpm", kind="dpm", N=4),
        dict(name="dpm_sde", kind="dpm", N=4, eta=1.0),
        dict(name="dpm_joint", kind="dpm", N=4, joint=True),
        dict(name="rk45", kind="rk45", N=0, rtol=1e-2),
        dict(name="forward_after", kind="forward", N=0),             # the routes of the runs are ended
        dict(name="forward_labels_after", kind="forward", N=0, **LABELS),
    ]
    return [dict(sp, B=2, ws=True) for sp in s]


SPECS = _specs()


def run_all(path=None):
    """{key: numpy array} of every case, from one fresh interpreter"""
    with tempfile.TemporaryDirectory() as d:
        return util_step_runs.run_specs(SPECS, {}, path or os.path.join(d, "engine.npz"))


def load_fixture(path=FIXTURE):
    return _load(path)


def _record(out_path, commit):
    first, second = run_all(), run_all()
    assert first.keys() == second.keys()
    keep, unstable = {}, []
    for k in first:
        if same_bits(first[k], second[k]):
            keep[k] = first[k]
        else:
            unstable.append(k)
            print(f"UNSTABLE {k}:\n  run 1 {first[k]!r}\n  run 2 {second[k]!r}")
    index, blob = _pack(keep)
    np.savez_compressed(out_path, index=np.array(index), blob=blob, unstable_keys=np.array(unstable, dtype=str), commit=np.array(commit))
    print(f"recorded {len(keep)} keys, {len(unstable)} unstable, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    util_step_runs.ROOT = os.path.abspath(sys.argv[1])               # the children import the package under ROOT
    _record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "")
