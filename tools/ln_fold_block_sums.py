#!/usr/bin/env python3
"""Per-step sums of the launches the LayerNorm fold touches, from two rocprofv3 --kernel-trace CSVs of bench.py (parent, change): mean and
standard deviation over 9 consecutive steps from the middle of each trace of
  parent: every layernorm_kernel launch and the linear launched right after it (in_proj after ln1, ff[0] after ln2);
  change: the folded linears, conv_igemm_kernel with nine template arguments (<1, 1, 1, 0, 1, FCO, FPX, 0, WS>), and any layernorm_kernel left;
of the attention cores as the control (unchanged code), and of the step's wall time and kernel count.  "won": the mean dropped by more
than three times the larger standard deviation.
    python tools/ln_fold_block_sums.py PARENT_kernel_trace.csv CHANGE_kernel_trace.csv [label]"""
import csv
import re
import statistics
import sys

N_STEPS = 9
FOLDED = re.compile(r"conv_igemm_kernel<1, 1, 1, 0, 1, \d, \d, 0, \d>")
GROUP, CONTROL = "LayerNorm + in_proj + ff[0], deep blocks", "mha_core (control)"


def steps_of(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "em_update_kernel" in r["Kernel_Name"]]
    k = max(0, len(ends) // 2 - N_STEPS // 2)
    return [rows[ends[j] + 1: ends[j + 1] + 1] for j in range(k, k + N_STEPS)]


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def touched(step):
    """indices of the launches of the group in one step"""
    idx = set()
    for i, r in enumerate(step):
        if "layernorm_kernel" in r["Kernel_Name"]:
            idx.add(i)
            if i + 1 < len(step) and "conv_igemm_kernel<1, 1, 1, 0" in step[i + 1]["Kernel_Name"]:
                idx.add(i + 1)
        elif FOLDED.search(r["Kernel_Name"]):
            idx.add(i)
    return sorted(idx)


def figures(steps):
    out = {"wall": [(int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e3 for s in steps], "kernels": [len(s) for s in steps]}
    out[GROUP] = [sum(us(s[i]) for i in touched(s)) for s in steps]
    out[GROUP + " launches"] = [len(touched(s)) for s in steps]
    out[CONTROL] = [sum(us(r) for r in s if "mha_core" in r["Kernel_Name"]) for s in steps]
    out[CONTROL + " launches"] = [sum(1 for r in s if "mha_core" in r["Kernel_Name"]) for s in steps]
    out["layernorm launches"] = [sum(1 for r in s if "layernorm_kernel" in r["Kernel_Name"]) for s in steps]
    return out


def main():
    parent, change = figures(steps_of(sys.argv[1])), figures(steps_of(sys.argv[2]))
    print(f"== {sys.argv[3] if len(sys.argv) > 3 else ''}")
    for tag, f in (("parent", parent), ("change", change)):
        print(f"   {tag} {N_STEPS} steps of {f['kernels'][0]} kernels ({f['layernorm launches'][0]} layernorm_kernel launches): "
              f"wall mean {statistics.mean(f['wall']):.1f} us sd {statistics.stdev(f['wall']):.1f}")
    for name in (GROUP, CONTROL, "wall"):
        pm, cm = statistics.mean(parent[name]), statistics.mean(change[name])
        ps, cs = statistics.stdev(parent[name]), statistics.stdev(change[name])
        n = f" (x{parent[name + ' launches'][0]} -> x{change[name + ' launches'][0]})" if name != "wall" else ""
        verdict = "won" if pm - cm > 3 * max(ps, cs) else "not won"
        print(f"  {name + n:58s} {pm:8.2f} us (sd {ps:.2f})  ->  {cm:8.2f} us (sd {cs:.2f})   gain {pm - cm:6.2f} us, "
              f"3 x larger sd = {3 * max(ps, cs):.2f}: {verdict}")
    for tag, f in (("parent", parent), ("change", change)):
        print(f"  {tag}, {N_STEPS} steps: " + " ".join(f"{v:.1f}" for v in f[GROUP]) + "      wall " + " ".join(f"{v:.1f}" for v in f["wall"]))


if __name__ == "__main__":
    main()
