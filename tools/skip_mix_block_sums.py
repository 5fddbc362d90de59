#!/usr/bin/env python3
"""Per-step sums of the launches the skip-in-the-mix route touches, from two rocprofv3 --kernel-trace CSVs of bench.py (parent, change):
mean and standard deviation over 9 consecutive steps from the middle of each trace of conv1 + pack_input + final_mix, of final_gather
alone, and of the step's wall time and kernel count.  "won": the mean dropped by more than three times the larger standard deviation.
    python tools/skip_mix_block_sums.py PARENT_kernel_trace.csv CHANGE_kernel_trace.csv [label]"""
import csv
import statistics
import sys

GROUPS = {"conv1 + pack_input + final_mix": ("conv_igemm_kernel<8, 8, 2, 3", "pack_input_kernel", "final_mix_kernel"),
          "final_gather": ("final_gather_kernel",)}
N_STEPS = 9


def steps_of(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "em_update_kernel" in r["Kernel_Name"]]
    k = max(0, len(ends) // 2 - N_STEPS // 2)
    return [rows[ends[j] + 1: ends[j + 1] + 1] for j in range(k, k + N_STEPS)]


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def figures(steps):
    out = {"wall": [(int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e3 for s in steps], "kernels": [len(s) for s in steps]}
    for name, pats in GROUPS.items():
        out[name] = [sum(us(r) for r in s if any(p in r["Kernel_Name"] for p in pats)) for s in steps]
        out[name + " launches"] = [sum(1 for r in s if any(p in r["Kernel_Name"] for p in pats)) for s in steps]
    return out


def main():
    parent, change = figures(steps_of(sys.argv[1])), figures(steps_of(sys.argv[2]))
    print(f"== {sys.argv[3] if len(sys.argv) > 3 else ''}")
    for tag, f in (("parent", parent), ("change", change)):
        print(f"   {tag} {N_STEPS} steps of {f['kernels'][0]} kernels: wall mean {statistics.mean(f['wall']):.1f} us sd {statistics.stdev(f['wall']):.1f}")
    for name in list(GROUPS) + ["wall"]:
        pm, cm = statistics.mean(parent[name]), statistics.mean(change[name])
        ps, cs = statistics.stdev(parent[name]), statistics.stdev(change[name])
        n = f" (x{parent[name + ' launches'][0]} -> x{change[name + ' launches'][0]})" if name in GROUPS else ""
        verdict = "won" if pm - cm > 3 * max(ps, cs) else "not won"
        print(f"  {name + n:52s} {pm:8.2f} us (sd {ps:.2f})  ->  {cm:8.2f} us (sd {cs:.2f})   gain {pm - cm:6.2f} us, "
              f"3 x larger sd = {3 * max(ps, cs):.2f}: {verdict}")


if __name__ == "__main__":
    main()
