"""GEMM and attention kernel time of a rocprofv3 kernel trace (csv), grouped by kernel and launch grid (work-items): the
`text_gemm_attention_by_grid_*.txt` listings under profiles/.  usage: kernel_time_by_grid.py <..._kernel_trace.csv>"""
import csv
import re
import sys
from collections import defaultdict


def main():
    by = defaultdict(lambda: [0, 0.0])
    totals = defaultdict(float)
    for r in csv.DictReader(open(sys.argv[1])):
        name = re.sub(r"\(.*", "", r["Kernel_Name"])
        if "gemm_nt" not in name and "attention16" not in name:
            continue
        grid = int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by[(name, grid)][0] += 1
        by[(name, grid)][1] += us
        totals[name] += us
    for (name, grid), (n, us) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print(f"{name:60s} grid={grid:8d} launches={n:5d} total_us={us:10.1f}")
    print("TOTALS:", {k: round(v, 1) for k, v in totals.items()})


if __name__ == "__main__":
    main()
