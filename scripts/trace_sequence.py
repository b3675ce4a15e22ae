"""Ordered kernel sequence of the LAST step in a rocprofv3 kernel trace (csv), with per-kernel duration: a reading aid for
launch-count work.  usage: trace_sequence.py [--launches] <p_kernel_trace.csv> <marker-kernel-substring>   (a step ends
after the last launch whose name contains the marker, e.g. adamw)

--launches: name, grid and workgroup size only, no times -- two trees that enqueue the same work give listings that
`diff` finds equal."""
import csv
import sys


def _dims(r, what):
    return "x".join(r[f"{what}_Size_{a}"] for a in "XYZ") if f"{what}_Size_X" in r else r.get(f"{what}_Size", "?")


def main():
    argv = [a for a in sys.argv[1:] if a != "--launches"]
    launches_only = len(argv) != len(sys.argv) - 1
    rows = sorted(csv.DictReader(open(argv[0])), key=lambda r: int(r["Start_Timestamp"]))
    marker = argv[1] if len(argv) > 1 else "adamw"
    ends = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
    if len(ends) < 2:
        raise SystemExit("fewer than two steps in the trace")
    lo, hi = ends[-2] + 1, ends[-1] + 1
    t0 = int(rows[lo]["Start_Timestamp"])
    prev_end = t0
    for r in rows[lo:hi]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        name = r["Kernel_Name"].replace("clipfs::", "").replace("void ", "")
        if launches_only:
            print(f"{name}  grid {_dims(r, 'Grid')}  wg {_dims(r, 'Workgroup')}")
            continue
        print(f"{(s - t0) / 1e3:9.1f} us  +{(e - s) / 1e3:7.1f}  gap {(s - prev_end) / 1e3:6.1f}  q{r.get('Queue_Id', '?'):>2s}  {name[:90]}")
        prev_end = max(prev_end, e)
    if launches_only:
        print(f"{hi - lo} launches")
    else:
        print(f"{hi - lo} launches, span {(int(rows[hi - 1]['End_Timestamp']) - t0) / 1e3:.1f} us")


if __name__ == "__main__":
    main()
