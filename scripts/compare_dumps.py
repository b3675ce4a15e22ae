"""Compare two `bench.py --dump-outputs` directories array by array: bitwise equality, max |a - b| and max |a|.
usage: compare_dumps.py <dir_a> <dir_b> [out.json]   (the `dump_first_step_vs_parent.json` files under profiles/)"""
import json
import os
import sys

import numpy as np


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(b_dir) if f.endswith(".npy")), "the two dumps hold different arrays"
    doc = {}
    for n in names:
        a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
        assert a.shape == b.shape and a.dtype == b.dtype, n
        doc[n] = dict(bitwise=bool(a.tobytes() == b.tobytes()),
                      max_abs_diff=float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0,
                      max_abs=float(np.max(np.abs(a))) if a.size else 0.0)
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
