"""Compare two `bench.py --dump-outputs` directories bit for bit: python tools/compare_dumps.py DIR_A DIR_B (exit 1 on a difference)."""
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")), (names, os.listdir(b))
same = {n: bool(np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))) for n in names}
for n in names:
    print(f"{n}: {np.load(os.path.join(a, n)).shape} {'equal' if same[n] else 'DIFFERENT'}")
sys.exit(0 if all(same.values()) else 1)
