"""Bytewise comparison of two bench.py --dump-outputs directories: python scripts/cmp_dumps.py DIR_A DIR_B
(exit status 1 if any array differs in shape, dtype or bytes)."""
import glob, os, sys
import numpy as np
a, b = sys.argv[1:3]
names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a, "*.npy")))
assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(b, "*.npy"))), (a, b)
bad = 0
for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    bad += not same
    print(f"{a} vs {b}: {n:24s} {str(x.shape):20s} {'bytewise equal' if same else 'DIFFERENT'}")
sys.exit(1 if bad else 0)
