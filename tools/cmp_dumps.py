"""Compare three bench.py --dump-outputs directories: two runs of a parent build (their own run-to-run spread) and one of this
tree.  Integer arrays and dictionaries must be equal; for the rest the largest absolute difference of each pair is printed.
usage: cmp_dumps.py PARENT_A PARENT_B RESULT"""
import json, os, sys
import numpy as np
a, b, r = sys.argv[1:4]
def load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        p = os.path.join(d, f)
        if f.endswith(".npy"):
            out[f] = np.load(p)
        elif f.endswith(".json"):
            out[f] = json.load(open(p))
    return out
A, B, R = load(a), load(b), load(r)
print("files:", sorted(A))
for k in sorted(A):
    if isinstance(A[k], dict):
        print(k, "parent a == parent b:", A[k] == B[k], " parent a == result:", A[k] == R[k])
        if A[k] != R[k]:
            print("   parent", A[k]); print("   result", R[k])
        continue
    x, y, z = A[k], B[k], R[k]
    if np.issubdtype(x.dtype, np.integer):
        print("%-16s parent a == parent b: %s   parent a == result: %s" % (k, np.array_equal(x, y), np.array_equal(x, z)))
    else:
        print("%-16s max |parent a - parent b| = %.3e   max |parent a - result| = %.3e   max |parent b - result| = %.3e   bit-equal a/result: %s" % (
            k, np.max(np.abs(x - y)), np.max(np.abs(x - z)), np.max(np.abs(y - z)), x.tobytes() == z.tobytes()))
