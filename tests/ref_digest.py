"""SHA-256 digests of what the reference's own nanoflann (oracle/_ref) returned on the CPU tests' seeded
clouds, recorded in tests/golden/ref_digests.json by tests/golden/make_golden.py.  They pin the oracle to
the reference where oracle/_ref is not built; where it is, the tests also compare live, array by array."""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")


def load():
    with open(PATH) as f:
        return json.load(f)


def arrays_digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def tree_digest(t):
    """An exported nanoflann tree (oracle.tree / oracle.ref_tree) in the terms oracle.same_tree compares:
    walked from the root, every node's divfeat, a leaf's vind range, an inner node's divlow / divhigh
    (-0 as +0), then vind.  The node numbering does not enter."""
    vind, nodes, div = t
    h = hashlib.sha256()
    st = [0]
    while st:
        x = st.pop()
        if nodes[x, 2] < 0:
            h.update(np.array([nodes[x, 2], nodes[x, 0], nodes[x, 1]], np.int32).tobytes())
            continue
        h.update(np.int32(nodes[x, 2]).tobytes())
        h.update((np.asarray(div[x], np.float32) + np.float32(0.0)).tobytes())
        st.append(int(nodes[x, 1]))
        st.append(int(nodes[x, 0]))
    h.update(np.ascontiguousarray(vind, np.int32).tobytes())
    return h.hexdigest()
