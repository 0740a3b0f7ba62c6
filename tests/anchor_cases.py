"""What the tests of the anchor operators share (profileover: test_profileover.py with profileover_ref.py; matrixover:
test_matrixover.py with matrixover_ref.py): the anchor table itself, the signals and anchor lists the GPU tests draw, and
the cases of the device's anchor check.

A genome is a list of numpy vectors; anchors are rows (vector index, position, strand +1 / -1).

The anchor check (gdsp_anchors.hip) is all that stands between a bad position on the device and a kernel that reads
outside its vector.  It runs at most 1024 workgroups of 256 threads, and a thread strides over the anchors beyond those:
CHECK_GRID + 1 is the smallest number of anchors whose last one only the stride loop sees, and 1, 256 and 257 are one
thread, one full workgroup and the first thread of a second."""
import numpy as np

CHECK_GRID = 1024 * 256
CHECK_COUNTS = (1, 256, 257, CHECK_GRID + 1)
CHECK_N = 100                                    # the one vector of the check's cases: np.arange(100.)
CHECK_GOOD, CHECK_BAD = (0, 50, 1), (0, CHECK_N, -1)


def anchors_array(anchors):
    return np.asarray(anchors, dtype=np.int64).reshape(-1, 3)


def check_anchors(count, bad_last=False):
    """count anchors, every one CHECK_GOOD -- or all but the last, which lies one base beyond the vector's end"""
    a = np.tile(np.array(CHECK_GOOD, dtype=np.int64), (count, 1))
    if bad_last:
        a[-1] = CHECK_BAD
    return a


def dev():
    import genodsp_amd as g
    g.set_device(0)
    return g


def up(g, vectors):
    return [g.DeviceVector.from_numpy(v) for v in vectors]


def real(n, rng):
    return rng.standard_normal(n) * 10.0


def depth(n, rng):
    return rng.integers(0, 60, n).astype(np.float64)


def every_base(n, c=0):
    return [(c, p, s) for p in range(n) for s in (1, -1)]


def random_anchors(vectors, count, rng):
    out = []
    for _ in range(count):
        c = int(rng.integers(0, len(vectors)))
        out.append((c, int(rng.integers(0, vectors[c].size)), int(rng.choice([1, -1]))))
    return out
