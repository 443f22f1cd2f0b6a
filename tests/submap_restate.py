"""include/qtr_submap_math.h restated in numpy: the host side of every submap comparison.  numpy never fuses a product
with a sum, so the float64 expressions below round exactly as the header's do under -ffp-contract=off."""
import numpy as np


def transform(T, vox):
    """vox: [n, 4] float32 records; T: 4 x 4 (rows 0 - 2 used).  Returns the [n, 4] float32 records under T, w copied."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    vox = np.ascontiguousarray(vox, dtype=np.float32)
    x, y, z = (vox[:, k].astype(np.float64) for k in range(3))
    out = vox.copy()  # (w keeps its bits)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def merge(voxels, poses=None):
    """The concatenation a merge runs its front end on: member k's records under poses[k] (None: identities), in member
    order, stored order within a member."""
    if poses is None:
        poses = [np.eye(4)] * len(voxels)
    return np.ascontiguousarray(np.concatenate([transform(T, v) for T, v in zip(poses, voxels)]))
