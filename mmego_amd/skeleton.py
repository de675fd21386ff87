"""Skeleton topology constants of the path and the ST-GCN adjacency (host-side, numpy).

Mirrors the values of the reference's Config/config.py:22-55 and the 'kinect_upper' graph of
Net/GCN.py:150-278.  The forward-kinematics walk orders live in csrc/geom.hip (make_plan).
"""
import numpy as np

JOINTS_ALL, JOINTS_UPPER, JOINTS_LOWER = 21, 15, 8
POINTS = 128
LOWER_POINTS = 64
FRAMES = 20

BONES_UPPER = [[20, 3], [3, 2], [2, 1], [2, 4], [2, 8], [4, 5], [5, 6], [6, 7], [8, 9], [9, 10], [10, 11],
               [1, 0], [0, 12], [0, 16]]
BONES_LOWER = [[12, 13], [13, 14], [14, 15], [16, 17], [17, 18], [18, 19]]
BONES_ALL = BONES_UPPER + BONES_LOWER
UPPER_MAP = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 20]
LOWER_MAP = [12, 13, 14, 15, 16, 17, 18, 19]
HAND_MAP = [7, 6, 11, 10]
KINECT_SELECTION = [0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 18, 19, 20, 21, 22, 23, 24, 25, 26]


def _walk(bones, joint_map):
    """[parent, child] pairs in the 21-joint numbering -> (child, parent) rows in the numbering of a net's own row (joint_map)."""
    return np.asarray([[joint_map.index(c), joint_map.index(p)] for p, c in bones], dtype=np.int32)


# Walk tables of the bone-length-preserving blend (ops.blend_bones): (child, parent) per bone in the numbering of the net's own row,
# parents before children as the nets' forward kinematics place them (csrc/geom.hip make_plan); bone k has row k of the body's bone set.
WALK_UPPER = _walk(BONES_UPPER, UPPER_MAP)          # one tree rooted at the head (joint 20, slot 14): 14 bones, body rows 0..13
WALK_LOWER = _walk(BONES_LOWER, LOWER_MAP)          # a forest rooted at the two hips (joints 12 and 16, slots 0 and 4): 6 bones
WALK_UPPER_ROWS = tuple(range(0, len(BONES_UPPER)))
WALK_LOWER_ROWS = tuple(range(len(BONES_UPPER), len(BONES_ALL)))
# Which of a net's rotations turns bone k (ops.blend_rot): Upper_Net's q [., 14, 3, 3] is indexed by the child's slot in its own row
# (the head, slot 14, is no bone's child), Lower_Net's q [., 6, 3, 3] by the child's position among the six leg joints below the hips.
ROT_UPPER = [int(c) for c in WALK_UPPER[:, 0]]
LOWER_ROT_MAP = sorted(c for _, c in BONES_LOWER)   # [13, 14, 15, 17, 18, 19]: the leg joints in joint order (Lower_Net.py:29)
ROT_LOWER = [LOWER_ROT_MAP.index(c) for _, c in BONES_LOWER]

GCN_EDGES = [(0, 12), (0, 13), (0, 1), (1, 2), (2, 3), (2, 4), (2, 8), (3, 14), (4, 5), (5, 6), (6, 7), (8, 9),
             (9, 10), (10, 11)]


def gcn_adjacency(strategy="distance", max_hop=1):
    """(K, 15, 15) float64 partitioned normalised adjacency: K=1 ('uniform') or max_hop+1 ('distance')."""
    n = JOINTS_UPPER
    link = np.eye(n)
    for i, j in GCN_EDGES:
        link[i, j] = link[j, i] = 1.0
    # hop distance up to max_hop (inf beyond)
    hop = np.full((n, n), np.inf)
    power = [np.linalg.matrix_power(link, d) > 0 for d in range(max_hop + 1)]
    for d in range(max_hop, -1, -1):
        hop[power[d]] = d
    reach = (hop <= max_hop).astype(np.float64)
    deg = reach.sum(axis=0)
    inv_sqrt = np.where(deg > 0, deg ** -0.5, 0.0)
    norm = (inv_sqrt[:, None] * reach) * inv_sqrt[None, :]
    if strategy == "uniform":
        return norm[None].copy()
    if strategy == "distance":
        return np.stack([np.where(hop == h, norm, 0.0) for h in range(max_hop + 1)])
    raise ValueError("unsupported graph strategy %r" % (strategy,))
