"""The closed forms of SCAN structural clustering (include/lpa.h: lpa_scan), shared by
tests/test_scan_host.py (the CPU reference on them) and tests/test_gpu_scan.py (the GPU on them).

CLOSED: name -> (V, edges, eps, mu, labels, roles) with roles as one letter per vertex:
c core, b border, h hub, o outlier."""
import numpy as np

LETTER = {"o": 0, "h": 1, "b": 2, "c": 3}


def clique_edges(members):
    return [(a, b) for i, a in enumerate(members) for b in members[i + 1:]]


def path_edges(n):
    return [(i, i + 1) for i in range(n - 1)]


DOUBLE_STAR = [(0, 1), (0, 2), (0, 3), (1, 4), (1, 5)]
BRIDGED = clique_edges([0, 1, 2]) + clique_edges([3, 4, 5]) + [(6, 0), (6, 3), (7, 6)]
CONTESTED = clique_edges([0, 1, 2, 3, 4]) + clique_edges([5, 6, 7, 8, 9]) + [(10, 0), (10, 1), (10, 5), (10, 6)]
# the same graph relabelled: the cliques' cores are 7, 8 and 5, 6
CONTESTED_RELABELLED = (clique_edges([7, 8, 0, 3, 4]) + clique_edges([5, 6, 1, 2, 9]) +
                        [(10, 7), (10, 8), (10, 5), (10, 6)])

CLOSED = {
    # sigma(0, 1) = 2 / sqrt(4 * 4) is exactly 0.5: the tie is similar
    "double-star-tie": (6, DOUBLE_STAR, 0.5, 2, [0] * 6, "cccccc"),
    "double-star-above": (6, DOUBLE_STAR, float(np.nextafter(0.5, 1)), 2, [0, 1, 0, 0, 1, 1], "cccccc"),
    "bridged-0.75": (8, BRIDGED, 0.75, 2, [0, 0, 0, 3, 3, 3, 6, 7], "ccccccho"),
    # sigma(6, 7) = 2 / sqrt(4 * 2) = 0.7071: 6 and 7 become a third cluster
    "bridged-0.7": (8, BRIDGED, 0.7, 2, [0, 0, 0, 3, 3, 3, 6, 6], "cccccccc"),
    "path6": (6, path_edges(6), 0.7, 2, [0, 0, 2, 3, 4, 4], "ccoocc"),
    "path5": (5, path_edges(5), 0.7, 2, [0, 0, 2, 3, 3], "cchcc"),
    "path6-mu3": (6, path_edges(6), 0.7, 3, [0, 1, 2, 3, 4, 5], "oooooo"),
    "contested": (11, CONTESTED, 0.5, 6, [0] * 5 + [5] * 5 + [0], "ccbbbccbbbb"),
    # the first clique now carries the larger label: 10 takes the smaller cluster label, 5
    "contested-relabelled": (11, CONTESTED_RELABELLED, 0.5, 6, [7, 5, 5, 7, 7, 5, 5, 7, 7, 5, 5], "bbbbbccccbb"),
    # mu = 1: every vertex is a core, the isolated one of its own cluster
    "mu1-isolated": (3, [(0, 1)], 0.7, 1, [0, 0, 2], "ccc"),
    "mu-above-V": (8, BRIDGED, 0.5, 9, list(range(8)), "oooooooo"),
}


def arrays(edges):
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()


def roles(letters):
    return np.array([LETTER[x] for x in letters], np.uint8)
