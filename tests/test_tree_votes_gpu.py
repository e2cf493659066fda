"""K13 class votes (tree_vote_coded_kernel) against the CPU FlatEnsemble (fp64 torch walk): exact."""
import numpy as np
import pytest
import torch

from shifu_amd.formats.tree_format import CATEGORICAL, CONTINUOUS, Node, Split, TreeModelFile, TreeRecord
from shifu_amd.scoring.tree_ensemble import TreeScorer

pytestmark = pytest.mark.gpu
N_CAT = 5                                      # categories of the last input column


def _forest(C, n_classes, bag_sizes, seed):
    """Depth-6 trees over C - 1 numeric inputs and one categorical; tree 1 of a bag is a single
    leaf.  Leaf values: classes, values outside [0, n_classes) and halves (0.5 -> 0, 1.5 -> 2)."""
    rng = np.random.default_rng(seed)
    leaf_values = np.concatenate([np.arange(-2, n_classes + 2), [0.5, 1.5, 2.5, n_classes - 1.5]])

    def grow(d, depth):
        if d == depth:
            return Node(0, class_value=float(rng.choice(leaf_values)))
        nd = Node(0)
        col = int(rng.integers(0, C))
        sub = {int(c) for c in rng.choice(N_CAT, size=2, replace=False)}
        nd.split = Split(col, CONTINUOUS, threshold=float(rng.normal())) if col < C - 1 else \
            Split(col, CATEGORICAL, is_left=bool(rng.random() < 0.5), categories=sub)
        nd.left, nd.right = grow(d + 1, depth), grow(d + 1, depth)
        return nd
    bags = [[TreeRecord(t, 0, grow(0, 0 if t == 1 else 6), 1.0) for t in range(T)] for T in bag_sizes]
    return TreeModelFile("RF", "entropy", True, False, C, {c: 0.0 for c in range(C)}, {c: f"c{c}" for c in range(C)},
                         {C - 1: [f"v{j}" for j in range(N_CAT)]}, {c: c for c in range(C)}, bags)


def _inputs(n, C, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, C))
    X[rng.random(size=X.shape) < 0.05] = np.nan               # NaN goes right
    X[:, C - 1] = rng.integers(-1, N_CAT + 2, size=n)         # incl. the unseen index and invalid ones
    return torch.from_numpy(X)


# C_in, n_classes, rows per block R (threads per row 256 / R, 4 chains each), trees, rows
@pytest.mark.parametrize("C,n_classes,R,T,n", [
    (3, 3, 256, 5, 5),              # n < R; one tree per group
    (3, 3, 256, 37, 30_003),        # 13 groups of 3 trees (short batch of chains), ragged last row block
    (600, 3, 16, 40, 35),           # codes bound R; n = 2R + 3; trees of a group < threads per row
    (3, 200, 32, 7, 67),            # counters bound R; n = 2R + 3
    (3, 200, 32, 70, 32_771),       # 2 groups of 35 trees over 8 threads per row: a full round and a short one
])
def test_votes_match_cpu_walk(C, n_classes, R, T, n):
    from shifu_amd.ops import _native
    assert _native.hip().shifu_tree_vote_rows(C, n_classes) == R
    m, X = _forest(C, n_classes, [T], seed=T), _inputs(n, C, seed=n)
    ref = TreeScorer(m, device="cpu").ens[0].votes(X, n_classes)
    got = TreeScorer(m, device="cuda").ens[0].votes(X.cuda(), n_classes)
    assert got.dtype == torch.int32 and int(ref.sum()) == n * T and torch.equal(got.cpu(), ref)


def test_class_votes_two_bags_bitwise():
    """Bags of 4 and 8 trees: torch divides a device tensor by a host scalar as a product with the
    rounded reciprocal, so cnt / T has the same bits on both devices only where 1 / T is exact."""
    m, X = _forest(4, 3, [4, 8], seed=2), _inputs(1000, 4, seed=3).numpy()
    table = {**{f"c{c}": X[:, c] for c in range(3)}, "c3": [f"v{int(v)}" for v in X[:, 3]]}   # v-1, v5, v6: unseen
    ref = TreeScorer(m, device="cpu").class_votes(table, 3)
    assert np.array_equal(TreeScorer(m, device="cuda").class_votes(table, 3), ref)
