"""GBT/RF training on features with more than 256 bins (uint16 wide columns): CPU oracle semantics."""
import numpy as np
import pytest
import torch

from shifu_amd.models.gbdt import BinnedData, TreeConfig, TreeTrainer, _gain_py

IMPS = {"variance": 0, "friedmanmse": 1, "entropy": 2, "gini": 3}


def wide_data(kind, n=3000, seed=0):
    """One wide feature (numeric nb 300: y = code > 270; categorical nb 1000 incl. the empty missing
    bin: y = category in a random half) + one narrow noise feature, 5 % label noise, weights from
    {0.5, 1, 1.5, 2} (exact in the trainer's fixed point, so a float64 brute force sees its sums)."""
    rng = np.random.default_rng(seed)
    nb = 300 if kind == "num" else 1000
    code = rng.integers(0, nb - (kind == "cat"), n)
    y = (code > 270) if kind == "num" else np.isin(code, rng.permutation(nb - 1)[:nb // 2])
    y = np.where(rng.random(n) < 0.05, 1 - y, y).astype(np.float32)
    codes = np.stack([code, rng.integers(0, 12, n)], 1).astype(np.int16)
    w = rng.choice([0.5, 1.0, 1.5, 2.0], n).astype(np.float32)
    return codes, y, w, np.array([nb, 12]), np.array([kind == "cat", 0], np.uint8)


def best_split_bruteforce(codes, y, w, nbins, is_cat, min_inst, imp):
    """float64 scan of every (feature, ordered cut); categorical order by s / w ascending, stable,
    an empty bin keyed 4.9e-324.  Returns (gain, feature, cut position, left bins)."""
    best = (-1.0, None, None, None)
    w, wy = w.astype(np.float64), w.astype(np.float64) * y
    for f, nb in enumerate(nbins):
        cw, cs = np.bincount(codes[:, f], w, nb), np.bincount(codes[:, f], wy, nb)
        order = np.arange(nb)
        if is_cat[f]:
            order = np.argsort(np.where(cw != 0, cs / np.where(cw != 0, cw, 1), 4.9e-324), kind="stable")
        pw, ps = np.cumsum(cw[order]), np.cumsum(cs[order])
        for b in range(nb - 1):
            lw, ls, rw, rs = pw[b], ps[b], pw[-1] - pw[b], ps[-1] - ps[b]
            if lw <= min_inst or rw <= min_inst:
                continue
            gain = _gain_py(imp, lw, ls, rw, rs)
            if gain > best[0] + 1e-12:
                best = (gain, f, b, set(order[:b + 1].tolist()))
    return best


@pytest.mark.parametrize("imp", list(IMPS))
@pytest.mark.parametrize("kind", ["num", "cat"])
def test_wide_root_split_matches_bruteforce(kind, imp):
    codes, y, w, nbins, is_cat = wide_data(kind)
    data = BinnedData.from_codes(codes, y, nbins, is_cat, sig=w)
    assert (data.codes().numpy() == codes).all() and data.bins[0, :, 0].sum() == 0
    tr = TreeTrainer(TreeConfig("GBT", tree_num=1, max_depth=2, impurity=imp, feature_subset_strategy="ALL",
                                min_instances_per_node=5), data)
    tr.train()
    t = tr.trees[0]
    gain, f, b, left = best_split_bruteforce(codes, y, w, nbins, is_cat, 5, IMPS[imp])
    assert f == 0 and t.feat[1] == 0
    if kind == "num":
        assert b > 255 and t.thr[1] == b
    else:
        assert {c for c in range(nbins[0]) if (t.cat_left[1, c >> 5] >> (c & 31)) & 1} == left
    assert abs(t.gain[1] - gain) < 1e-4 * max(1, abs(gain))


def test_wide_round_trip(tmp_path):
    """heap tree -> record -> .gbt file -> record -> heap tree, and the flattened scoring ensemble."""
    from shifu_amd.config.column_config import ColumnConfig
    from shifu_amd.formats import tree_format as tf
    from shifu_amd.scoring.tree_ensemble import TreeScorer
    rng = np.random.default_rng(3)
    n, ncat = 4000, 400
    codes = rng.integers(0, 10, (n, 4)).astype(np.int16)
    codes[:, 2] = rng.integers(0, ncat, n)
    y = (np.isin(codes[:, 2], rng.permutation(ncat)[:ncat // 2]) ^ (codes[:, 0] > 6)).astype(np.float32)
    nbins, is_cat = np.array([10, 10, ncat + 1, 10]), np.array([0, 0, 1, 0], np.uint8)
    data = BinnedData.from_codes(codes, y, nbins, is_cat)
    tr = TreeTrainer(TreeConfig("GBT", tree_num=3, max_depth=4, learning_rate=0.3, feature_subset_strategy="ALL"),
                     data)
    tr.train()
    assert any((t.feat == 2).any() for t in tr.trees)
    cols = []
    for f in range(4):          # numeric code c <-> raw value c + 0.5 under boundaries [-inf, 1, 2, ...]
        c = ColumnConfig({"columnNum": f, "columnName": f"c{f}", "columnType": "C" if is_cat[f] else "N"})
        if is_cat[f]:
            c.bin_category = [f"k{i}" for i in range(ncat)]
        else:
            c.bin_boundary = [-np.inf] + list(range(1, 10))
        cols.append(c)
    recs = [tf.heap_tree_to_record(t, i, cols, learning_rate=t.weight) for i, t in enumerate(tr.trees)]
    m = tf.TreeModelFile(algorithm="GBT", loss="squared", is_classification=False, is_one_vs_all=False,
                         input_count=4, numerical_means={}, names={c.num: c.name for c in cols},
                         categories={2: cols[2].bin_category}, column_mapping={f: f for f in range(4)}, bags=[recs])
    tf.write_tree_model(str(tmp_path / "m.gbt"), m)
    back = tf.read_tree_model(str(tmp_path / "m.gbt"))
    for t, rec in zip(tr.trees, back.bags[0]):
        t2 = tf.record_to_heap_tree(rec, cols, min_depth=t.max_depth)
        assert np.array_equal(t2.predict_bins(codes, is_cat), t.predict_bins(codes, is_cat))
    X = torch.from_numpy(np.where(is_cat.astype(bool), codes, codes + 0.5).astype(np.float64))
    assert np.allclose(TreeScorer(back).score_bags(X)[:, 0], tr.predict(data).numpy(), atol=1e-5)


def test_wide_refusals():
    codes = np.zeros((10, 2), np.int16)
    with pytest.raises(ValueError, match="feature 1 has 16385 bins"):
        BinnedData.from_codes(codes, np.zeros(10), [10, 16385])
    data = BinnedData.from_codes(codes, np.zeros(10), [10, 300])
    with pytest.raises(ValueError, match="multi-class"):
        TreeTrainer(TreeConfig("RF", impurity="gini", n_classes=3), data)
