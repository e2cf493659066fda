"""Wide-feature (257 .. 16384 bins) GBT/RF kernels against numpy and the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from shifu_amd.models.gbdt import BinnedData, TreeConfig, TreeTrainer, _pack_scale, _pad_bins

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gbdt_narrow_expect.npz")


# n = 5000 crosses the 4096-rows-per-copy unpack once at one LDS copy (nb 16384); 40000 rows cross
# it at eight copies (nb 257)
@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["root", "perm", "forest"])
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("n,nb", [(5000, 257), (5000, 1000), (5000, 16384), (40000, 257)])
def test_hist_wide_exact(n, nb, skew, rows):
    from shifu_amd.ops import _native as nat
    rng = np.random.default_rng(nb + skew)
    T = 2 if rows == "forest" else 1                      # forest: virtual rows t * n + row
    code = rng.integers(0, nb, n).astype(np.uint16)
    w = rng.uniform(0.01, 1.0, T * n).astype(np.float32)
    g = rng.normal(size=T * n).astype(np.float32)
    if skew:                                              # 90 % of the rows in one bin at the largest weight
        hot = rng.random(n) < 0.9
        code[hot] = nb - 1
        w[np.tile(hot, T)] = 1.0
    v = np.arange(n) if rows == "root" else rng.permutation(T * n)[: int(0.75 * T * n)]
    by_pos = rows == "perm"                               # (w, g) travel in position order
    scale_w = _pack_scale(float(w.max()), 16)
    scale_g = _pack_scale(float(np.abs(w * g).max()), 23, margin=16.0)
    qw = np.rint((w * np.float32(scale_w)).astype(np.float64)).astype(np.int64)[v]
    qg = np.rint(((w * g) * np.float32(scale_g)).astype(np.float64)).astype(np.int64)[v]
    nbp = _pad_bins(nb)
    want = np.zeros((2, 2, nbp), np.int64)                # item 0: the rows, item 1: empty -> zeros
    np.add.at(want[0, 0], code[v % n], qw)
    np.add.at(want[0, 1], code[v % n], qg)
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    items = t(np.array([[0, 0, len(v), 0], [0, 7, 7, 0]], np.int32))
    slab = torch.full((2, 2, nbp), -1, dtype=torch.int64, device=dev)
    wd, gd = (t(w[v]), t(g[v])) if by_pos else (t(w), t(g))
    nat.call_hip("shifu_gbdt_hist_wide", t(code.reshape(1, n)), n, t(np.array([nb], np.int32)),
                 None if rows == "root" else t(v.astype(np.int32)), wd, gd, int(by_pos), items, 2, slab, nbp,
                 scale_w, scale_g, n if rows == "forest" else 0, nat.stream_of(slab))
    assert np.array_equal(slab.cpu().numpy(), want)


def mixed_data(n=5000, seed=7):
    """40 narrow features (two 32-feature groups) + a wide numeric (300 bins) + a wide categorical
    (1000 bins), a planted rule on both wide features and narrow feature 3, Poisson bag weights."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 64, (n, 42)).astype(np.int16)
    codes[:, 40] = rng.integers(0, 300, n)
    codes[:, 41] = rng.integers(0, 999, n)
    y = ((codes[:, 40] > 270).astype(int) + 2 * np.isin(codes[:, 41], rng.permutation(999)[:500])
         + 4 * (codes[:, 3] > 40)).astype(np.float32) + rng.normal(0, 0.1, n).astype(np.float32)
    nbins = np.array([64] * 40 + [300, 1000])
    is_cat = np.array([0] * 41 + [1], np.uint8)
    return codes, y, rng.poisson(1.0, n).astype(np.float32), nbins, is_cat


@pytest.mark.gpu
@pytest.mark.parametrize("alg,trees", [("GBT", 3), ("RF", 2)])
def test_wide_trees_match_cpu(alg, trees):
    codes, y, w, nbins, is_cat = mixed_data()
    cfg = dict(algorithm=alg, tree_num=trees, max_depth=4, learning_rate=0.3, feature_subset_strategy="ALL")
    tc = TreeTrainer(TreeConfig(**cfg), BinnedData.from_codes(codes, y, nbins, is_cat, sig=w))
    data_g = BinnedData.from_codes(codes, y, nbins, is_cat, sig=w, device="cuda")
    tg = TreeTrainer(TreeConfig(**cfg), data_g)
    tc.train()
    tg.train()
    assert {40, 41} <= {int(f) for t in tg.trees for f in t.feat}
    for a, b in zip(tc.trees, tg.trees):
        assert (a.feat == b.feat).all() and (a.thr == b.thr).all() and (a.cat_left == b.cat_left).all()
        assert np.allclose(a.value, b.value, atol=1e-5)
    host = sum(t.weight * t.predict_bins(codes, is_cat) for t in tg.trees) / (trees if alg == "RF" else 1)
    assert np.allclose(tg.predict(data_g).cpu().numpy(), host, atol=1e-5)
    assert np.allclose(tg.pred.cpu().numpy() / (trees if alg == "RF" else 1), host, atol=1e-5)


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_narrow_data_unchanged(device):
    """No wide feature: the trees are the ones the CPU oracle grew before the wide path existed
    (tests/golden/gbdt_narrow_expect.npz: feat / thr / value of 3 GBT trees on this data)."""
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 256, (6000, 40)).astype(np.uint8)
    codes[:, 5] = rng.integers(0, 9, 6000)
    y = ((codes[:, 0] > 200) ^ np.isin(codes[:, 5], [1, 4, 6]) ^ (codes[:, 33] < 50)).astype(np.float32)
    y = np.where(rng.random(6000) < 0.08, 1 - y, y)
    nbins, is_cat = np.array([256] * 5 + [10] + [256] * 34), np.array([0] * 5 + [1] + [0] * 34, np.uint8)
    data = BinnedData.from_codes(codes, y, nbins, is_cat, device=device)
    assert data.wbins is None
    tr = TreeTrainer(TreeConfig("GBT", tree_num=3, max_depth=5, learning_rate=0.3, feature_subset_strategy="ALL"),
                     data)
    tr.train()
    exp = np.load(GOLDEN)
    assert np.array_equal(np.stack([t.feat for t in tr.trees]), exp["feat"])
    assert np.array_equal(np.stack([t.thr for t in tr.trees]), exp["thr"])
    assert np.array_equal(np.stack([t.cat_left for t in tr.trees]), exp["cat_left"])
    assert np.allclose(np.stack([t.value for t in tr.trees]), exp["value"], atol=1e-5)
