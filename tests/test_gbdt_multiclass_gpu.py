"""One-pass multi-class RF kernels (gbdt_mc_kernels.hip) against numpy and the CPU oracle."""
import numpy as np
import pytest
import torch

from shifu_amd.models.gbdt import NB, BinnedData, TreeConfig, TreeTrainer, _pack_scale

N, F = 2 * 4096 + 77, 40            # one full 32-feature group and a partial one


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["root", "perm", "forest"])
@pytest.mark.parametrize("C,nb", [(3, 10), (3, 256), (8, 256), (16, 256)])     # FI = 32, 16, 8, 4
def test_hist_mc_exact(C, nb, rows):
    from shifu_amd.ops import _native as nat
    rng = np.random.default_rng(C * 1000 + nb)
    T = 2 if rows == "forest" else 1                      # forest: virtual rows t * N + row
    codes = rng.integers(0, nb, (N, F)).astype(np.uint8)
    w = (rng.poisson(1.0, T * N) * 0.37).astype(np.float32)          # bag counts (zeros too) x significance
    y = rng.integers(0, C, T * N)
    y[rng.integers(0, T * N, 50)] = C + 2                 # labels outside [0, C): in no class
    y[rng.integers(0, T * N, 50)] = -1
    cls = np.where((y >= 0) & (y < C), y, 255).astype(np.uint8)
    if rows == "root":                                    # one node, two row chunks
        v, ranges = np.arange(N), [[(0, 4100), (4100, N)]]
    else:                                                 # two nodes, each an ascending subset
        pick = rng.permutation(T * N)[: int(0.75 * T * N)]
        side = (pick >= N) if T == 2 else (rng.random(len(pick)) < 0.4)
        v = np.concatenate([np.sort(pick[~side]), np.sort(pick[side])])
        m0 = int((~side).sum())
        ranges = [[(0, m0 // 2), (m0 // 2, m0)], [(m0, len(v))]]
    scale_g = _pack_scale(float(w.max()), 23, margin=16.0)
    q = np.rint((w * np.float32(scale_g)).astype(np.float64)).astype(np.int64)
    want = np.zeros((len(ranges), C, F, NB), np.int64)
    for nd, chunks in enumerate(ranges):
        r = v[chunks[0][0]: chunks[-1][1]]
        r = r[cls[r] < C]
        for f in range(F):
            np.add.at(want[nd, :, f], (cls[r], codes[r % N, f]), q[r])
    nbp = 1 << (nb - 1).bit_length()
    S = 32 // nat.hip().shifu_gbdt_mc_tier(C, nbp)
    G = (F + 31) // 32
    group_items = [(nd, lo, hi, g) for nd, chunks in enumerate(ranges) for lo, hi in chunks for g in range(G)]
    ni = np.full((len(ranges), G, 2), -1, np.int32)
    for i, (nd, lo, hi, g) in enumerate(group_items):
        ni[nd, g, [c[0] for c in ranges[nd]].index(lo)] = i
    items = np.array([(nd, lo, hi, g * S + s) for nd, lo, hi, g in group_items for s in range(S)], np.int32)
    bins = BinnedData.blocked(codes, "cuda")
    slab = torch.empty(len(items) * C * nbp * (32 // S), dtype=torch.int64, device="cuda")
    hist = torch.full((len(ranges), C, F, NB), -1, dtype=torch.int64, device="cuda")
    nat.call_hip("shifu_gbdt_hist_mc", bins, N * 128, None if rows == "root" else _t(v.astype(np.int32)), _t(w),
                 _t(cls), _t(items), len(items), slab, _t(ni), 2, _t(np.arange(len(ranges), dtype=np.int32)),
                 len(ranges), hist, C, F, nbp, scale_g, N if T == 2 else 0, nat.stream_of(hist))
    assert np.array_equal(hist.cpu().numpy(), want)


def _imp(x, imp):
    s = x.sum()
    p = x / (s if s > 0 else 1.0)
    if imp == "gini":
        return -float((p * p).sum())
    p = p[p > 0]
    return -float((p * np.log2(p)).sum())


def _scan(h, nbins, is_cat, mask, imp, inv, min_inst):
    """Plain fp64 scan of integer class histograms h [C, F, NB]: every admissible (gain, feature,
    position, class left, class right), best first (ties: lowest feature, then position)."""
    out = []
    for f in np.nonzero(mask)[0]:
        H = h[:, f].astype(np.float64) * inv
        order = list(range(NB))
        if is_cat[f]:
            den = H[0] + H[1]
            key = np.where(den != 0, H[1] / np.where(den != 0, den, 1), 0.0)
            key[nbins[f]:] = np.inf
            order = sorted(order, key=lambda b: (key[b], b))
        tot, left = H.sum(1), np.zeros(len(H))
        for i in range(nbins[f] - 1):
            left = left + H[:, order[i]]
            right = tot - left
            lw, rw, tw = left.sum(), right.sum(), tot.sum()
            if lw > min_inst and rw > min_inst:
                gain = _imp(tot, imp) - lw / tw * _imp(left, imp) - rw / tw * _imp(right, imp)
                if gain > 0:
                    out.append((gain, int(f), i, int(np.argmax(left)), int(np.argmax(right)), order))
    return sorted(out, key=lambda c: (-c[0], c[1], c[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("imp", ["entropy", "gini"])
def test_split_mc_matches_fp64_scan(imp):
    """Node 0 is built, node 1 derived (parent - node 0, written back).  Feature 1 is categorical
    with tied keys (bins 2, 5) and an empty category (3); each node has a masked-out feature."""
    from shifu_amd.ops import _native as nat
    from shifu_amd.models.gbdt import IMPURITY_IDS
    C, Fs, scale = 4, 6, 256.0
    rng = np.random.default_rng(3)
    nbins = np.array([10, 12, 256, 7, 200, 33], np.int32)
    is_cat = np.array([0, 1, 0, 0, 1, 0], np.uint8)
    h = rng.integers(0, 40, (2, C, Fs, NB)) * 37          # the two children, in units of 1 / scale
    for f in range(Fs):
        h[:, :, f, nbins[f]:] = 0
    h[:, :, 1, 5] = h[:, :, 1, 2]
    h[:, :, 1, 3] = 0
    prev = h.sum(0, keepdims=True)
    mask = np.array([[0, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1]], np.uint8)
    hist = _t(h.astype(np.int64))
    hist[1] = -1                                          # the derived node's histogram is an output
    cand = torch.empty(2, Fs, 10, dtype=torch.float64, device="cuda")
    order = torch.empty(2, Fs, NB, dtype=torch.uint8, device="cuda")
    best = torch.empty(2, 10, dtype=torch.float64, device="cuda")
    order_out = torch.empty(2, NB, dtype=torch.uint8, device="cuda")
    nat.call_hip("shifu_gbdt_split_mc", hist, _t(prev.astype(np.int64)), _t(np.array([-1, 0], np.int32)),
                 _t(np.array([0, 0], np.int32)), 2, _t(nbins), _t(is_cat), _t(mask), cand, order, C, Fs, NB,
                 IMPURITY_IDS[imp], 5.0, 0.0, 1.0 / scale, best, order_out, nat.stream_of(hist))
    assert np.array_equal(hist.cpu().numpy(), h)
    got = best.cpu().numpy()
    for nd in range(2):
        ref = _scan(h[nd], nbins, is_cat, mask[nd], imp, 1.0 / scale, 5.0)
        assert ref[0][0] - ref[1][0] > 1e-9               # a log2 ulp cannot decide the answer
        gain, f, pos, cl, cr, ordr = ref[0]
        assert got[nd, 7] == 1 and tuple(got[nd, [0, 1, 8, 9]]) == (f, pos, cl, cr)
        assert abs(got[nd, 2] - gain) < 1e-5
        assert np.array_equal(order_out.cpu().numpy()[nd], ordr)
        for c in ref:                                     # every scanned feature's order (ties, empty bin)
            assert np.array_equal(order.cpu().numpy()[nd, c[1]], c[5])


def _trainers(C, nb, imp, n, monkeypatch, kernel=True):
    rng = np.random.default_rng(C)
    codes = rng.integers(0, nb, (n, 6))
    y = ((codes[:, 0] * 3 // nb) + 2 * (codes[:, 1] % 3 == 0) + (codes[:, 4] > nb // 2)) % C
    y = np.where(rng.random(n) < 0.1, rng.integers(0, C, n), y).astype(np.float32)
    is_cat = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    cfg = dict(algorithm="RF", tree_num=3, max_depth=4, impurity=imp, feature_subset_strategy="ALL",
               bagging_sample_rate=1.0, n_classes=C, seed=5)
    monkeypatch.setenv("SHIFU_RF_BATCH", "2")
    monkeypatch.setenv("SHIFU_GBDT_MC_KERNEL", "1" if kernel else "0")
    out = []
    for dev in ("cpu", "cuda"):
        d = BinnedData.from_codes(codes, y, np.full(6, nb), is_cat, device=dev)
        tr = TreeTrainer(TreeConfig(**cfg), d)
        tr.train()
        out.append((tr, tr.predict(d).cpu().numpy()))
    return out


def _same_trees(a, b):
    for x, y in zip(a[0].trees, b[0].trees):
        for k in ("feat", "thr", "cat_left", "class_value"):
            assert np.array_equal(getattr(x, k), getattr(y, k)), k
    assert np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("imp", ["entropy", "gini"])
def test_mc_trees_match_cpu_and_c_pass(imp, monkeypatch):
    cpu, gpu = _trainers(5, 10, imp, 5000, monkeypatch)
    _same_trees(cpu, gpu)
    levels = gpu[0].last_tree_stats["levels"]
    assert levels and all(lv["hist_passes"] == 1 for lv in levels)
    _, old = _trainers(5, 10, imp, 5000, monkeypatch, kernel=False)
    assert all(lv["hist_passes"] == 5 for lv in old[0].last_tree_stats["levels"])
    _same_trees(old, gpu)


@pytest.mark.gpu
def test_mc_too_many_keys_takes_c_pass(monkeypatch):
    cpu, gpu = _trainers(17, 256, "gini", 3000, monkeypatch)             # 17 * 256 > 4096 class-keyed bins
    assert all(lv["hist_passes"] == 17 for lv in gpu[0].last_tree_stats["levels"])
    _same_trees(cpu, gpu)
