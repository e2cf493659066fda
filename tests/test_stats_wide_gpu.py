"""Columns with 1025-16384 bin boundaries on the GPU: K1/K2 statistics (column_stats_wide_kernel,
mixed with narrow columns in one batch) and int16 tree codes (K1' / the codes half of K5), exact
against numpy / the host oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, THR = 70000, 1e20            # two 65536-row chunks; numericalValueThreshold


def _bounds(rng, nb):
    return np.concatenate([[-np.inf], np.sort(rng.uniform(-1000, 1000, nb - 1))])


def _values(rng, b, skew):
    v = rng.uniform(b[1] - 50, b[-1] + 50, N)                # also below the first finite / above the last boundary
    v[:5000] = rng.choice(b[1:], 5000)                       # equal to boundaries
    if skew:
        v[rng.random(N) < 0.9] = b[len(b) // 2]
    for k, x in enumerate([np.nan, np.inf, -np.inf, 1e30]):  # 1e30 > THR: counted as missing
        v[rng.integers(0, N, 200 if k == 0 else 20)] = x
    return v


def _reference(v, pos, w, b):
    v = np.where(v > THR, np.nan, v)
    nb = len(b)
    idx = np.where(np.isnan(v), nb, np.clip(np.searchsorted(b, v, "right") - 1, 0, nb - 1))
    cnt, ws = np.zeros((2, nb + 1), np.int64), np.zeros((2, nb + 1), np.float64)
    for k, m in enumerate((pos, ~pos)):
        np.add.at(cnt[k], idx[m], 1)
        np.add.at(ws[k], idx[m], w[m])
    f = v[np.isfinite(v)]
    return cnt, ws, (f.size, f.sum(), (f ** 2).sum(), (f ** 3).sum(), (f ** 4).sum(), f.min(), f.max())


def _check_moments(got, ref):
    assert (got[0], got[5], got[6]) == (ref[0], ref[5], ref[6])
    assert list(got[1:5]) == pytest.approx(list(ref[1:5]), rel=1e-9, abs=1e-9)   # test_stats_kernels_gpu's


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("unit_w", [True, False])
@pytest.mark.parametrize("nb", [1025, 4097, 16384])
def test_column_stats_wide_matches_numpy(nb, unit_w, skew, binary):
    from shifu_amd.ops import stats_ops
    rng = np.random.default_rng(nb + 2 * unit_w + skew)
    bounds = [_bounds(rng, k) for k in (10, nb, 1025)]
    V = np.stack([_values(rng, b, skew) for b in bounds])
    y = (rng.random(N) < 0.3).astype(np.float32)
    w = np.ones(N) if unit_w else rng.integers(1, 257, N) / 64.0
    pos = y > 0.5 if binary else np.ones(N, bool)
    vals, yt, wt = torch.as_tensor(V).cuda(), torch.as_tensor(y).cuda(), torch.as_tensor(w).cuda()
    blist = [list(b) for b in bounds]
    single = stats_ops.column_stats(vals, yt, wt, blist, binary, THR)
    (cnt, ws, mom, boff), = stats_ops.column_stats_multi([vals], yt, wt, [blist], binary, THR)
    alone = stats_ops.column_stats(vals[:1], yt, wt, blist[:1], binary, THR)[0]
    for f, b in enumerate(bounds):
        rc, rw, rm = _reference(V[f], pos, w, b)
        k = len(b) + 1
        cp, cn, wp, wn, m = single[f]
        assert np.array_equal(np.stack([cp, cn]), rc) and np.array_equal(np.stack([wp, wn]), rw), f
        assert np.array_equal(cnt[f, :k].T, rc) and np.array_equal(ws[f, :k].T, rw), f
        assert not cnt[f, k:].any() and boff[f + 1] - boff[f] == len(b)
        _check_moments(m, rm)
        _check_moments(mom[f], rm)
    for a, s in zip(alone, single[0]):                       # the narrow column is not touched by its wide neighbours
        assert np.array_equal(np.asarray(a), np.asarray(s), equal_nan=True)


def test_int16_codes_match_host_oracle():
    from shifu_amd.algos.normalize import NormPlan, tree_bin_codes, tree_bin_codes_gpu
    from shifu_amd.config.column_config import ColumnConfig
    from shifu_amd.data.reader import Column, RawTable
    rng = np.random.default_rng(7)
    n = 64 * 3 + 5
    cols, data = [], {}
    for j, nb in enumerate([300, 5000] + [10] * 67):          # + the categorical: 70 columns, two 64-column tiles
        cc = ColumnConfig({"columnNum": j, "columnName": f"n{j}", "columnType": "N"})
        cc.bin_boundary = _bounds(rng, nb)
        cc.stats["mean"], cc.stats["stdDev"] = 3.0, 500.0
        v = rng.uniform(-1100, 1100, n)
        v[:20] = rng.choice(cc.bin_boundary[1:], 20)
        v[rng.integers(0, n, 9)] = np.nan
        cols.append(cc)
        data[cc.name] = Column(cc.name, "num", v)
    cat = ColumnConfig({"columnNum": 70, "columnName": "c", "columnType": "C"})
    names = [f"k{i}" for i in range(1010)]                    # 10 values outside the 1000 categories
    cat.bin_category = names[:1000]
    cols.insert(2, cat)
    data["c"] = Column("c", "str", rng.integers(-1, 1010, n).astype(np.int32), names)   # -1: missing
    table = RawTable([c.name for c in cols], data, n)
    mc = SimpleNamespace(norm_type="ZSCALE_ONEHOT", normalize={})   # the categorical is one-hot: two launches

    ref = tree_bin_codes(None, table, cols)
    got = tree_bin_codes_gpu(None, table, cols)
    assert got is not None
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    assert ref[0].max() > 4000 and (ref[0][:, 2] == 1000).any()
    cpu = NormPlan(mc, None, cols, want_codes=True).run(table)
    gpu = NormPlan(mc, None, cols, want_codes=True, device="cuda").run(table)
    plain = NormPlan(mc, None, cols, want_codes=False, device="cuda").run(table)
    assert gpu["codes"].dtype == np.int16 and np.array_equal(gpu["codes"], cpu["codes"])
    assert np.array_equal(gpu["codes"], ref[0])
    assert np.array_equal(gpu["X"], plain["X"]) and gpu["X"].shape == (n, 69 + 1001)
