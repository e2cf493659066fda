"""Device dictionary encoder of the categorical columns of a GPU-parsed block (K0c:
ops/csrc/csv_cat_kernels.hip + data/gpu_parse.py) against the host parser on the same bytes:
same codes, same dictionary strings in the same order, same numeric bits -- through the LDS front
table (few categories, several workgroups), its spill into the HBM table (thousands of values),
the hash word boundaries, missing tokens / trimming / CRLF / blank lines, forced hash collisions
and a table that is too small (both through the per-column host fallback), and a streamed
stats + norm run with the setting on and off.
"""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from shifu_amd.data import reader as R

pytestmark = pytest.mark.gpu

KINDS = [2, 1, 2, 2, 1, 1, 2]            # categorical columns first, adjacent, last
EDGE = ["", "?", "NA", " lead", "trail ", "\t both \t", "x", "sevenby", "eightbyt", "ninebytes", "z" * 70,
        "z" * 69 + "y", "abcdefgX", "abcdefgY", "abc", "abcd", "a b"]


def _block(rows, eol="\n", trailing=True):
    """Text block from lists of cell strings ('' rows give blank lines)."""
    text = eol.join("|".join(r) for r in rows)
    return (text + eol if trailing else text).encode()


def _rows(n, values, seed, blanks=False):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(values), size=(n, len(KINDS)))
    rows = [[values[pick[i, c]] if k == 2 else f"{(i * 7 + c) % 1000 / 8:.3f}" for c, k in enumerate(KINDS)]
            for i in range(n)]
    if blanks:
        for i in range(n - 5, 0, -n // 9):
            rows.insert(i, [" \t"] if i % 2 else [])
    return rows


def _check(data, miss=("", "?", "NA"), **attrs):
    """Parse ``data`` on the device and on the host; every column must agree.  -> the parser."""
    from shifu_amd.data.gpu_parse import GpuBlockParser
    pinned = torch.empty(len(data), dtype=torch.uint8, pin_memory=True).numpy()
    pinned[:] = np.frombuffer(data, np.uint8)
    gp = GpuBlockParser(KINDS, [c for c, k in enumerate(KINDS) if k == 1], "|", list(miss), torch.device("cuda", 0))
    for k, v in attrs.items():
        setattr(gp, k, v)
    n, bad, out = gp.parse(memoryview(pinned), 4)
    n2, bad2, ref = R.parse_block(bytearray(data), "|", KINDS, list(miss), 4)
    assert (n, bad) == (n2, bad2) and n > 0
    for c, k in enumerate(KINDS):
        if k == 1:
            assert out[c][1].host().tobytes() == ref[c][1].tobytes(), f"column {c}"
        else:
            assert out[c][0] == ref[c][0] == "str" and out[c][2] == ref[c][2], f"dictionary of column {c}"
            assert np.array_equal(np.asarray(out[c][1]), ref[c][1]), f"codes of column {c}"
    assert gp.stats["cat_device_cols"] + gp.stats["cat_overflow_cols"] == KINDS.count(2)
    return gp


MANY = [f"v{i * 2654435761 % 100003:x}" for i in range(5000)]


@pytest.mark.parametrize("values,n,eol,trailing,blanks,miss", [
    (["red", "green", "blue"], 20000, "\n", True, False, ("", "?", "NA")),     # LDS table, 5 workgroups
    (MANY, 20000, "\n", True, False, ("", "?", "NA")),                         # spills into the HBM table
    (EDGE, 3000, "\n", True, True, ("", "?", "NA")),
    (EDGE, 3000, "\r\n", True, True, ("", "?", "NA")),
    (EDGE, 3000, "\n", False, False, ("?",)),                                  # '' is a dictionary value
    (EDGE, 3000, "\r\n", False, True, ()),
])
def test_encoder_equals_host_parser(values, n, eol, trailing, blanks, miss):
    gp = _check(_block(_rows(n, values, 1, blanks), eol, trailing), miss)
    assert gp.stats["cat_overflow_cols"] == 0 and gp.stats["cat_device_cols"] == KINDS.count(2)


@pytest.mark.parametrize("attrs", [{"hash_bits": 4}, {"hash_bits": 12}, {"cat_cap": 1024}])
def test_collisions_and_small_table_fall_back_exactly(attrs):
    """Masked hashes collide (5000 values in 16 / 4096 hash values) and a 1024-slot table cannot
    hold 5000 values: the flagged columns are parsed on the host, the result is still exact."""
    gp = _check(_block(_rows(20000, MANY, 2)), **attrs)
    assert gp.stats["cat_overflow_cols"] > 0


def test_streamed_stats_and_norm_same_with_device_categoricals(tmp_path, monkeypatch):
    from shifu_amd.config import environment
    from shifu_amd.data import stream as DS
    from shifu_amd.steps.base import load_dataset_cache
    from shifu_amd.steps.create import run_init
    from shifu_amd.steps.norm import run_norm
    from shifu_amd.steps.stats import run_stats
    from shifu_amd.utils.synthetic import make_model_set
    a = make_model_set(str(tmp_path), "a", "NN", n_rows=20000, n_num=12, n_cat=4)
    run_init(a)
    b = str(tmp_path / "b")
    shutil.copytree(a, b)
    made, orig = [], DS.gpu_parser
    monkeypatch.setattr(DS, "gpu_parser", lambda *args: made.append(orig(*args)) or made[-1])
    P = environment.props()
    keys = ("shifu.data.gpuParse", "shifu.data.gpuParse.categorical", "shifu.stats.streaming", "shifu.norm.streaming",
            "shifu.stats.chunkMB", "shifu.norm.chunkMB")
    old = {k: P.get(k) for k in keys}
    try:
        P.update({"shifu.data.gpuParse": "true", "shifu.stats.streaming": "true", "shifu.norm.streaming": "true",
                  "shifu.stats.chunkMB": "0.5", "shifu.norm.chunkMB": "0.5"})
        for root, mode in ((a, "false"), (b, "auto")):
            P["shifu.data.gpuParse.categorical"] = mode
            made.clear()
            run_stats(root)
            run_norm(root)
            dev_cols = sum(p.stats["cat_device_cols"] for p in made if p is not None)
            assert max(p.stats["blocks"] for p in made if p is not None) >= 3
            assert (dev_cols > 0) == (mode == "auto")
    finally:
        for k, v in old.items():
            if v is None:
                P.pop(k, None)
            else:
                P[k] = v
    ca = json.load(open(os.path.join(a, "ColumnConfig.json")))
    cb = json.load(open(os.path.join(b, "ColumnConfig.json")))
    assert ca == cb and sum(1 for c in ca if c.get("columnType") == "C") >= 4
    ma, xa = load_dataset_cache(os.path.join(a, "tmp", "NormalizedData"), mmap=False)
    mb, xb = load_dataset_cache(os.path.join(b, "tmp", "NormalizedData"), mmap=False)
    assert ma["n"] == mb["n"] > 0
    for k in xa:
        assert np.asarray(xa[k]).tobytes() == np.asarray(xb[k]).tobytes(), k
