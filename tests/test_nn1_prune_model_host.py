"""tools/nn1_prune_model.py, the numpy model of which lane tiles the pruned nearest-neighbour kernel runs: at the benchmark's
shape (uniform clouds, 4096 x 4096) it keeps the share of tiles the counters show, and its cut is within 2 % of the cut with
every query's true nearest distance -- the floor of any rule that cuts per 32-query group with tile boxes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import nn1_prune_model as model  # noqa: E402


@pytest.fixture(scope="module")
def masks():
    rng = np.random.default_rng(1000)
    q, c = model.cloud("uniform", rng, 4096), model.cloud("uniform", rng, 4096)
    return model.keep_masks(q, c)


@pytest.fixture(scope="module")
def kept(masks):
    cur, true = masks
    return cur.sum(1).mean(), true.sum(1).mean(), cur.shape[1]


def test_hilbert_table_is_a_face_connected_curve():
    """(the model reads the kernel's own table) consecutive cells of the curve share a face"""
    t = model.hilbert_cells()
    u = np.stack([t & 7, (t >> 3) & 7, t >> 6], 1)
    assert np.all(np.abs(np.diff(u, axis=0)).sum(1) == 1)


def test_current_rule_keeps_the_measured_share(kept):
    cur, _, nt = kept
    print(f"current rule: {cur:.2f} of {nt} lane tiles ({cur / nt:.3f})")
    assert nt == 64 and 0.20 <= cur / nt <= 0.24   # SQ counters: 0.22 of the lane tiles run


def test_current_rule_never_below_the_true_distance_rule(masks, kept):
    """... for any wave-pass: what the true distances keep, the current rule keeps"""
    cur, true = masks
    print(f"current {kept[0]:.3f}  true-distance {kept[1]:.3f}")
    assert np.all(cur.sum(1) >= true.sum(1)) and np.all(cur | ~true)


def test_current_rule_within_two_percent_of_the_true_distance_rule(kept):
    cur, true, _ = kept
    print(f"current / true-distance = {cur / true:.4f}")
    assert cur <= 1.02 * true
