"""Connected components without a device: the host restatement (tests/components_util.py) against a naive flood fill and against
scipy.ndimage.label, components_plan's refusals, and DINOSeg.discover's composition on planted cell maps."""
import sys

import numpy as np
import pytest
import torch

from dino_amd import capi
from dino_amd import dense_plan as P
from tests import components_util as CU


def same_partition(a, b):
    """two id maps describe the same partition (and the same void set)"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if not np.array_equal(a < 0, b < 0):
        return False
    live = a >= 0
    pairs = np.unique(np.stack([a[live], b[live]]), axis=1)
    return pairs.shape[1] == np.unique(a[live]).size == np.unique(b[live]).size


def check_table(lab, out, b, M, ignore):
    """the table of frame b from its ids alone"""
    ids, count = out["ids"][b], int(out["count"][b])
    H, W = ids.shape
    assert count == (ids.max() + 1 if (ids >= 0).any() else 0)
    firsts = []
    for k in range(min(count, M)):
        ys, xs = np.nonzero(ids == k)
        first = int((ys * W + xs).min())
        firsts.append(first)
        assert out["first"][b, k] == first and out["label"][b, k] == lab.reshape(-1)[first] and out["area"][b, k] == ys.size
        assert tuple(out["box"][b, k]) == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
        assert np.all(lab[ys, xs] == lab.reshape(-1)[first])
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)
    k = min(count, M)
    assert np.all(out["first"][b, k:] == -1) and np.all(out["label"][b, k:] == -1)
    assert not out["area"][b, k:].any() and not out["box"][b, k:].any()
    assert np.array_equal(ids < 0, CU.void_of(lab, ignore))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("classes", [2, 3, 4])
def test_restatement_against_a_naive_flood_fill(connectivity, classes):
    for t, (H, W) in enumerate([(1, 1), (1, 9), (6, 1), (7, 11), (12, 12), (9, 20)]):
        lab = CU.random_map(100 * classes + t, H, W, classes=classes, void=0.15 if t % 2 else 0.0)
        ignore = classes - 1 if t % 3 == 0 else -1
        for M in (1, 5, 400):
            out = CU.components_host(lab[None], connectivity, ignore, M)
            ids, count = CU.flood_fill(lab, connectivity, ignore)
            assert count == out["count"][0]
            assert np.array_equal(ids, out["ids"][0])                   # (the fill visits first pixels in raster order: the same numbers)
            check_table(lab, out, 0, M, ignore)


def test_first_pixels_ascend_and_frames_do_not_interact():
    a, b = CU.random_map(1, 10, 14, p=0.59), CU.checkerboard(10, 14)
    both = CU.components_host(np.stack([a, b, a[:, ::-1]]), 8, -1, 64)
    for f, lab in enumerate((a, b, a[:, ::-1])):
        one = CU.components_host(lab[None], 8, -1, 64)
        for k in CU.FIELDS:
            assert np.array_equal(both[k][f], one[k][0]), k
        n = min(int(one["count"][0]), 64)
        assert np.all(np.diff(one["first"][0, :n]) > 0)
    assert both["count"][0] == both["count"][2] and both["count"][1] == 2
    assert CU.components_host(b[None], 4, -1, 8)["count"][0] == b.size


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_against_scipy_label_per_class(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for seed, classes in ((5, 2), (6, 3), (7, 4)):
        lab = CU.random_map(seed, 23, 31, classes=classes, void=0.1)
        out = CU.components_host(lab[None], connectivity, -1, 1024)
        want = np.full(lab.shape, -1, dtype=np.int64)
        total = 0
        for c in range(classes):
            l, n = ndimage.label(lab == c, structure=structure)
            want[l > 0] = l[l > 0] - 1 + total
            total += n
        assert total == out["count"][0]
        assert same_partition(want, out["ids"][0])


def test_components_plan_refuses_before_the_native_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("components_plan must not load the native library")
    monkeypatch.setattr(capi, "lib", no_lib)
    good = torch.zeros((2, 5, 7), dtype=torch.int32)
    plan = P.components_plan(good)
    assert plan == P.ComponentsPlan(2, 5, 7, 4, -1, 256, False)
    assert P.components_plan(torch.zeros((5, 7), dtype=torch.uint8), 8, 3, 9) == P.ComponentsPlan(1, 5, 7, 8, 3, 9, True)
    for dt in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        assert P.components_plan(torch.zeros((1, 2, 2), dtype=dt)).B == 1
    assert P.COMPONENTS_MAX_SIDE == 8192 and P.COMPONENTS_MAX_OBJECTS == 1 << 20
    wide = torch.zeros((1, 1, 1), dtype=torch.int8)
    bad = [
        dict(labels=np.zeros((2, 2), dtype=np.int32)), dict(labels=torch.zeros((1, 2, 2))), dict(labels=torch.zeros((1, 2, 2), dtype=torch.float16)),
        dict(labels=torch.zeros((4,), dtype=torch.int32)), dict(labels=torch.zeros((1, 1, 2, 2), dtype=torch.int32)),
        dict(labels=torch.zeros((0, 2, 2), dtype=torch.int32)), dict(labels=torch.zeros((1, 0, 2), dtype=torch.int32)),
        dict(labels=torch.zeros((1, 2, 0), dtype=torch.int32)),
        dict(labels=wide.expand(1, 8193, 1)), dict(labels=wide.expand(1, 1, 8193)), dict(labels=wide.expand(32, 8192, 8192)),
        dict(connectivity=6), dict(connectivity=0), dict(connectivity=True), dict(connectivity=4.0), dict(connectivity="8"),
        dict(ignore=1 << 31), dict(ignore=-(1 << 31) - 1), dict(ignore=0.5), dict(ignore=True),
        dict(max_objects=0), dict(max_objects=-1), dict(max_objects=(1 << 20) + 1), dict(max_objects=2.0), dict(max_objects=None),
    ]
    for kw in bad:
        args = dict(labels=good)
        args.update(kw)
        with pytest.raises(ValueError):
            P.components_plan(**args)
    assert P.components_plan(wide.expand(31, 8192, 8192)).B == 31      # 2^31 - 2^26 pixels: the largest batch of the largest frame
    assert P.components_plan(good, max_objects=1 << 20).max_objects == 1 << 20
    assert P.components_plan(good, ignore=-(1 << 31)).ignore == -(1 << 31)


def planted_cells(hp=9, wp=12):
    """two blobs: a 4 x 5 one and a 2 x 2 one, three background cells apart"""
    fg = np.zeros((hp, wp), dtype=np.uint8)
    fg[1:5, 1:6] = 1
    fg[6:8, 9:11] = 1
    return fg


def test_discover_composition_on_planted_cell_maps():
    hp, wp, p = 9, 12, 8
    fg = planted_cells(hp, wp)
    g = np.random.default_rng(3)
    margin = np.where(fg.reshape(-1) > 0, 1.0, -1.0).astype(np.float32) * (0.1 + g.random(hp * wp).astype(np.float32))
    small = 6 * wp + 9
    out = CU.discover_host(margin[None], fg.reshape(1, -1), [small], hp, wp, p)
    want = np.zeros((hp, wp), dtype=np.uint8)
    want[6:8, 9:11] = 1
    assert np.array_equal(out["cells"][0].reshape(hp, wp), want)
    assert tuple(out["box"][0]) == (9 * p, 6 * p, 11 * p, 8 * p) and out["area"][0] == 4 and out["found"][0] == 1
    assert np.array_equal(out["grid_labels"][0].reshape(hp, wp), want.astype(np.int32))
    assert np.all(out["margin"][0][want.reshape(-1) == 0] < 0) and np.array_equal(np.abs(out["margin"][0]), np.abs(margin))
    big = CU.discover_host(margin[None], fg.reshape(1, -1), [2 * wp + 3], hp, wp, p)
    assert big["area"][0] == 20 and tuple(big["box"][0]) == (1 * p, 1 * p, 6 * p, 5 * p)
    # a seed on a background cell
    none = CU.discover_host(margin[None], fg.reshape(1, -1), [0], hp, wp, p)
    assert none["found"][0] == 0 and not none["cells"].any() and not none["box"].any() and none["area"][0] == 0
    assert not none["grid_labels"].any()
    # a blob joined only diagonally splits at connectivity 4 and holds at 8
    diag = np.zeros((hp, wp), dtype=np.uint8)
    diag[1:3, 1:3] = 1
    diag[3:5, 3:6] = 1
    m2 = np.where(diag.reshape(-1) > 0, 0.5, -0.5).astype(np.float32)
    four = CU.discover_host(m2[None], diag.reshape(1, -1), [1 * wp + 1], hp, wp, p, 4)
    eight = CU.discover_host(m2[None], diag.reshape(1, -1), [1 * wp + 1], hp, wp, p, 8)
    assert four["area"][0] == 4 and tuple(four["box"][0]) == (p, p, 3 * p, 3 * p)
    assert eight["area"][0] == 10 and tuple(eight["box"][0]) == (p, p, 6 * p, 5 * p)
    assert np.array_equal(eight["cells"][0].reshape(hp, wp), diag)


def test_signatures_mirror_the_header_with_the_new_entries():
    names = capi.header_symbols()
    assert "dinoseg_op_components" in names and "dinoseg_components_scratch_bytes" in names
    assert sorted(capi.SIGNATURES) == names
    assert len(capi.SIGNATURES["dinoseg_op_components"][1]) == 16 and capi.SIGNATURES["dinoseg_components_scratch_bytes"][0] is capi._i64
    assert "dino_amd.capi" in sys.modules
