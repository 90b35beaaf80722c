"""The image-guided upsample without a device: the fp64 restatement of the rule (tests/guided_util.py) against an independent plain-loop
joint bilateral upsample, the edge-following property the feature exists for, and every refusal of the Python methods and of the C
entries that happens before any device use."""
import math

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, capi
from dino_amd.dinoseg import guided_params
from tests import guided_util as G

FAKE = 256      # never dereferenced: every call below is refused on the host


@pytest.mark.parametrize("shape", [(1, 3, 4, 3, 13, 17, 1), (1, 3, 4, 3, 13, 17, 3), (1, 1, 1, 3, 8, 8, 1), (1, 1, 1, 3, 8, 8, 3)])
def test_restatement_matches_plain_loop_joint_bilateral_upsample(shape):
    B, hp, wp, C, OH, OW, R = shape
    rng = np.random.default_rng(11)
    logp = G.make_logp(rng, B, hp, wp, C)
    for guide in G.make_guides(rng, B, OH, OW):
        got = G.guided_ref(logp, guide, hp, wp, R, 1.0, 0.1)
        want = G.jbu_plain(logp, guide, hp, wp, R, 1.0, 0.1)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"restatement vs plain loops {shape}: {err:.3e} relative")
        assert err <= 1e-12


def test_restatement_cell_colours_are_the_rounded_means():
    rng = np.random.default_rng(12)
    guide = rng.integers(0, 256, size=(2, 13, 17, 3), dtype=np.uint8)
    col = G.cell_colours(guide, 3, 4)
    for b in range(2):
        for r in range(3):
            for c in range(4):
                ys = [y for y in range(13) if (y * 3) // 13 == r]
                xs = [x for x in range(17) if (x * 4) // 17 == c]
                px = guide[b][np.ix_(ys, xs)].reshape(-1, 3).astype(np.int64)
                assert col[b, r, c].tolist() == [int(math.floor(v.sum() / len(px) + 0.5)) for v in px.T]
    packed = G.pack_cells(col)
    assert packed.dtype == np.uint32 and int(packed[1, 2, 3]) == int(col[1, 2, 3, 0] | col[1, 2, 3, 1] << 8 | col[1, 2, 3, 2] << 16)


def test_restatement_radius_zero_is_nearest_and_constant_guide_is_gaussian():
    rng = np.random.default_rng(13)
    logp = G.make_logp(rng, 1, 3, 4, 5)
    guide = rng.integers(0, 256, size=(1, 13, 17, 3), dtype=np.uint8)
    near = G.nearest_ref(logp.astype(np.float64), 3, 4, 13, 17)
    assert np.abs(G.guided_ref(logp, guide, 3, 4, 0, 1.0, 0.1) - near).max() <= 1e-14
    flat = np.full((1, 13, 17, 3), 77, dtype=np.uint8)
    a = G.guided_ref(logp, flat, 3, 4, 2, 1.0, 0.1)
    b = G.guided_ref(logp, flat, 3, 4, 2, 1.0, 50.0)        # no colour differences: the range sigma has nothing to act on
    assert np.array_equal(a, b)


@pytest.mark.parametrize("vertical", [True, False])
@pytest.mark.parametrize("e", [19, 21, 24, 29])
def test_labels_follow_the_guides_edge_not_the_patch_grid(e, vertical):
    """4 x 6 cells, 32 x 48 pixels, two classes: the labels equal the guide's edge at EVERY pixel for R = 1, 2, 3 at the default sigmas
    (smallest top-2 margin in fp64: 2.0), where the bilinear enlargement puts the boundary half-way between two cell centres."""
    logp, guide, want, hp, wp = G.edge_case(e, vertical)
    for R in (1, 2, 3):
        dense = G.guided_ref(logp, guide, hp, wp, R, 1.0, 0.1)
        lab, margin = G.first_argmax_and_margin(dense)
        print(f"edge {e} {'vertical' if vertical else 'horizontal'} R={R}: smallest margin {margin.min():.3f}")
        assert np.array_equal(lab, want)
        assert margin.min() >= 1.0
    # the contrast: the bilinear enlargement of the same log-probs (torch's, align_corners=False) misplaces the boundary unless the
    # edge lies half-way between two cell centres
    up = torch.nn.functional.interpolate(torch.from_numpy(logp.reshape(1, hp, wp, 2)).permute(0, 3, 1, 2), size=want.shape[1:],
                                         mode="bilinear", align_corners=False).argmax(1).numpy()
    wrong = int((up != want).sum())
    if e == 21:
        assert wrong == 96          # the boundary sits at column (row) 24: 3 columns x 32 rows
    assert (wrong == 0) == (e == 24)


def test_guided_params_ranges():
    assert guided_params(True) == (2, 1.0, 0.1)
    assert guided_params({"radius": 3, "sigma_range": 0.02}) == (3, 1.0, 0.02)
    for bad in (4, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="radius must be an integer in 0..3"):
            guided_params({"radius": bad})
    for bad in (0.0, -1.0, float("nan"), float("inf"), 0.49, 16.5):
        with pytest.raises(ValueError, match="sigma_spatial must be in"):
            guided_params({"sigma_spatial": bad})
    for bad in (0.0, -0.1, float("nan"), float("inf"), 9e-4, 1001.0):
        with pytest.raises(ValueError, match="sigma_range must be in"):
            guided_params({"sigma_range": bad})
    with pytest.raises(ValueError, match="guided takes radius / sigma_spatial / sigma_range"):
        guided_params({"sigma": 1.0})
    with pytest.raises(ValueError, match="guided must be True or a dict"):
        guided_params(False)


def test_guided_methods_have_no_cpu_path_and_check_their_arguments_first():
    m = DINOSeg(head="linear", n_blocks=1)
    assert m.device.type == "cpu"
    u8 = torch.zeros(2, 64, 96, 3, dtype=torch.uint8)
    f32 = torch.zeros(2, 3, 64, 96)
    y = torch.zeros(2, 64, 96, dtype=torch.long)
    img = np.zeros((70, 90, 3), np.uint8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_guided(u8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_guided(f32, guide=torch.zeros(2, 100, 131, 3, dtype=torch.uint8))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict_dense(img, guided=True)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.validation_step_dense((u8, y), guided={"radius": 1})
    # ValueError before any device use
    with pytest.raises(ValueError, match="fp32 frames carry no image to guide by"):
        m.segment_guided(f32)
    with pytest.raises(ValueError, match="fp32 frames carry no image to guide by"):
        m.validation_step_dense((f32, y), guided=True)
    with pytest.raises(ValueError, match="expected a uint8 guide"):
        m.segment_guided(u8, guide=torch.zeros(2, 64, 96, 3))
    with pytest.raises(ValueError, match="expected a uint8 guide"):
        m.segment_guided(u8, guide=torch.zeros(2, 3, 64, 96, dtype=torch.uint8))
    with pytest.raises(ValueError, match="the guide has 3 frames, the batch 2"):
        m.segment_guided(u8, guide=torch.zeros(3, 64, 96, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="differs from the guide's"):
        m.segment_guided(u8, guide=torch.zeros(2, 64, 96, 3, dtype=torch.uint8), size=(100, 131))
    with pytest.raises(ValueError, match="smaller than the patch grid"):
        m.segment_guided(u8, size=(7, 12))
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8"):
        m.segment_guided(torch.zeros(1, 70, 96, 3, dtype=torch.uint8))
    for radius in (4, -1):
        with pytest.raises(ValueError, match="radius must be an integer in 0..3"):
            m.segment_guided(u8, radius=radius)
    for s in (0.0, -1.0, float("nan"), 0.4, 17.0):
        with pytest.raises(ValueError, match="sigma_spatial must be in"):
            m.segment_guided(u8, sigma_spatial=s)
    for s in (0.0, -0.1, float("nan"), 1e-4, 2e3):
        with pytest.raises(ValueError, match="sigma_range must be in"):
            m.segment_guided(u8, sigma_range=s)
    with pytest.raises(ValueError, match="guided cannot be combined with window or scales"):
        m.predict_dense(img, guided=True, window=64)
    with pytest.raises(ValueError, match="guided cannot be combined with window or scales"):
        m.predict_dense(img, guided=True, scales=(0.5, 1.0))
    with pytest.raises(ValueError, match="guided cannot be combined with window or scales"):
        m.validation_step_dense((u8, y), guided=True, window=32)
    with pytest.raises(ValueError, match="guided cannot be combined with window or scales"):
        m.validation_step_dense((u8, y), guided={"radius": 1}, scales=(1.0,))
    with pytest.raises(ValueError, match="radius must be an integer"):
        m.predict_dense(img, guided={"radius": 7})


def test_guided_entries_refuse_bad_arguments_without_gpu():
    """Every refusal of the three C entries happens on the host, before any device use, with a message naming the entry."""
    lib = capi.lib()
    cells = lambda **kw: lib.dinoseg_op_guide_cells(*[kw.get(k, v) for k, v in (("guide", FAKE), ("B", 2), ("OH", 100), ("OW", 131), ("hp", 8),
                                                                                 ("wp", 16), ("cells", FAKE), ("stream", None))])
    ups = lambda **kw: lib.dinoseg_op_upsample_guided(*[kw.get(k, v) for k, v in (
        ("logp", FAKE), ("guide", FAKE), ("cells", FAKE), ("B", 2), ("hp", 8), ("wp", 16), ("C", 33), ("OH", 100), ("OW", 131), ("radius", 2),
        ("ss", 1.0), ("sr", 0.1), ("labels", FAKE), ("dense", None), ("stream", None))])
    fwd = lambda **kw: lib.dinoseg_forward_guided_hw(*[kw.get(k, v) for k, v in (
        ("h", None), ("x", FAKE), ("kind", 0), ("B", 2), ("H", 64), ("W", 96), ("guide", FAKE), ("OH", 64), ("OW", 96), ("radius", 2), ("ss", 1.0),
        ("sr", 0.1), ("logp", FAKE), ("cells", FAKE), ("labels", FAKE), ("dense", None), ("stream", None))])

    def refused(fn, text, **kw):
        assert fn(**kw) == -1
        assert text in capi.last_error(), capi.last_error()

    refused(cells, "dinoseg_op_guide_cells: null pointer", guide=None)
    refused(cells, "dinoseg_op_guide_cells: null pointer", cells=None)
    refused(cells, "dinoseg_op_guide_cells: bad argument (B=0 ", B=0)
    refused(cells, "dinoseg_op_guide_cells: bad argument", hp=-1)
    refused(cells, "dinoseg_op_guide_cells: guide 100x131 is smaller than the cell grid 8x132", wp=132)
    refused(cells, "dinoseg_op_guide_cells: guide 1048577x131", OH=(1 << 20) + 1)
    for name in ("logp", "guide", "cells"):
        refused(ups, "dinoseg_op_upsample_guided: null pointer", **{name: None})
    refused(ups, "dinoseg_op_upsample_guided: null pointer", labels=None, dense=None)
    refused(ups, "dinoseg_op_upsample_guided: radius=4 must be in 0..3", radius=4)
    refused(ups, "dinoseg_op_upsample_guided: radius=-1 must be in 0..3", radius=-1)
    for s in (0.0, -1.0, float("nan"), float("inf"), 0.49, 16.5):
        refused(ups, "dinoseg_op_upsample_guided: sigma_spatial=", ss=s)
    for s in (0.0, -0.1, float("nan"), float("inf"), 9e-4, 1001.0):
        refused(ups, "dinoseg_op_upsample_guided: sigma_range=", sr=s)
    refused(ups, "dinoseg_op_upsample_guided: bad argument (B=2 hp=8 wp=16 C=257", C=257)
    refused(ups, "dinoseg_op_upsample_guided: bad argument", B=0)
    refused(ups, "dinoseg_op_upsample_guided: output 7x131 is smaller than the input grid 8x16", OH=7)
    refused(ups, "dinoseg_op_upsample_guided: output 1048577x131", OH=(1 << 20) + 1, hp=1)
    refused(fwd, "dinoseg_forward_guided_hw: bad argument (null handle or frames")
    refused(fwd, "dinoseg_forward_guided_hw: bad argument (null handle or frames", h=FAKE, x=None)
    refused(fwd, "dinoseg_forward_guided_hw: bad argument (null handle or frames", h=FAKE, B=0)
    for name in ("guide", "logp", "cells"):
        refused(fwd, "dinoseg_forward_guided_hw: null pointer", h=FAKE, **{name: None})
    refused(fwd, "dinoseg_forward_guided_hw: null pointer", h=FAKE, labels=None, dense=None)
