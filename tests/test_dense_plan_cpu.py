"""dino_amd/dense_plan.py: the device-free half of the pixel-resolution modes -- the mode table, the one frame-layout check and the
plans -- as plain functions, and the same decisions through ``predict_dense`` / ``validation_step_dense`` of a model without a GPU."""
import itertools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, capi
from dino_amd.dense_plan import dense_mode, frame_layout, guide_plan, label_size, multiscale_plan, out_size, window_plan

GUIDED_MSG = "guided cannot be combined with window or scales"
WINDOW_MSG = "window and scales cannot be combined"
TABLE = list(itertools.product((None, (1.0,)), (None, 32), (None, True, {"radius": 1})))


def expected(scales, window, guided):
    """(kind, None) or (None, message): guided with anything comes first, then window with scales."""
    if guided is not None:
        return (None, GUIDED_MSG) if (window is not None or scales is not None) else ("guided", None)
    if window is not None:
        return (None, WINDOW_MSG) if scales is not None else ("windows", None)
    return ("multiscale" if scales is not None else "bilinear"), None


class Reached(Exception):
    pass


@pytest.fixture(scope="module")
def model():
    """A CPU model whose dispatcher reports the mode it was handed instead of running it (no device is ever asked for)."""
    m = DINOSeg(head="linear", n_blocks=1)
    m.set_resolution(64)
    m._require_gpu = lambda: None

    def spy(x, mode, size, **kw):
        raise Reached(mode.kind)
    m._segment_mode = spy
    return m


@pytest.mark.parametrize("scales,window,guided", TABLE)
def test_mode_table(model, scales, window, guided):
    kind, msg = expected(scales, window, guided)
    img = np.zeros((64, 64, 3), np.uint8)
    batch = (torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64, dtype=torch.long))
    calls = (lambda: dense_mode(scales, False, window, None, guided),
             lambda: model.predict_dense(img, scales=scales, window=window, guided=guided),
             lambda: model.validation_step_dense(batch, scales=scales, window=window, guided=guided))
    if msg is not None:
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == msg
        return
    mode = calls[0]()
    assert mode.kind == kind
    assert mode.args == {"bilinear": (), "multiscale": ((1.0,), False), "windows": (32, None), "guided": (1 if guided is not True else 2, 1.0, 0.1)}[kind]
    for call in calls[1:]:
        with pytest.raises(Reached) as e:
            call()
        assert str(e.value) == kind


def test_mode_record_is_immutable_and_checks_guided_once():
    with pytest.raises(AttributeError):
        dense_mode().kind = "windows"
    with pytest.raises(ValueError, match="radius must be an integer in 0..3"):
        dense_mode(guided={"radius": 7})
    with pytest.raises(ValueError, match="guided must be True or a dict"):
        dense_mode(guided=False)
    with pytest.raises(ValueError) as e:                 # guided outranks the window / scales pair, and its own parameters
        dense_mode(scales=(1.0,), window=32, guided={"radius": 7})
    assert str(e.value) == GUIDED_MSG


def test_frame_layout():
    u8, f32 = torch.zeros(2, 240, 320, 3, dtype=torch.uint8), torch.zeros(1, 3, 64, 128, dtype=torch.float64)
    for patch in (8, 16):
        assert frame_layout(u8, patch, multiple=True, one_patch=True, non_empty=True) == (capi.INPUT_U8_HWC, 2, 240, 320)
        assert frame_layout(f32, patch, multiple=True, one_patch=True, non_empty=True) == (capi.INPUT_F32_CHW, 1, 64, 128)
        for bad in (torch.zeros(1, 3, 240, 324), torch.zeros(1, 244, 320, 3, dtype=torch.uint8)):
            assert frame_layout(bad, patch, one_patch=True, non_empty=True)[1] == 1          # (any size without the switch)
            with pytest.raises(ValueError) as e:
                frame_layout(bad, patch, multiple=True)
            assert str(e.value) == f"Resolution should be a multiple of {patch}."
        small = torch.zeros(1, patch - 1, 4 * patch, 3, dtype=torch.uint8)
        assert frame_layout(small, patch) == (capi.INPUT_U8_HWC, 1, patch - 1, 4 * patch)
        with pytest.raises(ValueError) as e:
            frame_layout(small, patch, one_patch=True)
        assert str(e.value) == f"Resolution should be a multiple of {patch}."
    # the two layouts' own messages: a 3-D tensor, a wrong channel axis
    for bad, msg in ((torch.zeros(70, 100, 3, dtype=torch.uint8), "expected uint8 [B,H,W,3], got (70, 100, 3)"),
                     (torch.zeros(1, 3, 64, 96, dtype=torch.uint8), "expected uint8 [B,H,W,3], got (1, 3, 64, 96)"),
                     (torch.zeros(3, 64, 96), "expected [B,3,H,W], got (3, 64, 96)"),
                     (torch.zeros(1, 64, 96, 3), "expected [B,3,H,W], got (1, 64, 96, 3)")):
        with pytest.raises(ValueError) as e:
            frame_layout(bad, 8)
        assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        frame_layout(torch.zeros(1, 3, 64, 96), 8, u8_only=True)
    assert str(e.value) == "expected uint8 [B,H,W,3], got torch.float32 (1, 3, 64, 96)"
    empty = torch.zeros(0, 64, 96, 3, dtype=torch.uint8)
    assert frame_layout(empty, 8, multiple=True, one_patch=True) == (capi.INPUT_U8_HWC, 0, 64, 96)
    with pytest.raises(ValueError) as e:
        frame_layout(empty, 8, non_empty=True)
    assert str(e.value) == "empty batch"


def test_label_and_output_sizes():
    y = torch.zeros(2, 70, 100, dtype=torch.long)
    assert label_size(y, 2) == (70, 100) and label_size(y, 2, own=(70, 100)) == (70, 100)
    for bad, own, msg in ((y, None, "expected pixel labels [B=3, OH, OW], got (2, 70, 100)"),
                          (y[0], None, "expected pixel labels [B=3, OH, OW], got (70, 100)"),
                          (y, (64, 96), "expected pixel labels [B=3, 64, 96] (the frames' own size), got (2, 70, 100)")):
        with pytest.raises(ValueError) as e:
            label_size(bad, 3, own)
        assert str(e.value) == msg
    with pytest.raises(ValueError, match=r"\[B=2, 64, 96\] \(the frames' own size\)"):
        label_size(y, 2, own=(64, 96))
    assert out_size(None, (70, 100)) == (70, 100) and out_size([np.int64(10), 96.0], (70, 100)) == (10, 96)


def raised(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_plans_need_no_model_and_are_the_models():
    """The cases of test_window_cpu / test_guided_cpu / test_ensemble_cpu: the plan functions give, and refuse with the texts of,
    what the public methods of a model without a GPU give."""
    m = DINOSeg(head="linear", n_blocks=1)
    u8 = torch.zeros(1, 70, 100, 3, dtype=torch.uint8)
    assert window_plan(8, 70, 100, (32, 48), (24, 40)) == ((32, 48), (24, 40), (3, 3))
    assert window_plan(8, 70, 100, 480, None) == ((64, 96), (42, 64), (2, 2))        # clamped per axis, stride (2 w) // 3
    assert window_plan(16, 70, 100, 64, 48) == ((64, 64), (48, 48), (2, 2))
    text = raised(lambda: window_plan(8, 70, 100, 64, (1, 64)))
    assert text.startswith("vertical coverage 7: window 64 at stride 1 puts 7 windows over one pixel row (at most 4 per axis)")
    assert raised(lambda: m.segment_windows(u8, window=64, stride=(1, 64))) == text
    for window, stride in ((36, None), ((0, 48), None), (32, (0, 8)), (64, (64, 4))):
        assert raised(lambda: window_plan(8, 70, 100, window, stride)) == raised(lambda: m.segment_windows(u8, window, stride))
    assert raised(lambda: window_plan(8, 7, 100, 32, None)) == "frames of 7x100 are smaller than one 8x8 patch"

    u8 = torch.zeros(1, 64, 96, 3, dtype=torch.uint8)
    views, K, size = multiscale_plan(8, 64, 96, (0.5, 1.0), True, None)
    assert (views, K, size) == ([(32, 48, 0), (32, 48, 1), (64, 96, 0), (64, 96, 1)], 4, (64, 96))
    assert multiscale_plan(16, 64, 96, (1.5,), False, (75, 101)) == ([(96, 144, 0)], 1, (75, 101))
    thirteen = tuple(1.0 + 0.125 * i for i in range(13))
    text = raised(lambda: multiscale_plan(8, 64, 96, thirteen, False, None))
    assert text == "13 scales are 13 views; the ensemble takes 1 to 12"
    assert raised(lambda: m.segment_multiscale(u8, scales=thirteen, flip=False)) == text
    text = raised(lambda: multiscale_plan(8, 64, 96, (1.0, 1.5), True, (10, 96)))
    assert text.startswith("the 96x144 view's grid 12x18 exceeds the output size 10x96")
    assert raised(lambda: m.segment_multiscale(u8, scales=(1.0, 1.5), size=(10, 96))) == text
    assert raised(lambda: multiscale_plan(8, 64, 96, (1.0, -0.5), False, None)) == "scales must be positive, got (1.0, -0.5)"

    u8, f32 = torch.zeros(2, 64, 96, 3, dtype=torch.uint8), torch.zeros(2, 3, 64, 96)
    guide = torch.zeros(2, 100, 131, 3, dtype=torch.uint8)
    assert guide_plan(8, u8, None, None) == (capi.INPUT_U8_HWC, 2, 64, 96, 64, 96)
    assert guide_plan(8, u8, None, (100, 131)) == (capi.INPUT_U8_HWC, 2, 64, 96, 100, 131)
    assert guide_plan(16, f32, guide, None) == (capi.INPUT_F32_CHW, 2, 64, 96, 100, 131)
    for x, g, size in ((f32, None, None), (u8, guide.float(), None), (u8, guide[:1], None), (u8, guide, (64, 96)), (u8, None, (7, 12)),
                       (torch.zeros(1, 70, 96, 3, dtype=torch.uint8), None, None)):
        assert raised(lambda: guide_plan(8, x, g, size)) == raised(lambda: m.segment_guided(x, guide=g, size=size))
    assert raised(lambda: guide_plan(8, u8, None, (7, 12))) == "size (7, 12) is smaller than the patch grid (8, 12)"
