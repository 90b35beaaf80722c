"""CPU tests of sliding-window inference: the window rule against mmsegmentation's formula, the stated per-pixel rule of the merge
(include/dinoseg.h, dinoseg_op_window_merge) restated in fp64 numpy against torch's own interpolate / add / count / divide, the
host-side refusals of the two ops, and the class methods without a device."""
import ctypes

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, capi

from .test_dense_cpu import axis_table
from .window_util import CASES, IDS, case_data, mmseg_origins, windows_of


def c_origins(L, w, s, cap=None):
    lib = capi.lib()
    g = lib.dinoseg_window_origins(L, w, s, None, 0)
    if g < 0:
        return g
    cap = g if cap is None else cap
    out = (ctypes.c_int32 * max(cap, 1))()
    rc = lib.dinoseg_window_origins(L, w, s, out, cap)
    return rc if rc < 0 else list(out)[:rc]


def test_window_origins_are_mmsegs():
    assert dino_amd.window_origins(70, 32, 24) == [0, 24, 38]
    assert dino_amd.window_origins(75, 24, 16) == [0, 16, 32, 48, 51]
    assert dino_amd.window_origins(960, 480, 320) == [0, 320, 480]
    assert dino_amd.window_origins(960, 480, 480) == [0, 480]
    assert dino_amd.window_origins(43, 40, 40) == [0, 3]
    sweep = [(L, w, s) for L in (8, 9, 31, 64, 70, 100, 257) for w in (8, 16, 24, 64, 256) if w <= L
             for s in (1, 3, 7, 8, 16, 24, 63, 64, 65, 300, 2 ** 31 - 1)]
    assert any(L == w for L, w, s in sweep) and any(s > w for L, w, s in sweep) and any(s == 1 for L, w, s in sweep)
    assert any((L - w) % s != 0 for L, w, s in sweep)
    for L, w, s in sweep:
        want = mmseg_origins(L, w, s)
        assert want[0] == 0 and want[-1] == L - w and all(a <= b for a, b in zip(want, want[1:]))
        assert dino_amd.window_origins(L, w, s) == want, (L, w, s)
        assert c_origins(L, w, s) == want, (L, w, s)
    # refusals: a window larger than the frame, a stride below one, too little room
    lib = capi.lib()
    room = (ctypes.c_int32 * 8)()
    assert lib.dinoseg_window_origins(32, 40, 8, room, 8) == -1 and "window=40" in capi.last_error()
    assert lib.dinoseg_window_origins(32, 40, 8, None, 0) == -1
    assert lib.dinoseg_window_origins(64, 32, 0, room, 8) == -1 and "stride=0" in capi.last_error()
    assert lib.dinoseg_window_origins(64, 32, -3, room, 8) == -1
    assert lib.dinoseg_window_origins(64, 0, 8, room, 8) == -1
    assert lib.dinoseg_window_origins(70, 32, 24, room, 2) == -1 and "room for 2 origins, 3 needed" in capi.last_error()
    assert lib.dinoseg_window_origins(70, 32, 24, None, 3) == -1
    assert lib.dinoseg_window_origins(70, 32, 24, room, 3) == 3 and list(room)[:3] == [0, 24, 38]
    for bad in ((32, 40, 8), (64, 32, 0), (64, 0, 8)):
        with pytest.raises(ValueError, match="bad window rule"):
            dino_amd.window_origins(*bad)


def restated(case, logp):
    """The rule as the header states it, in fp64: per window the integer coordinates of the window's own upsample at the local
    pixel, x before y; the sum over the covering windows in window order; / n."""
    B, C, H, W, p, (wh, ww), _ = case
    oys, oxs, hp, wp = windows_of(case)
    x0, x1, rx, dx = axis_table(wp, ww)
    y0, y1, ry, dy = axis_table(hp, wh)
    lx, ly = rx / float(dx), ry / float(dy)
    grids = logp.numpy().astype(np.float64).reshape(B, len(oys), len(oxs), hp, wp, C)
    acc, n = np.zeros((B, C, H, W)), np.zeros((H, W))
    for gy, oy in enumerate(oys):
        for gx, ox in enumerate(oxs):
            v = grids[:, gy, gx].transpose(0, 3, 1, 2)
            a, b = v[:, :, :, x0], v[:, :, :, x1]
            h = a + (b - a) * lx
            a, b = h[:, :, y0, :], h[:, :, y1, :]
            acc[:, :, oy:oy + wh, ox:ox + ww] += a + (b - a) * ly[:, None]
            n[oy:oy + wh, ox:ox + ww] += 1
    return acc / n, n


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_stated_rule_is_torch_interpolate_add_count_divide(i):
    logp, ref = case_data(i)
    got, n = restated(CASES[i], logp)
    assert got.shape == tuple(ref.shape)
    assert float(np.abs(got - ref.numpy()).max()) <= 1e-12
    assert 1 <= n.min() and n.max() <= 16
    if i == 4:
        assert n.max() == 16            # the documented maximum: four window rows times four window columns
    if i == 0:
        assert sorted(set(n.reshape(-1).astype(int).tolist())) == [1, 2, 4]       # one or two windows per axis


FAKE = 256


def merge(**kw):
    a = dict(logp=FAKE, B=1, H=96, W=136, patch=8, win_h=64, win_w=64, stride_h=40, stride_w=40, C=7, labels=FAKE, dense=None)
    a.update(kw)
    return capi.lib().dinoseg_op_window_merge(a["logp"], a["B"], a["H"], a["W"], a["patch"], a["win_h"], a["win_w"], a["stride_h"],
                                              a["stride_w"], a["C"], a["labels"], a["dense"], None)


def crop(**kw):
    a = dict(x=FAKE, kind=0, B=2, H=43, W=75, win_h=40, win_w=24, stride_h=40, stride_w=16, first=0, count=20, out=FAKE)
    a.update(kw)
    return capi.lib().dinoseg_op_crop_windows(a["x"], a["kind"], a["B"], a["H"], a["W"], a["win_h"], a["win_w"], a["stride_h"],
                                              a["stride_w"], a["first"], a["count"], a["out"], None)


def test_window_ops_refuse_bad_arguments_without_gpu():
    """Every refusal happens on the host (-1 and a message) before anything is enqueued; the fake pointers are never dereferenced."""
    def refused(fn, msg, **change):
        assert fn(**change) == -1
        assert msg in capi.last_error(), capi.last_error()

    refused(merge, "window_merge: null pointer (logp)", logp=None)
    refused(merge, "window_merge: null pointer (at least one of labels / dense is required)", labels=None)
    refused(merge, "window_merge: 0 classes (1 <= C <= 256)", C=0)
    refused(merge, "window_merge: 257 classes (1 <= C <= 256)", C=257)
    refused(merge, "window_merge: patch 12 (8 or 16)", patch=12)
    refused(merge, "window_merge: vertical window 36 is not a multiple of 8", win_h=36)
    refused(merge, "window_merge: horizontal window 36 is not a multiple of 8", win_w=36)
    refused(merge, "window_merge: horizontal window 72 is not a multiple of 16", patch=16, win_w=72)
    refused(merge, "window_merge: vertical window 104 is larger than the frame (96)", win_h=104)
    refused(merge, "window_merge: horizontal window 144 is larger than the frame (136)", win_w=144)
    refused(merge, "window_merge: vertical stride 0 (strides must be positive)", stride_h=0)
    refused(merge, "window_merge: horizontal stride -1 (strides must be positive)", stride_w=-1)
    refused(merge, "window_merge: bad argument (B=0", B=0)
    refused(merge, "window_merge: bad argument (vertical: frame 96, window 0", win_h=0)
    refused(merge, "window_merge: bad argument (horizontal: frame 0", W=0)
    # L = 160, w = 64, s = 12: pixel 60 lies in the windows at 0, 12, .., 60
    refused(merge, "window_merge: vertical coverage 6: window 64 at stride 12 puts 6 windows over one pixel row (at most 4 per axis)",
            H=160, stride_h=12)
    refused(merge, "window_merge: horizontal coverage 6: window 64 at stride 12 puts 6 windows over one pixel column", W=160, stride_w=12)
    refused(merge, "window_merge: horizontal coverage 5:", W=160, stride_w=14)
    refused(merge, "window_merge: vertical frame side 8388608 is too large", H=1 << 23)
    refused(merge, "is too large", B=1 << 30)
    # the densest accepted coverage and either single output pass the argument checks: what is left is the missing device
    for ok in (dict(H=160, W=192, stride_h=16, stride_w=16), dict(labels=None, dense=FAKE), dict(stride_h=1 << 30, stride_w=22)):
        assert merge(**ok, logp=None) == -1 and "null pointer (logp)" in capi.last_error()

    refused(crop, "crop_windows: null pointer", x=None)
    refused(crop, "crop_windows: null pointer", out=None)
    refused(crop, "crop_windows: input kind 2", kind=2)
    refused(crop, "crop_windows: bad argument (B=0", B=0)
    refused(crop, "crop_windows: bad argument (vertical: frame 43, window 0", win_h=0)
    refused(crop, "crop_windows: bad argument (horizontal: frame -1", W=-1)
    refused(crop, "crop_windows: vertical window 48 is larger than the frame (43)", win_h=48)
    refused(crop, "crop_windows: horizontal window 80 is larger than the frame (75)", win_w=80)
    refused(crop, "crop_windows: horizontal window 20 is not a multiple of 8", win_w=20)
    refused(crop, "crop_windows: vertical stride 0", stride_h=0)
    refused(crop, "crop_windows: horizontal stride 0", stride_w=0)
    # 2 frames x 2 x 5 windows
    refused(crop, "crop_windows: windows -1 .. 0 are outside the list of 20", first=-1, count=2)
    refused(crop, "crop_windows: windows 3 .. 2 are outside the list of 20", first=3, count=0)
    refused(crop, "crop_windows: windows 16 .. 20 are outside the list of 20", first=16, count=5)
    refused(crop, "crop_windows: windows 20 .. 20 are outside the list of 20", first=20, count=1)
    refused(crop, "crop_windows: the destination is not 16-byte aligned", out=FAKE + 8)


def test_window_methods_have_no_cpu_path_and_check_their_arguments_first():
    m = DINOSeg(head="linear", n_blocks=1)
    assert m.device.type == "cpu"
    u8 = torch.zeros(1, 70, 100, 3, dtype=torch.uint8)          # no multiple of the patch: fine for windows
    y = torch.zeros(1, 70, 100, dtype=torch.long)
    img = np.zeros((100, 131, 3), np.uint8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_windows(u8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_windows(torch.zeros(1, 3, 70, 100), window=(32, 48), stride=(24, 40), want_logp=True, max_windows=4)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict_dense(img, window=64)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict_dense(img, window=(64, 64), stride=32, size=(100, 131))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.validation_step_dense((u8, y), window=(32, 48), stride=(24, 40))
    # ValueError before any device use
    with pytest.raises(ValueError, match="window and scales cannot be combined"):
        m.predict_dense(img, window=64, scales=(0.5, 1.0))
    with pytest.raises(ValueError, match="window and scales cannot be combined"):
        m.validation_step_dense((u8, y), window=32, scales=(1.0,))
    with pytest.raises(ValueError, match="segmented at its own size"):
        m.predict_dense(img, window=64, size=(64, 64))
    with pytest.raises(ValueError, match="the frames' own size"):
        m.validation_step_dense((u8, torch.zeros(1, 64, 96, dtype=torch.long)), window=32)
    for call in (lambda **kw: m.segment_windows(u8, **kw), lambda **kw: m.predict_dense(img, **kw),
                 lambda **kw: m.validation_step_dense((u8, y), **kw)):
        with pytest.raises(ValueError, match="window must be positive"):
            call(window=(0, 48))
        with pytest.raises(ValueError, match="window must be positive"):
            call(window=-8)
        with pytest.raises(ValueError, match="window 36 is not a multiple of the patch"):
            call(window=36)
        with pytest.raises(ValueError, match="stride must be positive"):
            call(window=32, stride=(0, 8))
        with pytest.raises(ValueError, match=r"horizontal coverage \d+: window 64 at stride 4 puts \d+ windows over one pixel column"):
            call(window=64, stride=(64, 4))
        with pytest.raises(ValueError, match=r"vertical coverage \d+: window 64 at stride 1 "):
            call(window=64, stride=(1, 64))
    with pytest.raises(ValueError, match="vertical coverage 7: window 64 at stride 1 puts 7 windows over one pixel row"):
        m.segment_windows(u8, window=64, stride=(1, 64))        # the 70-row frame: windows at 0 .. 6, every one over row 6
    with pytest.raises(ValueError, match="horizontal coverage 6: window 64 at stride 12 puts 6 windows over one pixel column"):
        m.predict_dense(img, window=64, stride=(64, 12))        # 131 columns: column 60 lies in the windows at 0, 12, .., 60
    with pytest.raises(ValueError, match="max_windows must be positive"):
        m.segment_windows(u8, max_windows=0)
    with pytest.raises(ValueError, match="smaller than one 8x8 patch"):
        m.segment_windows(torch.zeros(1, 7, 100, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected uint8"):
        m.segment_windows(torch.zeros(70, 100, 3, dtype=torch.uint8))
