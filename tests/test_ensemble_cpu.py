"""CPU tests of the multi-scale + flip ensemble: the view sizes of a protocol, the stated per-pixel rule (include/dinoseg.h,
dinoseg_op_upsample_ensemble) restated in fp64 numpy against torch's own bilinear + softmax, the host-side refusals of the op, and
the class methods without a device."""
import ctypes

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, capi

from .ensemble_util import CASES, IDS, case_data
from .test_dense_cpu import axis_table

SIX = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def test_view_sizes():
    assert dino_amd.view_sizes(480, 640, SIX, 8) == [(240, 320), (360, 480), (480, 640), (600, 800), (720, 960), (840, 1120)]
    assert dino_amd.view_sizes(480, 640, SIX, 16) == [(240, 320), (368, 480), (480, 640), (608, 800), (720, 960), (848, 1120)]
    # rounding to the nearest patch count, halves up: 100 * 0.5 / 8 = 6.25 -> 6, 104 * 0.5 / 8 = 6.5 -> 7, 100 * 0.75 / 8 = 9.375 -> 9,
    # 104 * 0.75 / 8 = 9.75 -> 10; 88 * 0.5 / 8 = 5.5 -> 6, 24 * 0.5 / 8 = 1.5 -> 2; 72 * 0.75 / 16 = 3.375 -> 3, 40 * 0.75 / 16 = 1.875 -> 2
    assert dino_amd.view_sizes(100, 104, (0.5, 0.75), 8) == [(48, 56), (72, 80)]
    assert dino_amd.view_sizes(88, 24, (0.5,), 8) == [(48, 16)]
    assert dino_amd.view_sizes(72, 40, (0.75, 0.5), 16) == [(48, 32), (32, 16)]
    # never below one patch
    assert dino_amd.view_sizes(8, 16, (0.1, 0.01), 8) == [(8, 8), (8, 8)]
    assert dino_amd.view_sizes(64, 64, (0.05,), 16) == [(16, 16)]
    assert dino_amd.view_sizes(64, 96, (), 8) == []


def restated(case, logps):
    """The rule as the header states it, in fp64: integer coordinates, the mirrored taps wp-1-i0 / wp-1-i1 with the same lambda,
    x before y, the softmax of each view, the sum in view order, / K."""
    B, C, OH, OW, views = case
    acc = np.zeros((B, C, OH, OW))
    for (hp, wp, flip), lp in zip(views, logps):
        v = lp.numpy().astype(np.float64).reshape(B, hp, wp, C).transpose(0, 3, 1, 2)
        x0, x1, rx, dx = axis_table(wp, OW)
        y0, y1, ry, dy = axis_table(hp, OH)
        if flip:
            x0, x1 = wp - 1 - x0, wp - 1 - x1
        lx, ly = rx / float(dx), ry / float(dy)
        a, b = v[:, :, :, x0], v[:, :, :, x1]
        h = a + (b - a) * lx
        a, b = h[:, :, y0, :], h[:, :, y1, :]
        u = a + (b - a) * ly[:, None]
        m = u.max(1, keepdims=True)
        lse = m + np.log(np.exp(u - m).sum(1, keepdims=True))
        acc += np.exp(u - lse)
    return acc / len(views)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_stated_rule_is_torch_interpolate_softmax_mean(i):
    logps, ref = case_data(i)
    got = restated(CASES[i], logps)
    assert got.shape == tuple(ref.shape)
    assert float(np.abs(got - ref.numpy()).max()) <= 1e-12


def call(lib, ptrs, hp, wp, flip, K, B, C, OH, OW, labels, conf, probs, scratch):
    n = max(len(ptrs), 1)
    return lib.dinoseg_op_upsample_ensemble((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int32 * n)(*hp), (ctypes.c_int32 * n)(*wp),
                                            (ctypes.c_int32 * n)(*flip), K, B, C, OH, OW, labels, conf, probs, scratch, None)


def test_ensemble_op_refuses_bad_arguments_without_gpu():
    """Every refusal happens on the host (-1 and a message) before anything is enqueued; the fake pointers are never dereferenced."""
    lib = capi.lib()
    fake = 256
    two = dict(ptrs=[fake, fake], hp=[4, 8], wp=[4, 8], flip=[0, 1])
    ok = dict(K=2, B=1, C=7, OH=32, OW=32, labels=fake, conf=None, probs=None, scratch=fake)

    def refused(msg, **change):
        args = {**two, **ok, **change}
        assert call(lib, **args) == -1
        assert msg in capi.last_error(), capi.last_error()

    refused("dinoseg_op_upsample_ensemble: 0 views (1 <= K <= 12)", K=0)
    refused("dinoseg_op_upsample_ensemble: 13 views (1 <= K <= 12)", K=13, ptrs=[fake] * 13, hp=[4] * 13, wp=[4] * 13, flip=[0] * 13)
    assert lib.dinoseg_op_upsample_ensemble(None, None, None, None, 2, 1, 7, 32, 32, fake, None, None, fake, None) == -1
    assert "null view table" in capi.last_error()
    refused("upsample_ensemble: view 1: null pointer", ptrs=[fake, None])
    refused("upsample_ensemble: view 0: flip is 2 (0 or 1)", flip=[2, 0])
    refused("upsample_ensemble: view 1: flip is -1 (0 or 1)", flip=[0, -1])
    refused("upsample_ensemble: view 1: output 7x32 is smaller than the input grid 8x8", OH=7)
    refused("upsample_ensemble: view 1: output 32x7 is smaller than the input grid 8x8", OW=7)
    refused("upsample_ensemble: view 0: output 3x32 is smaller than the input grid 4x4", OH=3)
    for C in (0, 257):
        refused("upsample_ensemble: view 0: bad argument (B=1 hp=4 wp=4 C=%d OH=32 OW=32" % C, C=C)
    refused("upsample_ensemble: view 0: bad argument", B=0)
    refused("upsample_ensemble: view 1: bad argument", hp=[4, 0])
    refused("upsample_ensemble: null pointer (at least one of labels / conf / probs is required)", labels=None)
    refused("upsample_ensemble: null scratch", scratch=None)
    refused("upsample_ensemble: view 0: output 8388608x32 (B=1) is too large", OH=1 << 23)
    # any single output is enough to pass the argument checks: the next refusal is the missing device's, not the host's
    for outs in (dict(labels=None, conf=fake), dict(labels=None, probs=fake)):
        args = {**two, **ok, **outs, "ptrs": [fake, None]}
        assert call(lib, **args) == -1 and "view 1: null pointer" in capi.last_error()

    size = lib.dinoseg_op_upsample_ensemble_scratch_bytes
    assert size(12, 2, 96, 136) == 4 * 12 * 2 * 96 * 136
    assert size(1, 1, 1, 1) == 4
    assert size(12, 32, 2048, 2048) == 4 * 12 * 32 * 2048 * 2048           # beyond 2^31: the size is 64-bit
    for bad in ((0, 1, 8, 8), (13, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -1)):
        assert size(*bad) == -1


def test_ensemble_methods_have_no_cpu_path_and_check_their_views_first():
    m = DINOSeg(head="linear", n_blocks=1)
    assert m.device.type == "cpu"
    u8 = torch.zeros(1, 64, 96, 3, dtype=torch.uint8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_multiscale(u8)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment_multiscale(torch.zeros(1, 3, 64, 96), scales=(1.0,), flip=False, size=(75, 101), want_conf=True, want_probs=True)
    # more than 12 views, and a view whose grid exceeds the output: ValueError before any forward (so also without a device)
    with pytest.raises(ValueError, match="14 views"):
        m.segment_multiscale(u8, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0))
    with pytest.raises(ValueError, match="13 views"):
        m.segment_multiscale(u8, scales=tuple(1.0 + 0.125 * i for i in range(13)), flip=False)
    with pytest.raises(ValueError, match="0 views"):
        m.segment_multiscale(u8, scales=())
    with pytest.raises(ValueError, match="grid 12x18 exceeds the output size 10x96"):
        m.segment_multiscale(u8, scales=(1.0, 1.5), size=(10, 96))
    with pytest.raises(ValueError, match="exceeds the output size 64x10"):
        m.segment_multiscale(u8, scales=(1.0,), flip=False, size=(64, 10))
    with pytest.raises(ValueError, match="multiple of 8"):
        m.segment_multiscale(torch.zeros(1, 60, 96, 3, dtype=torch.uint8))
    m.set_resolution(64)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict_dense(np.zeros((100, 131, 3), np.uint8), scales=(0.5, 1.0), flip=True)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.validation_step_dense((u8, torch.zeros(1, 64, 96, dtype=torch.long)), scales=(0.5, 1.0), flip=True)
