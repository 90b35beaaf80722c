"""CPU tests of the pixel-resolution output: the two C-ABI entries refuse bad arguments on the host, the class methods fail loudly
without a device, and the integer coordinate rule the kernel implements (include/dinoseg.h, dinoseg_op_upsample_argmax) is pinned
against torch's own fp64 bilinear."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dino_amd import DINOSeg, capi

# (B, hp, wp, C, OH, OW): the shapes the GPU tests run (tests/test_dense_gpu.py)
SHAPES = [
    (2, 60, 80, 7, 480, 640),
    (2, 60, 80, 150, 480, 640),
    (1, 60, 60, 256, 480, 480),
    (2, 30, 40, 21, 480, 640),
    (2, 30, 40, 21, 479, 641),
    (2, 60, 80, 7, 375, 500),
    (2, 8, 16, 33, 100, 131),
    (1, 60, 80, 150, 1080, 1920),
    (2, 4, 4, 2, 64, 64),
    (3, 1, 1, 5, 8, 8),
]


def axis_table(i: int, o: int):
    """The stated rule for one axis: (i0, i1, lambda as an exact fraction num % den over den) per output index."""
    d = np.arange(o, dtype=np.int64)
    num = np.maximum((2 * d + 1) * i - o, 0)
    den = 2 * o
    q = num // den
    rem = num % den
    edge = q >= i - 1
    i0 = np.minimum(q, i - 1)
    i1 = np.minimum(i0 + 1, i - 1)
    rem = np.where(edge, 0, rem)
    return i0, i1, rem, den


def upsample_restated(logp: np.ndarray, B, hp, wp, C, OH, OW, dtype=np.float64) -> np.ndarray:
    """a + (b - a) lambda along x, then along y: [B, hp*wp, C] -> [B, C, OH, OW] in `dtype`."""
    v = logp.reshape(B, hp, wp, C).transpose(0, 3, 1, 2).astype(dtype)
    x0, x1, rx, dx = axis_table(wp, OW)
    y0, y1, ry, dy = axis_table(hp, OH)
    lx = (rx.astype(dtype) / dtype(dx)).astype(dtype)
    ly = (ry.astype(dtype) / dtype(dy)).astype(dtype)
    a, b = v[:, :, :, x0], v[:, :, :, x1]
    h = a + (b - a) * lx                                     # [B, C, hp, OW]
    a, b = h[:, :, y0, :], h[:, :, y1, :]
    return a + (b - a) * ly[:, None]


def reference(logp: torch.Tensor, B, hp, wp, C, OH, OW) -> torch.Tensor:
    return F.interpolate(logp.double().view(B, hp, wp, C).permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%dx%d-%dx%d" % s for s in SHAPES])
def test_integer_coordinate_rule_is_torch_bilinear(shape):
    B, hp, wp, C, OH, OW = shape
    g = torch.Generator().manual_seed(hp * 1000 + OW)
    logp = torch.log_softmax(3.0 * torch.randn(B, hp * wp, C, generator=g), dim=-1)
    got = upsample_restated(logp.numpy(), B, hp, wp, C, OH, OW)
    ref = reference(logp, B, hp, wp, C, OH, OW).numpy()
    assert got.shape == ref.shape == (B, C, OH, OW)
    assert float(np.abs(got - ref).max()) <= 1e-12


def test_identity_and_edges_of_the_rule():
    i0, i1, rem, den = axis_table(60, 60)                    # identity: every output index reads its own cell, lambda 0
    assert np.array_equal(i0, np.arange(60)) and not rem.any()
    i0, i1, rem, den = axis_table(60, 480)                   # 8x: lambda is a multiple of 1/16, clamped half cells at both edges
    assert den == 960 and not (rem % 60).any()
    assert not rem[:4].any() and not i0[:4].any() and not rem[-4:].any() and (i0[-4:] == 59).all() and (i1[-4:] == 59).all()
    assert (np.diff(i0) >= 0).all() and np.diff(i0).max() == 1
    i0, i1, rem, den = axis_table(1, 8)
    assert not i0.any() and not i1.any() and not rem.any()


def test_dense_entries_refuse_bad_arguments_without_gpu():
    """Null logp, both outputs null, C = 0 / 257, OH < hp and non-positive sizes are refused on the host (-1 and a message);
    the fake pointers are never dereferenced."""
    lib = capi.lib()
    fake = 256
    op = lib.dinoseg_op_upsample_argmax
    assert op(None, 1, 4, 4, 7, 32, 32, fake, None, None) == -1
    assert "upsample_argmax: null pointer" in capi.last_error()
    assert op(fake, 1, 4, 4, 7, 32, 32, None, None, None) == -1
    assert "upsample_argmax: null pointer" in capi.last_error()
    for C in (0, 257):
        assert op(fake, 1, 4, 4, C, 32, 32, fake, fake, None) == -1
        assert "upsample_argmax: bad argument (B=1 hp=4 wp=4 C=%d OH=32 OW=32" % C in capi.last_error()
    assert op(fake, 1, 4, 4, 7, 3, 32, fake, None, None) == -1
    assert "output 3x32 is smaller than the input grid 4x4" in capi.last_error()
    assert op(fake, 1, 4, 4, 7, 32, 3, fake, None, None) == -1
    assert "output 32x3 is smaller than the input grid 4x4" in capi.last_error()
    for bad in ((0, 4, 4, 32, 32), (1, 0, 4, 32, 32), (1, 4, -4, 32, 32), (1, 4, 4, 0, 32), (1, 4, 4, 32, -1)):
        B, hp, wp, OH, OW = bad
        assert op(fake, B, hp, wp, 7, OH, OW, fake, None, None) == -1
        assert "upsample_argmax: bad argument" in capi.last_error()

    fwd = lib.dinoseg_forward_dense_hw
    h = ctypes.c_void_p()
    cfg = capi.Config(384, 6, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.BF16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert fwd(None, fake, 0, 1, 64, 64, 64, 64, None, None, fake, None, None) == -1
        assert "dinoseg_forward_dense_hw: bad argument" in capi.last_error()
        assert fwd(h, None, 0, 1, 64, 64, 64, 64, None, None, fake, None, None) == -1
        assert "dinoseg_forward_dense_hw: bad argument" in capi.last_error()
        assert fwd(h, fake, 0, 0, 64, 64, 64, 64, None, None, fake, None, None) == -1
        assert "dinoseg_forward_dense_hw: bad argument" in capi.last_error()
        assert fwd(h, fake, 0, 1, 64, 64, 64, 64, None, None, None, None, None) == -1
        assert "at least one of labels_out / dense_out" in capi.last_error()
        assert fwd(h, fake, 0, 1, 60, 64, 64, 64, None, None, fake, None, None) == -1
        assert "Resolution should be a multiple of 8." in capi.last_error()
        for OH, OW in ((7, 64), (64, 7)):
            assert fwd(h, fake, 0, 1, 64, 64, OH, OW, None, None, fake, fake, None) == -1
            assert "dinoseg_forward_dense_hw: output %dx%d is smaller than the input grid 8x8" % (OH, OW) in capi.last_error()
        for OH, OW in ((0, 64), (64, -64)):
            assert fwd(h, fake, 0, 1, 64, 64, OH, OW, None, None, fake, fake, None) == -1
            assert "dinoseg_forward_dense_hw: bad argument (B=1 hp=8 wp=8 C=7 OH=%d OW=%d" % (OH, OW) in capi.last_error()
        assert fwd(h, fake, 0, 1, 64, 64, 1 << 23, 64, None, None, fake, None, None) == -1
        assert "dinoseg_forward_dense_hw: output 8388608x64 (B=1) is too large" in capi.last_error()
        # (a handle whose weights were never packed: the forward's own state error, after every argument check passed)
        assert fwd(h, fake, 0, 1, 64, 64, 64, 64, None, None, fake, None, None) == -3
        assert "weights not packed" in capi.last_error()
    finally:
        assert lib.dinoseg_destroy(h) == 0


def test_dense_methods_have_no_cpu_path():
    m = DINOSeg(head="linear", n_blocks=1)
    assert m.device.type == "cpu"
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.segment(torch.zeros(1, 3, 64, 64), size=(100, 131), want_logp=True)
    m.set_resolution(64)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict_dense(np.zeros((100, 131, 3), np.uint8))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.validation_step_dense((torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64, dtype=torch.long)))
