"""CPU tests of the CLS attention maps (dinoseg_op_cls_attention / dinoseg_cls_attention_hw / DINOSeg.cls_attention): the entries
exist and refuse every bad argument on the host, the Python call raises before any device use, and the integer threshold rule and
the nearest coordinates of tests/attention_util.py -- what the GPU tests hold the kernel to -- agree with the plain fp64 sort rule on
the reference's own attention rows and with torch's nearest interpolation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, capi
from tests import attention_util as U

ENTRIES = ("dinoseg_op_cls_attention", "dinoseg_cls_attention_hw")
P = ctypes.c_void_p(4096)               # a fake, aligned, never dereferenced pointer


def test_header_library_and_signatures_list_both_entries():
    syms = set(capi.header_symbols())
    lib = capi.lib()
    for s in ENTRIES + ("dinoseg_cls_attention_max_tokens",):
        assert s in syms and s in capi.SIGNATURES and hasattr(lib, s), s
    # the scores of one (frame, head) beside 128 fixed words in the CU's 160 KiB of LDS
    assert lib.dinoseg_cls_attention_max_tokens() == 160 * 1024 // 4 - 128


def op(q=P, k=P, plane=1 << 40, planes=1, B=1, heads=2, ntok=16, npad=64, hp=3, wp=5, OH=3, OW=5, thr=0.6, attn=P, keep=None):
    return capi.lib().dinoseg_op_cls_attention(q, k, plane, planes, B, heads, ntok, npad, hp, wp, OH, OW, thr, attn, keep, None)


# every refusal happens before a launch: the pointers are never dereferenced and no device is needed
OP_REFUSALS = [
    (dict(q=None), "null pointer"),
    (dict(k=None), "null pointer"),
    (dict(attn=None, keep=None), "null pointer"),
    (dict(planes=0), "planes=0 must be 1 or 2"),
    (dict(planes=3), "planes=3 must be 1 or 2"),
    (dict(B=0), "bad argument (B=0 heads=2 hp=3 wp=5"),
    (dict(ntok=15), "ntok=15 is not hp*wp + 1 (hp=3 wp=5)"),
    (dict(ntok=17), "ntok=17 is not hp*wp + 1 (hp=3 wp=5)"),
    (dict(npad=15), "npad=15 is smaller than ntok=16"),
    (dict(planes=2, plane=2 * 64 * 64 - 8), "qkv_plane=8184 puts the lo plane inside the hi plane of 8192 elements"),
    (dict(planes=2, plane=2 * 64 * 64 + 4), "off a 16-byte boundary"),
    (dict(OH=2), "output 2x5 is smaller than the patch grid 3x5"),
    (dict(OW=4), "output 3x4 is smaller than the patch grid 3x5"),
    (dict(keep=P, thr=0.0), "threshold=0 must be inside (0, 1)"),
    (dict(keep=P, thr=1.0), "threshold=1 must be inside (0, 1)"),
    (dict(keep=P, thr=-0.5), "threshold=-0.5 must be inside (0, 1)"),
    (dict(keep=P, thr=float("nan")), "must be inside (0, 1)"),
    (dict(B=65536, heads=65536), "B*heads=4294967296 workgroups exceed the grid"),
    (dict(hp=1, wp=40832, ntok=40833, npad=40896, OH=1, OW=40832), "40833 tokens exceed the 40832"),
    (dict(hp=3, wp=5, OH=65536, OW=65536), "output 65536x65536 of a 3x5 grid is too large"),
    (dict(q=ctypes.c_void_p(4104)), "16-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", OP_REFUSALS)
def test_op_refuses_on_the_host(kw, msg):
    assert op(**kw) == -1
    assert "dinoseg_op_cls_attention" in capi.last_error() and msg in capi.last_error(), capi.last_error()


@pytest.fixture
def handle():
    lib = capi.lib()
    h = ctypes.c_void_p()
    cfg = capi.Config(384, 6, 12, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.FP16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, capi.last_error()
    yield h
    assert lib.dinoseg_destroy(h) == 0


def hw(h, x=P, kind=capi.INPUT_F32_CHW, B=1, H=64, W=128, OH=64, OW=128, thr=0.6, attn=P, keep=None):
    return capi.lib().dinoseg_cls_attention_hw(h, x, kind, B, H, W, OH, OW, thr, attn, keep, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(H=60), "Resolution should be a multiple of 8."),
    (dict(W=0), "Resolution should be a multiple of 8."),
    (dict(OH=7), "output 7x128 is smaller than the patch grid 8x16"),
    (dict(OW=15), "output 64x15 is smaller than the patch grid 8x16"),
    (dict(keep=P, thr=1.5), "threshold=1.5 must be inside (0, 1)"),
    (dict(keep=P, thr=float("nan")), "must be inside (0, 1)"),
    (dict(attn=None, keep=None), "null pointer (at least one of attn_out / keep_out is required)"),
    (dict(x=None), "bad argument"),
    (dict(B=0), "bad argument"),
    (dict(H=8, W=8 * 40832, OH=1, OW=40832), "40833 tokens exceed the 40832"),
])
def test_hw_entry_refuses_before_the_forward(handle, kw, msg):
    assert hw(handle, **kw) == -1
    assert msg in capi.last_error(), capi.last_error()


# --------------------------------------------------------------------------- Python
def test_python_call_raises_before_any_device_use():
    m = DINOSeg(head="mlp", n_blocks=1)
    f32, u8 = torch.zeros((1, 3, 64, 128)), torch.zeros((2, 64, 128, 3), dtype=torch.uint8)
    for bad in (torch.zeros((3, 64, 128)), torch.zeros((1, 4, 64, 128)), torch.zeros((1, 64, 128, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="expected"):
            m.cls_attention(bad)
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        m.cls_attention(torch.zeros((1, 3, 60, 128)))
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        m.cls_attention(torch.zeros((1, 64, 100, 3), dtype=torch.uint8))
    for size in ((7, 16), (8, 15)):
        with pytest.raises(ValueError, match="smaller than the patch grid"):
            m.cls_attention(f32, size=size)
    for thr in (0.0, 1.0, -0.1, 1.5, float("nan"), 1.0 - 1e-12):
        with pytest.raises(ValueError, match="threshold must be inside"):
            m.cls_attention(u8, threshold=thr)
    with pytest.raises(ValueError, match="40833 tokens, more than the 40832"):
        m.cls_attention(torch.zeros((1, 8, 8 * 40832, 3), dtype=torch.uint8))
    # and with valid arguments it fails like its siblings without a GPU
    for call in (lambda: m.cls_attention(f32), lambda: m.cls_attention(u8, size=(8, 16), threshold=0.6),
                 lambda: m.dino.cls_attention(f32, threshold=0.1)):
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            call()


# --------------------------------------------------------------------------- the rule
def _golden_rows(golden_dir):
    g = np.load(os.path.join(golden_dir, "g10_last_selfattention.npz"))
    rows = [r for r in g["tiny_r64_full"][0, :, 0, 1:]] + [r for r in g["vits8_L3_r96_cls_rows"][:, 1:]]
    assert len(rows) == 8 and rows[0].shape == (64,) and rows[-1].shape == (144,)
    return rows


@pytest.mark.parametrize("threshold", [0.1, 0.6, 0.9])
def test_integer_rule_is_the_fp64_sort_rule_on_the_references_rows(golden_dir, threshold):
    worst = 1.0
    for row in _golden_rows(golden_dir):
        want, margin = U.sort_rule_fp64(row, threshold)
        got = U.keep_rule(row, threshold)
        assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), want)
        assert 0 < int(got.sum()) < row.size
        worst = min(worst, margin)
    print(f"cls_attention rule threshold {threshold}: smallest margin to a cut {worst:.3e} of the mass")
    assert worst > 2.0 ** -24, "the rows decide no patch inside the rule's quantisation"


def test_integer_rule_on_random_softmax_rows():
    g_ = np.random.default_rng(77)
    checked = 0
    for n in (64, 3600, 16641):
        for threshold in (0.1, 0.6, 0.9):
            s = g_.standard_normal(n) * 2.0
            p = (np.exp(s) / np.exp(s).sum() * 0.9).astype(np.float32)          # (the CLS key holds the rest of the mass)
            want, margin = U.sort_rule_fp64(p, threshold)
            # n roundings of at most 2^-31 each move a cumulative sum by less than n 2^-30 of the patches' mass: beyond that margin
            # the two rules must agree at every patch
            if margin > n * 2.0 ** -30:
                checked += 1
                assert np.array_equal(U.keep_rule(p, threshold).astype(bool), want), (n, threshold)
    assert checked >= 7


def test_a_tied_group_is_kept_whole():
    p = np.array([0.1, 0.2, 0.2, 0.2, 0.3], dtype=np.float32)
    assert U.keep_rule(p, 0.6).tolist() == [0, 1, 1, 1, 1]
    # in any order, and as rows of a batch
    assert U.keep_rule(p[[2, 4, 0, 1, 3]], 0.6).tolist() == [1, 1, 0, 1, 1]
    assert U.keep_rule(np.stack([p, p[::-1]]), 0.6).tolist() == [[0, 1, 1, 1, 1], [1, 1, 1, 1, 0]]
    # a small threshold drops the whole group: only the largest value holds the top 25 % of the mass
    assert U.keep_rule(p, 0.25).tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("hp,wp", [(3, 5), (8, 8)])
@pytest.mark.parametrize("mult", [1, 8, 16])
def test_nearest_coordinates_are_torchs_for_integer_multiples(hp, wp, mult):
    grid = np.random.default_rng(hp * wp + mult).standard_normal((2, 3, hp, wp)).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(grid), scale_factor=mult, mode="nearest").numpy()
    got = U.nearest_gather(grid, hp * mult, wp * mult)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_nearest_coordinates_for_other_ratios():
    assert U.nearest_index(3, 7).tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert U.nearest_index(5, 11).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert U.nearest_index(1, 8).tolist() == [0] * 8
