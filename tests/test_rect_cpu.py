"""CPU tests of non-square frames (H x W, both multiples of 8): the `_hw` C-ABI entries exist and check their arguments without a
GPU, the Python module routes a rectangle to the library instead of refusing its shape, and the g15 fixtures -- captured from the
reference's VisionTransformer at 240x320, 480x640 and 64x128 (tools/gen_golden_rect.py) -- are restated here on the CPU with the
oracle's pieces and a two-axis bicubic resample of the position grid (vision_transformer.py:202-233)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames, synthetic_labels
from oracle import dinoseg_oracle as O

HW_ENTRIES = ("dinoseg_prepare_resolution_hw", "dinoseg_forward_hw", "dinoseg_last_selfattention_hw", "dinoseg_forward_mask_hw",
              "dinoseg_features_hw", "dinoseg_train_forward_hw", "dinoseg_train_step_hw", "dinoseg_workspace_bytes_hw",
              "dinoseg_op_pos_resample_hw", "dinoseg_op_patch_gather_hw")


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


# --------------------------------------------------------------------------- the two-axis resample, restated
def resample_pos_embed_hw(pos_embed: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """[1, g*g+1, D] -> [1, oh*ow+1, D]: rows at source coordinate (y + 0.5) * g / (oh + 0.1) - 0.5, columns at
    (x + 0.5) * g / (ow + 0.1) - 0.5, Keys cubic (A = -0.75), taps clamped; the stored grid itself only for oh == ow == g."""
    g = int(round(math.sqrt(pos_embed.shape[1] - 1)))
    D = pos_embed.shape[2]
    if oh == g and ow == g:
        return pos_embed
    grid = pos_embed[0, 1:].reshape(g, g, D)

    def taps(o):
        scale = float(g) / (float(o) + 0.1)
        src = (torch.arange(o, dtype=torch.float32) + 0.5) * scale - 0.5
        base = torch.floor(src)
        w = torch.stack(O._cubic_weights(src - base), dim=1)                                    # [o, 4]
        base = base.to(torch.int64)
        return w, torch.stack([(base + k).clamp(0, g - 1) for k in (-1, 0, 1, 2)], 1)          # [o, 4]

    wy, iy = taps(oh)
    wx, ix = taps(ow)
    rows = (grid[iy] * wy[:, :, None, None]).sum(1)                  # [oh, g, D]
    out = (rows[:, ix] * wx[None, :, :, None]).sum(2)                # [oh, ow, D]
    return torch.cat([pos_embed[:, :1], out.reshape(1, oh * ow, D)], dim=1)


def tokens_hw(x: torch.Tensor, W) -> torch.Tensor:
    """prepare_tokens (vision_transformer.py:224-235) of [B, 3, H, W] frames."""
    B, _, H, Wd = x.shape
    tok = torch.cat([W["dino.cls_token"].expand(B, -1, -1), O.patch_embed(x, W, 8)], dim=1)
    return tok + resample_pos_embed_hw(W["dino.pos_embed"], H // 8, Wd // 8)


def vit_hw(x, W, n_blocks, num_heads=6, eps=1e-6):
    t = tokens_hw(x, W)
    for i in range(n_blocks):
        t = O.block(t, W, i, num_heads, eps)
    return O.layer_norm(t, W["dino.norm.weight"], W["dino.norm.bias"], eps)


def logp_hw(x, W, n_blocks):
    t = vit_hw(x, W, n_blocks)[:, 1:]
    return O.head_forward(t.reshape(-1, t.shape[-1]), W)


# --------------------------------------------------------------------------- C-ABI
def test_header_declares_and_library_exports_every_hw_entry():
    syms = set(capi.header_symbols())
    assert set(HW_ENTRIES) <= syms
    assert set(capi.SIGNATURES) == syms
    lib = capi.lib()
    for s in HW_ENTRIES:
        assert hasattr(lib, s), s


@pytest.fixture
def handle():
    lib = capi.lib()
    h = ctypes.c_void_p()
    cfg = capi.Config(384, 6, 12, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.FP16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, capi.last_error()
    yield h
    assert lib.dinoseg_destroy(h) == 0


def test_workspace_bytes_hw(handle):
    lib = capi.lib()
    assert lib.dinoseg_workspace_bytes_hw(handle, 1, 480, 640) > 4801 * 384 * 4
    assert lib.dinoseg_workspace_bytes_hw(handle, 1, 480, 640) > lib.dinoseg_workspace_bytes(handle, 1, 480)
    for B, r in ((1, 480), (32, 480), (3, 224), (1, 8)):
        assert lib.dinoseg_workspace_bytes_hw(handle, B, r, r) == lib.dinoseg_workspace_bytes(handle, B, r)
    # the layout depends on the token count: a transposed frame needs the same memory
    assert lib.dinoseg_workspace_bytes_hw(handle, 2, 240, 320) == lib.dinoseg_workspace_bytes_hw(handle, 2, 320, 240)


@pytest.mark.parametrize("H,W", [(250, 320), (240, 250), (0, 320), (240, -8)])
def test_hw_entries_refuse_frames_that_are_not_multiples_of_8(handle, H, W):
    lib = capi.lib()
    assert lib.dinoseg_workspace_bytes_hw(handle, 1, H, W) == -1
    assert capi.last_error() == "Resolution should be a multiple of 8."
    assert lib.dinoseg_prepare_resolution_hw(handle, H, W, None) == -1
    assert capi.last_error() == "Resolution should be a multiple of 8."
    assert lib.dinoseg_op_patch_gather_hw(None, capi.INPUT_U8_HWC, 1, H, W, None, 0, 1, None) == -1
    assert capi.last_error() == "Resolution should be a multiple of 8."
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        capi.check(lib.dinoseg_forward_hw(handle, ctypes.c_void_p(16), capi.INPUT_U8_HWC, 1, H, W, None, None, -1, None, None))


def test_forward_mask_hw_refuses_as_many_masks_as_tokens(handle):
    lib = capi.lib()
    # 64 x 128: 8 x 16 patches, 129 tokens; the square entry refuses n_masks >= (r/8)^2 + 1 the same way
    assert lib.dinoseg_forward_mask_hw(handle, ctypes.c_void_p(16), capi.INPUT_F32_CHW, 64, 128, ctypes.c_void_p(16), 129,
                                       ctypes.c_void_p(16), None, None) == -1
    assert "must be smaller than the token count 129" in capi.last_error()


# --------------------------------------------------------------------------- Python module
def test_rectangular_input_reaches_the_device_check():
    """Without a GPU every entry point refuses a 240 x 320 batch for the lack of a device, not for its shape."""
    m = DINOSeg(head="mlp", n_blocks=1)
    x = torch.zeros((1, 3, 240, 320))
    u8 = torch.zeros((2, 240, 320, 3), dtype=torch.uint8)
    y = torch.zeros((1, 30 * 40), dtype=torch.int64)
    calls = [lambda: m(x), lambda: m.dino(x), lambda: m.features(u8), lambda: m.get_last_selfattention(x),
             lambda: m.forward_mask(x, torch.ones((2, 30, 40))), lambda: m.validation_step((x, y)),
             lambda: m.training_step((x, y)), lambda: m.fused_training_step((x, y)), lambda: m.forward_frames(u8)]
    for call in calls:
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            call()


def test_rectangular_input_still_needs_multiples_of_8():
    m = DINOSeg(head="mlp", n_blocks=1)
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        m._prep_batch(torch.zeros((1, 3, 240, 324)))
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        m._prep_batch(torch.zeros((1, 244, 320, 3), dtype=torch.uint8))
    x, kind, B, H, W = m._prep_batch(torch.zeros((2, 240, 320, 3), dtype=torch.uint8))
    assert (kind, B, H, W) == (capi.INPUT_U8_HWC, 2, 240, 320)
    x, kind, B, H, W = m._prep_batch(torch.zeros((1, 3, 64, 128), dtype=torch.float64))
    assert (kind, B, H, W) == (capi.INPUT_F32_CHW, 1, 64, 128) and x.dtype == torch.float32


# --------------------------------------------------------------------------- the resample rule
@pytest.mark.parametrize("oh,ow", [(30, 40), (60, 80), (8, 16), (1, 60), (28, 30), (16, 49), (28, 28), (29, 29), (60, 60)])
def test_two_axis_resample_is_torch_bicubic(oh, ow):
    pe = torch.from_numpy(procedural_state_dict(ViTConfig(n_blocks=0))["dino.pos_embed"])
    got = resample_pos_embed_hw(pe, oh, ow)
    assert got.shape == (1, oh * ow + 1, 384)
    g, D = 28, 384
    if (oh, ow) == (g, g):
        assert got is pe
    else:
        want = torch.nn.functional.interpolate(pe[:, 1:].reshape(1, g, g, D).permute(0, 3, 1, 2),
                                               scale_factor=((oh + 0.1) / g, (ow + 0.1) / g), mode="bicubic")
        assert want.shape[-2:] == (oh, ow)
        want = want.permute(0, 2, 3, 1).reshape(1, oh * ow, D)
        assert float((got[:, 1:] - want).abs().max()) <= 2e-6
    if oh == ow:
        assert torch.equal(got, O.resample_pos_embed(pe, oh))


def test_one_side_of_28_is_not_the_identity():
    """vision_transformer.py:205: the stored grid is returned only for a square 28 x 28 grid.  A 28-row rectangle resamples its
    rows at 28 / 28.1 too, and so does 16 x 49 (784 patches, the stored count)."""
    pe = torch.from_numpy(procedural_state_dict(ViTConfig(n_blocks=0))["dino.pos_embed"])
    got = resample_pos_embed_hw(pe, 28, 30)[0, 1:].reshape(28, 30, -1)
    rows_only = torch.nn.functional.interpolate(pe[:, 1:].reshape(1, 28, 28, -1).permute(0, 3, 1, 2), size=(28, 30),
                                                mode="bicubic").permute(0, 2, 3, 1)[0]
    assert float((got - rows_only).abs().max()) > 1e-4
    assert resample_pos_embed_hw(pe, 16, 49).shape == pe.shape
    assert not torch.equal(resample_pos_embed_hw(pe, 16, 49), pe)


# --------------------------------------------------------------------------- fixtures against the restatement
def _frames(B, H, W, seed):
    return O.preprocess(synthetic_frames(B, H, seed=seed, w=W))


@pytest.mark.parametrize("tag", ["240x320", "480x640", "64x128"])
def test_g15_l3_forward_matches_the_restatement(golden_dir, tag):
    g = _load(golden_dir, "g15_rect_vits8_L3")
    B, H, W = (int(v) for v in g[f"{tag}|shape"])
    Wt = O.to_torch(procedural_state_dict(ViTConfig(n_blocks=3)))
    with torch.no_grad():
        lp = logp_hw(_frames(B, H, W, int(g[f"{tag}|seed"])), Wt, 3)
    assert lp.shape == (B * (H // 8) * (W // 8), 7)
    assert float((lp - torch.from_numpy(g[f"{tag}|logp"])).abs().max()) <= 5e-5
    assert np.array_equal(lp.argmax(1).numpy(), g[f"{tag}|argmax"])
    assert float(g[f"{tag}|margin"].min()) >= 1e-3


def test_g15_l12_forward_matches_the_restatement(golden_dir):
    g = _load(golden_dir, "g15_rect_vits8_L12_480x640")
    B, H, W = (int(v) for v in g["shape"])
    Wt = O.to_torch(procedural_state_dict(ViTConfig(n_blocks=12)))
    with torch.no_grad():
        lp = logp_hw(_frames(B, H, W, int(g["seed"])), Wt, 12)
    assert lp.shape == (4800, 7)
    assert float((lp - torch.from_numpy(g["logp"])).abs().max()) <= 5e-5
    assert np.array_equal(lp.argmax(1).numpy(), g["argmax"])
    assert float(g["margin"].min()) >= 1e-3


def test_g15_backbone_matches_the_restatement(golden_dir):
    g = _load(golden_dir, "g15_rect_backbone_64x128")
    _, H, W = (int(v) for v in g["shape"])
    Wt = O.to_torch(procedural_state_dict(ViTConfig(n_blocks=3)))
    x = _frames(1, H, W, int(g["seed"]))
    masks = torch.from_numpy(g["masks"])
    assert masks.shape == (3, 8, 16)
    with torch.no_grad():
        tok = vit_hw(x, Wt, 3)
        t = tokens_hw(x, Wt)
        for i in range(2):
            t = O.block(t, Wt, i, 6, 1e-6)
        pre = "dino.blocks.2."
        t1 = O.layer_norm(t, Wt[pre + "norm1.weight"], Wt[pre + "norm1.bias"])
        _, pr = O.attention(t1, Wt, pre, 6, return_probs=True)
        y, mpr = O._masked_cls_attention(t1, Wt, pre, 6, masks)
        xm = t[:, 0:1, :].repeat(1, 3, 1) + y
        xm = xm + O.mlp(O.layer_norm(xm, Wt[pre + "norm2.weight"], Wt[pre + "norm2.bias"]), Wt, pre)
        emb = O.layer_norm(xm, Wt["dino.norm.weight"], Wt["dino.norm.bias"])[0]
    assert tok.shape == (1, 129, 384) and pr.shape == (1, 6, 129, 129)
    assert float((tok - torch.from_numpy(g["tokens"])).abs().max()) <= 5e-5
    assert float((pr[0, :, 0, :] - torch.from_numpy(g["attn_cls_rows"])).abs().max()) <= 5e-6
    assert float((pr[0, :, 77, :] - torch.from_numpy(g["attn_row77"])).abs().max()) <= 5e-6
    assert float((emb - torch.from_numpy(g["mask_emb"])).abs().max()) <= 5e-5
    assert float((mpr - torch.from_numpy(g["mask_attn"])).abs().max()) <= 5e-6


def test_g15_finetune_matches_the_restatement(golden_dir):
    g = _load(golden_dir, "g15_rect_finetune_240x320")
    B, H, W = (int(v) for v in g["shape"])
    sd = procedural_state_dict(ViTConfig(n_blocks=3))
    Wt = O.to_torch(sd, requires_grad=True)
    y = torch.from_numpy(synthetic_labels(B, (H // 8) * (W // 8), 7, seed=int(g["label_seed"]))).reshape(-1)
    loss = O.nll_loss(logp_hw(_frames(B, H, W, int(g["seed"])), Wt, 3), y)
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) <= 1e-5
    names = [k[len("gnorm|"):] for k in g.files if k.startswith("gnorm|")]
    assert len(names) == 48 and "dino.pos_embed" in names
    for k in names:
        gr = Wt[k].grad.reshape(-1)
        ref = float(g["gnorm|" + k])
        assert abs(float(gr.norm()) - ref) <= 1e-4 * ref + 1e-7, k
        assert float((gr[torch.from_numpy(g["gidx|" + k])] - torch.from_numpy(g["gval|" + k])).abs().max()) <= 1e-4 * ref + 1e-7, k
