"""Generate tests/golden/g15_rect_*.npz -- non-square frames -- from the REFERENCE ViT (build container only, no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rect.py

The reference's VisionTransformer reads ``B, nc, w, h = x.shape`` and resamples the 28 x 28 position grid with one scale per
axis (vision_transformer.py:202-233), so an H x W frame gives (H/8) x (W/8) patch tokens, row-major.  The helpers of
oracle/gen_golden.py load the reference at run time; only numbers are written.  Frames are uniform noise
(dino_amd.weights.synthetic_frames(B, H, seed, w=W)): the fixtures keep the seed, not the pixels.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden import (TorchHead, _sample_idx, margins, preprocess_np, ref_logp, ref_vit, save)  # noqa: E402
from dino_amd.weights import ViTConfig, procedural_state_dict, synthetic_frames, synthetic_labels  # noqa: E402

# (tag, B, H, W, frame seed): seeds picked so that no patch has a top-2 log-probability margin below 1e-3
L3_SHAPES = (("240x320", 2, 240, 320, 160), ("480x640", 1, 480, 640, 152), ("64x128", 1, 64, 128, 153))
L12_SHAPE = ("480x640", 1, 480, 640, 177)


def _logp(cfg, H, W, B, seed):
    sd = procedural_state_dict(cfg)
    vit, head = ref_vit(cfg, sd), TorchHead(cfg, sd)
    with torch.no_grad():
        return ref_logp(vit, head, preprocess_np(synthetic_frames(B, H, seed=seed, w=W)))


def forward_fixtures():
    out = {}
    for tag, B, H, W, seed in L3_SHAPES:
        lp = _logp(ViTConfig(n_blocks=3), H, W, B, seed)
        assert lp.shape[0] == B * (H // 8) * (W // 8)
        out[f"{tag}|seed"] = np.int64(seed)
        out[f"{tag}|shape"] = np.array([B, H, W], dtype=np.int64)
        out[f"{tag}|logp"] = lp.numpy()
        out[f"{tag}|argmax"] = lp.argmax(1).numpy().astype(np.uint8)
        out[f"{tag}|margin"] = margins(lp)
        print(tag, "min margin", float(margins(lp).min()))
    save("g15_rect_vits8_L3", **out)
    tag, B, H, W, seed = L12_SHAPE
    lp = _logp(ViTConfig(n_blocks=12), H, W, B, seed)
    print("L12", tag, "min margin", float(margins(lp).min()))
    save("g15_rect_vits8_L12_480x640", seed=np.int64(seed), shape=np.array([B, H, W], dtype=np.int64), logp=lp.numpy(),
         argmax=lp.argmax(1).numpy().astype(np.uint8), margin=margins(lp))


def backbone_fixtures():
    """model.dino(x), get_last_selfattention and forward_mask (3 masks) at 64 x 128 (8 x 16 patches, 129 tokens), ViT-S/8 L=3."""
    cfg = ViTConfig(n_blocks=3)
    vit = ref_vit(cfg, procedural_state_dict(cfg))
    H, W, seed = 64, 128, 155
    x = preprocess_np(synthetic_frames(1, H, seed=seed, w=W))
    hp, wp = H // 8, W // 8
    rng = np.random.default_rng(156)
    masks = (rng.random((3, hp, wp)) < 0.4).astype(np.float32)
    masks[0] = 1.0                                       # all keys
    masks[-1, : hp // 2] = 0.0                           # the top half of the frame masked out: the rows are not symmetric
    with torch.no_grad():
        tokens = vit(x)                                  # [1, N, D] final-norm tokens (vision_transformer.py:237-248)
        a = vit.get_last_selfattention(x)                # [1, heads, N, N]
        emb = vit.forward_mask(x, torch.from_numpy(masks))
        att = vit.get_last_selfattention(x, cls_mask=torch.from_numpy(masks))
    save("g15_rect_backbone_64x128", seed=np.int64(seed), shape=np.array([1, H, W], dtype=np.int64), tokens=tokens.numpy(),
         attn_cls_rows=a[0, :, 0, :].numpy().copy(), attn_row77=a[0, :, 77, :].numpy().copy(),
         attn_row_sums=a[0].sum(-1).numpy().copy(), masks=masks, mask_emb=emb.numpy(), mask_attn=att.numpy())


def finetune_fixture():
    """One G12-style fine-tune step, 1 frame at 240 x 320, ViT-S/8 L=3 unfrozen: loss, all 48 gradient norms, sampled entries."""
    cfg, B, H, W = ViTConfig(n_blocks=3), 1, 240, 320
    sd = procedural_state_dict(cfg)
    vit, head = ref_vit(cfg, sd), TorchHead(cfg, sd)
    vit.train(); head.train()
    frames = synthetic_frames(B, H, seed=157, w=W)
    labels = synthetic_labels(B, (H // 8) * (W // 8), cfg.n_classes, seed=158).astype(np.int64)
    y = torch.from_numpy(labels).reshape(-1).long()
    params = {("dino." + k): p for k, p in vit.named_parameters()}
    params.update({("clf." + k): p for k, p in head.named_parameters()})
    loss = torch.nn.functional.nll_loss(ref_logp(vit, head, preprocess_np(frames)), y)     # pl_torch_modules.py:261-265
    loss.backward()
    out = {"seed": np.int64(157), "label_seed": np.int64(158), "shape": np.array([B, H, W], dtype=np.int64),
           "loss": np.float32(loss.item())}
    assert len(params) == 48
    for i, (k, p) in enumerate(params.items()):
        g = p.grad.detach().reshape(-1)
        idx = _sample_idx(g.numel(), 64, seed=i)
        out[f"gnorm|{k}"] = np.float32(g.norm().item())
        out[f"gidx|{k}"] = idx
        out[f"gval|{k}"] = g[idx].numpy().copy()
    save("g15_rect_finetune_240x320", **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count() or 1)
    which = sys.argv[1:] or ["forward", "backbone", "finetune"]
    for w in which:
        {"forward": forward_fixtures, "backbone": backbone_fixtures, "finetune": finetune_fixture}[w]()
