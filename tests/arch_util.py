"""Shared by tests/test_arch_envelope_cpu.py and tests/test_arch_envelope_gpu.py: the architecture matrix -- one small model per corner
of what dinoseg_create accepts that no other test runs (widths 256 .. 1024, MLP ratios 1 .. 8, depth 0, one and two classes) -- its
frames, labels and weights, and the CPU oracle's outputs, each computed once per process and never modified."""
import functools
from collections import OrderedDict

import numpy as np
import torch

from dino_amd import ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames, synthetic_labels
from oracle import dinoseg_oracle as O


def _cfg(D, ratio, **kw):
    kw.setdefault("n_blocks", 2)
    return ViTConfig(embed_dim=D, num_heads=D // 64, mlp_ratio=ratio, **kw)


# tag -> config; what each one reaches first is in the comment
ARCH = OrderedDict([
    ("W256", _cfg(256, 4)),                                           # qkv N = 768 with dmodel % 384 != 0
    ("W512", _cfg(512, 4)),                                           # qkv N = 1536 = 4 * 384, fc1 N = 2048
    ("W640r2", _cfg(640, 2)),                                         # F = 1280 < 3 D = 1920
    ("W896r1", _cfg(896, 1, head="linear")),                          # F = D, 14 heads
    ("W1024p16", _cfg(1024, 4, patch=16, pos_grid=14)),               # the widest accepted model, F = 4096
    ("Sr1", _cfg(384, 1)),                                            # the K = 384 routes at F = 384 ...
    ("Sr3", _cfg(384, 3)),                                            # ... 1152 ...
    ("Sr8", _cfg(384, 8)),                                            # ... and 3072: gemm_ln fc1 at other N, no fused MLP (F != 1536)
    ("Br2", _cfg(768, 2)),                                            # gemm_rs fc1 at N = 1536, fc2 at K = 1536
    ("T2", _cfg(128, 2, n_classes=2)),                                # F = 256 = the head's padded hidden width; the smallest of everything
    ("L0", _cfg(384, 4, n_blocks=0)),                                 # patch embedding -> final norm -> head
    ("C1", _cfg(384, 4, n_classes=1, head="linear")),                 # log_softmax of one class
])
TAGS = list(ARCH)
B = 2
FRAME_SEED, LABEL_SEED = 7, 8
PRECISIONS = {"bf16": capi.BF16, "bf16x3": capi.BF16X3, "fp16": capi.FP16, "fp16x3": capi.FP16X3}


def side(cfg):
    """64 x 64 at patch 8 (65 tokens: one 64-key tile plus one key), 96 x 96 at patch 16 (37 tokens)"""
    return 64 if cfg.patch == 8 else 96


def n_patches(cfg):
    return (side(cfg) // cfg.patch) ** 2


def native_config(cfg, precision="bf16x3"):
    return capi.Config(cfg.embed_dim, cfg.num_heads, cfg.n_blocks, cfg.patch, cfg.mlp_ratio, cfg.n_classes,
                       capi.HEAD_MLP if cfg.head == "mlp" else capi.HEAD_LINEAR, cfg.pos_grid, cfg.ln_eps, PRECISIONS[precision])


@functools.lru_cache(maxsize=None)
def frames(tag, batch=B):
    """uint8 [batch, r, r, 3]"""
    f = synthetic_frames(batch, side(ARCH[tag]), seed=FRAME_SEED)
    f.setflags(write=False)
    return f


def tensor(a):
    """a torch copy of one of the read-only arrays of this module"""
    return torch.from_numpy(np.array(a))


@functools.lru_cache(maxsize=None)
def pixels(tag, batch=B):
    """the frames as the reference's transform leaves them: fp32 [batch, 3, r, r]"""
    return O.preprocess(np.array(frames(tag, batch)))




@functools.lru_cache(maxsize=None)
def state(tag):
    sd = procedural_state_dict(ARCH[tag])
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def oracle_logp(tag, batch=B):
    """fp32 log-probs [batch * n, C] of the CPU oracle"""
    cfg = ARCH[tag]
    with torch.no_grad():
        return O.dinoseg_forward(pixels(tag, batch), O.to_torch(state(tag)), cfg.num_heads, cfg.patch)


KINK = 1e-3


def head_kink_patches(cfg, W, x):
    """bool numpy [B * n]: the patches where an input of one of the MLP head's ReLUs is closer to 0 than KINK in the oracle.  The loss is
    not differentiable in the weights where such an input IS 0, and around it the derivative jumps: which side an implementation lands
    on is decided by its rounding (the oracle's own fp32 sums included), and one unit of one patch on the other side moves every gradient
    upstream of it by about that patch's share -- 1 % of the patch weight gradient here, at any precision.  The parity modes hold a value
    to 1e-3, so closer to 0 than that the side is not determined: these patches get the label -100 and carry no gradient, the others are
    compared at the full bars.  (GELU, softmax and LayerNorm are smooth; the linear head has no ReLU.)"""
    n = x.shape[0] * (x.shape[2] // cfg.patch) * (x.shape[3] // cfg.patch)
    if "clf.layer_2.weight" not in W:
        return np.zeros(n, dtype=bool)
    with torch.no_grad():
        t = O.vit_forward(x, W, cfg.num_heads, cfg.patch)[:, 1:].reshape(-1, cfg.embed_dim)
        a1 = O.linear(t, W["clf.layer_1.weight"], W["clf.layer_1.bias"])
        a2 = O.linear(torch.relu(a1), W["clf.layer_2.weight"], W["clf.layer_2.bias"])
    return (torch.minimum(a1.abs().amin(1), a2.abs().amin(1)) < KINK).numpy()


@functools.lru_cache(maxsize=None)
def kink_patches(tag):
    return head_kink_patches(ARCH[tag], O.to_torch(state(tag)), pixels(tag))


@functools.lru_cache(maxsize=None)
def labels(tag):
    """int64 [B, n] patch labels of the fine-tune step; -100 (ignored, as F.nll_loss ignores it) on the patches of kink_patches(tag)"""
    cfg = ARCH[tag]
    y = synthetic_labels(B, n_patches(cfg), cfg.n_classes, seed=LABEL_SEED)
    y[kink_patches(tag).reshape(y.shape)] = -100
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def oracle_margin(tag):
    """top-2 margin of every patch of oracle_logp(tag); +inf with a single class"""
    ref = oracle_logp(tag)
    if ref.shape[1] < 2:
        return torch.full((ref.shape[0],), float("inf"))
    top2 = ref.topk(2, dim=1).values
    return top2[:, 0] - top2[:, 1]


@functools.lru_cache(maxsize=None)
def oracle_quant_error(tag, fmt):
    """e_q: max |oracle with every linear's operands rounded to one 16-bit plane - oracle|, the yardstick of the one-plane modes"""
    cfg = ARCH[tag]
    q = {"bf16": O.quant_bf16, "fp16": O.quant_fp16}[fmt]
    with torch.no_grad():
        lp = O.dinoseg_forward(pixels(tag), O.to_torch(state(tag)), cfg.num_heads, cfg.patch, q=q)
    return float((lp - oracle_logp(tag)).abs().max())


@functools.lru_cache(maxsize=None)
def oracle_step(tag):
    """(loss, {name: gradient}) of F.nll_loss over the batch through the oracle's autograd (fp32)"""
    cfg = ARCH[tag]
    W = O.to_torch(state(tag), requires_grad=True)
    loss = O.nll_loss(O.dinoseg_forward(pixels(tag), W, cfg.num_heads, cfg.patch), tensor(labels(tag)).reshape(-1))
    loss.backward()
    return float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in W.items()}
