"""The launch sequence of the forward, pinned per route (-m gpu): how many launches each profile class counts (model.profile(2),
model.profile_read()) on every route the block loop can plan at a tiny shape.  What is under test is the route planning of
csrc/forward.hip (plan_block): a LayerNorm launch that went missing, a qkv launch that should have been the tail of the block
before, a projection that ran twice all show as a count that moved.

Cases.  ViT-S/8 with 3 blocks and the MLP head, 2 frames of 64 x 64 (65 tokens, 130 rows), streams = 1, in the four precisions, on the
routes of small_routes(); Br2 of tests/arch_util.py (embed_dim 768, 2 blocks: the model gemm_rs.hip takes) in bf16 and fp16 on the
row-stationary routes of wide_routes(); the side paths (features, get_last_selfattention, forward_mask with 2 masks) on the default
route.  Options that are read at the refresh (mlp_fused4, gemm_rs, gemm_rs_ln) are set before a forced refresh.

EXPECTED was recorded on the parent commit of the change that split the forward into stages -- not derived from the code under
test -- by running this file's body against that commit's build (the Python surface is the same on both sides):

    DINOSEG_LIB=<parent build>/libdinoseg_hip.so python tests/test_route_plan_gpu.py

which prints the table below.  tools/route_digest.py runs the same cases and prints a digest of every output, for a byte comparison
of two builds.
"""
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dino_amd  # noqa: E402
from dino_amd import DINOSeg, ViTConfig, procedural_state_dict  # noqa: E402
from dino_amd.weights import synthetic_frames  # noqa: E402
from oracle import dinoseg_oracle as O  # noqa: E402
from tests import arch_util as A  # noqa: E402
from tests.gpu_util import route_options  # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["bf16x3", "fp16x3", "bf16", "fp16"]
WIDE_TAG, WIDE_PRECISIONS = "Br2", ["bf16", "fp16"]


def small_routes(precision):
    """(name, options) of the 3-block ViT-S.  The tails of the fused launches (qkv_fused*, mlp_fused4) are run both alone -- at 130
    rows the fused launches are off by default and the option must change nothing -- and with mlp_fused = 2, where they decide"""
    routes = [("default", {}), ("gemm_ln=0", {"gemm_ln": 0}), ("gemm_ln=2", {"gemm_ln": 2}), ("gemm_big=0", {"gemm_big": 0}),
              ("gemm_big=2", {"gemm_big": 2}),
              ("mlp_fused=2,proj_fused=0", {"mlp_fused": 2, "proj_fused": 0}), ("mlp_fused=2,proj_fused=1", {"mlp_fused": 2, "proj_fused": 1})]
    if precision in ("bf16", "fp16"):
        tails = [{"qkv_fused": 0}, {"qkv_fused": 1}, {"mlp_fused4": 1, "qkv_fused4": 0}, {"mlp_fused4": 1, "qkv_fused4": 1}]
    else:
        tails = [{"qkv_fused3": 0}, {"qkv_fused3": 1}]
    for t in tails:
        for extra in ({}, {"mlp_fused": 2}):
            o = dict(t, **extra)
            routes.append((",".join(f"{k}={v}" for k, v in o.items()), o))
    return routes


def wide_routes():
    return [(f"gemm_rs_ln={ln},gemm_rs={rs}", {"gemm_rs_min_rows": 1, "gemm_rs_ln": ln, "gemm_rs": rs}) for ln in (1, 0) for rs in (1, 2, 3, 7)]


def small_model(precision):
    cfg = ViTConfig(n_blocks=3)
    m = DINOSeg(head="mlp", n_blocks=3, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    return m.to("cuda:0")


def small_frames():
    return torch.from_numpy(synthetic_frames(2, 64, seed=5)).cuda()


def wide_model(precision):
    cfg = A.ARCH[WIDE_TAG]
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: A.tensor(v) for k, v in A.state(WIDE_TAG).items()}, strict=True)
    return m.to("cuda:0")


def wide_frames():
    return A.tensor(A.frames(WIDE_TAG)).cuda()


def masks():
    """2 masks over the 8 x 8 patch grid: the left half, a checkerboard"""
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    return torch.from_numpy(np.stack([xx < 4, (yy + xx) % 2 == 0]).astype(np.float32)).cuda()


def side_paths(m, frames):
    """(name, call) of the backbone side paths; each call returns the tensor the path produces"""
    x = O.preprocess(frames.cpu().numpy()).cuda()
    return [("features(n_blocks=1)", lambda: m.features(x, n_blocks=1)), ("features()", lambda: m.features(x)),
            ("get_last_selfattention", lambda: m.get_last_selfattention(x)), ("forward_mask", lambda: m.forward_mask(x[:1], masks()))]


def counted(m, call):
    """(what the call returned, {profile class: launches} without the classes that counted none)"""
    m.profile(2)
    try:
        out = call()
        torch.cuda.synchronize()
        counts = {k: n for k, (_, n) in m.profile_read().items() if n}
    finally:
        m.profile(0)
    return out, counts


def run_cases(kind, precision):
    """yields (case id, outputs, counts) of one model: kind 'small', 'wide' or 'side'"""
    with route_options(streams=1):
        if kind == "side":
            m = small_model(precision)
            for name, call in side_paths(m, small_frames()):
                out, counts = counted(m, call)
                yield f"side/{precision}/{name}", (out,), counts
            return
        m, frames, routes = (small_model(precision), small_frames(), small_routes(precision)) if kind == "small" else \
                            (wide_model(precision), wide_frames(), wide_routes())
        for name, opts in routes:
            with route_options(m, **opts):
                out, counts = counted(m, lambda: m.forward_frames(frames))
            yield f"{kind}/{precision}/{name}", out, counts


ALL_CASES = [("small", p) for p in PRECISIONS] + [("wide", p) for p in WIDE_PRECISIONS] + [("side", p) for p in PRECISIONS]

# case id -> {profile class: launches}: recorded on the parent commit (module docstring)
EXPECTED = {
    'small/bf16x3/default': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/gemm_ln=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/gemm_ln=2': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/gemm_big=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/gemm_big=2': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/mlp_fused=2,proj_fused=0': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16x3/mlp_fused=2,proj_fused=1': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16x3/qkv_fused3=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/qkv_fused3=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16x3/qkv_fused3=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16x3/qkv_fused3=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16x3/default': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/gemm_ln=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/gemm_ln=2': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/gemm_big=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/gemm_big=2': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/mlp_fused=2,proj_fused=0': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16x3/mlp_fused=2,proj_fused=1': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16x3/qkv_fused3=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/qkv_fused3=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16x3/qkv_fused3=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16x3/qkv_fused3=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/default': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/gemm_ln=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/gemm_ln=2': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/gemm_big=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/gemm_big=2': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused=2,proj_fused=0': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused=2,proj_fused=1': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/qkv_fused=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/qkv_fused=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/qkv_fused=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/qkv_fused=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused4=1,qkv_fused4=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused4=1,qkv_fused4=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused4=1,qkv_fused4=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/bf16/mlp_fused4=1,qkv_fused4=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/default': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/gemm_ln=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/gemm_ln=2': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/gemm_big=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/gemm_big=2': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused=2,proj_fused=0': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused=2,proj_fused=1': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/qkv_fused=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/qkv_fused=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/qkv_fused=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/qkv_fused=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused4=1,qkv_fused4=0': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused4=1,qkv_fused4=0,mlp_fused=2': {'patch_embed': 3, 'layernorm': 4, 'qkv_gemm': 3, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused4=1,qkv_fused4=1': {'patch_embed': 3, 'layernorm': 7, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3, 'head': 3},
    'small/fp16/mlp_fused4=1,qkv_fused4=1,mlp_fused=2': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 3, 'fc1_gemm': 3, 'head': 3},
    'wide/bf16/gemm_rs_ln=1,gemm_rs=1': {'patch_embed': 3, 'layernorm': 3, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=1,gemm_rs=2': {'patch_embed': 3, 'layernorm': 3, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=1,gemm_rs=3': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=1,gemm_rs=7': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=0,gemm_rs=1': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=0,gemm_rs=2': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=0,gemm_rs=3': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/bf16/gemm_rs_ln=0,gemm_rs=7': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=1,gemm_rs=1': {'patch_embed': 3, 'layernorm': 3, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=1,gemm_rs=2': {'patch_embed': 3, 'layernorm': 3, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=1,gemm_rs=3': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=1,gemm_rs=7': {'patch_embed': 3, 'layernorm': 1, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=0,gemm_rs=1': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=0,gemm_rs=2': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=0,gemm_rs=3': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'wide/fp16/gemm_rs_ln=0,gemm_rs=7': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 2, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2, 'head': 3},
    'side/bf16x3/features(n_blocks=1)': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 1, 'proj_gemm': 1, 'fc1_gemm': 1, 'fc2_gemm': 1},
    'side/bf16x3/features()': {'patch_embed': 3, 'layernorm': 6, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3},
    'side/bf16x3/get_last_selfattention': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/bf16x3/forward_mask': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/fp16x3/features(n_blocks=1)': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 1, 'proj_gemm': 1, 'fc1_gemm': 1, 'fc2_gemm': 1},
    'side/fp16x3/features()': {'patch_embed': 3, 'layernorm': 6, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3},
    'side/fp16x3/get_last_selfattention': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/fp16x3/forward_mask': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/bf16/features(n_blocks=1)': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 1, 'proj_gemm': 1, 'fc1_gemm': 1, 'fc2_gemm': 1},
    'side/bf16/features()': {'patch_embed': 3, 'layernorm': 6, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3},
    'side/bf16/get_last_selfattention': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/bf16/forward_mask': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/fp16/features(n_blocks=1)': {'patch_embed': 3, 'layernorm': 2, 'qkv_gemm': 1, 'attention': 1, 'proj_gemm': 1, 'fc1_gemm': 1, 'fc2_gemm': 1},
    'side/fp16/features()': {'patch_embed': 3, 'layernorm': 6, 'qkv_gemm': 3, 'attention': 3, 'proj_gemm': 3, 'fc1_gemm': 3, 'fc2_gemm': 3},
    'side/fp16/get_last_selfattention': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
    'side/fp16/forward_mask': {'patch_embed': 3, 'layernorm': 5, 'qkv_gemm': 3, 'attention': 2, 'proj_gemm': 2, 'fc1_gemm': 2, 'fc2_gemm': 2},
}


@pytest.mark.parametrize("kind,precision", ALL_CASES)
def test_launch_counts_per_route(cuda, kind, precision):
    """Every route of the model enqueues the launches, class by class, the parent commit enqueued."""
    seen = 0
    for case, _, counts in run_cases(kind, precision):
        print(f"ROUTE_PLAN {case}: {counts}")
        assert case in EXPECTED, case
        assert counts == EXPECTED[case], (case, counts, EXPECTED[case])
        seen += 1
    assert seen == sum(1 for k in EXPECTED if k.startswith(f"{kind}/{precision}/"))


@pytest.mark.parametrize("precision", ["bf16", "fp16x3"])
def test_route_options_restore_the_forward(cuda, precision):
    """After a route_options scope that switched three routes (one of them read at the refresh), the forward is bit for bit the one
    from before it and every option of the library reads what it read before."""
    m, frames = small_model(precision), small_frames()[:1]
    names = dino_amd.option_names()
    before = {k: dino_amd.get_option(k) for k in names}
    logp0, amax0 = (t.clone() for t in m.forward_frames(frames))
    with route_options(m, gemm_ln=0, mlp_fused=2, gemm_rs=0):
        assert (dino_amd.get_option("gemm_ln"), dino_amd.get_option("mlp_fused"), dino_amd.get_option("gemm_rs")) == (0, 2, 0)
        m.forward_frames(frames)
    logp1, amax1 = m.forward_frames(frames)
    torch.cuda.synchronize()
    assert torch.equal(logp1, logp0) and torch.equal(amax1, amax0)
    assert {k: dino_amd.get_option(k) for k in names} == before


if __name__ == "__main__":
    print("EXPECTED = {")
    for kind, precision in ALL_CASES:
        for case, _, counts in run_cases(kind, precision):
            print(f"    {case!r}: {counts!r},", flush=True)
    print("}")
