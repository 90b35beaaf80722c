"""GPU box: cost of the patch size -- ViT-S x12 at 480 x 480, batch 32, patch 16 (30 x 30 patches, 901 tokens) against patch 8
(60 x 60, 3601 tokens), then ViT-B/16, fp16 and fp16x3 by default.  Per model and precision: the forward's frames/s with the
timers off (host clock around synchronised calls) and the per-class kernel time of one forward from the in-forward event timers
(model.profile(2) / profile_read(), dinoseg_profile).  By FLOP count a ViT-S block is 4.44 GFLOP per frame at patch 16 against
32.66 at patch 8 (7.4x), and attention's share falls from 61 % to 28 %: the GEMM-class launches carry the forward.

    python tools/patch_cost.py [--res 480] [--batch 32] [--precisions fp16,fp16x3] [--iters 20] [--models s8,s16,b16]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dino_amd import DINOSeg, VIT_B8, VIT_B16, VIT_S8, VIT_S16, ViTConfig, procedural_state_dict
from dino_amd.weights import synthetic_frames

MODELS = {"s8": ("ViT-S/8", VIT_S8), "s16": ("ViT-S/16", VIT_S16), "b8": ("ViT-B/8", VIT_B8), "b16": ("ViT-B/16", VIT_B16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precisions", default="fp16,fp16x3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--models", default="s8,s16,b16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_cost.py needs a ROCm device")
    for key in a.models.split(","):
        name, base = MODELS[key]
        cfg = ViTConfig(embed_dim=base.embed_dim, num_heads=base.num_heads, n_blocks=12, patch=base.patch, pos_grid=base.pos_grid)
        sd = {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}
        frames = torch.from_numpy(synthetic_frames(a.batch, a.res, seed=1)).cuda()
        for prec in a.precisions.split(","):
            m = DINOSeg(head="mlp", n_blocks=12, precision=prec, arch=cfg)
            m.load_state_dict(sd, strict=True)
            m.to("cuda:0")
            for _ in range(3):
                m.forward_frames(frames, want_logp=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                m.forward_frames(frames, want_logp=False)
            torch.cuda.synchronize()
            fps = a.batch * a.iters / (time.perf_counter() - t0)
            m.profile(2)
            m.profile_read()
            for _ in range(a.iters):
                m.forward_frames(frames, want_logp=False)
            prof = m.profile_read()
            m.profile(0)
            total = sum(ms for ms, _ in prof.values())
            print(json.dumps({"model": name, "res": a.res, "tokens": (a.res // cfg.patch) ** 2 + 1, "precision": prec, "batch": a.batch,
                              "frames_per_s": round(fps, 1),
                              "us_per_forward": {k: round(ms * 1e3 / a.iters, 1) for k, (ms, n) in prof.items() if n},
                              "launches_per_forward": {k: n // a.iters for k, (ms, n) in prof.items() if n},
                              "attention_share": round(prof["attention"][0] / total, 3) if total else None}), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
