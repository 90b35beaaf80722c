"""GPU box: cost of non-square frames -- ViT-S/8 x12, batch 32, 480x640 (60 x 80 patches, 4801 tokens) against 480x480 (3601
tokens), fp16 and fp16x3 by default.  Per shape and precision: the forward's frames/s with the timers off (host clock around
synchronised calls) and the per-class kernel time of one forward from the in-forward event timers (model.profile(2) /
profile_read(), dinoseg_profile).  Attention is quadratic in the token count: (4801 / 3601)^2 = 1.78x per frame.

    python tools/rect_cost.py [--shapes 480x480,480x640] [--batch 32] [--precisions fp16,fp16x3] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dino_amd import DINOSeg, ViTConfig, procedural_state_dict
from dino_amd.weights import synthetic_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="480x480,480x640")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precisions", default="fp16,fp16x3")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rect_cost.py needs a ROCm device")
    cfg = ViTConfig(n_blocks=12)
    sd = {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}
    for prec in a.precisions.split(","):
        m = DINOSeg(head="mlp", n_blocks=12, precision=prec, arch=cfg)
        m.load_state_dict(sd, strict=True)
        m.to("cuda:0")
        for shape in a.shapes.split(","):
            H, W = (int(v) for v in shape.split("x"))
            frames = torch.from_numpy(synthetic_frames(a.batch, H, seed=1, w=W)).cuda()
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
            print(json.dumps({"shape": shape, "tokens": (H // 8) * (W // 8) + 1, "precision": prec, "batch": a.batch,
                              "frames_per_s": round(fps, 1),
                              "us_per_forward": {k: round(ms * 1e3 / a.iters, 1) for k, (ms, n) in prof.items() if n},
                              "attention_share": round(prof["attention"][0] / total, 3) if total else None}), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
