"""GPU box: cost of the segmentation head at a narrow (7) and a wide (150) class count -- ViT-S/8 x12 @480, batch 32, fp16x3 by
default.  Per class count: the head's kernel time from the in-forward event timers (model.profile(2) / profile_read(): class
'head' = the head's launches) and the forward's frames/s with the timers off (host clock around synchronised calls).

    python tools/head_cost.py [--classes 7,150] [--head mlp] [--batch 32] [--res 480] [--precision fp16x3] [--iters 20]
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
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--head", default="mlp")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--precision", default="fp16x3")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_cost.py needs a ROCm device")
    frames = torch.from_numpy(synthetic_frames(a.batch, a.res, seed=1)).cuda()
    for C in (int(c) for c in a.classes.split(",")):
        cfg = ViTConfig(n_blocks=12, n_classes=C, head=a.head)
        m = DINOSeg(head=a.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
        m.to("cuda:0")
        m.set_resolution(a.res)
        for _ in range(3):
            m.forward_frames(frames)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            m.forward_frames(frames)
        torch.cuda.synchronize()
        fps = a.batch * a.iters / (time.perf_counter() - t0)
        m.profile(2)
        m.profile_read()
        for _ in range(a.iters):
            m.forward_frames(frames)
        prof = m.profile_read()
        m.profile(0)
        head_ms, launches = prof["head"]
        print(json.dumps({"n_classes": C, "head": a.head, "precision": a.precision, "batch": a.batch, "res": a.res,
                          "head_us_per_forward": round(head_ms * 1e3 / a.iters, 1), "head_launches_per_forward": launches / a.iters,
                          "frames_per_s": round(fps, 1)}), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
