"""GPU box: cost of pixel-resolution output -- ViT-S/8 x12 @480, batch 32, fp16, at 7 and 150 classes.  Three routes, interleaved
in one process after warm-up, each timed with a host clock around a synchronised call, medians over --rounds rounds (the difference of routes 2 and 1 is a
small part of two ~12 ms calls, so the upsample launch is also timed alone, back to back: upsample_op_ms):

  1. forward_frames alone (argmax at the patch grid only);
  2. segment(frames): the forward + the fused bilinear upsample + argmax (csrc/upsample.hip);
  3. the torch route on the log-probs of forward_frames: F.interpolate(..., mode="bilinear").argmax(1) -- timed alone, on
     log-probs computed beforehand; it is what a user does without segment().

Also the torch peak-memory delta of routes 2 and 3.  If the [B, C, H, W] fp32 transient of route 3 does not fit beside the other
tenants of the device, that leg runs at batch 8 and the line says so (torch_batch).  One JSON line per class count, appended to
--out (default profiles/dense_cost.jsonl).

    python tools/dense_cost.py [--classes 7,150] [--batch 32] [--res 480] [--precision fp16] [--rounds 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_cost.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_cost.py needs a ROCm device")
    B, r = a.batch, a.res
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    for C in (int(c) for c in a.classes.split(",")):
        cfg = ViTConfig(n_blocks=12, n_classes=C)
        m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
        m.to("cuda:0")
        m.set_resolution(r)
        hp = r // cfg.patch
        logp, _ = m.forward_frames(frames)

        def torch_route(lp, b):
            return F.interpolate(lp.view(b, hp, hp, C).permute(0, 3, 1, 2), size=(r, r), mode="bilinear").argmax(1)

        # the torch leg at the full batch if its transient fits in what the device has free, else at batch 8
        free, _total = torch.cuda.mem_get_info()
        transient = B * C * r * r * 4
        tb = B if 2.5 * transient < free else min(B, 8)
        lp_t = logp[: tb * hp * hp].contiguous()
        for _ in range(3):                                      # warm-up of every route
            m.forward_frames(frames, want_logp=False)
            m.segment(frames)
            torch_route(lp_t, tb)
        t_fwd, t_seg, t_torch = [], [], []
        for _ in range(a.rounds):
            t_fwd.append(timed(lambda: m.forward_frames(frames, want_logp=False))[0])
            t_seg.append(timed(lambda: m.segment(frames))[0])
            t_torch.append(timed(lambda: torch_route(lp_t, tb))[0])
        # the upsample launch alone: 20 back-to-back launches of the operator on the same log-probs
        lab = torch.empty((B, r, r), dtype=torch.int32, device="cuda")
        t_op = timed(lambda: [capi.check(capi.lib().dinoseg_op_upsample_argmax(logp.data_ptr(), B, hp, hp, C, r, r, lab.data_ptr(), None,
                                                                               capi.stream_ptr())) for _ in range(20)])[0] / 20
        mem_seg, (labels, _) = peak_delta(lambda: m.segment(frames))
        mem_torch, ref = peak_delta(lambda: torch_route(lp_t, tb))
        agree = float((labels[:tb].long() == ref).double().mean())
        del ref
        fwd, seg, tor = (statistics.median(t) for t in (t_fwd, t_seg, t_torch))
        line = {"n_classes": C, "precision": a.precision, "batch": B, "res": r, "rounds": a.rounds,
                "forward_ms": round(fwd, 3), "segment_ms": round(seg, 3), "segment_minus_forward_ms": round(seg - fwd, 3),
                "torch_upsample_argmax_ms": round(tor, 3), "torch_batch": tb,
                "torch_upsample_argmax_ms_scaled_to_batch": round(tor * B / tb, 3),
                "overhead_share_of_forward": round((seg - fwd) / fwd, 4), "upsample_op_ms": round(t_op, 4),
                "forward_ms_min_max": [round(min(t_fwd), 3), round(max(t_fwd), 3)],
                "segment_ms_min_max": [round(min(t_seg), 3), round(max(t_seg), 3)],
                "time_bar_holds": bool(seg - fwd <= tor * B / tb),
                "segment_peak_bytes": int(mem_seg), "torch_peak_bytes": int(mem_torch),
                "labels_agree_with_torch_fp32": round(agree, 6)}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del m, logp, lp_t, labels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
