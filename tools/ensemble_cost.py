"""GPU box: cost of the multi-scale + flip ensemble -- ViT-S/8 x12 @480, batch 8, fp16, at 7 and 150 classes, for the 12-view
protocol (scales 0.5 .. 1.75, each also mirrored) and a 3-scale protocol without flip.  Interleaved in one process after warm-up,
each leg timed with a host clock around a synchronised call, medians over --rounds rounds:

  1. segment_multiscale(frames) end to end: view construction, K forwards, the fused ensemble launch;
  2. the K forwards alone, on views built beforehand, in segment_multiscale's order (every change of resolution re-derives the
     position embedding and may regrow the workspace);
  3. the same K forwards in steady state: each view's forward repeated at ITS resolution, the repeats timed -- the difference of
     legs 2 and 3 is what switching resolution between views costs;
  4. the ensemble launch alone on ready low-res log-probs (csrc/upsample_ensemble.hip), 10 launches back to back;
  5. the torch route on the same ready log-probs: per view F.interpolate(bilinear) of the (flipped-back) grid, softmax, add; then
     argmax -- what a user builds from segment(..., want_logp=True).

Also the torch peak-memory delta of legs 1 and 5 and the share of pixels on which their labels agree.  One JSON line per (class
count, protocol), appended to --out (default profiles/ensemble_cost.jsonl).

    python tools/ensemble_cost.py [--classes 7,150] [--batch 8] [--res 480] [--precision fp16] [--rounds 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict, view_sizes
from dino_amd.weights import synthetic_frames

PROTOCOLS = {"12view": ((0.5, 0.75, 1.0, 1.25, 1.5, 1.75), True), "3scale": ((0.5, 1.0, 1.5), False)}


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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--protocols", default="12view,3scale")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_cost.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_cost.py needs a ROCm device")
    B, r = a.batch, a.res
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    lib = capi.lib()
    for C in (int(c) for c in a.classes.split(",")):
        cfg = ViTConfig(n_blocks=12, n_classes=C)
        m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
        m.to("cuda:0")
        p = cfg.patch
        for name in a.protocols.split(","):
            scales, flip = PROTOCOLS[name]
            views = []                                          # (frames of the view, H_k, W_k, flip_k)
            for Hk, Wk in view_sizes(r, r, scales, p):
                xv = frames if (Hk, Wk) == (r, r) else m._resize_view(frames, capi.INPUT_U8_HWC, Hk, Wk)
                for f in ((0, 1) if flip else (0,)):
                    views.append((torch.flip(xv, dims=[2]).contiguous() if f else xv, Hk, Wk, f))
            K = len(views)

            def forwards():
                return [m.forward_frames(x)[0] for x, _, _, _ in views]

            def steady():
                total = 0.0
                for x, _, _, _ in views:
                    m.forward_frames(x)
                    total += timed(lambda: [m.forward_frames(x) for _ in range(2)])[0] / 2
                return total

            logps = forwards()
            labels = torch.empty((B, r, r), dtype=torch.int32, device="cuda")
            scratch = torch.empty((lib.dinoseg_op_upsample_ensemble_scratch_bytes(K, B, r, r),), dtype=torch.uint8, device="cuda")
            i32 = lambda xs: (ctypes.c_int32 * K)(*xs)
            table = ((ctypes.c_void_p * K)(*[t.data_ptr() for t in logps]), i32([v[1] // p for v in views]),
                     i32([v[2] // p for v in views]), i32([v[3] for v in views]))

            def op():
                capi.check(lib.dinoseg_op_upsample_ensemble(*table, K, B, C, r, r, labels.data_ptr(), None, None, scratch.data_ptr(),
                                                            capi.stream_ptr()))

            def torch_route():
                acc = None
                for lp, (_, Hk, Wk, f) in zip(logps, views):
                    grid = lp.view(B, Hk // p, Wk // p, C).permute(0, 3, 1, 2)
                    if f:
                        grid = grid.flip(-1)
                    pr = torch.softmax(F.interpolate(grid, size=(r, r), mode="bilinear", align_corners=False), 1)
                    acc = pr if acc is None else acc.add_(pr)
                return acc.argmax(1)

            def e2e():
                return m.segment_multiscale(frames, scales=scales, flip=flip)[0]

            for _ in range(2):                                  # warm-up of every leg
                e2e(), forwards(), op(), torch_route()
            t_e2e, t_fwd, t_op, t_torch, t_steady = [], [], [], [], []
            for i in range(a.rounds):
                t_e2e.append(timed(e2e)[0])
                t_fwd.append(timed(forwards)[0])
                t_op.append(timed(lambda: [op() for _ in range(10)])[0] / 10)
                t_torch.append(timed(torch_route)[0])
                if i % 4 == 0:
                    t_steady.append(steady())
            mem_e2e, got = peak_delta(e2e)
            mem_torch, ref = peak_delta(torch_route)
            agree = float((got.long() == ref).double().mean())
            del ref, got
            med = statistics.median
            line = {"n_classes": C, "protocol": name, "scales": list(scales), "flip": flip, "views": K, "precision": a.precision, "batch": B,
                    "res": r, "rounds": a.rounds, "segment_multiscale_ms": round(med(t_e2e), 3), "forwards_ms": round(med(t_fwd), 3),
                    "forwards_steady_ms": round(med(t_steady), 3), "resolution_switch_ms": round(med(t_fwd) - med(t_steady), 3),
                    "ensemble_op_ms": round(med(t_op), 4), "torch_route_ms": round(med(t_torch), 3),
                    "segment_multiscale_ms_min_max": [round(min(t_e2e), 3), round(max(t_e2e), 3)],
                    "forwards_ms_min_max": [round(min(t_fwd), 3), round(max(t_fwd), 3)],
                    "segment_multiscale_peak_bytes": int(mem_e2e), "torch_route_peak_bytes": int(mem_torch),
                    "labels_agree_with_torch_fp32": round(agree, 6)}
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del logps, views, scratch, labels
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
