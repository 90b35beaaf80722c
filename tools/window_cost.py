"""GPU box: cost of sliding-window inference -- ViT-S/8 x12, fp16, 960 x 960 frames, batch 8 (the `960` configuration of
BASELINE.json), window 480 at strides 480 (4 windows per frame) and 320 (9 windows), at 7 and 150 classes.  Per configuration,
interleaved in one process after warm-up, each leg timed with a host clock around a synchronised call, medians over --rounds rounds:

  1. segment(frames) on the whole frame (the position embedding resampled to 120 x 120, attention over 14 401 tokens);
  2. segment_windows(frames) end to end: the crops, the forwards of the window batch in chunks of 32, the fused merge launch;
  3. its forwards alone, on window batches cropped beforehand;
  4. the crop launches alone (csrc/windows.hip);
  5. the merge launch alone on ready window log-probs, 10 launches back to back;
  6. the torch route on the same log-probs: per window F.interpolate(bilinear) added into a [B, C, H, W] fp32 accumulator, a count
     plane, the divide, the argmax -- what a user builds from forward_frames.

Also the torch peak-memory delta of legs 2 and 6 and the share of pixels on which their labels agree.  Every configuration runs in
a child process of its own under its own time limit, and the first one that fails ends the run.  One JSON line per configuration,
appended to --out (default profiles/window_cost.jsonl).

    python tools/window_cost.py [--classes 7,150] [--strides 480,320] [--batch 8] [--res 960] [--window 480] [--rounds 10]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_delta(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def one(a, C, stride):
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict, window_origins
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("window_cost.py needs a ROCm device")
    B, r, w, chunk = a.batch, a.res, a.window, 32
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    lib = capi.lib()
    cfg = ViTConfig(n_blocks=12, n_classes=C)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    p = cfg.patch
    origins = window_origins(r, w, stride)
    g, gp = len(origins), w // p
    total = B * g * g
    chunks = [(f, min(chunk, total - f)) for f in range(0, total, chunk)]
    crops = [torch.empty((n, w, w, 3), dtype=torch.uint8, device="cuda") for _, n in chunks]
    labels = torch.empty((B, r, r), dtype=torch.int32, device="cuda")

    def crop():
        for (f, n), buf in zip(chunks, crops):
            capi.check(lib.dinoseg_op_crop_windows(frames.data_ptr(), capi.INPUT_U8_HWC, B, r, r, w, w, stride, stride, f, n,
                                                   buf.data_ptr(), capi.stream_ptr()))

    def forwards():
        return torch.cat([m.forward_frames(buf)[0] for buf in crops])

    crop()
    logp = forwards().view(total, gp * gp, C).contiguous()

    def op():
        capi.check(lib.dinoseg_op_window_merge(logp.data_ptr(), B, r, r, p, w, w, stride, stride, C, labels.data_ptr(), None,
                                               capi.stream_ptr()))

    def torch_route():
        acc = torch.zeros((B, C, r, r), dtype=torch.float32, device="cuda")
        cnt = torch.zeros((1, 1, r, r), dtype=torch.float32, device="cuda")
        grids = logp.view(B, g, g, gp, gp, C)
        for gy, oy in enumerate(origins):
            for gx, ox in enumerate(origins):
                up = F.interpolate(grids[:, gy, gx].permute(0, 3, 1, 2), size=(w, w), mode="bilinear", align_corners=False)
                acc[:, :, oy:oy + w, ox:ox + w] += up
                cnt[:, :, oy:oy + w, ox:ox + w] += 1.0
        return acc.div_(cnt).argmax(1)

    def whole():
        return m.segment(frames)[0]

    def e2e():
        return m.segment_windows(frames, window=w, stride=stride, max_windows=chunk)[0]

    for _ in range(2):                                          # warm-up of every leg
        whole(), e2e(), crop(), forwards(), op(), torch_route()
    t = {k: [] for k in ("whole", "e2e", "fwd", "crop", "op", "torch")}
    for _ in range(a.rounds):
        t["whole"].append(timed(torch, whole)[0])
        t["e2e"].append(timed(torch, e2e)[0])
        t["fwd"].append(timed(torch, forwards)[0])
        t["crop"].append(timed(torch, lambda: [crop() for _ in range(10)])[0] / 10)
        t["op"].append(timed(torch, lambda: [op() for _ in range(10)])[0] / 10)
        t["torch"].append(timed(torch, torch_route)[0])
    mem_e2e, got = peak_delta(torch, e2e)
    mem_torch, ref = peak_delta(torch, torch_route)
    mem_whole, _ = peak_delta(torch, whole)
    agree = float((got.long() == ref).double().mean())
    med = {k: statistics.median(v) for k, v in t.items()}
    line = {"n_classes": C, "window": w, "stride": stride, "windows_per_frame": g * g, "precision": a.precision, "batch": B, "res": r,
            "rounds": a.rounds, "segment_whole_frame_ms": round(med["whole"], 3), "segment_windows_ms": round(med["e2e"], 3),
            "forwards_ms": round(med["fwd"], 3), "crop_ms": round(med["crop"], 4), "merge_op_ms": round(med["op"], 4),
            "torch_route_ms": round(med["torch"], 3),
            "segment_whole_frame_ms_min_max": [round(min(t["whole"]), 3), round(max(t["whole"]), 3)],
            "segment_windows_ms_min_max": [round(min(t["e2e"]), 3), round(max(t["e2e"]), 3)],
            "whole_frame_frames_per_s": round(1e3 * B / med["whole"], 1), "windows_frames_per_s": round(1e3 * B / med["e2e"], 1),
            "windows_over_whole_frame_speed_measured": round(med["whole"] / med["e2e"], 4),
            "segment_windows_peak_bytes": int(mem_e2e), "segment_whole_frame_peak_bytes": int(mem_whole),
            "torch_route_peak_bytes": int(mem_torch), "labels_agree_with_torch_fp32": round(agree, 6)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--strides", default="480,320")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=960)
    ap.add_argument("--window", type=int, default=480)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_cost.jsonl"))
    ap.add_argument("--one", default=None, help="(internal) run the single configuration CLASSES,STRIDE in this process")
    a = ap.parse_args()
    if a.one:
        C, stride = (int(v) for v in a.one.split(","))
        return one(a, C, stride)
    for C in a.classes.split(","):
        for stride in a.strides.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{C},{stride}", "--batch", str(a.batch), "--res", str(a.res),
                   "--window", str(a.window), "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"window_cost.py: {C} classes at stride {stride} ran past {a.limit} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"window_cost.py: {C} classes at stride {stride} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
