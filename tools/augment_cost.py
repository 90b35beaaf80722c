"""GPU box: cost of the device augmentation (csrc/augment.hip) beside the fine-tune step it feeds -- 480 x 480 uint8 frames and
masks to 480 x 480 normalised fp32 frames and pixel labels, at batch 8 and 32, for two parameter mixes: `recipe`, tables drawn by
draw_reference_augment (a quarter of the frames blurred, kernel sizes 3..41), and `k41`, the same tables with EVERY frame blurred at
kernel size 41 (the worst case).  Per configuration, interleaved in one process after warm-up, each leg timed with a host clock
around a synchronised call, medians over --rounds rounds:

  1. dinoseg_op_augment alone on ready device tensors (one launch, or two when a frame is blurred), 10 calls back to back;
  2. DINOSeg.augment end to end (table check on the host, upload, allocations, the launches);
  3. the torch route on the same tables and the same device: F.affine_grid + F.grid_sample (bilinear, reflection padding: torch
     has no reflect-101 for grid_sample, so its border pixels differ) for the frames and nearest for the masks, brightness, per
     blurred frame F.pad(reflect) + two grouped F.conv2d, normalise;
  4. fused_training_step_dense alone on a ready batch (ViT-S/8 x3, bf16, 7 classes: the finetune configuration of bench.py).

Every configuration runs in a child process of its own under its own time limit, and the first one that fails ends the run.  One JSON
line per configuration, appended to --out (default profiles/augment_cost.jsonl).

    python tools/augment_cost.py [--batches 8,32] [--mixes recipe,k41] [--res 480] [--rounds 20]
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


def child(a, B, mix):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, draw_reference_augment, procedural_state_dict
    from dino_amd.augment import gaussian_taps, unpack_table
    from dino_amd.weights import synthetic_frames

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if not torch.cuda.is_available():
        raise SystemExit("augment_cost.py needs a ROCm device")
    r, C = a.res, 7
    cfg = ViTConfig(n_blocks=a.blocks, n_classes=C)
    m = DINOSeg(head=cfg.head, n_blocks=a.blocks, n_classes=C, precision=a.precision, arch=cfg, freeze_backbone=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    m.unfreeze_bb()
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    rng = np.random.default_rng(3)
    masks = torch.from_numpy(rng.integers(0, C, (B, r, r)).astype(np.uint8)).cuda()
    table = draw_reference_augment(B, (r, r), (r, r), torch.Generator().manual_seed(7))
    if mix == "k41":
        table[:, 14] = 20
        table[:, 15:36] = torch.from_numpy(gaussian_taps(41).astype(np.float32).view(np.int32))
    f = unpack_table(table)
    rmax = int(f["radius"].max())
    dev_table = table.cuda()
    lib = capi.lib()
    img = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda")
    lab = torch.empty((B, r, r), dtype=torch.int64, device="cuda")
    scratch = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda") if rmax else None

    def op():
        capi.check(lib.dinoseg_op_augment(frames.data_ptr(), masks.data_ptr(), 0, B, r, r, dev_table.data_ptr(), rmax, r, r,
                                          capi.INPUT_F32_CHW, img.data_ptr(), lab.data_ptr(), None, 8, capi.ptr(scratch), capi.stream_ptr()))

    def method():
        return m.augment(frames, masks, table, out=(r, r))

    # the torch route: the table's inverse affine in affine_grid's normalised coordinates (edge convention, align_corners=False)
    A = f["a"].astype(np.float64) / 65536.0
    lin = A[:, [0, 1, 3, 4]].reshape(B, 2, 2)
    t = np.stack([A[:, 2] - 0.5 * (A[:, 0] + A[:, 1]), A[:, 5] - 0.5 * (A[:, 3] + A[:, 4])], axis=1)        # without the half pixel
    half = np.array([r / 2.0, r / 2.0])
    theta = np.concatenate([lin, ((lin @ half) + t - half)[:, :, None] / half[None, :, None]], axis=2)     # source = lin out + t, both / half - 1
    theta = torch.from_numpy(theta.astype(np.float32)).cuda()
    gain = torch.from_numpy(f["gain"]).cuda().view(B, 1, 1, 1)
    mean = torch.tensor((0.485, 0.456, 0.406), device="cuda").view(1, 3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device="cuda").view(1, 3, 1, 1)
    kernels = {}
    for b in range(B):
        rb = int(f["radius"][b])
        if rb and rb not in kernels:
            k = torch.from_numpy(np.array([f["w"][b][abs(d)] for d in range(-rb, rb + 1)], dtype=np.float32)).cuda()
            kernels[rb] = (k.view(1, 1, 1, -1).repeat(3, 1, 1, 1), k.view(1, 1, -1, 1).repeat(3, 1, 1, 1))

    def torch_route():
        grid = F.affine_grid(theta, (B, 3, r, r), align_corners=False)
        x = F.grid_sample(frames.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="reflection", align_corners=False)
        y = F.grid_sample(masks.view(B, 1, r, r).float(), grid, mode="nearest", padding_mode="reflection", align_corners=False)
        x = (x * gain).clamp_(0.0, 255.0)
        for b in range(B):
            rb = int(f["radius"][b])
            if rb:
                kh, kv = kernels[rb]
                v = F.conv2d(F.pad(x[b:b + 1], (rb, rb, 0, 0), mode="reflect"), kh, groups=3)
                x[b:b + 1] = F.conv2d(F.pad(v, (0, 0, rb, rb), mode="reflect"), kv, groups=3)
        return (x / 255.0 - mean) / std, y.view(B, r, r).long()

    y_pix = rng.integers(0, C, (B, r, r)).astype(np.int64)
    y_pix[rng.random((B, r, r)) < 0.1] = 255
    y_pix = torch.from_numpy(y_pix).cuda()
    ready = torch.randn(B, 3, r, r, device="cuda")

    def step():
        return m.fused_training_step_dense((ready, y_pix))["loss"]

    for _ in range(3):                                          # warm-up of every leg
        op(), method(), torch_route(), step()
    t = {k: [] for k in ("op", "method", "torch", "step")}
    for _ in range(a.rounds):
        t["op"].append(timed(lambda: [op() for _ in range(10)])[0] / 10)
        t["method"].append(timed(method)[0])
        t["torch"].append(timed(torch_route)[0])
        t["step"].append(timed(step)[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    line = {"mix": mix, "batch": B, "res": r, "precision": a.precision, "n_blocks": a.blocks, "rounds": a.rounds,
            "frames_blurred": int((f["radius"] > 0).sum()), "max_radius": rmax, "launches": 2 if rmax else 1,
            "augment_op_ms": round(med["op"], 4), "augment_method_ms": round(med["method"], 4), "torch_route_ms": round(med["torch"], 3),
            "dense_step_ms": round(med["step"], 3), "augment_op_over_step": round(med["op"] / med["step"], 5),
            "torch_over_op": round(med["torch"] / med["op"], 2), "augment_frames_per_s": round(1e3 * B / med["op"], 1),
            "step_frames_per_s": round(1e3 * B / med["step"], 1),
            "augment_op_ms_min_max": [round(min(t["op"]), 4), round(max(t["op"]), 4)],
            "dense_step_ms_min_max": [round(min(t["step"]), 3), round(max(t["step"]), 3)],
            "torch_route_ms_min_max": [round(min(t["torch"]), 3), round(max(t["torch"]), 3)]}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--mixes", default="recipe,k41")
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=int, default=180, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_cost.jsonl"))
    ap.add_argument("--one", default=None, help="(internal) run the single configuration BATCH,MIX in this process")
    a = ap.parse_args()
    if a.one:
        B, mix = a.one.split(",")
        return child(a, int(B), mix)
    for B in a.batches.split(","):
        for mix in a.mixes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{B},{mix}", "--res", str(a.res), "--blocks", str(a.blocks),
                   "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"augment_cost.py: batch {B}, mix {mix} ran past {a.limit} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"augment_cost.py: batch {B}, mix {mix} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
