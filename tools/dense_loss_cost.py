"""GPU box: cost of the fine-tune step on pixel labels -- ViT-S/8 x3 @480, batch 8, bf16, at 7 and 150 classes.  Three routes,
interleaved in one process after warm-up, each timed with a host clock around a synchronised call, medians over --rounds rounds:

  1. fused_training_step on patch labels [B, 3600] (what the step costs without pixel labels);
  2. fused_training_step_dense on pixel labels [B, 480, 480]: the forward, the fused upsample + cross-entropy + gradient
     (csrc/upsample_loss.hip) and the backward in one native call;
  3. the torch route a user writes without it: dinoseg_train_forward_hw, then F.interpolate + F.cross_entropy(ignore_index=255) +
     autograd on the low-res log-probs, then dinoseg_backward of the gradient autograd returns.

The loss launches alone are timed too (20 back-to-back calls of dinoseg_op_upsample_nll on the step's log-probs), and the torch
peak-memory delta of every route is recorded.  Each class count runs in a child process of its own under `timeout`; the first
child that fails ends the run.  One JSON line per class count, appended to --out (default profiles/dense_loss_cost.jsonl).

    python tools/dense_loss_cost.py [--classes 7,150] [--batch 8] [--res 480] [--blocks 3] [--precision bf16] [--rounds 200]
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


def child(a, C):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames, synthetic_labels

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

    if not torch.cuda.is_available():
        raise SystemExit("dense_loss_cost.py needs a ROCm device")
    B, r = a.batch, a.res
    cfg = ViTConfig(n_blocks=a.blocks, n_classes=C)
    m = DINOSeg(head=cfg.head, n_blocks=a.blocks, n_classes=C, precision=a.precision, arch=cfg, freeze_backbone=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    m.unfreeze_bb()
    hp = r // cfg.patch
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    y_patch = torch.from_numpy(synthetic_labels(B, hp * hp, C, seed=2)).cuda()
    rng = np.random.default_rng(3)
    y_pix = rng.integers(0, C, (B, r, r)).astype(np.int64)
    y_pix[rng.random((B, r, r)) < 0.1] = 255
    y_pix = torch.from_numpy(y_pix).cuda()
    lib = capi.lib()

    def torch_route():
        logp = torch.empty((B * hp * hp, C), dtype=torch.float32, device="cuda")
        capi.check(lib.dinoseg_train_forward_hw(m._handle, frames.data_ptr(), capi.INPUT_U8_HWC, B, r, r, logp.data_ptr(), capi.stream_ptr()))
        lp = logp.requires_grad_()
        up = F.interpolate(lp.view(B, hp, hp, C).permute(0, 3, 1, 2), size=(r, r), mode="bilinear", align_corners=False)
        loss = F.cross_entropy(up, y_pix, ignore_index=255)
        (d,) = torch.autograd.grad(loss, lp)
        d = d.contiguous()
        capi.check(lib.dinoseg_backward(m._handle, d.data_ptr(), capi.stream_ptr()))
        return loss.detach()

    routes = (lambda: m.fused_training_step((frames, y_patch))["loss"], lambda: m.fused_training_step_dense((frames, y_pix))["loss"],
              torch_route)
    for _ in range(3):                                          # warm-up of every route
        for fn in routes:
            fn()
    times = ([], [], [])
    for _ in range(a.rounds):
        for t, fn in zip(times, routes):
            t.append(timed(fn)[0])
    mem = [peak_delta(fn) for fn in routes]
    loss_dense, loss_torch = float(mem[1][1]), float(mem[2][1])
    # the loss launches alone, on the log-probs of the last step
    logp = m.fused_training_step_dense((frames, y_pix))["probs"]
    nbytes = lib.dinoseg_op_upsample_nll_scratch_bytes(B, hp, hp, C, r, r)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    loss = torch.zeros((), device="cuda")
    d = torch.empty_like(logp)
    op = lambda: capi.check(lib.dinoseg_op_upsample_nll(logp.data_ptr(), B, hp, hp, C, r, r, y_pix.data_ptr(), 255, loss.data_ptr(),
                                                       d.data_ptr(), None, None, scratch.data_ptr(), capi.stream_ptr()))
    op()
    t_op = timed(lambda: [op() for _ in range(20)])[0] / 20
    patch, dense, tor = (statistics.median(t) for t in times)
    line = {"n_classes": C, "precision": a.precision, "batch": B, "res": r, "n_blocks": a.blocks, "rounds": a.rounds,
            "patch_step_ms": round(patch, 3), "dense_step_ms": round(dense, 3), "torch_route_ms": round(tor, 3),
            "dense_minus_patch_ms": round(dense - patch, 3), "torch_over_dense": round(tor / dense, 3),
            "upsample_nll_op_ms": round(t_op, 4), "scratch_bytes": int(nbytes),
            "patch_step_ms_min_max": [round(min(times[0]), 3), round(max(times[0]), 3)],
            "dense_step_ms_min_max": [round(min(times[1]), 3), round(max(times[1]), 3)],
            "torch_route_ms_min_max": [round(min(times[2]), 3), round(max(times[2]), 3)],
            "patch_step_peak_bytes": int(mem[0][0]), "dense_step_peak_bytes": int(mem[1][0]), "torch_route_peak_bytes": int(mem[2][0]),
            "dense_loss": round(loss_dense, 6), "torch_loss": round(loss_torch, 6)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each class count's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_loss_cost.jsonl"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        child(a, a.child)
        return
    for C in (int(c) for c in a.classes.split(",")):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(C), "--batch",
               str(a.batch), "--res", str(a.res), "--blocks", str(a.blocks), "--precision", a.precision, "--rounds", str(a.rounds),
               "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"dense_loss_cost.py: the run at {C} classes ended with status {rc}; nothing further was started")


if __name__ == "__main__":
    main()
