"""GPU box: cost of the image-guided iterative refinement -- ViT-S/8 x12 @480, fp16, at 2, 7 and 21 classes, batch 1 and 8, PAMR's
dilations.  Every configuration (classes, batch) runs as a child process under its own time limit; the first child that fails ends
the run.  In a child five legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians over
--rounds rounds:

  1. one pass (dinoseg_op_refine_iterate, iters = 1, labels only) on a seeded state; also timed back to back (20 per synchronise);
  2. ten passes (iters = 10, labels only);
  3. segment_refined(frames): the forward + the seed + ten passes;
  4. segment(frames): the forward + the bilinear upsample + argmax;
  5. the torch route for one pass on a ready state with ready weights: F.pad(mode="replicate"), 48 shifted slices stacked into a
     [B, C, 48, OH, OW] tensor, times the weights, summed.

Also the torch peak-memory delta of legs 3, 4 and 5.  One JSON line per configuration, appended to --out (default
profiles/refine_cost.jsonl), with the prediction of one pass beside the measurement (DESIGN.md has its derivation): per class pass
about 1550 vector operations per pixel for the weights, 3 per tap and class for the walk, at 39e12 lane operations per second, plus
4.375 staged words per pixel and class at 4 TB/s, not overlapped.

    python tools/refine_cost.py [--classes 2,7,21] [--batches 1,8] [--res 480] [--precision fp16] [--rounds 30]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DILATIONS = (1, 2, 4, 8, 12, 24)
LANE_OPS_PER_S = 256 * 64 * 2.4e9       # one wave instruction per CU and clock
STAGE_BYTES_PER_S = 4e12


def predicted_ms(B, r, C):
    """one pass: the weights once per class pass of 3 (2 with two classes), the walk, the staging of a 112 x 80 footprint per tile"""
    pixels = B * r * r
    passes = -(-C // min(C, 3))
    valu = pixels * (passes * 1550 + C * 48 * 3) / LANE_OPS_PER_S
    stage = pixels * C * 4.375 * 4 / STAGE_BYTES_PER_S
    return (valu + stage) * 1e3


def child(a):
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("refine_cost.py needs a ROCm device")

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

    C, B, r = a.child_classes, a.child_batch, a.res
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    cfg = ViTConfig(n_blocks=12, n_classes=C)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    m.set_resolution(r)
    hp = r // cfg.patch
    logp, _ = m.forward_frames(frames)
    lib, S = capi.lib(), capi.stream_ptr
    scratch = torch.empty((2, B, C, r, r), dtype=torch.float32, device="cuda")
    lab = torch.empty((B, r, r), dtype=torch.int32, device="cuda")
    dil = (ctypes.c_int32 * len(DILATIONS))(*DILATIONS)
    capi.check(lib.dinoseg_op_refine_seed(logp.data_ptr(), 1, B, C, r, r, hp, hp, 1.0, scratch.data_ptr(), S()))
    state = scratch[0].clone()

    def passes(n):
        capi.check(lib.dinoseg_op_refine_iterate(frames.data_ptr(), scratch.data_ptr(), B, C, r, r, dil, len(DILATIONS), 0.1, n,
                                                 lab.data_ptr(), None, S()))

    # the torch route's ready weights [B, 48, OH, OW] (any positive weights cost the same)
    D = max(DILATIONS)
    offsets = [(dy, dx) for d in DILATIONS for dy in (-d, 0, d) for dx in (-d, 0, d) if (dy, dx) != (0, 0)]
    weights = torch.softmax(torch.randn((B, len(offsets), r, r), device="cuda"), dim=1)

    def torch_pass():
        p = F.pad(state, (D, D, D, D), mode="replicate")
        taps = torch.stack([p[:, :, D + dy:D + dy + r, D + dx:D + dx + r] for dy, dx in offsets], 2)
        return (taps * weights[:, None]).sum(2)

    for _ in range(3):                                          # warm-up of every leg
        passes(1)
        passes(10)
        m.segment_refined(frames)
        m.segment(frames)
        torch_pass()
    t_one, t_ten, t_ref, t_seg, t_torch = [], [], [], [], []
    for _ in range(a.rounds):
        t_one.append(timed(lambda: passes(1))[0])
        t_ten.append(timed(lambda: passes(10))[0])
        t_ref.append(timed(lambda: m.segment_refined(frames))[0])
        t_seg.append(timed(lambda: m.segment(frames))[0])
        t_torch.append(timed(torch_pass)[0])
    t_back = timed(lambda: [passes(1) for _ in range(20)])[0] / 20
    mem_ref, (labels, _) = peak_delta(lambda: m.segment_refined(frames))
    mem_seg, (plain, _) = peak_delta(lambda: m.segment(frames))
    mem_torch, _ = peak_delta(torch_pass)
    differ = float((labels != plain).double().mean())
    one, ten, rf, sg, tp = (statistics.median(t) for t in (t_one, t_ten, t_ref, t_seg, t_torch))
    line = {"n_classes": C, "precision": a.precision, "batch": B, "res": r, "dilations": list(DILATIONS), "rounds": a.rounds,
            "pass_synchronised_ms": round(one, 4), "pass_back_to_back_ms": round(t_back, 4), "ten_passes_ms": round(ten, 4),
            "predicted_pass_ms": round(predicted_ms(B, r, C), 4), "torch_pass_ms": round(tp, 3),
            "segment_refined_ms": round(rf, 3), "segment_ms": round(sg, 3), "refined_minus_segment_ms": round(rf - sg, 3),
            "segment_refined_ms_min_max": [round(min(t_ref), 3), round(max(t_ref), 3)],
            "segment_ms_min_max": [round(min(t_seg), 3), round(max(t_seg), 3)],
            "segment_refined_peak_bytes": int(mem_ref), "segment_peak_bytes": int(mem_seg), "torch_pass_peak_bytes": int(mem_torch),
            "labels_differ_from_bilinear": round(differ, 6)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="2,7,21")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--child-timeout", type=int, default=180, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_cost.jsonl"))
    ap.add_argument("--child-classes", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_classes is not None:
        return child(a)
    for C in (int(v) for v in a.classes.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--res", str(a.res), "--precision", a.precision, "--rounds", str(a.rounds),
                   "--out", a.out, "--child-classes", str(C), "--child-batch", str(B)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"refine_cost.py: classes={C} batch={B} ran past {a.child_timeout} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"refine_cost.py: classes={C} batch={B} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
