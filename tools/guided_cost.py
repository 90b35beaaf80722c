"""GPU box: cost of the image-guided pixel-resolution output -- ViT-S/8 x12 @480, fp16, at 7 and 150 classes, radius 2 and 3, batch 8
and 32.  Every configuration (classes, batch, radius) runs as a child process under its own time limit; the first child that fails
ends the run.  In a child three legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians
over --rounds rounds:

  1. segment_guided(frames): the forward + the cell colours + the guided upsample + argmax (csrc/upsample_guided.hip);
  2. the two launches alone (dinoseg_op_guide_cells + dinoseg_op_upsample_guided on log-probs computed beforehand), also timed back
     to back (20 pairs per synchronise: guided_launches_ms), since leg 1 minus leg 3 is a small difference of two ~13 ms calls;
  3. segment(frames): the forward + the bilinear upsample + argmax.

Also the torch peak-memory delta of legs 1 and 3.  One JSON line per configuration, appended to --out (default
profiles/guided_cost.jsonl), with the LDS-traffic prediction of the guided launch beside the measurement: one ds_read_b32 per pixel,
tap and class at 128 B/clk/CU (about 75 TB/s chip-wide).

    python tools/guided_cost.py [--classes 7,150] [--batches 8,32] [--radii 2,3] [--res 480] [--precision fp16] [--rounds 60]
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

LDS_READ_BYTES_PER_S = 75e12        # ds_read_b32, every CU streaming


def predicted_ms(B, r, C, R):
    """the guided launch from its LDS reads alone: B r^2 (2R+1)^2 C lane reads of 4 bytes"""
    return B * r * r * (2 * R + 1) ** 2 * C * 4 / LDS_READ_BYTES_PER_S * 1e3


def child(a):
    import torch

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("guided_cost.py needs a ROCm device")

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

    C, B, R, r = a.child_classes, a.child_batch, a.child_radius, a.res
    frames = torch.from_numpy(synthetic_frames(B, r, seed=1)).cuda()
    cfg = ViTConfig(n_blocks=12, n_classes=C)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=C, precision=a.precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    m.set_resolution(r)
    hp = r // cfg.patch
    logp, _ = m.forward_frames(frames)
    lib, S = capi.lib(), capi.stream_ptr
    cells = torch.empty((B, hp, hp), dtype=torch.int32, device="cuda")
    lab = torch.empty((B, r, r), dtype=torch.int32, device="cuda")

    def launches():
        capi.check(lib.dinoseg_op_guide_cells(frames.data_ptr(), B, r, r, hp, hp, cells.data_ptr(), S()))
        capi.check(lib.dinoseg_op_upsample_guided(logp.data_ptr(), frames.data_ptr(), cells.data_ptr(), B, hp, hp, C, r, r, R, 1.0, 0.1,
                                                  lab.data_ptr(), None, S()))

    def cells_only():
        capi.check(lib.dinoseg_op_guide_cells(frames.data_ptr(), B, r, r, hp, hp, cells.data_ptr(), S()))

    for _ in range(3):                                          # warm-up of every leg
        m.segment_guided(frames, radius=R)
        launches()
        m.segment(frames)
    t_guided, t_pair, t_seg = [], [], []
    for _ in range(a.rounds):
        t_guided.append(timed(lambda: m.segment_guided(frames, radius=R))[0])
        t_pair.append(timed(launches)[0])
        t_seg.append(timed(lambda: m.segment(frames))[0])
    t_back = timed(lambda: [launches() for _ in range(20)])[0] / 20
    t_cells = timed(lambda: [cells_only() for _ in range(20)])[0] / 20
    mem_guided, (labels, _) = peak_delta(lambda: m.segment_guided(frames, radius=R))
    mem_seg, (plain, _) = peak_delta(lambda: m.segment(frames))
    differ = float((labels != plain).double().mean())
    gd, pr, sg = (statistics.median(t) for t in (t_guided, t_pair, t_seg))
    line = {"n_classes": C, "precision": a.precision, "batch": B, "res": r, "radius": R, "rounds": a.rounds,
            "segment_guided_ms": round(gd, 3), "segment_ms": round(sg, 3), "guided_minus_segment_ms": round(gd - sg, 3),
            "launches_synchronised_ms": round(pr, 3), "guided_launches_ms": round(t_back, 4), "guide_cells_ms": round(t_cells, 4),
            "upsample_guided_ms": round(t_back - t_cells, 4), "predicted_lds_ms": round(predicted_ms(B, r, C, R), 4),
            "segment_guided_ms_min_max": [round(min(t_guided), 3), round(max(t_guided), 3)],
            "segment_ms_min_max": [round(min(t_seg), 3), round(max(t_seg), 3)],
            "segment_guided_peak_bytes": int(mem_guided), "segment_peak_bytes": int(mem_seg),
            "labels_differ_from_bilinear": round(differ, 6)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--radii", default="2,3")
    ap.add_argument("--res", type=int, default=480)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_cost.jsonl"))
    ap.add_argument("--child-classes", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-radius", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_classes is not None:
        return child(a)
    for C in (int(v) for v in a.classes.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            for R in (int(v) for v in a.radii.split(",")):
                cmd = [sys.executable, os.path.abspath(__file__), "--res", str(a.res), "--precision", a.precision, "--rounds", str(a.rounds),
                       "--out", a.out, "--child-classes", str(C), "--child-batch", str(B), "--child-radius", str(R)]
                try:
                    rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"guided_cost.py: classes={C} batch={B} radius={R} ran past {a.child_timeout} s; nothing more is started")
                if rc != 0:
                    raise SystemExit(f"guided_cost.py: classes={C} batch={B} radius={R} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
