"""GPU box: cost of the normalized cut's passes split over workgroups against the one-workgroup launch -- ViT-S/8 x12, fp16, 480 x 480
and 480 x 640 frames at batches of 1, 8 and 32, and 960 x 960 at batch 1 (split only: the one-workgroup entries refuse it).  Every
configuration (size, batch) runs as a child process under its own time limit; the first child that fails ends the run.  In a child
the legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians over --rounds rounds:

  1. the one-workgroup iterate launch on the ready graph (dinoseg_op_ncut_iterate) with --iters passes and with 0 passes;
  2. the split launches on the same graph (dinoseg_op_ncut_iterate_split) with --iters passes and with 0 passes, once per entry of
     --rows (0 = the library's choice of rows per workgroup); every output is compared with leg 1's, bit for bit;
  3. DINOSeg.ncut and DINOSeg.ncut(split=True) end to end (--iters passes, labels at the frames' size);
  4. the backbone forwards of that call alone (features() in the same chunks).

One JSON line per configuration, appended to --out (default profiles/ncut_split_cost.jsonl), with the prediction written BEFORE
anything was timed beside the measurement.  The prediction, per pass and row workgroup: the redundant preparation is five block sums
(an fp64 xor tree, a barrier, 16 slots: 0.4 us each) and four elementwise sweeps with an fp64 division or square (0.7 us per cell a
thread owns, ceil(n / 1024)); a wave's pair of rows costs a dependent chain of W words, one ds_read_b32, two selects and two adds
per word with the words' scalar loads in front (0.021 us per word: 1.2 us at 57 words), ceil(R / 32) pairs per wave; a launch behind
another on one stream starts 3 us after it ends.  --iters passes are that many such launches and two small ones (8 us each).

    python tools/ncut_split_cost.py [--batches 1,8,32] [--sizes 480x480,480x640] [--big 960x960] [--rows 0] [--rounds 9] [--iters 64]
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

BLOCK_SUM_US = 0.4
SWEEPS_US_PER_OWNED_CELL = 0.7
PAIR_US_PER_WORD = 0.021
LAUNCH_GAP_US = 3.0
SMALL_LAUNCH_US = 8.0
COMPUTE_UNITS = 256


def library_rows(B, n):
    """dinoseg_op_ncut_iterate_split's choice for rows_per_group = 0 (include/dinoseg.h)"""
    R = 32
    while R < n and R < 256 and B * -(-n // R) > COMPUTE_UNITS:
        R += 32
    return R


def predicted(B, n, R, iters):
    """(us of one pass, ms of `iters` passes) of the split launches with R rows per workgroup"""
    words = -(-n // 64)
    prep = 5 * BLOCK_SUM_US + SWEEPS_US_PER_OWNED_CELL * -(-n // 1024)
    waves_of_groups = -(-(B * -(-n // R)) // (2 * COMPUTE_UNITS))       # two workgroups of 1024 threads fit a compute unit
    rows = -(-R // 32) * words * PAIR_US_PER_WORD
    one = waves_of_groups * (prep + rows) + LAUNCH_GAP_US
    return one, (iters * one + 2 * SMALL_LAUNCH_US) / 1e3


def setup(a):
    import torch

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("ncut_split_cost.py needs a ROCm device")
    B, H, W = a.child_batch, a.child_h, a.child_w
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    frames = torch.from_numpy(synthetic_frames(B, H, seed=1, w=W)).cuda()
    return torch, capi, m, cfg, frames


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def append(a, line):
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def child(a):
    torch, capi, m, cfg, frames = setup(a)
    from dino_amd import ncut_start

    B, H, W, chunk = a.child_batch, a.child_h, a.child_w, 32
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n = hp * wp
    lib, S = capi.lib(), capi.stream_ptr
    old = n <= lib.dinoseg_ncut_max_cells()                             # the one-workgroup legs exist at this grid
    rows_list = [int(v) for v in a.rows.split(",")]
    tokens = torch.cat([m.features(frames[c:c + chunk]) for c in range(0, B, chunk)])
    planes = torch.empty((B, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n, D, planes.data_ptr(), S()))
    del tokens
    graph = torch.empty((lib.dinoseg_ncut_split_graph_bytes(B, n) // 8,), dtype=torch.int64, device="cuda")
    degree = torch.empty((B, n), dtype=torch.int32, device="cuda")
    capi.check(lib.dinoseg_op_ncut_graph_split(planes.data_ptr(), B, n, D, a.tau, graph.data_ptr(), degree.data_ptr(), S()))
    scratch = torch.empty((lib.dinoseg_ncut_split_scratch_bytes(B, n),), dtype=torch.uint8, device="cuda")
    start = ncut_start(n, 0).cuda().expand(B, n).contiguous()

    def outputs():
        return dict(z=torch.empty_like(start), rho=torch.empty((B, max(a.iters, 1)), dtype=torch.float32, device="cuda"),
                    fg=torch.empty((B, n), dtype=torch.uint8, device="cuda"), eig=torch.empty((B, n), dtype=torch.float32, device="cuda"),
                    seed=torch.empty((B,), dtype=torch.int32, device="cuda"))

    o1, o2 = outputs(), outputs()

    def iterate(iters):
        capi.check(lib.dinoseg_op_ncut_iterate(graph.data_ptr(), degree.data_ptr(), B, n, 1e-5, start.data_ptr(), iters, o1["z"].data_ptr(),
                                               o1["rho"].data_ptr(), o1["fg"].data_ptr(), o1["eig"].data_ptr(), None, o1["seed"].data_ptr(),
                                               S()))

    def split(iters, rows):
        capi.check(lib.dinoseg_op_ncut_iterate_split(graph.data_ptr(), degree.data_ptr(), B, n, 1e-5, start.data_ptr(), iters, rows,
                                                     o2["z"].data_ptr(), o2["rho"].data_ptr(), o2["fg"].data_ptr(), o2["eig"].data_ptr(),
                                                     None, o2["seed"].data_ptr(), scratch.data_ptr(), S()))

    def ncut(**kw):
        return m.ncut(frames, tau=a.tau, iters=a.iters, chunk=chunk, **kw)

    def forwards():
        for c in range(0, B, chunk):
            m.features(frames[c:c + chunk])

    same = None
    for _ in range(2):                                              # warm-up of every leg
        if old:
            iterate(0)
            iterate(a.iters)
        for rows in rows_list:
            split(0, rows)
            split(a.iters, rows)
            if old:                                                     # the same bits as the one-workgroup launch, every output
                torch.cuda.synchronize()
                same = (same is None or same) and all(torch.equal(o1[k].view(torch.uint8), o2[k].view(torch.uint8)) for k in o1)
    if old:
        ncut()
    ncut(split=True)
    forwards()
    t_iter, t_zero, t_ncut, t_ncut_split, t_fwd = [], [], [], [], []
    t_split = {rows: [] for rows in rows_list}
    t_split_zero = {rows: [] for rows in rows_list}
    for _ in range(a.rounds):
        if old:
            t_iter.append(timed(torch, lambda: iterate(a.iters))[0])
            t_zero.append(timed(torch, lambda: iterate(0))[0])
        for rows in rows_list:
            t_split[rows].append(timed(torch, lambda: split(a.iters, rows))[0])
            t_split_zero[rows].append(timed(torch, lambda: split(0, rows))[0])
        if old:
            t_ncut.append(timed(torch, ncut)[0])
        t_ncut_split.append(timed(torch, lambda: ncut(split=True))[0])
        t_fwd.append(timed(torch, forwards)[0])
    med = statistics.median
    line = {"frame": [H, W], "grid": [hp, wp], "batch": B, "cells": n, "tau": a.tau, "precision": a.precision, "rounds": a.rounds,
            "iters": a.iters, "library_rows_per_group": library_rows(B, n), "split": []}
    for rows in rows_list:
        R = rows or library_rows(B, n)
        one, total = predicted(B, n, R, a.iters)
        ms, zero = med(t_split[rows]), med(t_split_zero[rows])
        line["split"].append({"rows_per_group": rows, "rows": R, "row_workgroups": B * -(-n // R), "iterate_split_ms": round(ms, 4),
                              "iterate_split_ms_min_max": [round(min(t_split[rows]), 4), round(max(t_split[rows]), 4)],
                              "iterate_split_zero_passes_ms": round(zero, 4), "pass_us": round((ms - zero) / max(a.iters, 1) * 1e3, 3),
                              "predicted_pass_us": round(one, 2), "predicted_iterate_split_ms": round(total, 3)})
    if old:
        line.update({"iterate_ms": round(med(t_iter), 3), "iterate_ms_min_max": [round(min(t_iter), 3), round(max(t_iter), 3)],
                     "iterate_zero_passes_ms": round(med(t_zero), 3),
                     "iterate_over_split": round(med(t_iter) / med(t_split[rows_list[0]]), 2), "same_bits": bool(same),
                     "ncut_ms": round(med(t_ncut), 3), "ncut_ms_min_max": [round(min(t_ncut), 3), round(max(t_ncut), 3)]})
    line.update({"ncut_split_ms": round(med(t_ncut_split), 3),
                 "ncut_split_ms_min_max": [round(min(t_ncut_split), 3), round(max(t_ncut_split), 3)],
                 "backbone_forwards_ms": round(med(t_fwd), 3), "scratch_bytes": int(scratch.numel()), "graph_bytes": int(graph.numel() * 8)})
    append(a, line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--big", default="960x960", help="sizes run at batch 1 only (split only where the one-workgroup entries refuse them)")
    ap.add_argument("--rows", default="0", help="rows per workgroup to time, comma separated; 0 = the library's choice; the first is the ratio's")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncut_split_cost.jsonl"))
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_batch is not None:
        return child(a)
    configs = [(size, int(B)) for size in a.sizes.split(",") if size for B in a.batches.split(",")]
    configs += [(size, 1) for size in a.big.split(",") if size]
    for size, B in configs:
        H, W = (int(v) for v in size.split("x"))
        cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--iters", str(a.iters),
               "--tau", str(a.tau), "--rows", a.rows, "--out", a.out, "--child-batch", str(B), "--child-h", str(H), "--child-w", str(W)]
        try:
            rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"ncut_split_cost.py: {size} batch {B} ran past {a.child_timeout} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"ncut_split_cost.py: {size} batch {B} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
