"""GPU box: cost of multi-object discovery (DINOSeg.discover_all, dinoseg_op_maskcut) -- ViT-S/8 x12, fp16, 480 x 480 and 480 x 640
frames at batches of 1, 8 and 32, K = --objects rounds of --iters passes.  Every configuration (size, batch) runs as a child process
under its own time limit; the first child that fails ends the run.  In a child the legs are interleaved after warm-up, each timed with
a host clock around a synchronised call, medians over --rounds rounds:

  1. the entry alone on a ready graph (dinoseg_op_maskcut; the graph is restored from a copy outside the clock, the entry consumes it);
  2. K calls of dinoseg_op_ncut_iterate_split and K calls of dinoseg_op_components on the same buffers: what the rounds cost without
     the new launches; leg 1 minus these two is the new launches' share (init, K x (mask, candidates + records, select), count);
  3. DINOSeg.discover_all end to end (labels at the frames' size);
  4. the backbone forwards of that call alone (features() in the same chunks);
  5. the route the entry replaces, from the same ready graph on: per round the graph masked and the degree recounted by torch
     operators ON THE DEVICE (no copy to the host: the cheapest form of that route), dinoseg_op_ncut_iterate_split, then discover's own
     bookkeeping (DINOSeg._discover_from: dinoseg_op_components with the full table, the gathers and where, one enlargement per round)
     and the torch update of alive.  Its cells are compared with the entry's, round by round.

One JSON line per configuration, appended to --out (default profiles/maskcut_cost.jsonl), with the prediction written BEFORE anything
was timed beside the measurement.  The prediction is built from measured figures of the README: K x the split cut (64 passes: 0.87 /
1.39 / 4.96 ms at 480 x 480 and 1.04 / 2.16 / 8.68 ms at 480 x 640, batch 1 / 8 / 32, scaled by iters / 64), K x the components on the
patch grid (79 / 88 / 124 us), and per round three new launches: the mask streams 2 B n^2 / 8 bytes (read and written once: 3.2 MB at
3600 cells, 0.5 us at 6.3 TB/s) behind a 3 us launch boundary with 2 us of start-up and tail, the candidates launch 5 us, the select
launch (one workgroup per frame, ceil(n / 1024) cells per thread, two barriers) 8 us; init and count 5 us each once; one enlargement
of K + 1 channels 25 us.

    python tools/maskcut_cost.py [--batches 1,8,32] [--sizes 480x480,480x640] [--objects 3] [--rounds 9] [--iters 64]
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

ITERATE_MS_64 = {(3600, 1): 0.87, (3600, 8): 1.39, (3600, 32): 4.96, (4800, 1): 1.04, (4800, 8): 2.16, (4800, 32): 8.68}
COMPONENTS_US = {1: 79.0, 8: 88.0, 32: 124.0}
HBM_BYTES_PER_US = 6.3e6
LAUNCH_US = 5.0
SELECT_US = 8.0
ENLARGE_US = 25.0


def predicted(B, n, K, iters):
    """ms: (the entry, its new launches alone, discover_all after the forwards and the graph launch)"""
    mask = 3.0 + 2.0 + 2.0 * B * n * n / 8.0 / HBM_BYTES_PER_US
    new = 2 * LAUNCH_US + K * (mask + LAUNCH_US + SELECT_US)
    cut = ITERATE_MS_64.get((n, B))
    comp = COMPONENTS_US.get(B)
    if cut is None or comp is None:
        return None, round(new / 1e3, 4), None
    entry = K * (cut * iters / 64.0 + comp / 1e3) + new / 1e3
    return round(entry, 3), round(new / 1e3, 4), round(entry + ENLARGE_US / 1e3, 3)


def setup(a):
    import torch

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("maskcut_cost.py needs a ROCm device")
    B, H, W = a.child_batch, a.child_h, a.child_w
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    frames = torch.from_numpy(synthetic_frames(B, H, seed=1, w=W)).cuda()
    return torch, capi, m, cfg, frames


def timed(torch, fn, before=None):
    if before is not None:
        before()
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


def popcount64(torch, x):
    """set bits of every int64 element (SWAR; the shifts are arithmetic, the masks remove what they drag in)"""
    x = x - ((x >> 1) & 0x5555555555555555)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + ((x >> 4) & 0x0FFFFFFFFFFFFFFF)) & 0x0F0F0F0F0F0F0F0F
    for s in (8, 16, 32):
        x = x + ((x >> s) & ((1 << (64 - s)) - 1))
    return x & 0x7F


def child(a):
    torch, capi, m, cfg, frames = setup(a)
    from dino_amd import ncut_start

    B, H, W, chunk, K, iters = a.child_batch, a.child_h, a.child_w, 32, a.objects, a.iters
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n = hp * wp
    Wd = -(-n // 64)
    lib, S = capi.lib(), capi.stream_ptr
    pred = predicted(B, n, K, iters)                                   # (before anything is timed)
    tokens = torch.cat([m.features(frames[c:c + chunk]) for c in range(0, B, chunk)])
    planes = torch.empty((B, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n, D, planes.data_ptr(), S()))
    del tokens
    original = torch.empty((B, n, Wd), dtype=torch.int64, device="cuda")
    degree0 = torch.empty((B, n), dtype=torch.int32, device="cuda")
    capi.check(lib.dinoseg_op_ncut_graph_split(planes.data_ptr(), B, n, D, a.tau, original.data_ptr(), degree0.data_ptr(), S()))
    graph, degree = original.clone(), degree0.clone()
    start = ncut_start(n, 0).cuda().expand(B, n).contiguous()
    scratch = torch.empty((lib.dinoseg_maskcut_scratch_bytes(B, hp, wp, K),), dtype=torch.uint8, device="cuda")
    split_scratch = torch.empty((lib.dinoseg_ncut_split_scratch_bytes(B, n),), dtype=torch.uint8, device="cuda")
    cc_scratch = torch.empty((lib.dinoseg_components_scratch_bytes(B, hp, wp),), dtype=torch.uint8, device="cuda")

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device="cuda")

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device="cuda")

    def u8(*shape):
        return torch.empty(shape, dtype=torch.uint8, device="cuda")

    o = dict(cells=u8(B, K, n), found=u8(B, K), area=i32(B, K), box=i32(B, K, 4), score=f32(B, n, K + 1), count=i32(B), fg=u8(B, K, n),
             margin=f32(B, K, n), eigvec=f32(B, K, n), seed=i32(B, K), rho=f32(B, K, max(iters, 1)))
    w = dict(z=f32(B, n), rho=f32(B, max(iters, 1)), fg=u8(B, n), eig=f32(B, n), margin=f32(B, n), seed=i32(B))
    cc = dict(ids=i32(B, hp, wp), count=i32(B), first=i32(B, 1), label=i32(B, 1), area=i32(B, 1), box=i32(B, 1, 4), status=i32(B))

    def restore():
        graph.copy_(original)
        degree.copy_(degree0)

    def entry():
        capi.check(lib.dinoseg_op_maskcut(graph.data_ptr(), degree.data_ptr(), B, hp, wp, 1e-5, start.data_ptr(), iters, 0, 4, K,
                                          o["cells"].data_ptr(), o["found"].data_ptr(), o["area"].data_ptr(), o["box"].data_ptr(),
                                          o["score"].data_ptr(), o["count"].data_ptr(), o["fg"].data_ptr(), o["margin"].data_ptr(),
                                          o["eigvec"].data_ptr(), o["seed"].data_ptr(), o["rho"].data_ptr(), scratch.data_ptr(), S()))

    def iterate(g, d):
        capi.check(lib.dinoseg_op_ncut_iterate_split(g.data_ptr(), d.data_ptr(), B, n, 1e-5, start.data_ptr(), iters, 0, w["z"].data_ptr(),
                                                     w["rho"].data_ptr(), w["fg"].data_ptr(), w["eig"].data_ptr(), w["margin"].data_ptr(),
                                                     w["seed"].data_ptr(), split_scratch.data_ptr(), S()))

    def cuts_alone():
        for _ in range(K):
            iterate(graph, degree)

    def components_alone():
        cand = o["fg"][:, 0].to(torch.int32).view(B, hp, wp).contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            capi.check(lib.dinoseg_op_components(cand.data_ptr(), B, hp, wp, 4, 0, 1, cc["ids"].data_ptr(), cc["count"].data_ptr(),
                                                 cc["first"].data_ptr(), cc["label"].data_ptr(), cc["area"].data_ptr(), cc["box"].data_ptr(),
                                                 cc["status"].data_ptr(), cc_scratch.data_ptr(), S()))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    weights = (torch.ones((), dtype=torch.int64, device="cuda") << torch.arange(64, device="cuda")).view(1, 1, 64)

    def torch_route():
        """the replaced route on the device: returns the rounds' cells uint8 [B, K, n]"""
        g = original.clone()
        alive = torch.ones((B, n), dtype=torch.bool, device="cuda")
        cells_all = []
        for _ in range(K):
            padded = torch.zeros((B, Wd * 64), dtype=torch.int64, device="cuda")
            padded[:, :n] = alive
            words = (padded.view(B, Wd, 64) * weights).sum(2)          # (bit 63 wraps to the sign bit: the same 64 bits)
            g = torch.where(alive.view(B, n, 1), g & words.view(B, 1, Wd), torch.zeros_like(g))
            d = popcount64(torch, g).sum(2).to(torch.int32)
            iterate(g, d)
            fg = w["fg"] * alive.to(torch.uint8)
            _, _, _, cells, _ = m._discover_from(w["margin"], fg, w["seed"], hp, wp, H, W, 4)
            alive = alive & (cells == 0)
            cells_all.append(cells)
        return torch.stack(cells_all, dim=1)

    def end_to_end():
        return m.discover_all(frames, max_objects=K, tau=a.tau, iters=iters, chunk=chunk)

    def forwards():
        for c in range(0, B, chunk):
            m.features(frames[c:c + chunk])

    same = True
    for _ in range(2):                                                  # warm-up of every leg
        restore()
        entry()
        cuts_alone()
        components_alone()
        old_cells = torch_route()
        torch.cuda.synchronize()
        same = same and bool(torch.equal(old_cells, o["cells"]))
        end_to_end()
        forwards()
    t = {k: [] for k in ("entry", "cuts", "components", "torch_route", "discover_all", "forwards")}
    for _ in range(a.rounds):
        t["entry"].append(timed(torch, entry, before=restore)[0])
        t["cuts"].append(timed(torch, cuts_alone)[0])
        t["components"].append(components_alone())
        t["torch_route"].append(timed(torch, torch_route)[0])
        t["discover_all"].append(timed(torch, end_to_end)[0])
        t["forwards"].append(timed(torch, forwards)[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    line = {"frame": [H, W], "grid": [hp, wp], "batch": B, "cells": n, "objects": K, "iters": iters, "tau": a.tau, "precision": a.precision,
            "rounds": a.rounds, "predicted_entry_ms": pred[0], "predicted_new_launches_ms": pred[1],
            "predicted_discover_all_after_graph_ms": pred[2], "found": o["found"].cpu().tolist(), "torch_route_same_cells": same,
            "new_launches_ms": round(med["entry"] - med["cuts"] - med["components"], 4),
            "discover_all_minus_forwards_ms": round(med["discover_all"] - med["forwards"], 3),
            "torch_route_over_entry": round(med["torch_route"] / med["entry"], 2), "scratch_bytes": int(scratch.numel()),
            "graph_bytes": int(graph.numel() * 8)}
    for k, v in t.items():
        line[k + "_ms"] = round(med[k], 4)
        line[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    append(a, line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskcut_cost.jsonl"))
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_batch is not None:
        return child(a)
    for size, B in [(size, int(B)) for size in a.sizes.split(",") if size for B in a.batches.split(",")]:
        H, W = (int(v) for v in size.split("x"))
        cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--iters", str(a.iters),
               "--tau", str(a.tau), "--objects", str(a.objects), "--out", a.out, "--child-batch", str(B), "--child-h", str(H), "--child-w",
               str(W)]
        try:
            rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"maskcut_cost.py: {size} batch {B} ran past {a.child_timeout} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"maskcut_cost.py: {size} batch {B} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
