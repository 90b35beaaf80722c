"""GPU box: cost of the normalized cut on the 1-bit patch graph -- ViT-S/8 x12, fp16, 480 x 480 and 480 x 640 frames, batches of 1, 8
and 32.  Every configuration (size, batch) runs as a child process under its own time limit; the first child that fails ends the
run.  In a child four legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians over
--rounds rounds:

  1. the graph launch alone on ready planes (dinoseg_op_ncut_graph), also timed back to back (10 launches per synchronise);
  2. the iterate launch alone on the ready graph (dinoseg_op_ncut_iterate) with --iters passes and with 0 passes: per pass =
     (the difference) / iters;
  3. DINOSeg.ncut end to end (--iters passes, labels at the frames' size);
  4. the backbone forwards of that call alone (features() in the same chunks).

Also the torch peak-memory delta of legs 1 + 2 and of leg 3.  At batch 1 a further child, under its own generous time limit, runs the
torch route on the same ready features: bmm, threshold, the normalised matrix, torch.linalg.eigh (a few rounds: it may take seconds).
One JSON line per configuration, appended to --out (default profiles/ncut_cost.jsonl), with the prediction written BEFORE anything was
measured beside the measurement: the graph launch's MFMA work (3 . 2 n^2 D per frame at the 2.5 PFLOP/s dense peak) and its staging
traffic (every (query tile, key block, slice) stages 32 KiB from L2), and the iterate pass's LDS reads on ONE compute unit (n words
of 64 keys per row, 4 bytes per key, at 128 bytes per clock of ds_read_b32 and 2.4 GHz).

    python tools/ncut_cost.py [--batches 1,8,32] [--sizes 480x480,480x640] [--precision fp16] [--rounds 9] [--iters 64]
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

MFMA_FLOPS = 2.5e15                 # v_mfma_f32_32x32x16_f16, dense peak
L2_BYTES_PER_S = 1.0e13             # staged tiles, all compute units reading
LDS_BYTES_PER_CLK = 128             # ds_read_b32 on one compute unit
CLOCK_HZ = 2.4e9


def predicted(B, n, D):
    """(ms of the graph launch from the MFMA work alone, ms from its staging traffic alone, ms of one iterate pass from its LDS reads
    on one compute unit)"""
    tiles = (n + 63) // 64
    flops = B * 3 * 2 * n * n * D
    staged = B * tiles * tiles * (D // 64) * 32768
    lds = n * tiles * 64 * 4
    return flops / MFMA_FLOPS * 1e3, staged / L2_BYTES_PER_S * 1e3, lds / LDS_BYTES_PER_CLK / CLOCK_HZ * 1e3


def setup(a):
    import torch

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("ncut_cost.py needs a ROCm device")
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


def peak_delta(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


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
    tokens = torch.cat([m.features(frames[c:c + chunk]) for c in range(0, B, chunk)])
    planes = torch.empty((B, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n, D, planes.data_ptr(), S()))
    del tokens
    graph = torch.empty((lib.dinoseg_ncut_graph_bytes(B, n) // 8,), dtype=torch.int64, device="cuda")
    degree = torch.empty((B, n), dtype=torch.int32, device="cuda")
    start = ncut_start(n, 0).cuda().expand(B, n).contiguous()
    z = torch.empty_like(start)
    rho = torch.empty((B, max(a.iters, 1)), dtype=torch.float32, device="cuda")
    fg = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    eig = torch.empty((B, n), dtype=torch.float32, device="cuda")
    seed = torch.empty((B,), dtype=torch.int32, device="cuda")

    def build():
        capi.check(lib.dinoseg_op_ncut_graph(planes.data_ptr(), B, n, D, a.tau, graph.data_ptr(), degree.data_ptr(), S()))

    def iterate(iters):
        capi.check(lib.dinoseg_op_ncut_iterate(graph.data_ptr(), degree.data_ptr(), B, n, 1e-5, start.data_ptr(), iters, z.data_ptr(),
                                               rho.data_ptr(), fg.data_ptr(), eig.data_ptr(), None, seed.data_ptr(), S()))

    def ncut():
        return m.ncut(frames, tau=a.tau, iters=a.iters, chunk=chunk)

    def forwards():
        for c in range(0, B, chunk):
            m.features(frames[c:c + chunk])

    for _ in range(2):                                              # warm-up of every leg
        build()
        iterate(a.iters)
        iterate(0)
    ncut()
    forwards()
    t_build, t_iter, t_zero, t_ncut, t_fwd = [], [], [], [], []
    for _ in range(a.rounds):
        t_build.append(timed(torch, build)[0])
        t_iter.append(timed(torch, lambda: iterate(a.iters))[0])
        t_zero.append(timed(torch, lambda: iterate(0))[0])
        t_ncut.append(timed(torch, ncut)[0])
        t_fwd.append(timed(torch, forwards)[0])
    back_build = [timed(torch, lambda: [build() for _ in range(10)])[0] / 10 for _ in range(5)]
    mem_new, _ = peak_delta(torch, lambda: (build(), iterate(a.iters)))
    mem_ncut, res = peak_delta(torch, ncut)
    mf, st, lds = predicted(B, n, D)
    med = statistics.median
    per_pass = (med(t_iter) - med(t_zero)) / max(a.iters, 1)
    line = {"leg": "ncut", "frame": [H, W], "grid": [hp, wp], "batch": B, "cells": n, "tau": a.tau, "precision": a.precision,
            "rounds": a.rounds, "iters": a.iters, "graph_ms": round(med(back_build), 4), "graph_synchronised_ms": round(med(t_build), 3),
            "iterate_ms": round(med(t_iter), 3), "iterate_zero_passes_ms": round(med(t_zero), 3), "pass_ms": round(per_pass, 4),
            "predicted_graph_mfma_ms": round(mf, 4), "predicted_graph_staging_ms": round(st, 4), "predicted_pass_lds_ms": round(lds, 4),
            "ncut_ms": round(med(t_ncut), 3), "backbone_forwards_ms": round(med(t_fwd), 3),
            "ncut_ms_min_max": [round(min(t_ncut), 3), round(max(t_ncut), 3)],
            "iterate_ms_min_max": [round(min(t_iter), 3), round(max(t_iter), 3)],
            "graph_ms_min_max": [round(min(back_build), 4), round(max(back_build), 4)],
            "compute_units_iterating": B, "launches_peak_bytes": int(mem_new), "ncut_peak_bytes": int(mem_ncut),
            "graph_bytes": int(graph.numel() * 8), "planes_bytes": int(planes.numel() * 2),
            "mean_degree": round(float(degree.float().mean()), 1), "foreground_share": round(float(res.fg.float().mean()), 4),
            "rho_last": [round(float(v), 5) for v in res.rho[:4, -1]] if a.iters else []}
    append(a, line)


def torch_child(a):
    """the torch route at batch 1 on the same ready features: bmm, threshold, the normalised matrix, eigh"""
    torch, capi, m, cfg, frames = setup(a)
    import torch.nn.functional as F

    H, W = a.child_h, a.child_w
    n = (H // cfg.patch) * (W // cfg.patch)
    X = F.normalize(m.features(frames)[:, 1:], dim=2)

    def route():
        s = torch.bmm(X, X.transpose(1, 2))
        w = torch.where(s > a.tau, 1.0, 1e-5)
        r = w.sum(dim=2).rsqrt()
        lam, vec = torch.linalg.eigh(w * r[:, :, None] * r[:, None, :])
        v = vec[:, :, -2] * r
        return lam[:, -2], v > v.mean(dim=1, keepdim=True)

    route()
    times = [timed(torch, route)[0] for _ in range(a.torch_rounds)]
    mem, (lam2, _) = peak_delta(torch, route)
    append(a, {"leg": "torch", "frame": [H, W], "batch": 1, "cells": n, "tau": a.tau, "rounds": a.torch_rounds,
               "torch_route_ms": round(statistics.median(times), 2), "torch_route_ms_min_max": [round(min(times), 2), round(max(times), 2)],
               "torch_route_peak_bytes": int(mem), "affinity_bytes": 4 * n * n, "lambda_2": round(float(lam2[0]), 5)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--torch-timeout", type=int, default=300, help="seconds per torch-route configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncut_cost.jsonl"))
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-torch", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_batch is not None:
        return torch_child(a) if a.child_torch else child(a)
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        for B in (int(v) for v in a.batches.split(",")):
            for leg in (["ncut", "torch"] if B == 1 else ["ncut"]):
                cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--iters",
                       str(a.iters), "--tau", str(a.tau), "--torch-rounds", str(a.torch_rounds), "--out", a.out, "--child-batch",
                       str(B), "--child-h", str(H), "--child-w", str(W)] + (["--child-torch"] if leg == "torch" else [])
                limit = a.torch_timeout if leg == "torch" else a.child_timeout
                try:
                    rc = subprocess.run(cmd, timeout=limit).returncode
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"ncut_cost.py: {size} batch {B} ({leg}) ran past {limit} s; nothing more is started")
                if rc != 0:
                    raise SystemExit(f"ncut_cost.py: {size} batch {B} ({leg}) ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
