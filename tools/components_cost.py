"""GPU box: cost of connected components on the device (dinoseg_op_components, DINOSeg.components, DINOSeg.discover) against the route
it replaces -- the copy of the label map to the host and scipy.ndimage.label per class.  Label maps of 480 x 640 at batches of 1, 8
and 32 and of 1080 x 1920 at batch 1, three kinds each: `segment` of the procedural ViT-S/8 x12 model on synthetic frames (enlarged
to the map's size), a random 2-class map at p = 0.59 (near the percolation threshold), one serpentine component; and the 60 x 80 cell
grid of `discover`.  Every configuration (size, batch) runs as a child process under its own time limit; the first child that fails
ends the run.  In a child the legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians
over --rounds rounds:

  1. the operator alone on a device int32 map, outputs and scratch allocated once (connectivity 4, max_objects 256);
  2. DINOSeg.components end to end (its allocations included);
  3. the host route: labels.cpu() and scipy.ndimage.label of every class present, frame by frame (--host-rounds rounds; without
     scipy the copy alone, and the line says so);
  4. at 480 x 640 only: DINOSeg.discover against DINOSeg.ncut(split=True) on the frames, and the operator alone on the 60 x 80 grid.

One JSON line per configuration and kind of map, appended to --out (default profiles/components_cost.jsonl), with the prediction
written BEFORE anything was timed beside the measurement.  The prediction: the five launches move labels, parent (written, read), ids
(written, read, written) across HBM once each, 24 bytes per pixel, at 6.3 TB/s; in front of that one memset and five dependent
launches at 1.8 us of boundary each, and per launch 2 us of its own start-up and tail; the guess on top: the chains of the serpentine
and the atomics of a one-component map double the three launches that follow chains.

    python tools/components_cost.py [--batches 1,8,32] [--sizes 480x640] [--big 1080x1920] [--rounds 9] [--host-rounds 3]
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

HBM_BYTES_PER_US = 6.3e6
BYTES_PER_PIXEL = 24
LAUNCHES = 6                    # the memset and the five kernels
BOUNDARY_US = 1.8
OWN_US = 2.0
KINDS = ("segment", "random", "serpentine")


def predicted_us(B, H, W, kind):
    """the operator alone"""
    traffic = BYTES_PER_PIXEL * B * H * W / HBM_BYTES_PER_US
    fixed = LAUNCHES * (BOUNDARY_US + OWN_US)
    return (fixed + traffic) * (2.0 if kind == "serpentine" else 1.0)


def serpentine(H, W):
    import numpy as np
    m = np.full((H, W), -1, dtype=np.int32)
    m[0::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


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
    import numpy as np
    import torch

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("components_cost.py needs a ROCm device")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    B, H, W, M = a.child_batch, a.child_h, a.child_w, 256
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    frames = torch.from_numpy(synthetic_frames(B, 480, seed=1, w=640)).cuda()
    lib, S = capi.lib(), capi.stream_ptr
    g = np.random.default_rng(59)
    maps = {"segment": m.segment(frames, size=(H, W))[0].contiguous(),
            "random": torch.from_numpy((g.random((B, H, W)) < 0.59).astype(np.int32)).cuda(),
            "serpentine": torch.from_numpy(np.broadcast_to(serpentine(H, W), (B, H, W)).copy()).cuda()}

    def buffers(b, h, w):
        i32 = dict(dtype=torch.int32, device="cuda")
        return dict(ids=torch.empty((b, h, w), **i32), count=torch.empty((b,), **i32), first=torch.empty((b, M), **i32),
                    label=torch.empty((b, M), **i32), area=torch.empty((b, M), **i32), box=torch.empty((b, M, 4), **i32),
                    status=torch.empty((b,), **i32),
                    scratch=torch.empty((lib.dinoseg_components_scratch_bytes(b, h, w),), dtype=torch.uint8, device="cuda"))

    def operator(lab, o, ignore=-1):
        b, h, w = lab.shape
        capi.check(lib.dinoseg_op_components(lab.data_ptr(), b, h, w, 4, ignore, M, o["ids"].data_ptr(), o["count"].data_ptr(),
                                             o["first"].data_ptr(), o["label"].data_ptr(), o["area"].data_ptr(), o["box"].data_ptr(),
                                             o["status"].data_ptr(), o["scratch"].data_ptr(), S()))

    def host_route(lab):
        h = lab.cpu().numpy()
        t1 = time.perf_counter()
        n = 0
        if ndimage is not None:
            for f in h:
                for c in np.unique(f[f >= 0]):
                    n += ndimage.label(f == c)[1]
        return n, t1

    out = buffers(B, H, W)
    for kind in KINDS:
        lab = maps[kind]
        pred = predicted_us(B, H, W, kind)                              # (written before anything below is timed)
        for _ in range(2):
            operator(lab, out)
            m.components(lab)
        torch.cuda.synchronize()
        assert not bool(out["status"].any())
        counts = out["count"].cpu().tolist()
        t_op, t_e2e, t_host, t_copy = [], [], [], []
        for r in range(a.rounds):
            t_op.append(timed(torch, lambda: operator(lab, out))[0])
            t_e2e.append(timed(torch, lambda: m.components(lab))[0])
            if r < a.host_rounds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n, t1 = host_route(lab)
                t_host.append((time.perf_counter() - t0) * 1e3)
                t_copy.append((t1 - t0) * 1e3)
                if ndimage is not None:
                    assert n == sum(counts), (n, counts)
        med = statistics.median
        append(a, {"map": [H, W], "batch": B, "kind": kind, "connectivity": 4, "max_objects": M, "rounds": a.rounds,
                   "components_per_frame": counts[:4], "predicted_operator_us": round(pred, 1),
                   "operator_us": round(med(t_op) * 1e3, 1), "operator_us_min_max": [round(min(t_op) * 1e3, 1), round(max(t_op) * 1e3, 1)],
                   "components_end_to_end_us": round(med(t_e2e) * 1e3, 1),
                   "host_route_ms": round(med(t_host), 3), "host_copy_ms": round(med(t_copy), 3), "scipy": ndimage is not None,
                   "host_rounds": a.host_rounds, "scratch_bytes": int(out["scratch"].numel())})
    if (H, W) == (480, 640):
        hp, wp = H // cfg.patch, W // cfg.patch
        cut = m.ncut(frames, split=True)
        grid, small = cut.fg.view(B, hp, wp).to(torch.int32).contiguous(), buffers(B, hp, wp)
        pred = predicted_us(B, hp, wp, "grid")
        for _ in range(2):
            operator(grid, small, 0)
            m.discover(frames)
        t_grid, t_ncut, t_disc = [], [], []
        for _ in range(a.rounds):
            t_grid.append(timed(torch, lambda: operator(grid, small, 0))[0])
            t_ncut.append(timed(torch, lambda: m.ncut(frames, split=True))[0])
            t_disc.append(timed(torch, lambda: m.discover(frames))[0])
        med = statistics.median
        res = m.discover(frames)
        append(a, {"map": [hp, wp], "batch": B, "kind": "discover grid", "frame": [H, W], "rounds": a.rounds, "predicted_operator_us": round(pred, 1),
                   "operator_us": round(med(t_grid) * 1e3, 1), "ncut_split_ms": round(med(t_ncut), 3), "discover_ms": round(med(t_disc), 3),
                   "discover_minus_ncut_us": round((med(t_disc) - med(t_ncut)) * 1e3, 1), "found": res.found.cpu().tolist()[:4],
                   "box": res.box.cpu().tolist()[:2], "area_cells": res.area.cpu().tolist()[:4]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--sizes", default="480x640")
    ap.add_argument("--big", default="1080x1920", help="sizes run at batch 1 only")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_cost.jsonl"))
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
        cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--host-rounds",
               str(a.host_rounds), "--out", a.out, "--child-batch", str(B), "--child-h", str(H), "--child-w", str(W)]
        try:
            rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"components_cost.py: {size} batch {B} ran past {a.child_timeout} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"components_cost.py: {size} batch {B} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
