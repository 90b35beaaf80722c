"""GPU box: cost of video label propagation per target frame -- ViT-S/8 x12, fp16, 480 x 480 and 480 x 640 frames, full context
(8 frames), R = 12, k = 5, at 7 and 150 label classes.  Every configuration (frame size, classes) runs as a child process under its
own time limit; the first child that fails ends the run.  In a child four legs are interleaved after warm-up, each timed with a host
clock around a synchronised call, medians over --rounds rounds:

  1. the launches alone on ready tokens (dinoseg_op_normalize_tokens + dinoseg_op_propagate + dinoseg_op_upsample_argmax), also timed
     back to back (20 per synchronise: launches_ms), since a synchronised call of a fraction of a millisecond is mostly the host;
  2. LabelPropagator.step(frame) end to end, its ring full;
  3. the backbone forward of that frame alone (features());
  4. the torch route on the same ready features, as the DINO script writes it: normalise, bmm, exp, times the neighbourhood mask (built
     once outside the timing, as the script caches it), topk over all context candidates, zero below the k-th, renormalise, mm.

Also the torch peak-memory delta of legs 2 and 4.  One JSON line per configuration, appended to --out (default
profiles/propagate_cost.jsonl), with the prediction written BEFORE anything was measured beside the measurement: the MFMA work (three
fp16 products per (query, window key, context frame) pair at the 2.5 PFLOP/s dense peak) and the plane traffic as the scores kernel
stages it (query tile and key block, hi + lo, once per 64 keys and 64 columns) at the Infinity Cache's 8.6 TB/s.

    python tools/propagate_cost.py [--sizes 480x480,480x640] [--classes 7,150] [--precision fp16] [--rounds 30]
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
CACHE_BYTES_PER_S = 8.6e12          # Infinity Cache, random rows


def predicted(hp, wp, D, n_ctx, R):
    """(ms from the MFMA work alone, ms from the staged plane traffic alone) of the scores launch"""
    pairs, staged = 0, 0
    for ty in range((hp + 7) // 8):
        for tx in range((wp + 7) // 8):
            rows = min(min(ty * 8 + 7, hp - 1) + R, hp - 1) - max(ty * 8 - R, 0) + 1
            cols = min(min(tx * 8 + 7, wp - 1) + R, wp - 1) - max(tx * 8 - R, 0) + 1
            blocks = (rows * cols + 63) // 64
            pairs += 64 * 64 * blocks
            staged += blocks * (D // 64) * 32768
    return n_ctx * pairs * 3 * 2 * D / MFMA_FLOPS * 1e3, n_ctx * staged / CACHE_BYTES_PER_S * 1e3


def child(a):
    import ctypes

    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, LabelPropagator, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("propagate_cost.py needs a ROCm device")

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

    H, W, C = a.child_h, a.child_w, a.child_classes
    n_context, R, k, tau = 7, 12, 5, 0.1
    T = n_context + 2                                               # frame 0, a full queue, the target
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n = hp * wp
    frames = torch.from_numpy(synthetic_frames(T, H, seed=1, w=W)).cuda()
    first = (torch.arange(H)[:, None] // 40 + torch.arange(W)[None, :] // 40) % C
    lib, S = capi.lib(), capi.stream_ptr

    # ready features and context segs of the target frame T - 1: what legs 1 and 4 start from
    tokens = m.features(frames)
    _, seg_all = m.propagate(frames, first, n_classes=C, want_seg=True)
    planes = torch.empty((T, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), T, n, D, planes.data_ptr(), S()))
    ctx = [0] + list(range(T - 1 - n_context, T - 1))
    cp = (ctypes.c_void_p * len(ctx))(*[planes[c].data_ptr() for c in ctx])
    cs = (ctypes.c_void_p * len(ctx))(*[seg_all[c].data_ptr() for c in ctx])
    tq = torch.empty((2, n, D), dtype=torch.float16, device="cuda")
    seg_out = torch.empty((n, C), dtype=torch.float32, device="cuda")
    labels = torch.empty((H, W), dtype=torch.int32, device="cuda")
    scratch = torch.empty((lib.dinoseg_propagate_scratch_bytes(hp, wp, len(ctx), k),), dtype=torch.uint8, device="cuda")
    tok_t = tokens[T - 1:T]

    def launches():
        capi.check(lib.dinoseg_op_normalize_tokens(tok_t.data_ptr(), 1, n, D, tq.data_ptr(), S()))
        capi.check(lib.dinoseg_op_propagate(tq.data_ptr(), cp, cs, len(ctx), hp, wp, D, C, R, k, tau, seg_out.data_ptr(), None, None,
                                            scratch.data_ptr(), S()))
        capi.check(lib.dinoseg_op_upsample_argmax(seg_out.data_ptr(), 1, hp, wp, C, H, W, labels.data_ptr(), None, S()))

    stream = LabelPropagator(m, frames[0], first, n_classes=C)
    for t in range(1, T - 1):
        stream.step(frames[t])                                      # the ring is full from here on
    target = frames[T - 1]

    r_, c_ = torch.arange(n, device="cuda") // wp, torch.arange(n, device="cuda") % wp
    mask = (((r_[:, None] - r_[None, :]).abs() <= R) & ((c_[:, None] - c_[None, :]).abs() <= R)).float()
    ctx_tok = tokens[ctx][:, 1:]
    ctx_seg = seg_all[ctx].reshape(-1, C)

    def torch_route():
        ft = F.normalize(tok_t[0, 1:], dim=1)
        fc = F.normalize(ctx_tok, dim=2)
        aff = torch.exp(torch.bmm(fc, ft.T.expand(len(ctx), -1, -1)) / tau) * mask
        aff = aff.reshape(-1, n)
        kth = torch.topk(aff, k=k, dim=0).values[-1]
        aff = torch.where(aff < kth, torch.zeros_like(aff), aff)
        aff = aff / aff.sum(dim=0, keepdim=True)
        return (ctx_seg.T @ aff).T

    for _ in range(3):                                              # warm-up of every leg
        launches()
        stream.step(target)
        m.features(target[None])
        torch_route()
    t_launch, t_step, t_fwd, t_torch = [], [], [], []
    for _ in range(a.rounds):
        t_launch.append(timed(launches)[0])
        t_step.append(timed(lambda: stream.step(target))[0])
        t_fwd.append(timed(lambda: m.features(target[None]))[0])
        t_torch.append(timed(torch_route)[0])
    t_back = timed(lambda: [launches() for _ in range(20)])[0] / 20
    mem_step, _ = peak_delta(lambda: stream.step(target))
    mem_torch, ref = peak_delta(torch_route)
    launches()
    agree = float((seg_out - ref).abs().max())
    mf, tr = predicted(hp, wp, D, len(ctx), R)
    la, st, fw, to = (statistics.median(t) for t in (t_launch, t_step, t_fwd, t_torch))
    line = {"frame": [H, W], "grid": [hp, wp], "n_classes": C, "precision": a.precision, "context_frames": len(ctx), "radius": R, "topk": k,
            "rounds": a.rounds, "launches_ms": round(t_back, 4), "launches_synchronised_ms": round(la, 3), "step_ms": round(st, 3),
            "backbone_forward_ms": round(fw, 3), "torch_route_ms": round(to, 3),
            "predicted_mfma_ms": round(mf, 4), "predicted_plane_traffic_ms": round(tr, 4),
            "step_ms_min_max": [round(min(t_step), 3), round(max(t_step), 3)],
            "torch_route_ms_min_max": [round(min(t_torch), 3), round(max(t_torch), 3)],
            "step_peak_bytes": int(mem_step), "torch_route_peak_bytes": int(mem_torch),
            "ring_bytes": int(stream._runner.planes.numel() * 2 + stream._runner.segs.numel() * 4 + stream._runner.scratch.numel()),
            "max_abs_seg_difference_to_torch_fp32": round(agree, 7)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagate_cost.jsonl"))
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-classes", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_h is not None:
        return child(a)
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        for C in (int(v) for v in a.classes.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out,
                   "--child-h", str(H), "--child-w", str(W), "--child-classes", str(C)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"propagate_cost.py: {H}x{W} classes={C} ran past {a.child_timeout} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"propagate_cost.py: {H}x{W} classes={C} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
