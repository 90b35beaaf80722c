"""GPU box: cost of the CLS attention maps at pixel resolution -- ViT-S/8 x12, fp16, 480 x 480 at batch 1 and 8, 960 x 960 at batch 1.
Per configuration, interleaved in one process after warm-up, each leg timed with a host clock around a synchronised call, medians
over --rounds rounds:

  1. cls_attention(frames, threshold=0.6) end to end: the forward up to the last block's qkv and the launch of csrc/cls_attention.hip;
  2. that launch alone (dinoseg_op_cls_attention on fp16 planes of the same shape), 10 launches back to back;
  3. the route it replaces, on the same device: get_last_selfattention(x)[:, :, 0, 1:], torch sort / cumsum / threshold (the
     arithmetic of dt_utils.process_attentions, for every frame), F.interpolate(mode="nearest") of both maps.

Also the torch peak-memory delta of legs 1 and 3, the largest |difference| of the two routes' maps and the share of pixels on which
their thresholded maps agree.

Prediction, written down before the first measurement (`predicted_launch_us` of every line).  One workgroup per (frame, head) reads
its K once (3601 x 128 B = 0.46 MB at 480, 1.84 MB at 960) at the ~10 B / clock a single CU draws from HBM: 19 us / 77 us; 31
bisection steps over 3600 / 14 400 words of LDS: 2 us / 8 us; 1.15 MB / 4.6 MB of stores per workgroup at a few tens of bytes per
clock: 10 us / 40 us.  So about 30 us at 480 -- at batch 1 (6 workgroups) as at batch 8 (48 workgroups, still under one per CU) --
and about 125 us at 960.  End to end the call is the forward without the last block's attention and MLP plus those microseconds;
its torch memory is its outputs alone (5 bytes per pixel and head: 6.9 MB per 480 x 480 frame), where the old route allocates the
[B, heads, N, N] matrix (311 MB per frame at 480, 5.0 GB at 960).

Every configuration runs in a child process of its own under its own time limit, and the first one that fails ends the run.  One
JSON line per configuration, appended to --out (default profiles/attention_cost.jsonl).

    python tools/attention_cost.py [--configs 480x1,480x8,960x1] [--rounds 10]
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
PREDICTED_LAUNCH_US = {480: 30.0, 960: 125.0}


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


def one(a, r, B):
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames
    from oracle import dinoseg_oracle as O

    if not torch.cuda.is_available():
        raise SystemExit("attention_cost.py needs a ROCm device")
    thr = 0.6
    frames_np = synthetic_frames(B, r, seed=1)
    frames = torch.from_numpy(frames_np).cuda()
    x32 = O.preprocess(frames_np).cuda()
    lib = capi.lib()
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    p, heads = cfg.patch, cfg.num_heads
    hp = wp = r // p
    ntok = hp * wp + 1
    npad = (ntok + 63) // 64 * 64
    G = B * heads
    gen = torch.Generator(device="cuda").manual_seed(2)
    q = (torch.randn((G, npad, 64), device="cuda", generator=gen) * 0.27).to(torch.float16)
    k = (torch.randn((G, npad, 64), device="cuda", generator=gen) * 1.5).to(torch.float16)
    attn = torch.empty((B, heads, r, r), dtype=torch.float32, device="cuda")
    keep = torch.empty((B, heads, r, r), dtype=torch.uint8, device="cuda")

    def op():
        capi.check(lib.dinoseg_op_cls_attention(q.data_ptr(), k.data_ptr(), 0, 1, B, heads, ntok, npad, hp, wp, r, r, thr,
                                                attn.data_ptr(), keep.data_ptr(), capi.stream_ptr()))

    def e2e():
        return m.cls_attention(frames, threshold=thr)

    def torch_route():
        row = m.get_last_selfattention(x32)[:, :, 0, 1:]                   # [B, heads, n] (a view of the N x N matrix)
        val, idx = torch.sort(row, dim=-1)
        val = val / val.sum(dim=-1, keepdim=True)
        th = torch.cumsum(val, dim=-1) > (1 - thr)
        kept = torch.zeros_like(th).scatter_(-1, idx, th)
        up = F.interpolate(row.reshape(B, heads, hp, wp), scale_factor=p, mode="nearest")
        kup = F.interpolate(kept.reshape(B, heads, hp, wp).float(), scale_factor=p, mode="nearest")
        return up, kup

    capi.check(lib.dinoseg_set_option(b"op_fmt", 1))
    for _ in range(2):                                          # warm-up of every leg
        e2e(), op(), torch_route()
    t = {key: [] for key in ("e2e", "op", "torch")}
    for _ in range(a.rounds):
        t["e2e"].append(timed(torch, e2e)[0])
        t["op"].append(timed(torch, lambda: [op() for _ in range(10)])[0] / 10)
        t["torch"].append(timed(torch, torch_route)[0])
    capi.check(lib.dinoseg_set_option(b"op_fmt", 0))
    mem_new, (a_new, k_new) = peak_delta(torch, e2e)
    mem_old, (a_old, k_old) = peak_delta(torch, torch_route)
    diff = float((a_new - a_old).abs().max())
    agree = float((k_new.float() == k_old).double().mean())
    med = {key: statistics.median(v) for key, v in t.items()}
    line = {"model": "ViT-S/8 x12", "precision": a.precision, "res": r, "batch": B, "tokens": ntok, "threshold": thr, "rounds": a.rounds,
            "predicted_launch_us": PREDICTED_LAUNCH_US.get(r),
            "cls_attention_ms": round(med["e2e"], 3), "launch_alone_us": round(1e3 * med["op"], 1),
            "old_route_ms": round(med["torch"], 3),
            "cls_attention_ms_min_max": [round(min(t["e2e"]), 3), round(max(t["e2e"]), 3)],
            "old_route_ms_min_max": [round(min(t["torch"]), 3), round(max(t["torch"]), 3)],
            "old_over_new_time_measured": round(med["torch"] / med["e2e"], 3),
            "cls_attention_peak_bytes": int(mem_new), "outputs_bytes": int(a_new.numel() * 4 + k_new.numel()),
            "old_route_peak_bytes": int(mem_old), "attn_max_abs_diff": diff, "keep_agree_with_torch_fp32": round(agree, 6)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="480x1,480x8,960x1", help="RESxBATCH, comma separated")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_cost.jsonl"))
    ap.add_argument("--one", default=None, help="(internal) run the single configuration RESxBATCH in this process")
    a = ap.parse_args()
    if a.one:
        r, B = (int(v) for v in a.one.split("x"))
        return one(a, r, B)
    for c in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", c, "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"attention_cost.py: {c} ran past {a.limit} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"attention_cost.py: {c} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
