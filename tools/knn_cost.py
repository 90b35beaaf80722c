"""GPU box: cost of k-NN label retrieval per frame -- ViT-S/8 x12, fp16, one 480 x 480 and one 480 x 640 frame against a bank of
M = 10^4, 10^5, 10^6 rows, k = 10, at 7 and 150 classes, soft and hard labels.  Every (frame size, M) runs as a child process under
its own time limit and walks the four (classes, label kind) combinations on one bank of random unit rows; the first child that
fails ends the run.  In a child the legs are interleaved after warm-up, each timed with a host clock around a synchronised call,
medians over --rounds rounds:

  1. the two launches alone on ready query planes (dinoseg_op_knn_labels): one synchronised call (launches_synchronised_ms, what
     the torch leg is compared with: both include the host's launch and synchronise), and as a leg of its own in the same rounds
     10 calls back to back per synchronise (launches_ms, what the prediction is compared with), since a synchronised call of a
     fraction of a millisecond is mostly the host;
  2. DINOSeg.segment_knn(frame, bank) end to end;
  3. the backbone forward of that frame alone (features());
  4. the torch route on the same ready unit features in fp32: mm, topk, exp, renormalise, gather (soft) or one-hot scatter (hard).
     Skipped, and recorded as skipped, where its [N, M] fp32 score matrix exceeds --torch-limit-gib.

Also the torch peak-memory delta of legs 1 and 4.  One JSON line per (frame size, M, classes, kind), appended to --out (default
profiles/knn_cost.jsonl), with the prediction written BEFORE anything was measured beside the measurement: the MFMA work (three fp16
products per (query, bank row) pair, 3 * 2 N M D flop at the 2.5 PFLOP/s dense peak) and the staging traffic as the scores kernel
stages it (the bank range, hi + lo, streamed once per 64-query tile, and the query tile beside every key block: 32 KiB per tile,
key block and 64 columns) at the Infinity Cache's 8.6 TB/s.  --predict prints the prediction alone and needs no device.

    python tools/knn_cost.py [--sizes 480x480,480x640] [--rows 10000,100000,1000000] [--classes 7,150] [--rounds 30] [--predict]
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
PATCH, WIDTH, TOPK, TAU = 8, 384, 10, 0.1
BACK_TO_BACK = 10                   # launches per synchronise in the back-to-back leg


def predicted(N, M, D):
    """(ms from the MFMA work alone, ms from the staged plane traffic alone) of the scores launch"""
    tiles, blocks = (N + 63) // 64, (M + 63) // 64
    return 3 * 2 * N * M * D / MFMA_FLOPS * 1e3, tiles * blocks * (D // 64) * 32768 / CACHE_BYTES_PER_S * 1e3


def child(a):
    import torch

    from dino_amd import DINOSeg, MemoryBank, ViTConfig, capi, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("knn_cost.py needs a ROCm device")

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

    H, W, M, k = a.child_h, a.child_w, a.child_rows, TOPK
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n = hp * wp
    lib, S = capi.lib(), capi.stream_ptr
    frame = torch.from_numpy(synthetic_frames(1, H, seed=1, w=W)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(2)

    # the bank's rows: random unit rows (retrieval cost does not depend on what the rows are), written as planes in slabs
    bank_planes = torch.empty((2, M, D), dtype=torch.float16, device="cuda")
    slab = torch.empty((1, 2, 1 << 16, D), dtype=torch.float16, device="cuda")
    for r0 in range(0, M, 1 << 16):
        r = min(1 << 16, M - r0)
        tok = torch.randn((1, r + 1, D), generator=gen, device="cuda")
        capi.check(lib.dinoseg_op_normalize_tokens(tok.data_ptr(), 1, r, D, slab.data_ptr(), S()))
        bank_planes[:, r0:r0 + r] = slab.view(-1)[:2 * r * D].view(2, r, D)
    del slab, tok
    tokens = m.features(frame)
    qp = torch.empty((1, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), 1, n, D, qp.data_ptr(), S()))
    splits = lib.dinoseg_knn_splits(n, M, k)
    scratch = torch.empty((lib.dinoseg_knn_scratch_bytes(n, M, k, 0),), dtype=torch.uint8, device="cuda")
    torch_fits = 4 * n * M <= a.torch_limit_gib * (1 << 30)
    if torch_fits:
        q32 = ((qp[0, 0].float() + qp[0, 1].float()) * 2.0 ** -10).contiguous()
        b32 = ((bank_planes[0].float() + bank_planes[1].float()) * 2.0 ** -10).contiguous()
    mf, tr = predicted(n, M, D)

    for C in (int(v) for v in a.classes.split(",")):
        for hard in (False, True):
            bank = MemoryBank(m, C, M, hard=hard)
            bank.planes = bank_planes                               # (a tool's shortcut: the rows are ready, add() is not what is timed)
            if hard:
                bank.labels.copy_(torch.randint(0, C, (M,), generator=gen, device="cuda").to(torch.uint8))
            else:
                bank.labels.copy_(torch.softmax(2.0 * torch.randn((M, C), generator=gen, device="cuda"), dim=1))
            bank.size = M
            seg = torch.empty((n, C), dtype=torch.float32, device="cuda")

            def launches():
                capi.check(lib.dinoseg_op_knn_labels(qp.data_ptr(), 1, n, bank.planes.data_ptr(), M, M, bank.labels.data_ptr(),
                                                     1 if hard else 0, D, C, k, TAU, 0, seg.data_ptr(), None, None, scratch.data_ptr(),
                                                     S()))

            def torch_route():
                s = q32 @ b32.T
                top, idx = torch.topk(s, k, dim=1)
                w = torch.exp((top - top[:, :1]) / TAU)
                w = w / w.sum(dim=1, keepdim=True)
                if hard:
                    lab = bank.labels[idx].to(torch.int64)
                    return torch.zeros((n, C), device="cuda").scatter_add_(1, lab, w)
                return torch.einsum("qk,qkc->qc", w, bank.labels[idx])

            legs = [launches, lambda: m.segment_knn(frame, bank, topk=k, temperature=TAU), lambda: m.features(frame),
                    lambda: [launches() for _ in range(BACK_TO_BACK)]]
            if torch_fits:
                legs.append(torch_route)
            for _ in range(2):                                      # warm-up of every leg
                for leg in legs:
                    leg()
            times = [[] for _ in legs]
            for _ in range(a.rounds):
                for t, leg in zip(times, legs):
                    t.append(timed(leg)[0])
            mem_launch, _ = peak_delta(launches)
            med = [statistics.median(t) for t in times]
            t_back = med[3] / BACK_TO_BACK
            line = {"frame": [H, W], "queries": n, "bank_rows": M, "n_classes": C, "labels": "hard" if hard else "soft", "topk": k,
                    "precision": a.precision, "splits": splits, "rounds": a.rounds, "launches_ms": round(t_back, 4),
                    "launches_synchronised_ms": round(med[0], 3), "segment_knn_ms": round(med[1], 3),
                    "backbone_forward_ms": round(med[2], 3), "predicted_mfma_ms": round(mf, 4),
                    "predicted_plane_traffic_ms": round(tr, 4), "launches_over_prediction": round(t_back / max(mf, tr), 2),
                    "segment_knn_ms_min_max": [round(min(times[1]), 3), round(max(times[1]), 3)],
                    "launches_peak_bytes": int(mem_launch), "scratch_bytes": int(scratch.numel()),
                    "bank_bytes": int(bank_planes.numel() * 2 + bank.labels.numel() * bank.labels.element_size())}
            if torch_fits:
                mem_torch, ref = peak_delta(torch_route)
                launches()
                line.update({"torch_route_ms": round(med[4], 3), "torch_over_launches": round(med[4] / med[0], 2),
                             "torch_route_ms_min_max": [round(min(times[4]), 3), round(max(times[4]), 3)],
                             "torch_route_peak_bytes": int(mem_torch),
                             "max_abs_seg_difference_to_torch_fp32": round(float((seg - ref).abs().max()), 7)})
                del ref
            else:
                line.update({"torch_route_ms": None, "torch_route_skipped": f"its [N, M] fp32 score matrix is {4 * n * M / 2 ** 30:.1f} GiB, "
                                                                            f"above the limit of {a.torch_limit_gib} GiB"})
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del bank, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x480,480x640")
    ap.add_argument("--rows", default="10000,100000,1000000")
    ap.add_argument("--classes", default="7,150")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--torch-limit-gib", type=float, default=8.0, help="largest [N, M] fp32 score matrix the torch leg may form")
    ap.add_argument("--predict", action="store_true", help="print the predicted cost of every (frame size, M) and stop: no device")
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per (frame size, M)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_cost.jsonl"))
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-rows", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_h is not None:
        return child(a)
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        for M in (int(v) for v in a.rows.split(",")):
            if a.predict:
                n = (H // PATCH) * (W // PATCH)
                mf, tr = predicted(n, M, WIDTH)
                print(json.dumps({"frame": [H, W], "queries": n, "bank_rows": M, "predicted_mfma_ms": round(mf, 4),
                                  "predicted_plane_traffic_ms": round(tr, 4)}))
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out,
                   "--classes", a.classes, "--torch-limit-gib", str(a.torch_limit_gib), "--child-h", str(H), "--child-w", str(W),
                   "--child-rows", str(M)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"knn_cost.py: {H}x{W} M={M} ran past {a.child_timeout} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"knn_cost.py: {H}x{W} M={M} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
