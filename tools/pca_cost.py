"""GPU box: cost of the PCA of patch features -- ViT-S/8 x12, fp16.  Every configuration runs as a child process under its own time
limit; the first child that fails ends the run.  In a child the legs are interleaved after warm-up, each timed with a host clock
around a synchronised call, medians over --rounds rounds; the launch legs also run 10 calls back to back per synchronise, since a
synchronised call of a fraction of a millisecond is mostly the host.  Three kinds of child:

  ops      a batch of --batch frames of one size: the three launches alone on ready tokens (dinoseg_op_token_moments with outer,
           dinoseg_op_pca_project at q = 3 and 64, dinoseg_op_pca_colour at the frames' size), DINOSeg.pca_fit and pca_map end to
           end, the backbone forward alone, and the torch route on the same ready features (centre, X.T @ X, eigh, mm, F.interpolate
           into [B, 3, H, W] fp32, scale, clamp, convert) in time and peak memory.
  knn      one frame against a bank of M rows: DINOSeg.segment_knn and the two k-NN launches alone for the unprojected bank (width
           384) and for banks with project at q = 64 and 128 (random rows projected on a random orthonormal basis: retrieval cost
           does not depend on what the rows are).
  overlap  reported, not asserted: the share of the unprojected top-k that the projected search keeps, on a bank of synthetic frames
           with the PCA fitted on those frames.

One JSON line per child, appended to --out (default profiles/pca_cost.jsonl), with the prediction written BEFORE anything was
measured beside the measurement: the moments' MFMA work (the upper triangle of tile pairs, 2 N 4096 P flop at the 155 TF/s of the
fp32-input MFMA) and their staged reads (each 64-column tile re-read by T + 1 tile pairs from L2 / Infinity Cache at 4.3 - 8.6
TB/s), the projection as one pass over the tokens at HBM's 4 TB/s, the k-NN launches by the staging model of tools/knn_cost.py.
--predict prints the predictions alone and needs no device.

    python tools/pca_cost.py [--sizes 480x480] [--batch 32] [--rows 100000,1000000] [--rounds 20] [--predict]
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

F32_MFMA_FLOPS = 155e12             # v_mfma_f32_32x32x2_f32, measured peak
F16_MFMA_FLOPS = 2.5e15
CACHE_BYTES_PER_S = (4.3e12, 8.6e12)
HBM_BYTES_PER_S = 4.0e12
PATCH, WIDTH, TOPK, TAU = 8, 384, 10, 0.1
BACK_TO_BACK = 10


def predicted_ops(B, n, D):
    N, T = B * n, D // 64
    P = T * (T + 1) // 2
    reads = 2 * P * N * 64 * 4                                          # two 64-column operand tiles per pair and row
    return {"predicted_moments_mfma_ms": round(2 * N * 4096 * P / F32_MFMA_FLOPS * 1e3, 4),
            "predicted_moments_reads_ms": [round(reads / bw * 1e3, 4) for bw in reversed(CACHE_BYTES_PER_S)],
            "predicted_project_ms": round(B * (n + 1) * D * 4 / HBM_BYTES_PER_S * 1e3, 4)}


def predicted_knn(N, M, D):
    tiles, blocks = (N + 63) // 64, (M + 63) // 64
    return {"predicted_mfma_ms": round(3 * 2 * N * M * D / F16_MFMA_FLOPS * 1e3, 4),
            "predicted_plane_traffic_ms": round(tiles * blocks * (D // 64) * 32768 / CACHE_BYTES_PER_S[1] * 1e3, 4)}


def child(a):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, MemoryBank, ViTConfig, capi, pca_solve, procedural_state_dict
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("pca_cost.py needs a ROCm device")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def peak_delta(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    def medians(legs, rounds):
        for _ in range(2):
            for leg in legs.values():
                leg()
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for k, leg in legs.items():
                times[k].append(timed(leg))
        return {k: statistics.median(v) for k, v in times.items()}

    def back_to_back(fn):
        return lambda: [fn() for _ in range(BACK_TO_BACK)]

    H, W = a.child_h, a.child_w
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n = hp * wp
    lib, S = capi.lib(), capi.stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(2)
    line = {"kind": a.child, "frame": [H, W], "precision": a.precision, "rounds": a.rounds}

    def random_basis(q):
        return torch.linalg.qr(torch.randn((D, q), generator=gen, device="cuda"))[0].T.contiguous()

    if a.child == "ops":
        B = a.batch
        x = torch.from_numpy(synthetic_frames(B, H, seed=1, w=W)).cuda()
        tokens = m.features(x)
        pca = m.pca_fit(x, q=64)
        mean, basis, _ = pca.on(m.device)
        shift = mean.clone()
        s, o, cnt = (torch.zeros(sh, dtype=dt, device="cuda") for sh, dt in (((D,), torch.float64), ((D, D), torch.float64), ((1,), torch.int64)))
        scratch = torch.empty((lib.dinoseg_pca_scratch_bytes(B, n, D),), dtype=torch.uint8, device="cuda")
        out3, out64 = (torch.empty((B, n + 1, q), dtype=torch.float32, device="cuda") for q in (3, 64))
        rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
        lo, inv = torch.full((3,), -1.0, device="cuda"), torch.full((3,), 0.5, device="cuda")

        def moments():
            capi.check(lib.dinoseg_op_token_moments(tokens.data_ptr(), None, B, n, D, shift.data_ptr(), s.data_ptr(), o.data_ptr(),
                                                    cnt.data_ptr(), scratch.data_ptr(), S()))

        def project(q, out):
            return lambda: capi.check(lib.dinoseg_op_pca_project(tokens.data_ptr(), B, n, D, mean.data_ptr(), basis.data_ptr(), None, q,
                                                                 out.data_ptr(), S()))

        def colour():
            capi.check(lib.dinoseg_op_pca_colour(out3.data_ptr(), B, hp, wp, 3, lo.data_ptr(), inv.data_ptr(), None, H, W, rgb.data_ptr(), S()))

        def torch_fit():
            X = tokens[:, 1:, :].reshape(-1, D)
            Xc = X - X.mean(dim=0)
            w, v = torch.linalg.eigh((Xc.T @ Xc) / (Xc.shape[0] - 1))
            return X.mean(dim=0), v[:, -3:].T.flip(0).contiguous()

        t_mean, t_basis = torch_fit()

        def torch_map():
            y = (tokens[:, 1:, :] - t_mean) @ t_basis.T
            lo_, hi_ = y.amin(dim=(0, 1)), y.amax(dim=(0, 1))
            up = F.interpolate(y.view(B, hp, wp, 3).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
            t = (up - lo_.view(1, 3, 1, 1)) / (hi_ - lo_).view(1, 3, 1, 1)
            return (t.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

        pca3 = m.pca_fit(x, q=3)
        legs = {"moments": moments, "project_q3": project(3, out3), "project_q64": project(64, out64), "colour": colour,
                "moments_x10": back_to_back(moments), "project_q3_x10": back_to_back(project(3, out3)),
                "project_q64_x10": back_to_back(project(64, out64)), "colour_x10": back_to_back(colour),
                "pca_fit": lambda: m.pca_fit(x, q=3), "pca_map": lambda: m.pca_map(x, pca3), "backbone_forward": lambda: m.features(x),
                "torch_fit": torch_fit, "torch_map": torch_map}
        med = medians(legs, a.rounds)
        line.update({"batch": B, "cells": n, "width": D, "ranges": lib.dinoseg_pca_ranges(B * n, D), "scratch_bytes": int(scratch.numel())})
        line.update(predicted_ops(B, n, D))
        for k in ("moments", "project_q3", "project_q64", "colour"):
            line[k + "_synchronised_ms"] = round(med[k], 4)
            line[k + "_ms"] = round(med[k + "_x10"] / BACK_TO_BACK, 4)
        for k in ("pca_fit", "pca_map", "backbone_forward", "torch_fit", "torch_map"):
            line[k + "_ms"] = round(med[k], 3)
        line["fit_beyond_forward_ms"] = round(med["pca_fit"] - med["backbone_forward"], 3)
        line["map_beyond_forward_ms"] = round(med["pca_map"] - med["backbone_forward"], 3)
        line["moments_peak_bytes"] = int(peak_delta(moments)[0])
        line["map_launches_peak_bytes"] = int(peak_delta(lambda: (project(3, out3)(), colour()))[0])
        line["torch_fit_peak_bytes"] = int(peak_delta(torch_fit)[0])
        line["torch_map_peak_bytes"] = int(peak_delta(torch_map)[0])
    elif a.child == "knn":
        M, k = a.child_rows, TOPK
        frame = torch.from_numpy(synthetic_frames(1, H, seed=1, w=W)).cuda()
        line.update({"queries": n, "bank_rows": M, "topk": k})
        legs = {"backbone_forward": lambda: m.features(frame)}
        tokens = m.features(frame)
        keepalive = []
        for q in (0, 64, 128):
            width = q or D
            pca = None
            if q:
                pca = pca_solve(np.zeros(D), np.eye(D), 2, None, q)      # a valid FeaturePCA; its basis is replaced by a random one
                pca.basis.copy_(random_basis(q).cpu())
            bank = MemoryBank(m, 7, M, project=pca)
            slab = torch.empty((1, 2, 1 << 16, width), dtype=torch.float16, device="cuda")
            for r0 in range(0, M, 1 << 16):
                r = min(1 << 16, M - r0)
                tok = bank._rows(torch.randn((1, r + 1, D), generator=gen, device="cuda"), r)
                capi.check(lib.dinoseg_op_normalize_tokens(tok.data_ptr(), 1, r, width, slab.data_ptr(), S()))
                bank.planes[:, r0:r0 + r] = slab.view(-1)[:2 * r * width].view(2, r, width)
            del slab, tok
            bank.labels.copy_(torch.softmax(2.0 * torch.randn((M, 7), generator=gen, device="cuda"), dim=1))
            bank.size = M
            qp = torch.empty((1, 2, n, width), dtype=torch.float16, device="cuda")
            capi.check(lib.dinoseg_op_normalize_tokens(bank._rows(tokens, n).data_ptr(), 1, n, width, qp.data_ptr(), S()))
            seg = torch.empty((n, 7), dtype=torch.float32, device="cuda")
            scratch = torch.empty((lib.dinoseg_knn_scratch_bytes(n, M, k, 0),), dtype=torch.uint8, device="cuda")

            def launches(bank=bank, qp=qp, seg=seg, scratch=scratch, width=width):
                capi.check(lib.dinoseg_op_knn_labels(qp.data_ptr(), 1, n, bank.planes.data_ptr(), M, M, bank.labels.data_ptr(), 0, width, 7, k,
                                                     TAU, 0, seg.data_ptr(), None, None, scratch.data_ptr(), S()))

            tag = f"q{q}" if q else "unprojected"
            legs[f"{tag}_launches_x10"] = back_to_back(launches)
            legs[f"{tag}_segment_knn"] = lambda bank=bank: m.segment_knn(frame, bank, topk=k, temperature=TAU)
            line[f"{tag}_bank_bytes"] = int(bank.planes.numel() * 2)
            line[f"{tag}_prediction"] = predicted_knn(n, M, width)
            keepalive.append((bank, qp, seg, scratch))
        med = medians(legs, a.rounds)
        line["backbone_forward_ms"] = round(med["backbone_forward"], 3)
        for tag in ("unprojected", "q64", "q128"):
            line[f"{tag}_launches_ms"] = round(med[f"{tag}_launches_x10"] / BACK_TO_BACK, 4)
            line[f"{tag}_segment_knn_ms"] = round(med[f"{tag}_segment_knn"], 3)
    else:
        k, frames_in_bank = TOPK, 8
        xb = torch.from_numpy(synthetic_frames(frames_in_bank, H, seed=3, w=W)).cuda()
        yb = torch.from_numpy(np.random.default_rng(4).integers(0, 7, (frames_in_bank, H, W))).cuda()
        frame = torch.from_numpy(synthetic_frames(1, H, seed=5, w=W)).cuda()
        plain = MemoryBank(m, 7, frames_in_bank * n)
        plain.add(xb, yb)
        want = m.segment_knn(frame, plain, topk=k, want_idx=True)
        line.update({"queries": n, "bank_rows": plain.size, "topk": k, "frames": "synthetic (uniform noise): features with little structure"})
        for q in (64, 128):
            pca = m.pca_fit(xb, q=q)
            bank = MemoryBank(m, 7, frames_in_bank * n, project=pca)
            bank.add(xb, yb)
            got = m.segment_knn(frame, bank, topk=k, want_idx=True)
            same = (got.idx[0].unsqueeze(2) == want.idx[0].unsqueeze(1)).any(dim=2).float().mean()
            line[f"q{q}_share_of_unprojected_topk_kept"] = round(float(same), 4)
            line[f"q{q}_labels_equal_share"] = round(float((got.labels == want.labels).float().mean()), 4)
            line[f"q{q}_variance_explained"] = round(float(pca.eigenvalues.double().sum()) / pca.total_variance, 4)
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x480")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--predict", action="store_true", help="print the predicted costs and stop: no device")
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_cost.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-rows", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a)
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        n = (H // PATCH) * (W // PATCH)
        jobs = [("ops", 0)] + [("knn", int(v)) for v in a.rows.split(",")] + [("overlap", 0)]
        for kind, M in jobs:
            if a.predict:
                if kind == "ops":
                    print(json.dumps(dict({"kind": kind, "frame": [H, W], "batch": a.batch}, **predicted_ops(a.batch, n, WIDTH))))
                elif kind == "knn":
                    print(json.dumps({"kind": kind, "frame": [H, W], "bank_rows": M,
                                      **{f"width_{w}": predicted_knn(n, M, w) for w in (WIDTH, 64, 128)}}))
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--out", a.out,
                   "--batch", str(a.batch), "--child", kind, "--child-h", str(H), "--child-w", str(W), "--child-rows", str(M)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"pca_cost.py: {kind} {H}x{W} M={M} ran past {a.child_timeout} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"pca_cost.py: {kind} {H}x{W} M={M} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
