"""GPU box: cost of spherical k-means over patch features per Lloyd iteration -- ViT-S/8 x12, fp16, 480 x 480 frames, batches of 8 and
32, K = 8, 64 and 256.  Every configuration (batch, K) runs as a child process under its own time limit; the first child that fails
ends the run.  In a child four legs are interleaved after warm-up, each timed with a host clock around a synchronised call, medians
over --rounds rounds:

  1. the new launches alone on ready planes: one iteration = dinoseg_op_kmeans_assign + dinoseg_op_kmeans_update (four launches), also
     timed back to back (20 iterations per synchronise: iteration_ms), since a synchronised call of a fraction of a millisecond is
     mostly the host;
  2. the torch route on the same ready features, normalised once outside the timing: mm, argmax, index_add_, normalize per iteration,
     also back to back;
  3. DINOSeg.cluster end to end (--iters iterations, sample init, labels at the frames' size);
  4. the backbone forwards of that call alone (features() in the same chunks).

Also the torch peak-memory delta of one iteration of legs 1 and 2 and of leg 3.  One JSON line per configuration, appended to --out
(default profiles/kmeans_cost.jsonl), with the prediction written BEFORE anything was measured beside the measurement: the plane
traffic (the assign launch stages the point tile once per block of 64 centroids, the update gathers every row once; hi + lo, 4 bytes
per element) at 5 TB/s of HBM, and the MFMA work (three fp16 products per (point, centroid of a padded block) pair) at the 2.5 PFLOP/s
dense peak.

    python tools/kmeans_cost.py [--batches 8,32] [--ks 8,64,256] [--size 480x480] [--precision fp16] [--rounds 15] [--iters 10]
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
HBM_BYTES_PER_S = 5.0e12            # streaming reads, achievable


def predicted(N, D, K):
    """(ms from the plane traffic alone, ms from the MFMA work alone) of one iteration"""
    blocks = (K + 63) // 64
    traffic = N * D * 4 * (blocks + 1)
    flops = N * blocks * 64 * D * 2 * 3
    return traffic / HBM_BYTES_PER_S * 1e3, flops / MFMA_FLOPS * 1e3


def child(a):
    import torch
    import torch.nn.functional as F

    from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict, sample_indices
    from dino_amd.weights import synthetic_frames

    if not torch.cuda.is_available():
        raise SystemExit("kmeans_cost.py needs a ROCm device")

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

    B, K, H, W, chunk = a.child_batch, a.child_k, a.child_h, a.child_w, 32
    cfg = ViTConfig(n_blocks=12)
    m = DINOSeg(head=cfg.head, n_blocks=12, n_classes=cfg.n_classes, precision=a.precision, arch=cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in procedural_state_dict(cfg).items()}, strict=True)
    m.to("cuda:0")
    hp, wp, D = H // cfg.patch, W // cfg.patch, cfg.embed_dim
    n, N = hp * wp, B * hp * wp
    frames = torch.from_numpy(synthetic_frames(B, H, seed=1, w=W)).cuda()
    lib, S = capi.lib(), capi.stream_ptr

    # ready features: what legs 1 and 2 start from
    tokens = torch.cat([m.features(frames[c:c + chunk]) for c in range(0, B, chunk)])
    planes = torch.empty((B, 2, n, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n, D, planes.data_ptr(), S()))
    X = F.normalize(tokens[:, 1:].reshape(N, D), dim=1)
    del tokens
    idx = sample_indices(N, K, 0).cuda()
    cent = torch.empty((K, D), dtype=torch.float32, device="cuda")
    cpl = torch.empty((2, K, D), dtype=torch.float16, device="cuda")
    capi.check(lib.dinoseg_op_kmeans_init(X[idx].contiguous().data_ptr(), K, D, 1, cent.data_ptr(), cpl.data_ptr(), S()))
    assign = torch.empty((N,), dtype=torch.int32, device="cuda")
    best = torch.empty((N,), dtype=torch.float32, device="cuda")
    counts = torch.empty((K,), dtype=torch.int32, device="cuda")
    objective = torch.empty((1,), dtype=torch.float32, device="cuda")
    moved = torch.empty((1,), dtype=torch.int32, device="cuda")
    scratch = torch.empty((lib.dinoseg_kmeans_scratch_bytes(B, n, K, D),), dtype=torch.uint8, device="cuda")

    def iteration():
        capi.check(lib.dinoseg_op_kmeans_assign(planes.data_ptr(), B, n, cpl.data_ptr(), K, D, assign.data_ptr(), assign.data_ptr(),
                                                best.data_ptr(), None, objective.data_ptr(), moved.data_ptr(), scratch.data_ptr(), S()))
        capi.check(lib.dinoseg_op_kmeans_update(planes.data_ptr(), B, n, assign.data_ptr(), cent.data_ptr(), cpl.data_ptr(), K, D,
                                                cent.data_ptr(), cpl.data_ptr(), counts.data_ptr(), scratch.data_ptr(), S()))

    def assign_only():
        capi.check(lib.dinoseg_op_kmeans_assign(planes.data_ptr(), B, n, cpl.data_ptr(), K, D, assign.data_ptr(), assign.data_ptr(),
                                                best.data_ptr(), None, objective.data_ptr(), moved.data_ptr(), scratch.data_ptr(), S()))

    state = {"C": X[idx].clone()}

    def torch_iteration():
        a_ = (X @ state["C"].T).argmax(dim=1)
        state["C"] = F.normalize(torch.zeros_like(state["C"]).index_add_(0, a_, X), dim=1)

    def cluster():
        return m.cluster(frames, K, iters=a.iters, chunk=chunk)

    def forwards():
        for c in range(0, B, chunk):
            m.features(frames[c:c + chunk])

    for _ in range(3):                                              # warm-up of every leg
        iteration()
        torch_iteration()
    cluster()
    forwards()
    t_iter, t_torch, t_cluster, t_fwd = [], [], [], []
    for _ in range(a.rounds):
        t_iter.append(timed(iteration)[0])
        t_torch.append(timed(torch_iteration)[0])
        t_cluster.append(timed(cluster)[0])
        t_fwd.append(timed(forwards)[0])
    back_new, back_assign, back_torch = [], [], []
    for _ in range(5):                                              # back to back, the legs still interleaved
        back_new.append(timed(lambda: [iteration() for _ in range(20)])[0] / 20)
        back_assign.append(timed(lambda: [assign_only() for _ in range(20)])[0] / 20)
        back_torch.append(timed(lambda: [torch_iteration() for _ in range(20)])[0] / 20)
    mem_new, _ = peak_delta(iteration)
    mem_torch, _ = peak_delta(torch_iteration)
    mem_cluster, res = peak_delta(cluster)
    tr, mf = predicted(N, D, K)
    med = statistics.median
    line = {"frame": [H, W], "grid": [hp, wp], "batch": B, "points": N, "k": K, "precision": a.precision, "rounds": a.rounds,
            "iters": a.iters, "iteration_ms": round(med(back_new), 4), "assign_alone_ms": round(med(back_assign), 4),
            "iteration_synchronised_ms": round(med(t_iter), 3),
            "torch_iteration_ms": round(med(back_torch), 4), "torch_iteration_synchronised_ms": round(med(t_torch), 3),
            "predicted_plane_traffic_ms": round(tr, 4), "predicted_mfma_ms": round(mf, 4),
            "cluster_ms": round(med(t_cluster), 3), "backbone_forwards_ms": round(med(t_fwd), 3),
            "cluster_ms_min_max": [round(min(t_cluster), 3), round(max(t_cluster), 3)],
            "iteration_ms_min_max": [round(min(back_new), 4), round(max(back_new), 4)],
            "torch_iteration_ms_min_max": [round(min(back_torch), 4), round(max(back_torch), 4)],
            "iteration_peak_bytes": int(mem_new), "torch_iteration_peak_bytes": int(mem_torch), "cluster_peak_bytes": int(mem_cluster),
            "scratch_bytes": int(scratch.numel()), "planes_bytes": int(planes.numel() * 2),
            "final_objective_per_point": round(float(res.objective[-1]) / N, 5), "empty_clusters": int((res.counts == 0).sum())}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--ks", default="8,64,256")
    ap.add_argument("--size", default="480x480")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_cost.jsonl"))
    ap.add_argument("--child-batch", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-k", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-h", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-w", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_batch is not None:
        return child(a)
    H, W = (int(v) for v in a.size.split("x"))
    for B in (int(v) for v in a.batches.split(",")):
        for K in (int(v) for v in a.ks.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--precision", a.precision, "--rounds", str(a.rounds), "--iters",
                   str(a.iters), "--out", a.out, "--child-batch", str(B), "--child-k", str(K), "--child-h", str(H), "--child-w", str(W)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"kmeans_cost.py: batch {B} K={K} ran past {a.child_timeout} s; nothing more is started")
            if rc != 0:
                raise SystemExit(f"kmeans_cost.py: batch {B} K={K} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
