"""GPU box: a sha256 of every output of the feature-space operators (csrc/propagate.hip, knn.hip, kmeans.hip, ncut.hip,
ncut_split.hip) on seeded inputs, one line per output, for a byte comparison of two builds of the library (a change to the shared pair
walk of csrc/pair_common.h, to the selection of csrc/select_common.h or to the pass pieces of csrc/ncut_common.h must not move a bit):
    DINOSEG_LIB=<build A>/libdinoseg_hip.so python tools/feature_digest.py > a.txt
    python tools/feature_digest.py > b.txt && cmp a.txt b.txt
The shapes and inputs are the CASES of tests/test_propagate_gpu.py and tests/knn_util.py, CASES x KINDS of tests/test_kmeans_gpu.py
and PARAMS of tests/test_ncut_gpu.py, and one ragged shape for the two row kernels; the whole run takes a few seconds.
  normalize_tokens   planes; kmeans_init: centroids, planes (with and without the normalisation)
  propagate          the candidate scores and indices left in the scratch, seg, topk_idx, topk_w
  knn_labels         the same five, at the library's number of ranges (splits 0) and at one range
  kmeans_assign      assign, best, scores, objective, moved and the tile records left in the scratch
  kmeans_update      centroids, planes, counts and the partial sums and counts left in the scratch
  ncut_graph         words, degree
  ncut_iterate       z_out, rho, fg, eigvec, margin, seed_cell after 4 passes and after 0, from the one-workgroup entry and from the
                     split entry at rows_per_group 0 and 32"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import knn_util as KU  # noqa: E402
from tests import test_kmeans_gpu as K  # noqa: E402
from tests import test_knn_gpu as KN  # noqa: E402
from tests import test_ncut_gpu as NC  # noqa: E402
from tests import test_ncut_split_gpu as NS  # noqa: E402
from tests import test_propagate_gpu as P  # noqa: E402


def show(what, names, tensors):
    torch.cuda.synchronize()
    for name, t in zip(names, tensors):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        print(f"{what} {name} {tuple(t.shape)} {h}", flush=True)


def ident(case):
    return "x".join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------ the row kernels
B, n, D, Kc = 2, 37, 192, 5
rng = np.random.default_rng(900)
tok = torch.from_numpy(rng.standard_normal((B, n + 1, D)).astype(np.float32)).cuda()
show(f"normalize_tokens/{B}x{n}x{D}", ("planes",), (P.normalize(tok).view(torch.int16),))
rows = torch.from_numpy(rng.standard_normal((Kc, D)).astype(np.float32)).cuda()
for norm in (True, False):
    cent, cpl = K.km_init(rows, normalize_rows=norm)
    show(f"kmeans_init/{Kc}x{D}/normalize{int(norm)}", ("centroids", "planes"), (cent, cpl.view(torch.int16)))

# ------------------------------------------------------------------------------------------------ propagate
for i, case in enumerate(P.CASES):
    hp, wp, D, C, n_ctx, R, k = case
    n = hp * wp
    tq, cp, sg = P.device_case(i)
    out = (torch.empty((n, C), dtype=torch.float32, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
           torch.empty((n, k), dtype=torch.float32, device="cuda"),
           torch.zeros((P.scratch_bytes(hp, wp, n_ctx, k),), dtype=torch.uint8, device="cuda"))
    seg, idx, w = P.run_propagate(tq, cp, sg, hp, wp, R, k, out=out)
    cand = out[3].view(torch.int32).view(2, n_ctx, n, k)                # fp32 scores, then int32 indices
    show(f"propagate/{ident(case)}", ("cand_scores", "cand_idx", "seg", "topk_idx", "topk_w"), (cand[0], cand[1], seg, idx, w))

# ------------------------------------------------------------------------------------------------ k-NN retrieval
for i, case in enumerate(KU.CASES):
    B, n, M, rows, D, C, k, kind = case
    N = B * n
    qp, bp, labels = KN.device_case(i)
    for splits in (0, 1):
        out = (torch.empty((N, C), dtype=torch.float32, device="cuda"), torch.empty((N, k), dtype=torch.int32, device="cuda"),
               torch.empty((N, k), dtype=torch.float32, device="cuda"),
               torch.zeros((KN.scratch_bytes(N, M, k, splits),), dtype=torch.uint8, device="cuda"))
        seg, idx, w, scratch = KN.run_knn(qp, bp, M, labels, C, k, splits=splits, out=out)
        cand = scratch.view(torch.int32).view(2, -1, N, k)              # fp32 scores, then int32 indices, [S][N][k] each
        show(f"knn_labels/{ident(case)}/splits{splits}", ("cand_scores", "cand_idx", "seg", "topk_idx", "topk_w"),
             (cand[0], cand[1], seg, idx, w))

# ------------------------------------------------------------------------------------------------ k-means
for i, case in enumerate(K.CASES):
    B, hp, wp, D, Kc = case
    n, N = hp * wp, B * hp * wp
    tiles = (N + 63) // 64
    for kind in K.KINDS:
        planes, _ = K.device_points(i, kind)
        scratch = K.scratch_for(B, n, Kc, D)
        cent, cpl = K.km_init(K.dev(K.inputs(i, kind)[1]))
        a, best, scores, obj, moved = K.km_assign(planes, cpl, scratch, want_scores=True)
        torch.cuda.synchronize()
        records = scratch[-8 * tiles:].clone()                          # [tiles] fp32 objective shares, [tiles] int32 moved counts
        show(f"kmeans_assign/{ident(case)}/{kind}", ("assign", "best", "scores", "objective", "moved", "tile_records"),
             (a, best, scores, obj, moved, records))
        c2, p2, counts = K.km_update(planes, a, cent, cpl, scratch)
        torch.cuda.synchronize()
        show(f"kmeans_update/{ident(case)}/{kind}", ("centroids", "planes", "counts", "partials"),
             (c2, p2.view(torch.int16), counts, scratch[:-8 * tiles]))
        a2, best2, _, obj2, moved2 = K.km_assign(planes, p2, scratch, prev=a)
        show(f"kmeans_assign/{ident(case)}/{kind}/second", ("assign", "best", "objective", "moved"), (a2, best2, obj2, moved2))

# ------------------------------------------------------------------------------------------------ normalized cut
for p in NC.PARAMS:
    i, kind, tau = p
    B, hp, wp, D = NC.CASES[i]
    n = hp * wp
    graph, degree = NC.nc_graph(NC.device_points(i, kind)[0], tau)
    show(f"ncut_graph/{NC.pid(p)}", ("words", "degree"), (graph, degree))
    for iters in (4, 0):
        got = NC.nc_iterate(graph, degree, NC.start_for(B, n), iters)
        show(f"ncut_iterate/{NC.pid(p)}/iters{iters}", NS.KEYS, [got[k] for k in NS.KEYS])
        for rows_per_group in (0, 32):
            got = NS.split_iterate(graph, degree, NC.start_for(B, n), iters, rows_per_group)
            show(f"ncut_iterate_split/{NC.pid(p)}/iters{iters}/rows{rows_per_group}", NS.KEYS, [got[k] for k in NS.KEYS])
