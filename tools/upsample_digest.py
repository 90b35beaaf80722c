"""GPU box: a sha256 of every output of the four pixel-resolution operators (csrc/upsample.hip, upsample_loss.hip,
upsample_ensemble.hip, windows.hip) on seeded inputs, one line per output, for a byte comparison of two builds of the library (a
change to the shared tile walk of csrc/upsample_common.h must not move a bit):
    DINOSEG_LIB=<build A>/libdinoseg_hip.so python tools/upsample_digest.py > a.txt
    python tools/upsample_digest.py > b.txt && cmp a.txt b.txt
The shapes are the SHAPES / CASES of tests/test_dense_gpu.py, tests/test_dense_loss_gpu.py, tests/test_ensemble_gpu.py and
tests/test_window_gpu.py, and one the lists do not hold: eight views at the output's own size, the ensemble's large-LDS path
(tests/ensemble_util.py LARGE_LDS_CASE, the case of test_many_views_near_identity_size_take_the_large_lds).
  upsample_argmax    labels, dense
  upsample_nll       loss, n_valid, dL, under option deterministic (the loss is then a fixed-order sum; dL is a gather either way)
  upsample_ensemble  labels, conf, probs, and the per-view log-sum-exps left in the caller's scratch
  window_merge       labels, dense"""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dino_amd  # noqa: E402
from dino_amd import capi  # noqa: E402
from tests import ensemble_util, window_util  # noqa: E402
from tests import test_dense_gpu as D  # noqa: E402
from tests import test_dense_loss_gpu as L  # noqa: E402
from tests import test_window_gpu as W  # noqa: E402


def show(what, names, tensors):
    torch.cuda.synchronize()
    for name, t in zip(names, tensors):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        print(f"{what} {name} {tuple(t.shape)} {h}", flush=True)


def ensemble(logps, case):
    """tests/test_ensemble_gpu.py's run_op, with the scratch kept: (labels, conf, probs, lse [K, B, OH, OW])."""
    B, C, OH, OW, views = case
    K = len(views)
    lab = torch.full((B, OH, OW), -7, dtype=torch.int32, device="cuda")
    cf = torch.full((B, OH, OW), float("nan"), device="cuda")
    pr = torch.full((B, C, OH, OW), float("nan"), device="cuda")
    lib = capi.lib()
    lse = torch.full((lib.dinoseg_op_upsample_ensemble_scratch_bytes(K, B, OH, OW) // 4,), float("nan"), device="cuda")
    i32 = lambda xs: (ctypes.c_int32 * K)(*xs)
    capi.check(lib.dinoseg_op_upsample_ensemble((ctypes.c_void_p * K)(*[t.data_ptr() for t in logps]), i32([v[0] for v in views]),
                                                i32([v[1] for v in views]), i32([v[2] for v in views]), K, B, C, OH, OW,
                                                lab.data_ptr(), cf.data_ptr(), pr.data_ptr(), lse.data_ptr(), capi.stream_ptr()))
    return lab, cf, pr, lse.view(K, B, OH, OW)


for shape, name in zip(D.SHAPES, D.IDS):
    B, hp, wp, C, OH, OW = shape
    logp = D.random_logp(B, hp, wp, C, seed=hp * 1000 + OW + C).cuda()
    show(f"upsample_argmax/{name}", ("labels", "dense"), D.run_op(logp, *shape))
    show(f"upsample_argmax/{name}/labels-only", ("labels",), D.run_op(logp, *shape, want_dense=False)[:1])

with dino_amd.options(deterministic=1):
    for i, (shape, name) in enumerate(zip(L.SHAPES, L.IDS)):
        logp, t = L.random_case(shape, seed=100 + i)
        loss, dlogp, nv = L.run_op(logp.cuda(), t.cuda(), shape, ignore=255 if shape[3] <= 255 else -100)
        show(f"upsample_nll/{name}", ("loss", "n_valid", "dL"), (loss, nv, dlogp))

for case, name in list(zip(ensemble_util.CASES, ensemble_util.IDS)) + [(ensemble_util.LARGE_LDS_CASE, "B1-C5-40x70-K8-identity")]:
    logps = [lp.cuda() for lp in ensemble_util.random_views(case)]
    show(f"upsample_ensemble/{name}", ("labels", "conf", "probs", "lse"), ensemble(logps, case))

for case, name in zip(window_util.CASES, window_util.IDS):
    logp = window_util.random_logp(case).cuda()
    show(f"window_merge/{name}", ("labels", "dense"), W.run_merge(logp, case))
    show(f"window_merge/{name}/labels-only", ("labels",), W.run_merge(logp, case, dense=False)[:1])
