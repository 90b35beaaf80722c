"""GPU box: a sha256 of every output of the cases of tests/test_route_plan_gpu.py, one line per output, for a byte comparison of two
builds of the library (a host-side change must not move a bit):
    DINOSEG_LIB=<build A>/libdinoseg_hip.so python tools/route_digest.py > a.txt
    python tools/route_digest.py > b.txt && cmp a.txt b.txt
Per route: forward_frames' log-probs and argmax; on the default route also segment() at 100 x 100 and the side paths; the two-stream
split (streams = 2, split_min = 2); the loss and every bound gradient of one fused_training_step with option deterministic in bf16 and
bf16x3, for gemm_ln 0 and 1."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dino_amd  # noqa: E402
from dino_amd.weights import synthetic_labels  # noqa: E402
from tests import test_route_plan_gpu as T  # noqa: E402
from tests.gpu_util import route_options  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def show(what, tensors):
    for i, t in enumerate(tensors):
        if t is not None:
            print(f"{what} [{i}] {tuple(t.shape)} {digest(t)}", flush=True)


for kind, precision in T.ALL_CASES:
    for case, out, counts in T.run_cases(kind, precision):
        show(case, out)
for precision in T.PRECISIONS:
    m, frames = T.small_model(precision), T.small_frames()
    with route_options(m, streams=1):
        show(f"segment/{precision}", m.segment(frames, size=(100, 100), want_logp=True))
    with route_options(m, streams=2, split_min=2):
        show(f"split/{precision}", m.forward_frames(frames))
        show(f"split-segment/{precision}", m.segment(frames, size=(100, 100), want_logp=True))
labels = torch.from_numpy(synthetic_labels(2, 64, 7, seed=6)).cuda()
for precision in ("bf16", "bf16x3"):
    for gemm_ln in (0, 1):
        m = T.small_model(precision)
        m.unfreeze_bb()
        with route_options(m, deterministic=1, gemm_ln=gemm_ln):
            out = m.fused_training_step((T.small_frames(), labels), 0)
            torch.cuda.synchronize()
            show(f"train/{precision}/gemm_ln={gemm_ln}/loss", [out["loss"], out["probs"]])
            for name, p in m.named_parameters():
                show(f"train/{precision}/gemm_ln={gemm_ln}/{name}", [p.grad])
