"""Shared by tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py: the cases of the multi-scale + flip ensemble
(dinoseg_op_upsample_ensemble), their inputs and the fp64 yardstick on the CPU."""
import functools

import torch
import torch.nn.functional as F

# (B, C, OH, OW, [(hp, wp, flip), ...])
CASES = [
    (2, 7, 70, 100, [(5, 7, 0), (9, 13, 1), (12, 17, 0), (9, 13, 0)]),                  # ragged tiles on both axes
    (2, 150, 96, 136, [(6, 9, 0), (6, 9, 1), (12, 17, 0), (12, 17, 1), (18, 26, 0), (18, 26, 1)]),
    (1, 256, 64, 64, [(8, 8, 0), (8, 8, 1)]),
    (1, 21, 128, 160, [(h, w, f) for h, w in ((8, 10), (12, 15), (16, 20), (20, 25), (24, 30), (28, 35)) for f in (0, 1)]),
    (2, 33, 20, 24, [(20, 24, 0), (10, 12, 1)]),                                        # one view at identity size
    (2, 2, 64, 64, [(4, 4, 0), (4, 4, 1)]),
    (1, 150, 480, 640, [(30, 40, 0), (60, 80, 1), (90, 120, 0)]),                       # production ratio
    (3, 1, 8, 8, [(1, 1, 0), (1, 1, 1)]),
]
# eight views at the output's own size: the large-LDS path (tests/test_ensemble_gpu.py, tools/upsample_digest.py)
LARGE_LDS_CASE = (1, 5, 40, 70, [(40, 70, k & 1) for k in range(8)])
IDS = ["B%d-C%d-%dx%d-K%d" % (c[0], c[1], c[2], c[3], len(c[4])) for c in CASES]


def random_views(case):
    """log_softmax(3 randn) per view, fp32 [B, hp*wp, C] on the CPU (seeded as tests/test_dense_gpu.py seeds its inputs)."""
    B, C, OH, OW, views = case
    out = []
    for k, (hp, wp, _) in enumerate(views):
        g = torch.Generator().manual_seed(hp * 1000 + OW + C + 7919 * k)
        out.append(torch.log_softmax(3.0 * torch.randn(B, hp * wp, C, generator=g), dim=-1))
    return out


def reference_probs(case, logps):
    """sum_k softmax(F.interpolate(grid_k[.flip(-1)].double(), size, mode="bilinear", align_corners=False), 1) / K in fp64."""
    B, C, OH, OW, views = case
    acc = torch.zeros((B, C, OH, OW), dtype=torch.float64)
    for (hp, wp, flip), lp in zip(views, logps):
        grid = lp.double().view(B, hp, wp, C).permute(0, 3, 1, 2)
        if flip:
            grid = grid.flip(-1)
        acc += torch.softmax(F.interpolate(grid, size=(OH, OW), mode="bilinear", align_corners=False), 1)
    return acc / len(views)


@functools.lru_cache(maxsize=None)
def case_data(i: int):
    """(inputs, fp64 mean probabilities) of CASES[i], computed once per process and never modified."""
    logps = random_views(CASES[i])
    return logps, reference_probs(CASES[i], logps)
