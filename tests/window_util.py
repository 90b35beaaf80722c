"""Shared by tests/test_window_cpu.py and tests/test_window_gpu.py: the cases of the sliding-window merge (dinoseg_op_window_merge),
their inputs and the fp64 yardstick on the CPU."""
import functools

import torch
import torch.nn.functional as F

# (B, C, H, W, patch, (win_h, win_w), (stride_h, stride_w))
CASES = [
    (2, 7, 70, 100, 8, (32, 48), (24, 40)),         # frame no patch multiple; origins y 0, 24, 38 and x 0, 40, 52; ragged tiles
    (1, 150, 96, 136, 8, (64, 64), (40, 40)),
    (1, 256, 64, 64, 8, (64, 64), (64, 64)),        # one window, equal to the frame
    (2, 33, 96, 96, 16, (64, 64), (32, 32)),        # patch 16
    (1, 21, 160, 192, 8, (64, 64), (16, 16)),       # 63 windows; 16 over interior pixels, the documented maximum
    (2, 2, 43, 75, 8, (40, 24), (40, 16)),          # origins y 0, 3 and x 0, 16, 32, 48, 51
    (3, 1, 16, 24, 8, (8, 8), (8, 8)),              # one class
    (1, 150, 480, 640, 8, (240, 240), (160, 160)),  # production ratio; 12 windows
]
IDS = ["B%d-C%d-%dx%d-p%d-w%dx%d-s%dx%d" % (c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], c[6][0], c[6][1]) for c in CASES]


def mmseg_origins(L, w, s):
    """mmsegmentation's slide_inference, one axis: grids = max(L - w + s - 1, 0) // s + 1; start = idx * s; end = min(start + w, L);
    start = max(end - w, 0)."""
    return [max(min(i * s + w, L) - w, 0) for i in range(max(L - w + s - 1, 0) // s + 1)]


def windows_of(case):
    """(origins along y, origins along x, grid rows, grid columns of one window)."""
    B, C, H, W, p, (wh, ww), (sh, sw) = case
    return mmseg_origins(H, wh, sh), mmseg_origins(W, ww, sw), wh // p, ww // p


def random_logp(case):
    """log_softmax(3 randn), fp32 [B*gh*gw, hp*wp, C] on the CPU (seeded as tests/ensemble_util.py seeds its inputs)."""
    B, C, H, W = case[:4]
    oys, oxs, hp, wp = windows_of(case)
    g = torch.Generator().manual_seed(hp * 1000 + W + C)
    return torch.log_softmax(3.0 * torch.randn(B * len(oys) * len(oxs), hp * wp, C, generator=g), dim=-1)


def reference_mean(case, logp):
    """Per window F.interpolate(grid.double(), size=window, mode="bilinear", align_corners=False) added into a [B, C, H, W]
    accumulator at the window's origin, ones into a count plane, then the quotient: fp64 on the CPU."""
    B, C, H, W, p, (wh, ww), _ = case
    oys, oxs, hp, wp = windows_of(case)
    acc = torch.zeros((B, C, H, W), dtype=torch.float64)
    cnt = torch.zeros((1, 1, H, W), dtype=torch.float64)
    grids = logp.double().view(B, len(oys), len(oxs), hp, wp, C)
    for gy, oy in enumerate(oys):
        for gx, ox in enumerate(oxs):
            up = F.interpolate(grids[:, gy, gx].permute(0, 3, 1, 2), size=(wh, ww), mode="bilinear", align_corners=False)
            acc[:, :, oy:oy + wh, ox:ox + ww] += up
            cnt[:, :, oy:oy + wh, ox:ox + ww] += 1.0
    assert float(cnt.min()) >= 1.0
    return acc / cnt


@functools.lru_cache(maxsize=3)
def case_data(i: int):
    """(inputs, fp64 mean log-probs) of CASES[i], shared by the tests that need them and never modified."""
    logp = random_logp(CASES[i])
    return logp, reference_mean(CASES[i], logp)


def value_bar(logp):
    """16 * 2^-24 * max(1, max|logp|) absolute: an interpolated value carries at most 8 * 2^-24 M (the bar of
    tests/test_dense_gpu.py); the n - 1 <= 15 fp32 adds of partial sums <= n M and the division add (n - 1) / 2 + 1 / 2 units of
    2^-24 M to the mean: 16 units at n = 16."""
    return 16.0 * 2.0 ** -24 * max(1.0, float(logp.abs().max()))
