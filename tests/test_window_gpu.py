"""Sliding-window inference on the GPU (-m gpu): dinoseg_op_window_merge and dinoseg_op_crop_windows (csrc/windows.hip) as operators
against torch's own fp64 route on the CPU, and through DINOSeg.segment_windows / validation_step_dense / predict_dense.

Yardstick: per window F.interpolate(grid.double(), size=window, mode="bilinear", align_corners=False) added into a [B, C, H, W]
accumulator at the window's origin, ones into a count plane, the quotient (tests/window_util.py) -- independent of the code under
test.

Value bar on dense: 16 * 2^-24 * max(1, max|logp|) absolute.  An interpolated value carries at most 8 * 2^-24 M (the bar of
tests/test_dense_gpu.py); the n - 1 <= 15 fp32 adds of partial sums <= n M and the division add (n - 1) / 2 + 1 / 2 units to the
mean: 16 units at n = 16.
Label bar: equal to the fp64 argmax wherever the fp64 top-2 margin exceeds twice the value bar; at most 1e-3 of the pixels may be
excluded that way (the reference alone excludes 0 .. 1.3e-4 on these cases), and no wrong label among the rest."""
import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict, window_origins
from dino_amd.weights import synthetic_frames

from .window_util import CASES, IDS, case_data, random_logp, reference_mean, value_bar, windows_of

pytestmark = pytest.mark.gpu
S = capi.stream_ptr


def run_merge(logp, case, labels=True, dense=True):
    """dinoseg_op_window_merge on a device tensor [B*G, n, C] -> (labels or None, dense or None)."""
    B, C, H, W, p, (wh, ww), (sh, sw) = case
    oys, oxs, hp, wp = windows_of(case)
    assert logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous()
    assert tuple(logp.shape) == (B * len(oys) * len(oxs), hp * wp, C)
    lab = torch.full((B, H, W), -7, dtype=torch.int32, device=logp.device) if labels else None
    den = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device=logp.device) if dense else None
    capi.check(capi.lib().dinoseg_op_window_merge(logp.data_ptr(), B, H, W, p, wh, ww, sh, sw, C, capi.ptr(lab), capi.ptr(den), S()))
    return lab, den


def run_upsample(logp, B, hp, wp, C, OH, OW):
    lab = torch.empty((B, OH, OW), dtype=torch.int32, device=logp.device)
    den = torch.empty((B, C, OH, OW), dtype=torch.float32, device=logp.device)
    capi.check(capi.lib().dinoseg_op_upsample_argmax(logp.data_ptr(), B, hp, wp, C, OH, OW, lab.data_ptr(), den.data_ptr(), S()))
    return lab, den


def first_maximum(dense: torch.Tensor) -> np.ndarray:
    """The smallest class index that attains the maximum over classes, on the CPU (np.argmax returns the first occurrence)."""
    d = dense.cpu().numpy()
    return np.argmax(d == d.max(axis=1, keepdims=True), axis=1)


def check_bars(name, logp, labels, dense, ref):
    """The value bar on dense and the label bar on labels against the fp64 mean `ref` (CPU tensors / fp64)."""
    B, C = ref.shape[0], ref.shape[1]
    bar = value_bar(logp)
    got, err = dense.cpu(), 0.0
    for c0 in range(0, C, 16):
        err = max(err, float((got[:, c0:c0 + 16].double() - ref[:, c0:c0 + 16]).abs().max()))
    top = ref.topk(min(2, C), dim=1)
    if C > 1:
        decided = (top.values[:, 0] - top.values[:, 1]) > 2.0 * bar
    else:
        decided = torch.ones(ref.shape[0:1] + ref.shape[2:], dtype=torch.bool)
    excluded = 1.0 - float(decided.double().mean())
    wrong = int((labels.cpu().long() != top.indices[:, 0])[decided].sum())
    print(f"window merge {name}: max |dense - fp64| {err:.3e} (bar {bar:.3e}), excluded share {excluded:.2e}, "
          f"{wrong} wrong labels of {int(decided.sum())}")
    assert err <= bar
    assert excluded <= 1e-3
    assert wrong == 0


def build(cfg, precision):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the op against fp64
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_op_against_fp64(cuda, i):
    logp, ref = case_data(i)
    dev = logp.cuda()
    labels, dense = run_merge(dev, CASES[i])
    l_only = run_merge(dev, CASES[i], dense=False)
    d_only = run_merge(dev, CASES[i], labels=False)
    torch.cuda.synchronize()
    assert l_only[1] is None and torch.equal(l_only[0], labels)
    assert d_only[0] is None and torch.equal(d_only[1], dense)
    assert np.array_equal(labels.cpu().numpy(), first_maximum(dense)), "labels are not the first maximum of dense"
    check_bars(IDS[i], logp, labels, dense, ref)
    if CASES[i][1] == 1:
        assert int(labels.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 2., 3. exact properties
@pytest.mark.parametrize("case", [CASES[2], (2, 7, 40, 72, 8, (40, 72), (40, 72))], ids=["B1-C256-64x64", "B2-C7-40x72"])
def test_one_window_equal_to_the_frame_is_upsample_argmax(cuda, case):
    B, C, H, W, p = case[:5]
    dev = random_logp(case).cuda()
    labels, dense = run_merge(dev, case)
    want = run_upsample(dev, B, H // p, W // p, C, H, W)
    assert torch.equal(labels, want[0]) and torch.equal(dense, want[1])


@pytest.mark.parametrize("case", [(2, 33, 64, 96, 8, (32, 32), (32, 32)), CASES[6]], ids=["B2-C33-64x96-w32", IDS[6]])
def test_non_overlapping_windows_are_each_window_alone(cuda, case):
    """stride == window on a frame that is a multiple of the window: every window's region is upsample_argmax of that window."""
    B, C, H, W, p, (wh, ww), _ = case
    oys, oxs, hp, wp = windows_of(case)
    assert oys == list(range(0, H, wh)) and oxs == list(range(0, W, ww))
    dev = random_logp(case).cuda()
    labels, dense = run_merge(dev, case)
    alone = run_upsample(dev, dev.shape[0], hp, wp, C, wh, ww)     # every window as a frame of its own
    for b in range(B):
        for gy, oy in enumerate(oys):
            for gx, ox in enumerate(oxs):
                wi = (b * len(oys) + gy) * len(oxs) + gx
                assert torch.equal(labels[b, oy:oy + wh, ox:ox + ww], alone[0][wi]), (b, gy, gx)
                assert torch.equal(dense[b, :, oy:oy + wh, ox:ox + ww], alone[1][wi]), (b, gy, gx)


def test_ties_take_the_first_maximum(cuda):
    case = (2, 9, 70, 100, 8, (32, 48), (24, 40))
    n_win, cells = 2 * 3 * 3, 4 * 6
    flat = torch.full((n_win, cells, 9), -2.1972246, dtype=torch.float32, device="cuda")
    labels, dense = run_merge(flat, case)
    assert int(labels.abs().max()) == 0                         # all classes equal: label 0 everywhere
    g = torch.Generator().manual_seed(11)
    two = torch.log_softmax(3.0 * torch.randn(n_win, cells, 9, generator=g), dim=-1) - 5.0
    two[:, :, 2] = -0.25
    two[:, :, 6] = -0.25
    labels, dense = run_merge(two.cuda(), case)
    assert torch.equal(dense[:, 2], dense[:, 6])
    assert bool((labels == 2).all())                            # two equal maxima: the lower index
    # two windows that disagree, with means that tie exactly: an 8 x 12 frame, 8 x 8 windows at x = 0 and 4, one cell each.
    # Window 0 alone says class 1, window 1 alone class 2; where both cover, (-1 + -3) / 2 = (-3 + -1) / 2 = -2: the first.
    case = (1, 3, 8, 12, 8, (8, 8), (8, 4))
    assert windows_of(case)[:2] == ([0], [0, 4])
    lp = torch.tensor([[[-8.0, -1.0, -3.0]], [[-8.0, -3.0, -1.0]]], device="cuda")
    labels, dense = run_merge(lp, case)
    assert torch.equal(dense[0, :, 0, 5].cpu(), torch.tensor([-8.0, -2.0, -2.0]))
    assert labels[0, :, :4].eq(1).all() and labels[0, :, 4:8].eq(1).all() and labels[0, :, 8:].eq(2).all()


def test_sixteen_fold_coverage_repeats_bit_for_bit(cuda):
    dev = case_data(4)[0].cuda()
    a = run_merge(dev, CASES[4])
    b = run_merge(dev, CASES[4])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 4. guard words
G = 4096                                                         # guard words on both sides of each buffer
SENT = 0x7F7F7F7F                                                # (as fp32: a NaN pattern the kernels never produce)


@pytest.mark.parametrize("i", [0, 5], ids=[IDS[0], IDS[5]])
def test_nothing_is_written_outside_the_outputs(cuda, i):
    B, C, H, W, p, (wh, ww), (sh, sw) = CASES[i]
    dev = case_data(i)[0].cuda()
    before = dev.clone()
    n1, nC = B * H * W, B * C * H * W
    merge = capi.lib().dinoseg_op_window_merge
    bufs = {name: torch.full((n + 2 * G,), SENT, dtype=torch.int32, device="cuda") for name, n in (("labels", n1), ("dense", nC))}
    at = lambda name: bufs[name].data_ptr() + 4 * G
    capi.check(merge(dev.data_ptr(), B, H, W, p, wh, ww, sh, sw, C, at("labels"), at("dense"), S()))
    torch.cuda.synchronize()
    for name, n in (("labels", n1), ("dense", nC)):
        assert bool((bufs[name][:G] == SENT).all()) and bool((bufs[name][G + n:] == SENT).all()), name
    labels, dense = run_merge(dev, CASES[i])
    assert torch.equal(bufs["labels"][G:G + n1].view(B, H, W), labels)
    assert torch.equal(bufs["dense"][G:G + nC].view(torch.float32).view(B, C, H, W), dense)
    assert torch.equal(dev, before)
    # labels only: the labels again, and not a word anywhere else
    for b in bufs.values():
        b.fill_(SENT)
    capi.check(merge(dev.data_ptr(), B, H, W, p, wh, ww, sh, sw, C, at("labels"), None, S()))
    torch.cuda.synchronize()
    assert bool((bufs["dense"] == SENT).all())
    assert bool((bufs["labels"][:G] == SENT).all()) and bool((bufs["labels"][G + n1:] == SENT).all())
    assert torch.equal(bufs["labels"][G:G + n1].view(B, H, W), labels)
    assert torch.equal(dev, before)


# ------------------------------------------------------------------------------------------------ 5. the crop
def sliced_windows(x, u8, wh, ww, sh, sw):
    """Every window of the batch by torch slicing with window_origins, in list order."""
    H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
    out = []
    for b in range(x.shape[0]):
        for oy in window_origins(H, wh, sh):
            for ox in window_origins(W, ww, sw):
                out.append(x[b, oy:oy + wh, ox:ox + ww] if u8 else x[b, :, oy:oy + wh, ox:ox + ww])
    return torch.stack(out)


@pytest.mark.parametrize("u8", [True, False], ids=["uint8-hwc", "fp32-chw"])
@pytest.mark.parametrize("shape", [(2, 43, 75, (40, 24), (40, 16)), (2, 70, 100, (32, 48), (24, 40))], ids=["2x43x75", "2x70x100"])
def test_crop_windows_is_torch_slicing(cuda, u8, shape):
    B, H, W, (wh, ww), (sh, sw) = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    if u8:
        x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        x = torch.randn(B, 3, H, W, generator=g).cuda()
    want = sliced_windows(x, u8, wh, ww, sh, sw)
    total = want.shape[0]
    assert total == B * len(window_origins(H, wh, sh)) * len(window_origins(W, ww, sw)) and total >= 8
    per = want[0].numel() * want.element_size()                 # bytes of one window
    gb = 4 * G
    # the whole list, a chunk inside the first frame, and one that spans the frame boundary
    for first, count in ((0, total), (3, 5), (total // B - 2, 5)):
        buf = torch.full((count * per + 2 * gb,), 0x7F, dtype=torch.uint8, device="cuda")
        capi.check(capi.lib().dinoseg_op_crop_windows(x.data_ptr(), 0 if u8 else 1, B, H, W, wh, ww, sh, sw, first, count,
                                                      buf.data_ptr() + gb, S()))
        torch.cuda.synchronize()
        assert bool((buf[:gb] == 0x7F).all()) and bool((buf[gb + count * per:] == 0x7F).all())
        got = buf[gb:gb + count * per].view(want.dtype).view((count,) + tuple(want.shape[1:]))
        assert torch.equal(got, want[first:first + count])


# ------------------------------------------------------------------------------------------------ 6. model level
@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
@pytest.mark.parametrize("n_classes", [7, 150])
def test_segment_windows_equals_op_on_forward_windows(cuda, precision, n_classes):
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=n_classes), precision)
    B, H, W, win, chunk = 2, 70, 100, (32, 48), 4
    stride = ((2 * win[0]) // 3, (2 * win[1]) // 3)             # the documented default: (21, 32)
    frames = torch.from_numpy(synthetic_frames(B, H, seed=37, w=W)).cuda()
    case = (B, n_classes, H, W, 8, win, stride)
    # the documented rule through the public entries: torch slicing, forward_frames on the same chunks
    crops = sliced_windows(frames, True, *win, *stride)
    assert crops.shape[0] == 18
    parts = [m.forward_frames(crops[f:f + chunk].contiguous())[0] for f in range(0, crops.shape[0], chunk)]
    logp = torch.cat(parts).view(crops.shape[0], (win[0] // 8) * (win[1] // 8), n_classes).contiguous()
    want = run_merge(logp, case)
    labels, dense = m.segment_windows(frames, window=win, want_logp=True, max_windows=chunk)
    assert labels.dtype == torch.int32 and labels.shape == (B, H, W) and dense.shape == (B, n_classes, H, W)
    assert torch.equal(labels, want[0]) and torch.equal(dense, want[1])
    lean = m.segment_windows(frames, window=win, stride=stride, max_windows=chunk)
    assert lean[1] is None and torch.equal(lean[0], want[0])
    check_bars(f"segment_windows {precision} C={n_classes}", logp.cpu(), labels, dense, reference_mean(case, logp.cpu()))


def test_window_equal_to_the_frame_is_segment(cuda):
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=150), "fp16")
    frames = torch.from_numpy(synthetic_frames(2, 64, seed=33, w=96)).cuda()
    want = m.segment(frames, want_logp=True)
    for kw in (dict(window=(64, 96)), dict(), dict(window=(64, 96), stride=(5, 7), max_windows=2)):
        labels, dense = m.segment_windows(frames, want_logp=True, **kw)     # (the default 480 x 480 window is clamped to the frame)
        assert torch.equal(labels, want[0]) and torch.equal(dense, want[1])


def test_validation_step_dense_with_window(cuda):
    n_classes = 7
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=n_classes), "bf16x3")
    B, H, W = 2, 70, 100
    frames = torch.from_numpy(synthetic_frames(B, H, seed=51, w=W)).cuda()
    rng = np.random.default_rng(9)
    gt = rng.integers(0, n_classes, (B, H, W)).astype(np.int64)
    gt[0, :7, :] = 255
    batch = (frames, torch.from_numpy(gt))
    out = m.validation_step_dense(batch, window=(32, 48), stride=(24, 40))
    assert set(out) == {"pred", "gt", "probs", "confusion"}
    assert torch.equal(out["pred"], m.segment_windows(frames, window=(32, 48), stride=(24, 40))[0])
    assert out["probs"].shape == (B * 3 * 3, 4 * 6, n_classes)
    pred = out["pred"].cpu().numpy().astype(np.int64).reshape(-1)
    flat = gt.reshape(-1)
    keep = flat != 255
    want = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(want, (flat[keep], pred[keep]), 1)
    assert np.array_equal(out["confusion"].cpu().numpy(), want)
    metrics = m.validation_epoch_end([out, out])
    assert all(np.isfinite(v) for v in metrics.values())


def test_predict_dense_with_window(cuda):
    m = build(ViTConfig(n_blocks=1), "bf16x3")
    m.set_resolution(64)
    img = np.random.default_rng(7).integers(0, 256, (100, 131, 3), dtype=np.uint8)
    plain = m.predict_dense(img)
    out = m.predict_dense(img, window=(64, 64), stride=(32, 40))
    assert out.dtype == np.int64 and out.shape == (100, 131)
    want = m.segment_windows(torch.from_numpy(img).cuda().unsqueeze(0), window=(64, 64), stride=(32, 40))[0]
    assert np.array_equal(out, want[0].cpu().numpy())
    assert np.array_equal(m.predict_dense(img, window=64, stride=(32, 40), size=(100, 131)), out)
    assert np.array_equal(m.predict_dense(img), plain)


# ------------------------------------------------------------------------------------------------ 7. no large transient
def test_segment_windows_allocates_no_dense_transient(cuda):
    """B = 1, C = 150, 192 x 256, nine 96 x 128 windows: one [B, C, H, W] fp32 tensor is 29.5 MB; the call allocates the windows'
    log-probs (1.0 MB), one batch of cropped windows (0.3 MB) and the labels (0.2 MB).  The peak stays below the dense tensor
    alone, so none can have existed."""
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=150), "fp16")
    B, H, W, C, win = 1, 192, 256, 150, (96, 128)
    frames = torch.from_numpy(synthetic_frames(B, H, seed=61, w=W)).cuda()
    m.segment_windows(frames, window=win)                        # warm-up: weights packed, workspace at its largest
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, dense = m.segment_windows(frames, window=win)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    one_dense = 4 * B * C * H * W
    small = 4 * 9 * (12 * 16) * C + 9 * 96 * 128 * 3 + 4 * B * H * W
    print(f"segment_windows peak-memory delta {delta} bytes; one dense tensor would be {one_dense}, the windows' log-probs, "
          f"the window batch and the labels are {small}")
    assert dense is None and labels.shape == (B, H, W)
    assert delta < one_dense
