"""Pixel-resolution output on the GPU (-m gpu): the fused bilinear upsample + argmax of the log-probs (csrc/upsample.hip) as an
operator against torch's own fp64 bilinear on the CPU, and through DINOSeg.segment / predict_dense / validation_step_dense.

Yardstick: F.interpolate(logp.double().view(B, hp, wp, C).permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear",
align_corners=False) on the CPU -- independent of the code under test.

Value bar: every element of `dense` within 8 * 2^-24 * max|logp| of it.  Log-probs share a sign, so each a + (b - a) lambda has
three roundings of at most 2^-24 max|v|; two chained lerps give 6, and 8 leaves room for contraction-order differences.
Label bar: equal to the fp64 argmax wherever the fp64 top-2 margin exceeds twice the value bar; at most 1e-3 of the pixels may be
excluded that way (inputs log_softmax(3 randn): the reference alone stays at or under 4e-5)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames

pytestmark = pytest.mark.gpu
S = capi.stream_ptr

# (B, hp, wp, C, OH, OW)
SHAPES = [
    (2, 60, 80, 7, 480, 640),
    (2, 60, 80, 150, 480, 640),
    (1, 60, 60, 256, 480, 480),
    (2, 30, 40, 21, 480, 640),
    (2, 30, 40, 21, 479, 641),
    (2, 60, 80, 7, 375, 500),
    (2, 8, 16, 33, 100, 131),
    (1, 60, 80, 150, 1080, 1920),
    (2, 4, 4, 2, 64, 64),
    (3, 1, 1, 5, 8, 8),
]
IDS = ["%dx%dx%dx%d-%dx%d" % s for s in SHAPES]


def random_logp(B, hp, wp, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(3.0 * torch.randn(B, hp * wp, C, generator=g), dim=-1)


def reference(logp, B, hp, wp, C, OH, OW):
    return F.interpolate(logp.double().view(B, hp, wp, C).permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False)


def run_op(logp, B, hp, wp, C, OH, OW, want_dense=True, want_labels=True):
    """dinoseg_op_upsample_argmax on a device tensor [B, hp*wp, C] -> (labels or None, dense or None)."""
    assert logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous() and logp.numel() == B * hp * wp * C
    labels = torch.full((B, OH, OW), -7, dtype=torch.int32, device=logp.device) if want_labels else None
    dense = torch.full((B, C, OH, OW), float("nan"), dtype=torch.float32, device=logp.device) if want_dense else None
    capi.check(capi.lib().dinoseg_op_upsample_argmax(logp.data_ptr(), B, hp, wp, C, OH, OW, capi.ptr(labels), capi.ptr(dense), S()))
    return labels, dense


def build(cfg, precision):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


def op_on_frames(m, frames, OH, OW):
    """The op applied to the log-probs forward_frames returns for `frames`: what segment() must reproduce bit for bit."""
    B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    hp, wp = H // m.cfg.patch, W // m.cfg.patch
    lp, am = m.forward_frames(frames)
    labels, _ = run_op(lp, B, hp, wp, m.cfg.n_classes, OH, OW, want_dense=False)
    return labels, lp, am


# ------------------------------------------------------------------------------------------------ 1. the op against fp64
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_op_against_fp64_bilinear(cuda, shape):
    B, hp, wp, C, OH, OW = shape
    logp = random_logp(B, hp, wp, C, seed=hp * 1000 + OW + C)
    dev = logp.cuda()
    labels, dense = run_op(dev, B, hp, wp, C, OH, OW)
    only, none = run_op(dev, B, hp, wp, C, OH, OW, want_dense=False)
    _, dense_only = run_op(dev, B, hp, wp, C, OH, OW, want_labels=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(only, labels), "labels-only launch differs from the launch with dense_out"
    assert torch.equal(dense_only, dense)
    ref = reference(logp, B, hp, wp, C, OH, OW)
    bound = 8.0 * 2.0 ** -24 * float(logp.abs().max())
    got = dense.cpu()
    err = 0.0
    for c0 in range(0, C, 16):                                  # (class slabs: the 1080 x 1920 x 150 case is 2.5 GB in fp64)
        err = max(err, float((got[:, c0:c0 + 16].double() - ref[:, c0:c0 + 16]).abs().max()))
    top = ref.topk(2, dim=1)
    margin = top.values[:, 0] - top.values[:, 1]
    decided = margin > 2.0 * bound
    excluded = 1.0 - float(decided.double().mean())
    wrong = int((labels.cpu().long() != top.indices[:, 0])[decided].sum())
    print(f"upsample {IDS[SHAPES.index(shape)]}: max |dense - fp64| {err:.3e} (bound {bound:.3e}), excluded share {excluded:.2e}, "
          f"{wrong} wrong labels of {int(decided.sum())}")
    assert err <= bound
    assert excluded <= 1e-3
    assert wrong == 0


# ------------------------------------------------------------------------------------------------ 2. exact cases
def test_small_integers_at_8x_are_exact(cuda):
    """Small-integer inputs at an 8x ratio: lambda is a multiple of 1/16 and every product is exact, so the labels equal the fp64
    labels everywhere and dense equals the fp64 result bit for bit."""
    B, hp, wp, C, OH, OW = 2, 6, 9, 5, 48, 72
    g = torch.Generator().manual_seed(3)
    logp = -torch.randint(0, 16, (B, hp * wp, C), generator=g).float()
    labels, dense = run_op(logp.cuda(), B, hp, wp, C, OH, OW)
    ref = reference(logp, B, hp, wp, C, OH, OW)
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(dense.cpu(), ref.float())
    assert torch.equal(labels.cpu().long(), ref.argmax(1))


def test_ties_take_the_first_maximum(cuda):
    B, hp, wp, C, OH, OW = 2, 5, 7, 9, 40, 61
    flat = torch.full((B, hp * wp, C), -2.1972246, dtype=torch.float32)
    labels, _ = run_op(flat.cuda(), B, hp, wp, C, OH, OW)
    assert int(labels.abs().max()) == 0                         # all classes equal: label 0 everywhere
    two = random_logp(B, hp, wp, C, seed=11) - 5.0
    two[:, :, 2] = -0.25
    two[:, :, 6] = -0.25
    labels, dense = run_op(two.cuda(), B, hp, wp, C, OH, OW)
    assert torch.equal(dense[:, 2], dense[:, 6])
    assert bool((labels == 2).all())                            # two equal maxima: the lower index


def test_identity_size_copies(cuda):
    B, hp, wp, C = 2, 12, 20, 33
    logp = random_logp(B, hp, wp, C, seed=5)
    labels, dense = run_op(logp.cuda(), B, hp, wp, C, hp, wp)
    assert torch.equal(dense.cpu(), logp.view(B, hp, wp, C).permute(0, 3, 1, 2))
    assert torch.equal(labels.cpu().long(), logp.argmax(-1).view(B, hp, wp))


# ------------------------------------------------------------------------------------------------ 3. guard bytes
@pytest.mark.parametrize("shape", [SHAPES[5], SHAPES[6]], ids=[IDS[5], IDS[6]])
def test_nothing_is_written_outside_the_outputs(cuda, shape):
    B, hp, wp, C, OH, OW = shape
    G = 4096                                                     # guard elements on both sides of each output
    SENT = 0x7F7F7F7F                                            # (as fp32: a NaN pattern no interpolation produces)
    dev = random_logp(B, hp, wp, C, seed=21).cuda()
    nl, nd = B * OH * OW, B * C * OH * OW
    lab = torch.full((nl + 2 * G,), SENT, dtype=torch.int32, device="cuda")
    den = torch.full((nd + 2 * G,), SENT, dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(dev.data_ptr(), B, hp, wp, C, OH, OW, lab.data_ptr() + 4 * G, den.data_ptr() + 4 * G,
                                                     S()))
    torch.cuda.synchronize()
    for buf, n in ((lab, nl), (den, nd)):
        assert bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all())
    inner = lab[G:G + nl]
    assert int(inner.min()) >= 0 and int(inner.max()) < C
    vals = den[G:G + nd].view(torch.float32)
    assert bool(torch.isfinite(vals).all()) and float(vals.max()) <= 0.0
    labels, dense = run_op(dev, B, hp, wp, C, OH, OW)
    assert torch.equal(inner.view(B, OH, OW), labels) and torch.equal(vals.view(B, C, OH, OW), dense)


# ------------------------------------------------------------------------------------------------ 4. model level
# (id, config, batch, H, W, output size or None = the frames' own)
MODEL_CASES = [
    ("batch1", ViTConfig(n_blocks=2), 1, 64, 64, None),
    ("rect64x128", ViTConfig(n_blocks=1), 2, 64, 128, (100, 131)),
    ("patch16", ViTConfig(n_blocks=1, patch=16, pos_grid=14), 2, 64, 96, None),
    ("classes150", ViTConfig(n_blocks=1, head="linear", n_classes=150), 2, 64, 64, (75, 64)),
    ("linear-head", ViTConfig(n_blocks=1, head="linear"), 3, 64, 64, None),
]


@pytest.mark.parametrize("precision", ["fp16x3", "fp16", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_segment_equals_op_on_forward_frames(cuda, precision, case):
    _, cfg, B, H, W, size = case
    m = build(cfg, precision)
    frames = torch.from_numpy(synthetic_frames(B, H, seed=31, w=W)).cuda()
    OH, OW = size or (H, W)
    want, lp, am = op_on_frames(m, frames, OH, OW)
    labels, dense = m.segment(frames, size=size)
    assert dense is None and labels.dtype == torch.int32 and labels.shape == (B, OH, OW)
    assert torch.equal(labels, want)
    labels2, dense2 = m.segment(frames, size=size, want_logp=True)
    assert torch.equal(labels2, want) and dense2.shape == (B, cfg.n_classes, OH, OW)
    assert torch.equal(dense2, run_op(lp, B, H // cfg.patch, W // cfg.patch, cfg.n_classes, OH, OW)[1])
    # fp32 CHW input, as the training and validation steps take it: the same frames normalised on the host
    from oracle import dinoseg_oracle as O
    x = O.preprocess(frames.cpu().numpy()).cuda()
    with torch.no_grad():
        lpx = m(x)
    hp, wp = H // cfg.patch, W // cfg.patch
    assert torch.equal(m.segment(x, size=size)[0], run_op(lpx.contiguous(), B, hp, wp, cfg.n_classes, OH, OW, want_dense=False)[0])
    # the low-res outputs of the dense entry are those of dinoseg_forward_hw
    n = hp * wp
    lo_lp = torch.empty((B * n, cfg.n_classes), dtype=torch.float32, device="cuda")
    lo_am = torch.empty((B * n,), dtype=torch.int32, device="cuda")
    lab = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_forward_dense_hw(m._handle, frames.data_ptr(), capi.INPUT_U8_HWC, B, H, W, OH, OW, lo_lp.data_ptr(),
                                                   lo_am.data_ptr(), lab.data_ptr(), None, S()))
    assert torch.equal(lo_lp, lp) and torch.equal(lo_am, am) and torch.equal(lab, want)


@pytest.mark.parametrize("precision", ["fp16x3", "fp16", "bf16x3", "bf16"])
def test_segment_under_the_two_stream_split(cuda, precision):
    """A batch at split_min: each half upsamples from its own workspace on its own stream into its slice.  streams = 2, streams = 1 and
    the op on forward_frames' log-probs give the same labels (and dense values), also for an odd batch."""
    m = build(ViTConfig(n_blocks=2), precision)
    for B in (8, 9):
        frames = torch.from_numpy(synthetic_frames(B, 64, seed=41 + B)).cuda()
        with dino_amd.options(streams=1):
            want, lp, _ = op_on_frames(m, frames, 100, 131)
            one, one_d = m.segment(frames, size=(100, 131), want_logp=True)
            dino_amd.set_option("streams", 2)
            for _ in range(2):
                two, two_d = m.segment(frames, size=(100, 131), want_logp=True)
                assert torch.equal(two, one) and torch.equal(two_d, one_d)
            lean, _ = m.segment(frames, size=(100, 131))            # log-probs in the two workspaces
        assert torch.equal(one, want) and torch.equal(lean, want)


# ------------------------------------------------------------------------------------------------ 5. predict_dense
def test_predict_dense(cuda):
    m = build(ViTConfig(n_blocks=2), "bf16x3")
    m.set_resolution(64)
    rng = np.random.default_rng(7)
    for rows, cols in ((100, 131), (480, 640)):
        img = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        old = m.predict(img)
        out = m.predict_dense(img)
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (rows, cols)
        resized = torch.empty((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
        src = torch.from_numpy(img).cuda()
        capi.check(capi.lib().dinoseg_op_resize_u8(src.data_ptr(), rows, cols, resized.data_ptr(), 64, 64, S()))
        want, _, am = op_on_frames(m, resized, rows, cols)
        assert np.array_equal(out, want[0].cpu().numpy().astype(np.int64))
        assert np.array_equal(m.predict_dense(img, size=(64, 64)), op_on_frames(m, resized, 64, 64)[0][0].cpu().numpy())
        # predict() keeps its map: the 8 x 8 argmax in 60 x 60 blocks, before and after the dense call
        kron = np.kron(am.cpu().numpy().astype(np.int64).reshape(8, 8), np.ones((60, 60), dtype=np.int64))
        assert np.array_equal(old, kron) and np.array_equal(m.predict(img), kron)


# ------------------------------------------------------------------------------------------------ 6. validation_step_dense
@pytest.mark.parametrize("n_classes", [7, 150])
def test_validation_step_dense(cuda, n_classes):
    cfg = ViTConfig(n_blocks=1, head="linear", n_classes=n_classes)
    m = build(cfg, "bf16x3")
    B, OH, OW = 2, 100, 131
    frames = torch.from_numpy(synthetic_frames(B, 64, seed=51)).cuda()
    rng = np.random.default_rng(9)
    gt = rng.integers(0, n_classes, (B, OH, OW)).astype(np.int64)
    gt[0, :7, :] = 255                                          # "void" in ADE20K / COCO-Stuff style masks
    gt[1, :, 5:9] = -100                                        # F.nll_loss's ignore_index
    out = m.validation_step_dense((frames, torch.from_numpy(gt)))
    assert set(out) == set(m.validation_step((frames, torch.zeros(B, 64, dtype=torch.long)))), "same keys as validation_step"
    labels = m.segment(frames, size=(OH, OW))[0]
    assert torch.equal(out["pred"], labels) and torch.equal(out["probs"], m.forward_frames(frames)[0])
    pred = labels.cpu().numpy().astype(np.int64).reshape(-1)
    flat = gt.reshape(-1)
    keep = (flat >= 0) & (flat < n_classes)
    want = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(want, (flat[keep], pred[keep]), 1)
    assert int(want.sum()) == B * OH * OW - 7 * OW - OH * 4
    assert np.array_equal(out["confusion"].cpu().numpy(), want)
    metrics = m.validation_epoch_end([out, out])
    assert len(metrics) == 3 and all(np.isfinite(v) for v in metrics.values())
    assert metrics == m.validation_epoch_end([out])             # (ratios: counting every pixel twice changes nothing)


# ------------------------------------------------------------------------------------------------ 7. no large transient
def test_segment_allocates_no_dense_transient(cuda):
    """C = 150, B = 4 at 480 x 640: the [B, C, OH, OW] fp32 tensor the torch route materialises would be 737 MB; segment() may
    allocate at most twice its own results plus the low-res log-probs (about 12 MB)."""
    cfg = ViTConfig(n_blocks=1, head="linear", n_classes=150)
    m = build(cfg, "fp16")
    B, H, W = 4, 480, 640
    frames = torch.from_numpy(synthetic_frames(B, H, seed=61, w=W)).cuda()
    m.segment(frames)                                            # warm-up: weights packed, workspace allocated
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, dense = m.segment(frames, want_logp=False)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    results = labels.numel() * labels.element_size()
    low_res = B * (H // 8) * (W // 8) * 150 * 4
    print(f"segment peak-memory delta {delta} bytes; results {results}, low-res log-probs {low_res}, dense would be {B * 150 * H * W * 4}")
    assert dense is None and labels.shape == (B, H, W)
    assert delta <= 2 * (results + low_res)


# ------------------------------------------------------------------------------------------------ 8. capture
def test_forward_dense_is_graph_capturable(cuda):
    """One dinoseg_forward_dense_hw (a batch at split_min: both streams, both upsamples) captured after a warm-up call and replayed
    gives the eager labels."""
    m = build(ViTConfig(n_blocks=2), "fp16")
    B, H, W, OH, OW = 8, 64, 64, 100, 131
    frames = torch.from_numpy(synthetic_frames(B, H, seed=71)).cuda()
    eager = m.segment(frames, size=(OH, OW))[0].clone()
    labels = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda")

    def call():
        capi.check(capi.lib().dinoseg_forward_dense_hw(m._handle, frames.data_ptr(), capi.INPUT_U8_HWC, B, H, W, OH, OW, None, None,
                                                       labels.data_ptr(), None, S()))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()                                                   # warm-up outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.synchronize()
    labels.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(labels, eager)
