"""The multi-scale + flip ensemble on the GPU (-m gpu): dinoseg_op_upsample_ensemble (csrc/upsample_ensemble.hip) as an operator
against torch's own fp64 route on the CPU, and through DINOSeg.segment_multiscale / validation_step_dense / predict_dense.

Yardstick: sum_k softmax(F.interpolate(grid_k[.flip(-1)].double(), size, mode="bilinear", align_corners=False), 1) / K on the CPU
(tests/ensemble_util.py) -- independent of the code under test.

Value bar on probs and conf: 32 * 2^-24 * max(1, max|logp|) absolute.  An interpolated value carries at most 8 * 2^-24 * M (the bar
of tests/test_dense_gpu.py), the log-sum-exp built from such values the same again, the sums and expf / logf another 8 * 2^-24 * M:
24 * 2^-24 * M relative on a probability <= 1, rounded up to 32.
Label bar: equal to the fp64 argmax of the mean probability wherever its fp64 top-2 margin exceeds twice the value bar; at most 1e-2
of the pixels may be excluded that way (the reference alone excludes at most 4.6e-3 on these cases)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict, view_sizes
from dino_amd.weights import synthetic_frames

from .ensemble_util import CASES, IDS, LARGE_LDS_CASE, case_data, random_views, reference_probs

pytestmark = pytest.mark.gpu
S = capi.stream_ptr


def run_op(logps, views, B, C, OH, OW, labels=True, conf=True, probs=True):
    """dinoseg_op_upsample_ensemble on device tensors [B, hp*wp, C] -> (labels or None, conf or None, probs or None)."""
    K = len(views)
    for lp, (hp, wp, _) in zip(logps, views):
        assert lp.is_cuda and lp.dtype == torch.float32 and lp.is_contiguous() and lp.numel() == B * hp * wp * C
    dev = logps[0].device
    lab = torch.full((B, OH, OW), -7, dtype=torch.int32, device=dev) if labels else None
    cf = torch.full((B, OH, OW), float("nan"), dtype=torch.float32, device=dev) if conf else None
    pr = torch.full((B, C, OH, OW), float("nan"), dtype=torch.float32, device=dev) if probs else None
    lib = capi.lib()
    need = lib.dinoseg_op_upsample_ensemble_scratch_bytes(K, B, OH, OW)
    assert need == 4 * K * B * OH * OW
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    i32 = lambda xs: (ctypes.c_int32 * K)(*xs)
    capi.check(lib.dinoseg_op_upsample_ensemble((ctypes.c_void_p * K)(*[t.data_ptr() for t in logps]), i32([v[0] for v in views]),
                                                i32([v[1] for v in views]), i32([v[2] for v in views]), K, B, C, OH, OW,
                                                capi.ptr(lab), capi.ptr(cf), capi.ptr(pr), scratch.data_ptr(), S()))
    return lab, cf, pr


def value_bar(logps):
    return 32.0 * 2.0 ** -24 * max(1.0, max(float(lp.abs().max()) for lp in logps))


def build(cfg, precision):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the op against fp64
def check_against_fp64(name, case, logps, ref):
    """Every output of the op on `case` against the fp64 mean probabilities `ref`: the output subsets, the value and label bars."""
    B, C, OH, OW, views = case
    dev = [lp.cuda() for lp in logps]
    labels, conf, probs = run_op(dev, views, B, C, OH, OW)
    # output subsets: each single-output launch is bit-identical to the all-outputs launch
    l_only = run_op(dev, views, B, C, OH, OW, conf=False, probs=False)
    c_only = run_op(dev, views, B, C, OH, OW, labels=False, probs=False)
    p_only = run_op(dev, views, B, C, OH, OW, labels=False, conf=False)
    torch.cuda.synchronize()
    assert l_only[1] is None and l_only[2] is None and torch.equal(l_only[0], labels)
    assert c_only[0] is None and c_only[2] is None and torch.equal(c_only[1], conf)
    assert p_only[0] is None and p_only[1] is None and torch.equal(p_only[2], probs)
    assert torch.equal(conf, probs.amax(1)), "conf is not the maximum of probs"

    bar = value_bar(logps)
    got, top = probs.cpu(), ref.topk(min(2, C), dim=1)
    err_p = 0.0
    for c0 in range(0, C, 16):
        err_p = max(err_p, float((got[:, c0:c0 + 16].double() - ref[:, c0:c0 + 16]).abs().max()))
    err_c = float((conf.cpu().double() - top.values[:, 0]).abs().max())
    if C > 1:
        decided = (top.values[:, 0] - top.values[:, 1]) > 2.0 * bar
    else:
        decided = torch.ones((B, OH, OW), dtype=torch.bool)
    excluded = 1.0 - float(decided.double().mean())
    wrong = int((labels.cpu().long() != top.indices[:, 0])[decided].sum())
    print(f"ensemble {name}: max |probs - fp64| {err_p:.3e}, max |conf - fp64| {err_c:.3e} (bar {bar:.3e}), excluded share "
          f"{excluded:.2e}, {wrong} wrong labels of {int(decided.sum())}")
    assert err_p <= bar and err_c <= bar
    assert excluded <= 1e-2
    assert wrong == 0
    return labels, conf, probs


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_op_against_fp64(cuda, i):
    logps, ref = case_data(i)
    labels, conf, probs = check_against_fp64(IDS[i], CASES[i], logps, ref)
    if CASES[i][1] == 1:                                        # one class: label 0, probability exactly 1
        assert int(labels.abs().max()) == 0
        assert bool((probs == 1.0).all()) and bool((conf == 1.0).all())


def test_many_views_near_identity_size_take_the_large_lds(cuda):
    """Eight views at the output's own size: under one 64 x 32 tile their footprints add up to 8 * 65 * 33 = 17160 cells, which
    with the coordinate tables is more than 64 KiB even at one class per pass -- the launch asks for more of the CU's LDS.  Two
    tiles on each axis, both ragged; the mirrored views read the frame's other edge."""
    case = LARGE_LDS_CASE
    logps = random_views(case)
    check_against_fp64("B1-C5-40x70-K8-identity", case, logps, reference_probs(case, logps))


# ------------------------------------------------------------------------------------------------ 2. exact properties
@pytest.mark.parametrize("i", [0, 3, 4], ids=[IDS[0], IDS[3], IDS[4]])
def test_flipped_view_of_a_mirrored_grid_is_the_unflipped_view(cuda, i):
    """flip = 1 fed grid.flip(width) reads the very cells flip = 0 reads from grid, in the same order: bit-identical outputs."""
    B, C, OH, OW, views = CASES[i]
    logps, _ = case_data(i)
    dev = [lp.cuda() for lp in logps]
    mirrored = [lp.view(B, hp, wp, C).flip(2).contiguous().view(B, hp * wp, C) for lp, (hp, wp, _) in zip(dev, views)]
    swapped = [(hp, wp, 1 - f) for hp, wp, f in views]
    a = run_op(dev, views, B, C, OH, OW)
    b = run_op(mirrored, swapped, B, C, OH, OW)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_ties_take_the_first_maximum(cuda):
    B, C, OH, OW = 2, 9, 40, 61
    views = [(5, 7, 0), (5, 7, 1), (8, 11, 0)]
    flat = [torch.full((B, hp * wp, C), -2.1972246, dtype=torch.float32, device="cuda") for hp, wp, _ in views]
    labels, conf, probs = run_op(flat, views, B, C, OH, OW)
    assert int(labels.abs().max()) == 0                         # all classes equal: label 0 everywhere
    two = []
    for k, (hp, wp, _) in enumerate(views):
        g = torch.Generator().manual_seed(11 + k)
        t = torch.log_softmax(3.0 * torch.randn(B, hp * wp, C, generator=g), dim=-1) - 5.0
        t[:, :, 2] = -0.25
        t[:, :, 6] = -0.25
        two.append(t.cuda())
    labels, conf, probs = run_op(two, views, B, C, OH, OW)
    assert torch.equal(probs[:, 2], probs[:, 6])
    assert bool((labels == 2).all())                            # two equal maxima: the lower index
    assert torch.equal(conf, probs[:, 2])


def test_twelve_views_repeat_bit_for_bit(cuda):
    B, C, OH, OW, views = CASES[3]
    assert len(views) == 12
    dev = [lp.cuda() for lp in case_data(3)[0]]
    a = run_op(dev, views, B, C, OH, OW)
    b = run_op(dev, views, B, C, OH, OW)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. guard words
@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_nothing_is_written_outside_the_outputs_and_the_scratch(cuda, i):
    B, C, OH, OW, views = CASES[i]
    K = len(views)
    G = 4096                                                     # guard words on both sides of each buffer
    SENT = 0x7F7F7F7F                                            # (as fp32: a NaN pattern the kernel never produces)
    dev = [lp.cuda() for lp in case_data(i)[0]]
    n1, nC, nS = B * OH * OW, B * C * OH * OW, K * B * OH * OW
    bufs = {name: torch.full((n + 2 * G,), SENT, dtype=torch.int32, device="cuda")
            for name, n in (("labels", n1), ("conf", n1), ("probs", nC), ("scratch", nS))}
    assert capi.lib().dinoseg_op_upsample_ensemble_scratch_bytes(K, B, OH, OW) == 4 * nS
    i32 = lambda xs: (ctypes.c_int32 * K)(*xs)
    at = lambda name: bufs[name].data_ptr() + 4 * G
    capi.check(capi.lib().dinoseg_op_upsample_ensemble((ctypes.c_void_p * K)(*[t.data_ptr() for t in dev]), i32([v[0] for v in views]),
                                                       i32([v[1] for v in views]), i32([v[2] for v in views]), K, B, C, OH, OW,
                                                       at("labels"), at("conf"), at("probs"), at("scratch"), S()))
    torch.cuda.synchronize()
    for name, n in (("labels", n1), ("conf", n1), ("probs", nC), ("scratch", nS)):
        assert bool((bufs[name][:G] == SENT).all()) and bool((bufs[name][G + n:] == SENT).all()), name
    labels, conf, probs = run_op(dev, views, B, C, OH, OW)
    assert torch.equal(bufs["labels"][G:G + n1].view(B, OH, OW), labels)
    assert torch.equal(bufs["conf"][G:G + n1].view(torch.float32).view(B, OH, OW), conf)
    assert torch.equal(bufs["probs"][G:G + nC].view(torch.float32).view(B, C, OH, OW), probs)
    assert bool(torch.isfinite(bufs["scratch"][G:G + nS].view(torch.float32)).all())    # one log-sum-exp per view and pixel


# ------------------------------------------------------------------------------------------------ 4. model level
def resize_u8(frames, Hk, Wk):
    B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    out = torch.empty((B, Hk, Wk, 3), dtype=torch.uint8, device="cuda")
    for b in range(B):
        capi.check(capi.lib().dinoseg_op_resize_u8(frames[b].data_ptr(), H, W, out[b].data_ptr(), Hk, Wk, S()))
    return out


def views_by_the_documented_rule(m, x, scales, flip):
    """[(low-res log-probs, hp, wp, flip)] of the views segment_multiscale documents, through the public forward entries."""
    u8 = x.dtype == torch.uint8
    H, W = (x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3])
    p, out = m.cfg.patch, []
    for Hk, Wk in view_sizes(H, W, scales, p):
        if (Hk, Wk) == (H, W):
            xv = x
        elif u8:
            xv = resize_u8(x, Hk, Wk)
        else:
            xv = F.interpolate(x, size=(Hk, Wk), mode="bilinear", align_corners=False)
        for f in ((0, 1) if flip else (0,)):
            xin = torch.flip(xv, dims=[2 if u8 else 3]) if f else xv
            with torch.no_grad():
                lp = m.forward_frames(xin.contiguous())[0] if u8 else m(xin.contiguous())
            out.append((lp.contiguous(), Hk // p, Wk // p, f))
    return out


@pytest.mark.parametrize("precision", ["fp16", "bf16x3"])
@pytest.mark.parametrize("n_classes", [7, 150])
def test_segment_multiscale_equals_op_on_forward_views(cuda, precision, n_classes):
    cfg = ViTConfig(n_blocks=1, head="linear", n_classes=n_classes)
    m = build(cfg, precision)
    B, H, W, scales = 2, 64, 96, (0.5, 1.0, 1.5)
    frames = torch.from_numpy(synthetic_frames(B, H, seed=31, w=W)).cuda()
    from oracle import dinoseg_oracle as O
    x32 = O.preprocess(frames.cpu().numpy()).cuda()
    plain = m.segment(frames)[0]
    for x in (frames, x32):
        made = views_by_the_documented_rule(m, x, scales, True)
        assert [(hp, wp, f) for _, hp, wp, f in made] == [(4, 6, 0), (4, 6, 1), (8, 12, 0), (8, 12, 1), (12, 18, 0), (12, 18, 1)]
        for size in (None, (75, 101)):
            OH, OW = size or (H, W)
            want = run_op([v[0] for v in made], [v[1:] for v in made], B, n_classes, OH, OW)
            labels, conf, probs = m.segment_multiscale(x, scales=scales, flip=True, size=size, want_conf=True, want_probs=True)
            assert labels.dtype == torch.int32 and labels.shape == (B, OH, OW) and probs.shape == (B, n_classes, OH, OW)
            assert torch.equal(labels, want[0]) and torch.equal(conf, want[1]) and torch.equal(probs, want[2])
            lean = m.segment_multiscale(x, scales=scales, flip=True, size=size)
            assert lean[1] is None and lean[2] is None and torch.equal(lean[0], want[0])
    # the forwards the ensemble ran leave the plain entries as they were
    assert torch.equal(m.segment(frames)[0], plain)


def test_single_view_agrees_with_segment(cuda):
    cfg = ViTConfig(n_blocks=1, head="linear", n_classes=150)
    m = build(cfg, "fp16")
    B, H, W, OH, OW = 2, 64, 96, 75, 101
    frames = torch.from_numpy(synthetic_frames(B, H, seed=33, w=W)).cuda()
    labels, conf, probs = m.segment_multiscale(frames, scales=(1.0,), flip=False, size=(OH, OW), want_conf=True)
    plain = m.segment(frames, size=(OH, OW))[0]
    lp = m.forward_frames(frames)[0].cpu()
    case = (B, 150, OH, OW, [(H // 8, W // 8, 0)])
    top = reference_probs(case, [lp]).topk(2, dim=1)
    decided = (top.values[:, 0] - top.values[:, 1]) > 2.0 * value_bar([lp])
    assert float(decided.double().mean()) >= 0.99
    assert torch.equal(labels.cpu()[decided], plain.cpu()[decided])
    assert torch.equal(labels.cpu().long()[decided], top.indices[:, 0][decided])


def test_validation_step_dense_with_scales(cuda):
    n_classes = 7
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=n_classes), "bf16x3")
    B, H, W, OH, OW = 2, 64, 96, 100, 131
    frames = torch.from_numpy(synthetic_frames(B, H, seed=51, w=W)).cuda()
    rng = np.random.default_rng(9)
    gt = rng.integers(0, n_classes, (B, OH, OW)).astype(np.int64)
    gt[0, :7, :] = 255
    gt[1, :, 5:9] = -100
    batch = (frames, torch.from_numpy(gt))
    before = m.validation_step_dense(batch)
    out = m.validation_step_dense(batch, scales=(0.5, 1.0), flip=True)
    assert set(out) == set(before)
    assert torch.equal(out["pred"], m.segment_multiscale(frames, scales=(0.5, 1.0), flip=True, size=(OH, OW))[0])
    assert torch.equal(out["probs"], m.forward_frames(frames)[0])             # the unflipped scale-1.0 view's log-probs
    pred = out["pred"].cpu().numpy().astype(np.int64).reshape(-1)
    flat = gt.reshape(-1)
    keep = (flat >= 0) & (flat < n_classes)
    want = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(want, (flat[keep], pred[keep]), 1)
    assert np.array_equal(out["confusion"].cpu().numpy(), want)
    # without a scale-1.0 view: the first view's log-probs
    half = m.validation_step_dense(batch, scales=(0.5,), flip=True)
    assert torch.equal(half["probs"], m.forward_frames(resize_u8(frames, 32, 48))[0])
    # without the new arguments: exactly what it returned before the ensemble ran
    after = m.validation_step_dense(batch)
    assert torch.equal(after["pred"], m.segment(frames, size=(OH, OW))[0])
    for key in before:
        assert torch.equal(after[key], before[key]), key


def test_predict_dense_with_scales(cuda):
    m = build(ViTConfig(n_blocks=1), "bf16x3")
    m.set_resolution(64)
    img = np.random.default_rng(7).integers(0, 256, (100, 131, 3), dtype=np.uint8)
    plain = m.predict_dense(img)
    out = m.predict_dense(img, scales=(0.5, 1.0), flip=True)
    assert out.dtype == np.int64 and out.shape == (100, 131)
    resized = resize_u8(torch.from_numpy(img).cuda().unsqueeze(0), 64, 64)
    want = m.segment_multiscale(resized, scales=(0.5, 1.0), flip=True, size=(100, 131))[0]
    assert np.array_equal(out, want[0].cpu().numpy())
    assert np.array_equal(m.predict_dense(img), plain)


# ------------------------------------------------------------------------------------------------ 5. no large transient
def test_segment_multiscale_allocates_no_dense_transient(cuda):
    """B = 2, C = 150, 96 x 136: one [B, C, OH, OW] fp32 tensor is 15.7 MB and the torch route needs at least two; the whole
    12-view call (resized frames, 12 low-res log-prob grids, 4 bytes per view and pixel of scratch, the labels) stays under half
    of one."""
    m = build(ViTConfig(n_blocks=1, head="linear", n_classes=150), "fp16")
    B, H, W, C = 2, 96, 136, 150
    frames = torch.from_numpy(synthetic_frames(B, H, seed=61, w=W)).cuda()
    m.segment_multiscale(frames)                                 # warm-up: weights packed, workspace at its largest
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, conf, probs = m.segment_multiscale(frames)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    dense = 4 * B * C * H * W
    print(f"segment_multiscale peak-memory delta {delta} bytes; one dense tensor would be {dense}")
    assert conf is None and probs is None and labels.shape == (B, H, W)
    assert delta < dense // 2
