"""Pixel-resolution training loss on the GPU (-m gpu): dinoseg_op_upsample_nll (csrc/upsample_loss.hip) against torch's fp64
F.interpolate + F.cross_entropy + autograd on the CPU, its behaviour on ignored / out-of-range labels, determinism and write
containment, and the model's steps on pixel labels (fused_training_step_dense, training_step_dense, fit()).

Bars of the op, per element, U = 2^-24, e_u = 8 U max|logp| (the dense-value bar of test_dense_gpu.py), n = valid pixels:
    loss:  |loss - ref| <= (2 e_u + 8 U) + (4 sqrt(n) + 8) U sum|l_pix| / n
    dL:    |dL - ref|   <= ( T(E) + (4 sqrt(S) + 8) U T(|g|) ) / n
           g = (p - onehot) valid,  E = (p (2 e_u + (4 + 2 |U_c - lse|) U) + 2 U) valid,  S = (2 ceil(OH/hp)) (2 ceil(OW/wp)),
           T = the transposed bilinear map (autograd of F.interpolate in fp64)
Two lerp errors enter U_c - lse; the exp and its argument scaling add a few ulp plus |arg| U; the support sum of S terms
accumulates in fp32."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames
from oracle import dinoseg_oracle as O

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
U = 2.0 ** -24

# (B, hp, wp, C, OH, OW)
SHAPES = [
    (2, 4, 4, 2, 64, 64),           # 16x ratio
    (3, 1, 1, 5, 8, 8),             # a single source cell
    (2, 8, 16, 33, 100, 131),       # non-integer ratio, C > 32
    (1, 6, 9, 150, 48, 72),         # wide class count
    (1, 5, 7, 256, 40, 61),         # C at the limit
    (2, 7, 5, 7, 7, 5),             # identity
    (2, 15, 20, 21, 120, 160),      # 8x ratio
    (2, 3, 5, 150, 95, 97),         # ratios near 32 and 19
    (1, 60, 80, 7, 480, 640),       # the production grid, many tiles
]
IDS = ["%dx%dx%dx%d-%dx%d" % s for s in SHAPES]


def random_case(shape, seed, ignored=True):
    """logp = log_softmax(3 randn) [B, hp*wp, C]; labels uniform in [0, C) with 10 % set to 255 and 3 % to -100.  At C = 256 the
    label 255 is a class (the op refuses it as ignore_index): there the same 10 % are set to -100 as well."""
    B, hp, wp, C, OH, OW = shape
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(3.0 * torch.randn(B, hp * wp, C, generator=g), dim=-1)
    t = torch.randint(0, C, (B, OH, OW), generator=g, dtype=torch.int64)
    if ignored:
        r = torch.rand(B, OH, OW, generator=g)
        t[r < 0.10] = 255 if C <= 255 else -100
        t[r > 0.97] = -100
    return logp, t


def scratch_for(shape):
    n = capi.lib().dinoseg_op_upsample_nll_scratch_bytes(*shape)
    assert n > 0
    return torch.empty((n,), dtype=torch.uint8, device="cuda")


def run_op(logp, t, shape, ignore=255, want_grad=True, flags=None, loss=None, dlogp=None, scratch=None):
    """dinoseg_op_upsample_nll on device tensors -> (loss [1], dlogp [B, hp*wp, C] or None, n_valid [1])."""
    B, hp, wp, C, OH, OW = shape
    assert logp.is_cuda and logp.dtype == torch.float32 and logp.is_contiguous() and logp.numel() == B * hp * wp * C
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B * OH * OW
    loss = torch.full((1,), float("nan"), device="cuda") if loss is None else loss
    if want_grad and dlogp is None:
        dlogp = torch.full((B, hp * wp, C), float("nan"), device="cuda")
    nv = torch.full((1,), -1.0, device="cuda")
    scratch = scratch_for(shape) if scratch is None else scratch
    capi.check(capi.lib().dinoseg_op_upsample_nll(logp.data_ptr(), B, hp, wp, C, OH, OW, t.data_ptr(), ignore, loss.data_ptr(),
                                                  capi.ptr(dlogp) if want_grad else None, nv.data_ptr(), capi.ptr(flags),
                                                  scratch.data_ptr(), S()))
    return loss, (dlogp if want_grad else None), nv


def reference(logp, t, shape):
    """fp64 on the CPU: (loss, dL [B, hp*wp, C], n, loss bound, dL bound [B, hp*wp, C])."""
    B, hp, wp, C, OH, OW = shape
    Lr = logp.double().view(B, hp, wp, C).clone().requires_grad_()
    up = F.interpolate(Lr.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False)
    t_ref = t.clone()
    if C <= 255:
        t_ref[t_ref == 255] = -100
    loss = F.cross_entropy(up, t_ref, ignore_index=-100)
    (dL,) = torch.autograd.grad(loss, Lr, retain_graph=True)
    T = lambda Z: torch.autograd.grad(up, Lr, Z, retain_graph=True)[0]
    with torch.no_grad():
        valid = ((t >= 0) & (t < C)).unsqueeze(1).double()
        n = float(valid.sum())
        tc = t.clamp(0, C - 1).unsqueeze(1)
        lse = torch.logsumexp(up, dim=1, keepdim=True)
        p = torch.exp(up - lse)
        g = (p - torch.zeros_like(p).scatter_(1, tc, 1.0)) * valid
        l_pix = (lse - up.gather(1, tc)) * valid
        e_u = 8.0 * U * float(logp.abs().max())
        E = (p * (2.0 * e_u + (4.0 + 2.0 * (up - lse).abs()) * U) + 2.0 * U) * valid
        Ssup = (2 * math.ceil(OH / hp)) * (2 * math.ceil(OW / wp))
    bound_dL = (T(E) + (4.0 * math.sqrt(Ssup) + 8.0) * U * T(g.abs())) / n
    bound_loss = (2.0 * e_u + 8.0 * U) + (4.0 * math.sqrt(n) + 8.0) * U * float(l_pix.abs().sum()) / n
    return float(loss.detach()), dL.reshape(B, hp * wp, C), n, bound_loss, bound_dL.detach().reshape(B, hp * wp, C)


# ------------------------------------------------------------------------------------------------ 1. the op against fp64
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_op_against_fp64(cuda, shape):
    logp, t = random_case(shape, seed=shape[1] * 1000 + shape[5] + shape[3])
    loss, dlogp, nv = run_op(logp.cuda(), t.cuda(), shape, ignore=255 if shape[3] <= 255 else -100)
    torch.cuda.synchronize()
    ref_loss, ref_dL, n, b_loss, b_dL = reference(logp, t, shape)
    assert float(nv) == n
    err_loss = abs(float(loss) - ref_loss)
    err = (dlogp.cpu().double() - ref_dL).abs()
    ratio = torch.where(b_dL > 0, err / b_dL.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"upsample_nll {IDS[SHAPES.index(shape)]}: loss error/bound {err_loss / b_loss:.3e} (|dloss| {err_loss:.3e}), "
          f"worst dL error/bound {float(ratio.max()):.3e} (max |ddL| {float(err.max()):.3e}, max |dL| {float(ref_dL.abs().max()):.3e})")
    assert torch.isfinite(dlogp).all()
    assert err_loss <= b_loss
    assert bool((err <= b_dL).all())


# ------------------------------------------------------------------------------------------------ 2. behaviour of the op
def test_identity_is_nll_loss(cuda):
    """(OH, OW) == (hp, wp), no ignored label: U = L exactly and |lse| <= C 2^-24, so the loss is F.nll_loss's."""
    shape = (2, 7, 5, 7, 7, 5)
    logp, t = random_case(shape, seed=5, ignored=False)
    dev = logp.cuda()
    loss, _, nv = run_op(dev, t.cuda(), shape)
    want = F.nll_loss(dev.view(-1, 7), t.cuda().view(-1))
    print(f"identity: loss {float(loss):.9f}, F.nll_loss {float(want):.9f}")
    assert float(nv) == 70.0
    assert abs(float(loss) - float(want)) <= 1e-6


def test_ignored_and_out_of_range_labels(cuda):
    shape = (2, 6, 9, 7, 48, 72)
    B, hp, wp, C, OH, OW = shape
    logp, t = random_case(shape, seed=11)
    t[1] = 255                                                  # one frame entirely void
    flags = torch.zeros((1,), dtype=torch.int32, device="cuda")
    loss, dlogp, nv = run_op(logp.cuda(), t.cuda(), shape, flags=flags)
    assert int(flags) == 0 and torch.isfinite(loss).all()
    assert float(nv) == float(((t >= 0) & (t < C)).sum())
    assert bool((dlogp[1] == 0).all()) and bool((dlogp[0] != 0).any())
    # every pixel ignored: NaN loss (torch: the mean over zero pixels), gradient all zeros
    loss0, d0, nv0 = run_op(logp.cuda(), torch.full((B, OH, OW), -100, dtype=torch.int64, device="cuda"), shape, flags=flags)
    assert math.isnan(float(loss0)) and float(nv0) == 0.0 and bool((d0 == 0).all()) and int(flags) == 0
    # a label C + 3 is treated as ignored and latches the flag
    t2 = t.clone()
    t2[0, 5, 7] = C + 3
    t3 = t.clone()
    t3[0, 5, 7] = 255
    loss2, d2, _ = run_op(logp.cuda(), t2.cuda(), shape, flags=flags)
    loss3, d3, _ = run_op(logp.cuda(), t3.cuda(), shape)
    assert int(flags) == 1
    assert torch.equal(d2, d3) and abs(float(loss2) - float(loss3)) <= 1e-5       # (the loss sum's atomics land in any order)


def test_check_labels_reports_a_bad_pixel_label_once(cuda):
    m, frames, y = small_model_and_batch()
    y = y.clone()
    y[1, 3, 4] = 7 + 3
    m.fused_training_step_dense((frames, y))
    with pytest.raises(IndexError):
        m.check_labels()
    m.check_labels()                                            # reported once
    y[1, 3, 4] = 255
    m.fused_training_step_dense((frames, y))
    m.check_labels()
    y[0, 0, 0] = -3
    x = O.preprocess(frames.cpu().numpy()).cuda()
    m.training_step_dense((x, y))
    with pytest.raises(IndexError):
        m.check_labels()
    m.check_labels()


def test_loss_only_call_and_determinism(cuda):
    """dL is bit-identical run to run whatever the options; under option deterministic the loss is too, and a loss-only call
    (dlogp_out = NULL) gives the same bits."""
    shape = (2, 8, 16, 33, 100, 131)
    logp, t = random_case(shape, seed=21)
    dev, td = logp.cuda(), t.cuda()
    runs = [run_op(dev, td, shape) for _ in range(3)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    with dino_amd.options(deterministic=1):
        det = [run_op(dev, td, shape) for _ in range(3)]
        only, none, _ = run_op(dev, td, shape, want_grad=False)
        torch.cuda.synchronize()
    assert none is None
    for l, d, _ in det:
        assert torch.equal(l, det[0][0]) and torch.equal(d, runs[0][1])
    assert torch.equal(only, det[0][0])
    assert abs(float(det[0][0]) - float(runs[0][0])) <= 1e-5


def test_writes_stay_inside_the_outputs(cuda):
    shape = (2, 8, 16, 33, 100, 131)
    B, hp, wp, C, OH, OW = shape
    logp, t = random_case(shape, seed=31)
    n = B * hp * wp * C
    pad = 4096
    big = torch.full((n + 2 * pad,), -7.25, device="cuda")
    lbuf = torch.full((257,), -7.25, device="cuda")
    for det in (0, 1):
        with dino_amd.options(deterministic=det):
            big.fill_(-7.25)
            lbuf.fill_(-7.25)
            _, d, _ = run_op(logp.cuda(), t.cuda(), shape, loss=lbuf[128:129], dlogp=big[pad:pad + n].view(B, hp * wp, C))
            torch.cuda.synchronize()
        assert bool((big[:pad] == -7.25).all()) and bool((big[pad + n:] == -7.25).all())
        assert bool((lbuf[:128] == -7.25).all()) and bool((lbuf[129:] == -7.25).all())
        assert torch.isfinite(lbuf[128]) and bool((d != -7.25).all())


def test_op_is_graph_capturable(cuda):
    shape = (2, 8, 16, 33, 100, 131)
    logp, t = random_case(shape, seed=41)
    dev, td = logp.cuda(), t.cuda()
    with dino_amd.options(deterministic=1):
        eager_loss, eager_d, _ = run_op(dev, td, shape)
        loss = torch.zeros((1,), device="cuda")
        d = torch.zeros_like(eager_d)
        scratch = scratch_for(shape)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            run_op(dev, td, shape, loss=loss, dlogp=d, scratch=scratch)     # warm-up outside the capture
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                run_op(dev, td, shape, loss=loss, dlogp=d, scratch=scratch)
        torch.cuda.synchronize()
        loss.fill_(-1.0)
        d.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss) and torch.equal(d, eager_d)


# ------------------------------------------------------------------------------------------------ 3. the model
def build(cfg, precision, **kw):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0"), sd


def pixel_labels(B, OH, OW, C, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, (B, OH, OW)).astype(np.int64)
    y[rng.random((B, OH, OW)) < 0.1] = 255
    y[0, :3, :] = 255
    return torch.from_numpy(y)


def small_model_and_batch():
    """ViT-S/8, two blocks, 7 classes, bf16x3, unfrozen; B = 2 frames at 64 x 96 with 64 x 96 pixel labels."""
    m, _ = build(ViTConfig(n_blocks=2), "bf16x3")
    m.unfreeze_bb()
    frames = torch.from_numpy(synthetic_frames(2, 64, seed=5, w=96)).cuda()
    return m, frames, pixel_labels(2, 64, 96, 7, seed=6).cuda()


def test_fused_step_equals_its_three_parts(cuda):
    """dinoseg_train_forward_hw + dinoseg_op_upsample_nll + dinoseg_backward by hand: the same loss bits and gradients under option
    deterministic; the step's pred is dinoseg_op_upsample_argmax of its own probs."""
    m, frames, y = small_model_and_batch()
    B, H, W, hp, wp, C = 2, 64, 96, 8, 12, 7
    shape = (B, hp, wp, C, H, W)
    lib = capi.lib()
    with dino_amd.options(deterministic=1):
        out = m.fused_training_step_dense((frames, y))
        want = {k: p.grad.clone() for k, p in m.named_parameters()}
        assert all(torch.isfinite(v).all() for v in want.values()) and float(want["clf.layer_3.weight"].abs().max()) > 0
        logp = torch.empty((B * hp * wp, C), device="cuda")
        capi.check(lib.dinoseg_train_forward_hw(m._handle, frames.data_ptr(), capi.INPUT_U8_HWC, B, H, W, logp.data_ptr(), S()))
        loss, dlogp, _ = run_op(logp, y.contiguous(), shape)
        capi.check(lib.dinoseg_backward(m._handle, dlogp.data_ptr(), S()))
        torch.cuda.synchronize()
    assert torch.equal(logp, out["probs"]) and torch.equal(loss.reshape(()), out["loss"])
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, want[k]), k
    assert out["pred"].dtype == torch.int32 and out["pred"].shape == (B, H, W)
    assert out["gt"].dtype == torch.int64 and torch.equal(out["gt"], y.reshape(-1))
    pred = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    capi.check(lib.dinoseg_op_upsample_argmax(out["probs"].data_ptr(), B, hp, wp, C, H, W, pred.data_ptr(), None, S()))
    assert torch.equal(out["pred"], pred)


def test_autograd_sibling_equals_fused_step(cuda):
    m, frames, y = small_model_and_batch()
    x = O.preprocess(frames.cpu().numpy()).cuda()
    fused = m.fused_training_step_dense((x, y))
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    out = m.training_step_dense((x, y))
    assert out["loss"].grad_fn is not None and out["probs"].shape == (2 * 96, 7)
    out["loss"].backward()
    assert abs(float(out["loss"]) - float(fused["loss"])) <= 1e-6
    assert torch.equal(out["pred"], fused["pred"]) and torch.equal(out["gt"], fused["gt"])
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        scale = float(want[k].abs().max()) + 1e-12
        assert float((p.grad - want[k]).abs().max()) <= 2e-5 * scale, k
    # dense_nll_loss alone: its gradient is the op's dlogp times the incoming gradient
    lp = out["probs"].clone().requires_grad_()
    (3.0 * dino_amd.dense_nll_loss(lp, y, grid=(8, 12))).backward()
    _, d, _ = run_op(out["probs"].contiguous(), y.contiguous(), (2, 8, 12, 7, 64, 96))
    assert torch.equal(lp.grad, (3.0 * d).view(-1, 7))


def test_fused_step_against_the_oracle(cuda):
    """The CPU restatement + fp32 F.interpolate + F.cross_entropy + autograd, with the G12 bars of the patch-label step
    (test_g15_finetune_step_bf16x3): loss within 2e-4, every gradient within 2e-3 of its norm."""
    from tests.test_rect_cpu import logp_hw
    cfg = ViTConfig(n_blocks=2)
    m, sd = build(cfg, "bf16x3")
    m.unfreeze_bb()
    frames = synthetic_frames(2, 64, seed=5, w=96)
    y = pixel_labels(2, 64, 96, 7, seed=6)
    out = m.fused_training_step_dense((torch.from_numpy(frames).cuda(), y.cuda()))
    Wt = O.to_torch(sd, requires_grad=True)
    lp = logp_hw(O.preprocess(frames), Wt, 2)
    up = F.interpolate(lp.view(2, 8, 12, 7).permute(0, 3, 1, 2), size=(64, 96), mode="bilinear", align_corners=False)
    loss = F.cross_entropy(up, y, ignore_index=255)
    loss.backward()
    dloss = abs(float(out["loss"]) - float(loss.detach()))
    worst, worst_k = 0.0, None
    for k, p in m.named_parameters():
        ref = Wt[k].grad.reshape(-1)
        rel = float((p.grad.detach().cpu().reshape(-1) - ref).abs().max()) / (float(ref.norm()) + 1e-30)
        if rel > worst:
            worst, worst_k = rel, k
    print(f"dense step vs oracle: |dloss| {dloss:.3e}, worst max|dgrad| / |grad| {worst:.3e} ({worst_k})")
    assert dloss <= 2e-4
    for k, p in m.named_parameters():
        ref = Wt[k].grad.reshape(-1)
        assert float((p.grad.detach().cpu().reshape(-1) - ref).abs().max()) <= 2e-3 * float(ref.norm()) + 1e-7, k


def test_fit_on_pixel_labels(cuda, tmp_path):
    cfg = ViTConfig(embed_dim=128, num_heads=2, n_blocks=1, n_classes=7, head="mlp")
    m = DINOSeg(arch=cfg, head="mlp", n_blocks=1, n_classes=7, lr=1e-3, optimizer=torch.optim.Adam, freeze_backbone=False,
                max_epochs=1, write_path=str(tmp_path), precision="bf16x3").to("cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()})
    frames = torch.from_numpy(synthetic_frames(6, 64, seed=3))
    y = pixel_labels(6, 64, 64, 7, seed=4)
    train = [(frames[0:2], y[0:2]), (frames[2:4], y[2:4])]
    val = [(frames[4:6], y[4:6])]
    out = m.fit(train_dataloader=train, val_dataloader=val, test_dataloader=val)
    h = out["history"]
    assert len(h) == 1 and math.isfinite(h[0]["train_loss"]) and math.isfinite(h[0]["val_acc"]) and math.isfinite(h[0]["train_acc"])
    assert set(out["test"]) == {"test_acc", "test_iou", "test_F1"}
    assert m.best_ck is not None and os.path.exists(m.best_ck)
    # patch labels run as before
    lab = (frames.float().reshape(6, 8, 8, 8, 8, 3).mean(dim=(2, 4, 5)) // 37).long().reshape(6, 64)
    out2 = m.fit(train_dataloader=[(frames[0:2], lab[0:2]), (frames[2:4], lab[2:4])], val_dataloader=[(frames[4:6], lab[4:6])])
    assert len(out2["history"]) == 1 and math.isfinite(out2["history"][0]["train_loss"]) and out2["test"] is None


def test_dense_step_is_graph_capturable(cuda):
    """dinoseg_train_step_dense_hw on a warm handle (workspaces, the d logp buffer and the events exist) captured and replayed:
    the eager loss and gradients, bit for bit under option deterministic."""
    m, frames, y = small_model_and_batch()
    B, H, W = 2, 64, 96
    yf = y.reshape(-1).contiguous()
    with dino_amd.options(deterministic=1):
        eager = m.fused_training_step_dense((frames, y))
        want = {k: p.grad.clone() for k, p in m.named_parameters()}
        loss = torch.zeros((), device="cuda")

        def call():
            capi.check(capi.lib().dinoseg_train_step_dense_hw(m._handle, frames.data_ptr(), capi.INPUT_U8_HWC, B, H, W, H, W, yf.data_ptr(),
                                                              255, loss.data_ptr(), None, S()))
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            call()                                              # warm-up on this stream outside the capture
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                call()
        torch.cuda.synchronize()
        loss.fill_(-1.0)
        for p in m.parameters():
            p.grad.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(loss, eager["loss"])
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, want[k]), k


def test_dense_step_allocates_no_dense_transient(cuda):
    """150 classes, B = 2 at 240 x 320: the torch route's [B, C, OH, OW] fp32 copy alone is 92 MB; the step may allocate its results
    (pred, the low-res log-probs), a copy of the labels and 1 MB."""
    cfg = ViTConfig(n_blocks=1, head="linear", n_classes=150)
    m, _ = build(cfg, "bf16")
    m.unfreeze_bb()
    B, H, W = 2, 240, 320
    frames = torch.from_numpy(synthetic_frames(B, H, seed=61, w=W)).cuda()
    y = pixel_labels(B, H, W, 150, seed=62).cuda()
    m.fused_training_step_dense((frames, y))                    # warm-up: weights packed, workspaces and gradient buffers allocated
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m.fused_training_step_dense((frames, y))
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    allowed = y.numel() * 8 + B * H * W * 4 + B * (H // 8) * (W // 8) * 150 * 4 + (1 << 20)
    print(f"dense step peak-memory delta {delta} bytes; allowed {allowed}; a [B, C, OH, OW] fp32 tensor would be {B * 150 * H * W * 4}")
    assert torch.isfinite(out["loss"]) and delta <= allowed
