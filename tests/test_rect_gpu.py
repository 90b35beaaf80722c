"""Non-square frames on the GPU (-m gpu): H x W inputs through forward, model.dino(x), get_last_selfattention, forward_mask and the
fine-tune step, against the g15 fixtures captured from the reference's VisionTransformer (tools/gen_golden_rect.py; the reference
reads `B, nc, w, h = x.shape` and resamples the position grid with one scale per axis, vision_transformer.py:202-233).  Square
frames through the `_hw` entries are the `r` entries bit for bit."""
import os

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames, synthetic_labels
from oracle import dinoseg_oracle as O
from tests.gpu_util import seeded, unpack

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
TOL = 1e-3                              # the parity modes' bar on the square fixtures (test_model_gpu.py)
L3_TAGS = ["240x320", "480x640", "64x128"]


def build(cfg, precision, **kw):
    if isinstance(cfg, int):
        cfg = ViTConfig(n_blocks=cfg)
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0"), sd


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def fixture(golden_dir, L, tag):
    """(B, H, W, seed, logp, argmax, margin) of a g15 forward fixture."""
    if L == 12:
        g = load(golden_dir, "g15_rect_vits8_L12_480x640")
        key = lambda k: k
    else:
        g = load(golden_dir, "g15_rect_vits8_L3")
        key = lambda k: f"{tag}|{k}"
    B, H, W = (int(v) for v in g[key("shape")])
    return B, H, W, int(g[key("seed")]), torch.from_numpy(g[key("logp")]), g[key("argmax")].astype(np.int64), g[key("margin")]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("precision", ["bf16x3", "fp16x3", "fp16", "bf16"])
@pytest.mark.parametrize("L,tag", [(3, t) for t in L3_TAGS] + [(12, "480x640")])
def test_g15_forward(cuda, golden_dir, precision, L, tag):
    """Every g15 shape in every precision with the bars the square fixtures use: the parity modes 1e-3 and no flip; fp16
    FP16_BOUND (test_fp16_gpu.py), and for the one-frame 64x128 (129 tokens) smoke()'s small-frame fp16 bar of 0.1 (4.4e-2
    measured at 64x64; 4.36e-2 here); bf16 0.2 and 1 % flips (test_model_gpu.py); a flip only where the reference's top-2
    margin sits inside twice the error."""
    B, H, W, seed, ref, ref_am, margin = fixture(golden_dir, L, tag)
    m, _ = build(L, precision)
    lp, am = m.forward_frames(torch.from_numpy(synthetic_frames(B, H, seed=seed, w=W)).cuda())
    torch.cuda.synchronize()
    assert lp.shape == ref.shape and am.shape == (B * (H // 8) * (W // 8),)
    assert torch.isfinite(lp).all()
    err = float((lp.cpu() - ref).abs().max())
    flips = am.cpu().numpy().astype(np.int64) != ref_am
    print(f"{precision} L={L} {B}x{tag}: max|dlogp| {err:.3e}, {int(flips.sum())} flips of {flips.size}")
    if precision in ("bf16x3", "fp16x3"):
        assert err <= TOL and not flips.any()
        return
    tol, flip_frac = ((0.1 if tag == "64x128" else 4.0e-2), 12 / 3600) if precision == "fp16" else (0.2, 0.01)
    assert err <= tol and flips.mean() <= flip_frac
    assert np.all(margin[flips] <= 2 * err)


@pytest.mark.parametrize("tag", ["240x320", "64x128"])
def test_uint8_and_fp32_inputs_agree(cuda, golden_dir, tag):
    B, H, W, seed, ref, _, _ = fixture(golden_dir, 3, tag)
    m, _ = build(3, "bf16x3")
    frames = synthetic_frames(B, H, seed=seed, w=W)
    lp8, am8 = m.forward_frames(torch.from_numpy(frames).cuda())
    x = O.preprocess(frames).cuda()
    assert x.shape == (B, 3, H, W)
    with torch.no_grad():
        lp = m(x)
    assert float((lp - lp8).abs().max()) <= 1e-5          # (Normalize fused into the gather vs done by torch: same formula)
    assert torch.equal(am8.long(), lp.argmax(1))
    lpg = m(x)                                             # with autograd: the training forward (its own routes), same bar
    assert lpg.grad_fn is not None
    for out in (lp, lpg):
        assert float((out.detach().cpu() - ref).abs().max()) <= TOL


@pytest.mark.parametrize("precision", ["fp16x3", "bf16"])
@pytest.mark.parametrize("r", [480, 224])
def test_hw_entry_with_a_square_is_the_r_entry(cuda, precision, r):
    """dinoseg_forward_hw(H = W = r) and dinoseg_forward(r) on one handle: bit-identical log-probabilities and argmax, for one frame
    and for 8 (the split two-stream forward), each entry called before and after the other."""
    m, _ = build(3, precision)
    m._sync_weights()
    lib = capi.lib()
    for B in (1, 8):
        x = torch.from_numpy(synthetic_frames(B, r, seed=B)).cuda()
        outs = []
        for hw in (False, True, False):
            n = B * (r // 8) ** 2
            lp = torch.empty((n, 7), device="cuda")
            am = torch.empty((n,), dtype=torch.int32, device="cuda")
            if hw:
                rc = lib.dinoseg_forward_hw(m._handle, x.data_ptr(), capi.INPUT_U8_HWC, B, r, r, lp.data_ptr(), am.data_ptr(), -1,
                                            None, S())
            else:
                rc = lib.dinoseg_forward(m._handle, x.data_ptr(), capi.INPUT_U8_HWC, B, r, lp.data_ptr(), am.data_ptr(), -1, None, S())
            capi.check(rc)
            outs.append((lp, am))
        torch.cuda.synchronize()
        for lp, am in outs[1:]:
            assert torch.equal(lp, outs[0][0]) and torch.equal(am, outs[0][1])


@pytest.mark.parametrize("precision", ["bf16", "fp16x3"])
def test_two_stream_split_at_240x320_equals_one_stream(cuda, precision):
    m, _ = build(3, precision)
    frames = torch.from_numpy(synthetic_frames(32, 240, seed=9, w=320)).cuda()
    lp2, am2 = m.forward_frames(frames)                    # the default: two half-batches on two streams
    with dino_amd.options(streams=1):
        lp1, am1 = m.forward_frames(frames)
    torch.cuda.synchronize()
    assert torch.equal(lp1, lp2) and torch.equal(am1, am2)
    lp0, _ = m.forward_frames(frames[17:18])               # a frame of the second half: its own rows of the batched output
    assert float((lp0 - lp2[17 * 1200:18 * 1200]).abs().max()) <= (TOL if precision == "fp16x3" else 0.15)


# ------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("oh,ow", [(1, 60), (16, 49), (28, 29), (30, 40), (60, 80), (28, 28), (60, 60)])
def test_pos_resample_hw(cuda, oh, ow):
    """8x480, 128x392 (784 patches: not the identity), 224x232 (28 rows: resampled at 28 / 28.1), 240x320, 480x640; squares."""
    g, D = 28, 64
    pe = seeded((1, g * g + 1, D), 11)
    out = torch.full((oh * ow + 1, D), float("nan"), device="cuda")
    capi.check(capi.lib().dinoseg_op_pos_resample_hw(pe.data_ptr(), g, D, oh, ow, out.data_ptr(), S()))
    torch.cuda.synchronize()
    pc = pe.cpu()
    if (oh, ow) == (g, g):
        assert torch.equal(out.cpu(), pc[0])
        return
    want = torch.nn.functional.interpolate(pc[:, 1:].reshape(1, g, g, D).permute(0, 3, 1, 2),
                                           scale_factor=((oh + 0.1) / g, (ow + 0.1) / g), mode="bicubic")
    want = torch.cat([pc[0, :1], want.permute(0, 2, 3, 1).reshape(oh * ow, D)])
    assert float((out.cpu() - want).abs().max()) <= 1e-5
    if oh == ow:
        sq = torch.zeros_like(out)
        capi.check(capi.lib().dinoseg_op_pos_resample(pe.data_ptr(), g, D, oh, sq.data_ptr(), S()))
        torch.cuda.synchronize()
        assert torch.equal(sq, out)


@pytest.mark.parametrize("H,W", [(8, 480), (128, 392), (224, 232), (240, 320), (64, 64)])
def test_patch_gather_hw(cuda, H, W):
    B = 2
    frames = np.random.default_rng(H + W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    x = O.preprocess(frames)
    hp, wp = H // 8, W // 8
    n = B * hp * wp
    want = x.reshape(B, 3, hp, 8, wp, 8).permute(0, 2, 4, 1, 3, 5).reshape(n, 192)
    lib = capi.lib()
    fr = torch.from_numpy(frames).cuda()
    out = torch.zeros((2, n, 192), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_patch_gather_hw(fr.data_ptr(), capi.INPUT_U8_HWC, B, H, W, out.data_ptr(), n * 192, 2, S()))
    xc = x.cuda().contiguous()
    out1 = torch.zeros((1, n, 192), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_patch_gather_hw(xc.data_ptr(), capi.INPUT_F32_CHW, B, H, W, out1.data_ptr(), n * 192, 1, S()))
    torch.cuda.synchronize()
    assert float((unpack(out).cpu() - want).abs().max()) <= 2.0 ** -15 * 3
    assert torch.equal(out1.view(torch.bfloat16)[0].cpu(), want.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ backbone outputs
def test_g15_features_attention_and_masks(cuda, golden_dir):
    g = load(golden_dir, "g15_rect_backbone_64x128")
    _, H, W = (int(v) for v in g["shape"])
    m, _ = build(3, "bf16x3")
    x = O.preprocess(synthetic_frames(1, H, seed=int(g["seed"]), w=W)).cuda()
    tok = m.dino(x).cpu()
    assert tok.shape == (1, 129, 384)
    assert float((tok - torch.from_numpy(g["tokens"])).abs().max()) <= 3e-4
    assert torch.equal(m.features(x).cpu(), tok)
    assert torch.equal(m.dino(x, all=False).cpu(), tok[:, 0])
    a = m.dino.get_last_selfattention(x).cpu()
    assert a.shape == (1, 6, 129, 129)
    assert float((a.sum(-1) - 1).abs().max()) <= 1e-5
    assert float((a[0, :, 0] - torch.from_numpy(g["attn_cls_rows"])).abs().max()) <= 2e-4
    assert float((a[0, :, 77] - torch.from_numpy(g["attn_row77"])).abs().max()) <= 2e-4
    masks = torch.from_numpy(g["masks"])
    emb = m.dino.forward_mask(x, masks).cpu()
    att = m.dino.get_last_selfattention(x, cls_mask=masks).cpu()
    assert emb.shape == (3, 384) and att.shape == (1, 6, 3, 129)
    assert float((emb - torch.from_numpy(g["mask_emb"])).abs().max()) <= TOL
    assert float((att - torch.from_numpy(g["mask_attn"])).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        m.forward_mask(x, torch.ones((2, 8, 15)))
    dbg = m.debug_tokens(x, 0)
    assert dbg.shape == (1, 129, 384) and torch.isfinite(dbg).all()


def test_predict_graph_survives_an_interleaved_rectangle(cuda, golden_dir):
    """predict() replays a captured graph that bakes in the cached position rows; a rectangular forward in between re-fills the
    cache for another grid (a new state generation), so the next predict() re-captures and returns the same map."""
    g = load(golden_dir, "g5_predict_L3")
    m, _ = build(3, "bf16x3")
    frame = g["frame_r480"]
    m.set_resolution(480)
    m.predict_graph = False
    eager = m.predict(frame)
    m.predict_graph = True
    a = m.predict(frame)
    assert 480 in m._pred_graphs
    gen = capi.lib().dinoseg_state_generation(m._handle)
    m.forward_frames(torch.from_numpy(synthetic_frames(1, 480, seed=3, w=640)).cuda())
    assert capi.lib().dinoseg_state_generation(m._handle) != gen
    b = m.predict(frame)
    m.forward_frames(torch.from_numpy(synthetic_frames(2, 240, seed=4, w=320)).cuda())
    c = m.predict(frame)
    assert np.array_equal(a, eager) and np.array_equal(b, eager) and np.array_equal(c, eager)


# ------------------------------------------------------------------------------------------------ fine-tune
def _step(m, g):
    B, H, W = (int(v) for v in g["shape"])
    frames = torch.from_numpy(synthetic_frames(B, H, seed=int(g["seed"]), w=W)).cuda()
    labels = torch.from_numpy(synthetic_labels(B, (H // 8) * (W // 8), 7, seed=int(g["label_seed"]))).cuda()
    return m.fused_training_step((frames, labels), 0), frames, labels


def test_g15_finetune_step_bf16x3(cuda, golden_dir):
    """The G12 bars (test_train_gpu.py): loss within 2e-4, every one of the 48 gradients within 2e-3 of its norm -- pos_embed through
    the transpose of the 28 -> 30 x 40 resample."""
    g = load(golden_dir, "g15_rect_finetune_240x320")
    m, _ = build(3, "bf16x3")
    m.unfreeze_bb()
    out, _, _ = _step(m, g)
    assert abs(float(out["loss"]) - float(g["loss"])) <= 2e-4
    n = 0
    for k, p in m.named_parameters():
        gn = float(g[f"gnorm|{k}"])
        gv = p.grad.detach().cpu().reshape(-1)
        assert torch.isfinite(gv).all(), k
        assert abs(float(gv.norm()) - gn) <= 2e-3 * gn + 1e-7, (k, float(gv.norm()), gn)
        idx = torch.from_numpy(g[f"gidx|{k}"])
        assert float((gv[idx] - torch.from_numpy(g[f"gval|{k}"])).abs().max()) <= 2e-3 * gn + 1e-7, k
        n += 1
    assert n == 48


def test_g15_finetune_step_bf16(cuda, golden_dir):
    """The one-plane mode with the G12 bf16 bars (test_train_gpu.py BF16_STEP_BOUNDS['vits8_L3_r480_B1'])."""
    g = load(golden_dir, "g15_rect_finetune_240x320")
    m, _ = build(3, "bf16")
    m.unfreeze_bb()
    out, _, _ = _step(m, g)
    dloss = abs(float(out["loss"]) - float(g["loss"]))
    worst_norm, worst_rel = 0.0, 0.0
    for k, p in m.named_parameters():
        gv = p.grad.detach().cpu().reshape(-1)
        assert torch.isfinite(gv).all(), k
        gn = float(g[f"gnorm|{k}"])
        ref = torch.from_numpy(g[f"gval|{k}"])
        worst_norm = max(worst_norm, abs(float(gv.norm()) / gn - 1.0))
        worst_rel = max(worst_rel, float((gv[torch.from_numpy(g[f"gidx|{k}"])] - ref).pow(2).mean().sqrt()) / (gn / gv.numel() ** 0.5))
    print(f"bf16 step 240x320: |dloss| {dloss:.3e}, worst norm ratio error {worst_norm:.3e}, worst sampled relative error {worst_rel:.3e}")
    assert dloss <= 1.8e-3 and worst_norm <= 1.0e-2 and worst_rel <= 7.3e-2


def test_autograd_step_equals_fused_step_at_240x320(cuda, golden_dir):
    g = load(golden_dir, "g15_rect_finetune_240x320")
    m, _ = build(3, "bf16x3")
    m.unfreeze_bb()
    fused, frames, labels = _step(m, g)
    x = O.preprocess(frames.cpu().numpy()).cuda()
    fused_f32 = m.fused_training_step((x, labels), 0)
    assert abs(float(fused_f32["loss"]) - float(fused["loss"])) <= 1e-6
    want = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    probs = m(x)
    assert probs.shape == (1200, 7) and probs.grad_fn is not None
    loss = torch.nn.functional.nll_loss(probs, labels.reshape(-1))
    loss.backward()
    assert abs(float(loss) - float(fused_f32["loss"])) <= 1e-6
    exact = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        scale = float(want[k].abs().max()) + 1e-12
        assert float((p.grad - want[k]).abs().max()) <= 2e-5 * scale, k
        exact += int(torch.equal(p.grad, want[k]))
    assert exact >= len(want) // 3
    out = m.training_step((x, labels), 0)
    assert out["probs"].shape == (1200, 7)


def test_validation_step_at_240x320(cuda):
    m, _ = build(3, "bf16x3")
    frames = torch.from_numpy(synthetic_frames(2, 240, seed=21, w=320)).cuda()
    labels = torch.from_numpy(np.random.default_rng(22).integers(0, 7, (2, 1200))).cuda()
    o = m.validation_step((frames, labels), 0)
    pred = o["pred"].cpu().numpy().astype(np.int64)
    gt = labels.cpu().numpy().reshape(-1)
    want = np.zeros((7, 7), dtype=np.float64)
    np.add.at(want, (gt, pred), 1.0)
    assert np.array_equal(o["confusion"].cpu().numpy().astype(np.float64), want) and want.sum() == 2400
    lp, am = m.forward_frames(frames)
    assert torch.equal(o["pred"], am) and torch.equal(o["probs"], lp)


def test_finetune_step_on_a_strip_one_patch_high(cuda):
    """8 x 480 (1 x 60 patches, 61 tokens): fewer token rows than the pos-embed gradient's row pass needs as scratch
    ([28][60][384] floats) -- the workspace is sized for it.  Loss and gradients against the CPU restatement's autograd."""
    from tests.test_rect_cpu import logp_hw
    cfg = ViTConfig(n_blocks=3)
    m, sd = build(cfg, "bf16x3")
    m.unfreeze_bb()
    frames = synthetic_frames(1, 8, seed=31, w=480)
    labels = torch.from_numpy(synthetic_labels(1, 60, 7, seed=32))
    out = m.fused_training_step((torch.from_numpy(frames).cuda(), labels.cuda()), 0)
    Wt = O.to_torch(sd, requires_grad=True)
    loss = O.nll_loss(logp_hw(O.preprocess(frames), Wt, 3), labels.reshape(-1))
    loss.backward()
    assert abs(float(out["loss"]) - float(loss.detach())) <= 2e-4
    for k, p in m.named_parameters():
        ref = Wt[k].grad.reshape(-1)
        gv = p.grad.detach().cpu().reshape(-1)
        assert float((gv - ref).abs().max()) <= 2e-3 * float(ref.norm()) + 1e-7, k
