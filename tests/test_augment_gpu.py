"""The device augmentation on the GPU (-m gpu): dinoseg_op_augment (csrc/augment.hip) as an operator against the stated rule
restated in int64 / fp64 numpy (tests/augment_util.py, itself checked against torch's grid_sample / pad + conv2d in
tests/test_augment_cpu.py), and through DINOSeg.augment / fit(augment=...).

Bars, from the rounding count.  On the 0..255 scale a value passes through 3 lerps (one fp32 rounding each), at most 6 roundings
of the colour step (gain / bias, three terms of the gray, the difference, the saturation fma) and one rounding per tap and pass of
the blur, 2 (2r + 1) in all; every one is at most half a unit in the last place of the largest magnitude in play,
M = max(256, 255 |gain| + |bias|), i.e. 2^-24 M.  With slack for the fp32 constants of the gray and the taps' own rounding:

    bar_255 = (16 + 2 (2r + 1)) 2^-24 max(256, 255 |gain| + |bias|)          per frame (tests/augment_util.py: value_bar)

The normalised fp32 output (v / 255 - mean) / std divides that by 255 std >= 255 * 0.224 and adds its own three roundings:
bar_255 / (255 * 0.224) + 4 * 2^-24 * max|ref|.  The uint8 output is rintf of the clamped value: within 0.5 + bar_255 of the fp64
value at EVERY pixel.  Pixel labels and patch labels are integers of an integer rule: exactly equal."""
import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import Augmenter, DINOSeg, ViTConfig, augment_table, capi, procedural_state_dict
from dino_amd.augment import unpack_table

from . import augment_util as U

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
G = 4096                                                         # guard words on both sides of each buffer
SENT = 0x7F7F7F7F                                                # (as fp32: a NaN pattern the kernels never produce)


class Guard:
    """`n` payload bytes (rounded up to whole words) between 4096 sentinel words on either side."""

    def __init__(self, nbytes):
        self.words = (nbytes + 3) // 4
        self.buf = torch.full((self.words + 2 * G,), SENT, dtype=torch.int32, device="cuda")
        self.nbytes = nbytes

    def ptr(self):
        return self.buf.data_ptr() + 4 * G

    def payload(self, dtype, shape):
        return self.buf[G:G + self.words].view(torch.uint8)[:self.nbytes].view(dtype).view(shape)

    def guards_untouched(self):
        tail = self.buf[G:G + self.words].view(torch.uint8)[self.nbytes:]
        return bool((self.buf[:G] == SENT).all()) and bool((self.buf[G + self.words:] == SENT).all()) and bool((tail == 0x7F).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def run_op(frames, masks, table, OH, OW, out_kind="f32", max_radius=None, pixel=True, patch=None, scratch="auto"):
    """dinoseg_op_augment on device tensors -> (image, pixel labels or None, patch labels or None)."""
    B, H, W = frames.shape[:3]
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and table.is_cuda and table.dtype == torch.int32
    if max_radius is None:
        max_radius = int(table[:, 14].max())
    img = (torch.full((B, OH, OW, 3), 77, dtype=torch.uint8, device="cuda") if out_kind == "u8" else
           torch.full((B, 3, OH, OW), float("nan"), dtype=torch.float32, device="cuda"))
    pix = torch.full((B, OH, OW), -7, dtype=torch.int64, device="cuda") if masks is not None and pixel else None
    pat = torch.full((B, (OH // patch) * (OW // patch)), -7, dtype=torch.int64, device="cuda") if masks is not None and patch else None
    if scratch == "auto":
        scratch = torch.full((B, 3, OH, OW), float("nan"), dtype=torch.float32, device="cuda") if max_radius > 0 else None
    kind = 0
    if masks is not None:
        assert masks.is_cuda and masks.is_contiguous() and masks.dtype in (torch.uint8, torch.int64)
        kind = 0 if masks.dtype == torch.uint8 else 1
    capi.check(capi.lib().dinoseg_op_augment(frames.data_ptr(), capi.ptr(masks), kind, B, H, W, table.data_ptr(), max_radius, OH, OW,
                                             capi.INPUT_U8_HWC if out_kind == "u8" else capi.INPUT_F32_CHW, img.data_ptr(), capi.ptr(pix),
                                             capi.ptr(pat), patch or 8, capi.ptr(scratch), S()))
    return img, pix, pat


def batch(B, H, W, seed=0):
    frames, masks = U.random_batch(B, H, W, seed=seed)
    return frames, masks, torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda()


def check_against_fp64(name, frames, masks, table, OH, OW, patch=None, max_radius=None):
    """Both output kinds and both mask kinds against the restatement, at the bars of the module docstring."""
    ref = U.restate(frames, masks, table, OH, OW, patch=patch, max_radius=20 if max_radius is None else max_radius)
    bar = U.value_bar(table, 20 if max_radius is None else max_radius)[:, None, None, None]
    dev_f, dev_t = torch.from_numpy(frames).cuda(), table.cuda()
    dev_m = torch.from_numpy(masks).cuda()
    f32, pix, pat = run_op(dev_f, dev_m, dev_t, OH, OW, "f32", max_radius, patch=patch)
    u8, pix64, pat64 = run_op(dev_f, dev_m.long(), dev_t, OH, OW, "u8", max_radius, patch=patch)
    torch.cuda.synchronize()
    err_n = np.abs(f32.cpu().numpy().astype(np.float64) - ref["norm"])
    bar_n = bar / (255.0 * 0.224) + 4.0 * 2.0 ** -24 * float(np.abs(ref["norm"]).max())
    err_u = np.abs(u8.cpu().numpy().astype(np.float64) - np.clip(ref["value"], 0.0, 255.0))
    print(f"augment {name}: max |f32 - fp64| / bar {float((err_n / bar_n).max()):.3f} (bars {float(bar_n.min()):.2e} .. "
          f"{float(bar_n.max()):.2e}); max |u8 - fp64| {float(err_u.max()):.6f} (0.5 + {float(bar.min()):.1e} .. {float(bar.max()):.1e})")
    assert bool(np.isfinite(f32.cpu().numpy()).all())
    assert (err_n <= bar_n).all()
    assert (err_u <= 0.5 + bar).all()
    for got in (pix, pix64):
        assert np.array_equal(got.cpu().numpy(), ref["labels"])
    if patch:
        for got in (pat, pat64):
            assert np.array_equal(got.cpu().numpy(), ref["patch_labels"])
    return ref, u8, pix


# ------------------------------------------------------------------------------------------------ 1. exact properties
@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int64], ids=["mask-u8", "mask-i64"])
def test_identity_flip_and_integer_crop_are_exact(cuda, mask_dtype):
    frames, masks, x, y = batch(2, 43, 75)
    y = y.to(mask_dtype)
    img, pix, _ = run_op(x, y, augment_table(2, (43, 75), (43, 75)).cuda(), 43, 75, "u8")
    assert torch.equal(img, x) and torch.equal(pix, y.long())
    img, pix, _ = run_op(x, y, augment_table(2, (43, 75), (43, 75), flip=True).cuda(), 43, 75, "u8")
    assert torch.equal(img, torch.flip(x, dims=(2,))) and torch.equal(pix, torch.flip(y.long(), dims=(2,)))
    # an integer crop per frame, to 40 x 72 (a multiple of the patch: the patch labels are every 8th pixel label)
    table = augment_table(2, (43, 75), (40, 72), crop=[(3, 2, 40, 72), (0, 3, 40, 72)]).cuda()
    img, pix, pat = run_op(x, y, table, 40, 72, "u8", patch=8)
    want = torch.stack([x[0, 3:43, 2:74], x[1, 0:40, 3:75]])
    want_y = torch.stack([y[0, 3:43, 2:74], y[1, 0:40, 3:75]]).long()
    assert torch.equal(img, want) and torch.equal(pix, want_y)
    assert torch.equal(pat, want_y[:, ::8, ::8].reshape(2, -1))
    # patch labels alone, and patch 16 on a 32 x 64 crop
    assert torch.equal(run_op(x, y, table, 40, 72, "u8", pixel=False, patch=8)[2], pat)
    table = augment_table(2, (43, 75), (32, 64), crop=(5, 7, 32, 64), flip=[False, True]).cuda()
    img, pix, pat = run_op(x, y, table, 32, 64, "u8", patch=16)
    assert torch.equal(img[0], x[0, 5:37, 7:71]) and torch.equal(img[1], torch.flip(x[1, 5:37, 7:71], dims=(1,)))
    assert torch.equal(pat, pix[:, ::16, ::16].reshape(2, -1)) and tuple(pat.shape) == (2, 8)
    # no masks: the image alone
    assert torch.equal(run_op(x, None, table, 32, 64, "u8")[0], img)


# ------------------------------------------------------------------------------------------------ 2. warp and colour against fp64
def test_warp_and_colour_against_fp64_3x43x75_to_40x72(cuda):
    frames, masks = U.random_batch(3, 43, 75)
    table = augment_table(3, (43, 75), (40, 72),
                          crop=[(0, 0, 43, 75), (2.5, 4.25, 38, 66.5), (-4000, -9000, 64 * 40, 64 * 72)],      # frame 2: 64x, outside
                          angle=[30, -20, 0], scale=[1.0, 0.7, 1.0], shift=[(0.3, -0.2), (-0.1, 0.25), (0, 0)], flip=[False, True, False],
                          border=["reflect", "constant", "constant"], void_label=[255, 255, 9], gain=[1.0, 1.5, 1.0], bias=[0, 40, 0],
                          sat=[1.7, 0.0, 1.0])
    Ux, Uy = U.source_coords(unpack_table(table)["a"][1], 40, 72)
    assert Ux.min() < -65536 and Ux.max() > 76 << 16 and Uy.min() < -65536 and Uy.max() > 44 << 16     # taps beyond every edge
    ref, u8, pix = check_against_fp64("3x43x75->40x72", frames, masks, table, 40, 72, patch=8)
    assert float(ref["value"][1].max()) == 255.0 and float(ref["value"][0].min()) == 0.0                # both clamps are reached
    # the 64x minification whose footprint lies outside the frame: all fill, all void
    assert bool((u8[2].cpu() == torch.tensor([124, 116, 104], dtype=torch.uint8)).all()) and bool((pix[2] == 9).all())
    assert bool((pix[1] == 255).any()) and bool((pix[1] != 255).any())


def test_warp_and_colour_against_fp64_2x70x100_to_96x136(cuda):
    """Upscaling with ragged tiles in both axes (96 = 3 x 32, 136 = 2 x 64 + 8)."""
    frames, masks = U.random_batch(2, 70, 100)
    table = augment_table(2, (70, 100), (96, 136), angle=[10, -12], scale=[1.2, 0.8], shift=[(0.2, -0.15), (0.35, -0.3)], flip=[True, False],
                          border=["reflect", "constant"], fill=(10, 250, 30), void_label=-100, gain=[0.4, 1.0], bias=[-60, 0],
                          sat=[1.0, 0.0])
    ref, u8, pix = check_against_fp64("2x70x100->96x136", frames, masks, table, 96, 136, patch=8)
    assert float(ref["value"][0].min()) == 0.0 and bool((pix[1] == -100).any())


def test_a_source_of_side_one(cuda):
    frames, masks = U.random_batch(2, 1, 9)
    table = augment_table(2, (1, 9), (8, 16), angle=[0, 25], border=["reflect", "constant"], gain=[1.2, 1.0])
    check_against_fp64("2x1x9->8x16", frames, masks, table, 8, 16, patch=8)
    frames, masks = U.random_batch(1, 1, 1)
    ref, u8, pix = check_against_fp64("1x1x1->8x8", frames, masks, augment_table(1, (1, 1), (8, 8), angle=45), 8, 8)
    assert bool((u8.cpu() == torch.from_numpy(frames).view(1, 1, 1, 3)).all()) and bool((pix.cpu() == int(masks[0, 0, 0])).all())


# ------------------------------------------------------------------------------------------------ 3. the blur against fp64
@pytest.mark.parametrize("src,out", [((43, 75), (40, 72)), ((70, 100), (70, 100))], ids=["43x75->40x72", "70x100->70x100"])
def test_blur_with_mixed_radii_against_fp64(cuda, src, out):
    frames, masks = U.random_batch(4, *src)
    table = augment_table(4, src, out, angle=[0, 12, -8, 3], flip=[False, True, False, True], gain=[1, 1.3, 0.8, 1], bias=[0, -20, 30, 0],
                          border=["reflect", "constant", "reflect", "reflect"], ksize=[0, 3, 15, 41])
    assert unpack_table(table)["radius"].tolist() == [0, 1, 7, 20]
    check_against_fp64(f"blur {src}->{out}", frames, masks, table, *out, patch=8 if out == (40, 72) else None)


def test_blur_at_the_smallest_legal_output(cuda):
    """21 x 24 with r = 20: the halo folds across the whole frame."""
    frames, masks = U.random_batch(2, 21, 24)
    table = augment_table(2, (21, 24), (21, 24), ksize=[41, 7], flip=[True, False])
    check_against_fp64("blur 21x24 r=20", frames, masks, table, 21, 24)


@pytest.mark.parametrize("out_kind", ["f32", "u8"])
def test_zero_radii_under_a_blur_launch_equal_the_one_launch_result(cuda, out_kind):
    frames, masks, x, y = batch(3, 43, 75)
    table = augment_table(3, (43, 75), (40, 72), angle=[5, -30, 0], scale=[1, 0.6, 1.1], border=["reflect", "constant", "reflect"],
                          gain=[1, 1.4, 0.7], bias=[0, 25, -10], sat=[1, 0.3, 1.6]).cuda()
    one = run_op(x, y, table, 40, 72, out_kind, 0, patch=8)
    two = run_op(x, y, table, 40, 72, out_kind, 20, patch=8)
    assert torch.equal(one[0].view(torch.uint8), two[0].view(torch.uint8))                  # bit for bit, NaNs included
    assert torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
    # a radius above max_radius is clamped to it on the device: max_radius = 0 turns the blur off
    blurred = augment_table(3, (43, 75), (40, 72), angle=[5, -30, 0], scale=[1, 0.6, 1.1], border=["reflect", "constant", "reflect"],
                            gain=[1, 1.4, 0.7], bias=[0, 25, -10], sat=[1, 0.3, 1.6], ksize=[9, 0, 41]).cuda()
    clamped = run_op(x, y, blurred, 40, 72, out_kind, 0, patch=8)
    assert torch.equal(clamped[0].view(torch.uint8), one[0].view(torch.uint8))


# ------------------------------------------------------------------------------------------------ 5. containment, repeatability
@pytest.mark.parametrize("out_kind", ["f32", "u8"])
def test_nothing_is_written_outside_the_outputs(cuda, out_kind):
    B, H, W, OH, OW, p = 3, 43, 75, 40, 72, 8
    frames, masks, x, y = batch(B, H, W)
    table = augment_table(B, (H, W), (OH, OW), angle=[7, -15, 0], flip=[False, True, False], border=["reflect", "constant", "reflect"],
                          gain=[1, 1.2, 0.9], ksize=[0, 41, 5]).cuda()
    x0, y0, t0 = x.clone(), y.clone(), table.clone()
    want = run_op(x, y, table, OH, OW, out_kind, patch=p)
    again = run_op(x, y, table, OH, OW, out_kind, patch=p)
    bits = (lambda t: t.view(torch.uint8)) if out_kind == "u8" else (lambda t: t.view(torch.int32))
    assert torch.equal(bits(want[0]), bits(again[0])) and torch.equal(want[1], again[1]) and torch.equal(want[2], again[2])
    npix = B * OH * OW
    img_bytes = npix * 3 * (1 if out_kind == "u8" else 4)
    g = {"img": Guard(img_bytes), "pix": Guard(8 * npix), "pat": Guard(8 * B * (OH // p) * (OW // p)), "scratch": Guard(4 * 3 * npix)}
    kind = capi.INPUT_U8_HWC if out_kind == "u8" else capi.INPUT_F32_CHW
    img_shape = (B, OH, OW, 3) if out_kind == "u8" else (B, 3, OH, OW)
    img_dtype = torch.uint8 if out_kind == "u8" else torch.float32
    op = capi.lib().dinoseg_op_augment

    def refill():
        for v in g.values():
            v.buf.fill_(SENT)
    # everything at once, two launches
    capi.check(op(x.data_ptr(), y.data_ptr(), 0, B, H, W, table.data_ptr(), 20, OH, OW, kind, g["img"].ptr(), g["pix"].ptr(), g["pat"].ptr(),
                  p, g["scratch"].ptr(), S()))
    torch.cuda.synchronize()
    assert all(v.guards_untouched() for v in g.values()), [k for k, v in g.items() if not v.guards_untouched()]
    assert torch.equal(bits(g["img"].payload(img_dtype, img_shape)), bits(want[0]))
    assert torch.equal(g["pix"].payload(torch.int64, (B, OH, OW)), want[1])
    assert torch.equal(g["pat"].payload(torch.int64, (B, -1)), want[2])
    # the image alone (no masks): no label word is written
    refill()
    capi.check(op(x.data_ptr(), None, 0, B, H, W, table.data_ptr(), 20, OH, OW, kind, g["img"].ptr(), None, None, p, g["scratch"].ptr(), S()))
    torch.cuda.synchronize()
    assert g["pix"].untouched() and g["pat"].untouched() and g["img"].guards_untouched() and g["scratch"].guards_untouched()
    assert torch.equal(bits(g["img"].payload(img_dtype, img_shape)), bits(want[0]))
    # one launch (max_radius = 0) with masks and patch labels alone: the scratch and the pixel labels are never written
    refill()
    capi.check(op(x.data_ptr(), y.data_ptr(), 0, B, H, W, table.data_ptr(), 0, OH, OW, kind, g["img"].ptr(), None, g["pat"].ptr(), p,
                  g["scratch"].ptr(), S()))
    torch.cuda.synchronize()
    assert g["scratch"].untouched() and g["pix"].untouched() and g["img"].guards_untouched() and g["pat"].guards_untouched()
    assert torch.equal(g["pat"].payload(torch.int64, (B, -1)), want[2])
    assert torch.equal(x, x0) and torch.equal(y, y0) and torch.equal(table, t0)


# ------------------------------------------------------------------------------------------------ 6. model level
def build(cfg, precision="bf16x3", **kw):
    m = DINOSeg(arch=cfg, head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)
    return m.to("cuda:0")


SMALL = dict(embed_dim=128, num_heads=2, n_blocks=1, n_classes=7, head="mlp")


def test_model_augment_equals_the_op_and_feeds_the_dense_step(cuda):
    m = build(ViTConfig(**SMALL), lr=1e-3, optimizer=torch.optim.Adam, freeze_backbone=False)
    frames, masks, x, y = batch(2, 70, 100)
    table = augment_table(2, (70, 100), (64, 96), angle=[10, -5], scale=[1.1, 0.8], flip=[True, False], border=["reflect", "constant"],
                          gain=[1.3, 0.8], ksize=[0, 9])
    for out_kind in ("f32", "u8"):
        for labels in ("pixel", "patch"):
            img, lab = m.augment(torch.from_numpy(frames), torch.from_numpy(masks), table, out=(64, 96), out_kind=out_kind, labels=labels)
            want = run_op(x, y, table.cuda(), 64, 96, out_kind, patch=8)
            assert torch.equal(img.view(torch.uint8), want[0].view(torch.uint8))
            assert lab.dtype == torch.int64 and torch.equal(lab, want[1] if labels == "pixel" else want[2])
    img, lab = m.augment(x, None, table, out=(64, 96))
    assert lab is None and torch.equal(img.view(torch.int32), run_op(x, None, table.cuda(), 64, 96, "f32")[0].view(torch.int32))
    same, lab = m.augment(x, y.to(torch.int32), augment_table(2, (70, 100), (70, 100)), out_kind="u8")      # out=None: the frames' size
    assert torch.equal(same, x) and torch.equal(lab, y.long())
    # the normalised output and the pixel labels are what the dense step takes
    img, lab = m.augment(x, y, table, out=(64, 96))
    assert bool((lab == 255).any())
    out = m.fused_training_step_dense((img, lab))
    m.check_labels()
    assert bool(torch.isfinite(out["loss"])) and float(out["loss"]) > 0
    img, lab = m.augment(x, y, table, out=(64, 96), labels="patch")
    out = m.fused_training_step((img, torch.where(lab == 255, torch.full_like(lab, -100), lab)))
    m.check_labels()
    assert bool(torch.isfinite(out["loss"]))


class Counting(Augmenter):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def __call__(self, model, x, y):
        self.calls.append(tuple(x.shape))
        return super().__call__(model, x, y)


def test_fit_with_an_augmenter(cuda, tmp_path):
    m = build(ViTConfig(**SMALL), lr=1e-3, optimizer=torch.optim.Adam, freeze_backbone=False, max_epochs=1, write_path=str(tmp_path))
    frames, masks = U.random_batch(4, 70, 100)
    vf, vm = U.random_batch(2, 64, 96)
    train = [(torch.from_numpy(frames[0:2]), torch.from_numpy(masks[0:2])), (torch.from_numpy(frames[2:4]), torch.from_numpy(masks[2:4]))]
    val = [(torch.from_numpy(vf), torch.from_numpy(vm).long())]
    aug = Counting(out=(64, 96), seed=3, labels="pixel")
    out = m.fit(train_dataloader=train, val_dataloader=val, test_dataloader=val, max_epochs=1, augment=aug)
    h = out["history"]
    assert len(h) == 1 and all(np.isfinite(h[0][k]) for k in ("train_loss", "train_acc", "val_acc")) and np.isfinite(out["test"]["test_acc"])
    assert aug.calls == [(2, 70, 100, 3)] * 2                       # once per train batch, never for validation or test
    # patch labels through the patch step
    aug = Counting(out=(64, 96), seed=3, labels="patch")
    out = m.fit(train_dataloader=train, val_dataloader=[(torch.from_numpy(vf), torch.zeros(2, 96, dtype=torch.long))], max_epochs=1, augment=aug)
    assert len(aug.calls) == 2 and np.isfinite(out["history"][0]["train_loss"])


def test_fit_without_an_augmenter_equals_a_pass_through_hook(cuda, tmp_path):
    """The hook adds nothing else: the same model, data and (deterministic) steps give the same history with augment=None and with a
    hook that returns its inputs."""
    vf, vm = U.random_batch(6, 64, 96)
    data = [(torch.from_numpy(vf[i:i + 2]), torch.from_numpy(vm[i:i + 2]).long()) for i in (0, 2, 4)]
    hist = []
    with dino_amd.options(deterministic=1):
        for hook in (None, lambda model, x, y: (x, y)):
            m = build(ViTConfig(**SMALL), lr=1e-3, optimizer=torch.optim.Adam, freeze_backbone=False, max_epochs=2, write_path=str(tmp_path))
            hist.append(m.fit(train_dataloader=data[:2], val_dataloader=data[2:], augment=hook)["history"])
    assert len(hist[0]) == 2 and len(hist[1]) == 2
    for a, b in zip(*hist):
        assert a.keys() == b.keys() and np.isfinite(a["train_loss"])
        assert all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a), (a, b)
