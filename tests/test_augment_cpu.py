"""CPU tests of the device augmentation: the stated rule of dinoseg_op_augment (include/dinoseg.h) restated in int64 / fp64 numpy
(tests/augment_util.py) against torch's own grid_sample / pad + conv2d in fp64, the host functions that fill the parameter table
(dino_amd/augment.py), the host-side refusals of the op, and the class methods without a device.

On the translation words: the table's a2 / a5 CONTAIN the output half-pixel term (a0 + a1) / 2 resp. (a3 + a4) / 2 (the contract
of include/dinoseg.h), so the exact cases below compare a2 - (a0 + a1) / 2 with the plain translation: 0 for the identity (the words
themselves are 32768), W << 16 for a mirrored frame."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_amd
from dino_amd import Augmenter, DINOSeg, augment_table, capi, draw_reference_augment
from dino_amd.augment import draw_reference_parameters, gaussian_taps, unpack_table

from . import augment_util as U


def plain_translation(a):
    """(tx, ty) of a table row without the half-pixel term, in Q16."""
    assert (a[0] + a[1]) % 2 == 0 and (a[3] + a[4]) % 2 == 0
    return a[2] - (a[0] + a[1]) // 2, a[5] - (a[3] + a[4]) // 2


# ------------------------------------------------------------------------------------------------ the restatement against torch
WARP_TABLES = [
    dict(angle=30.0, scale=0.8, shift=(0.2, -0.1)),
    dict(angle=-17.0, scale=1.3, flip=True),
    dict(crop=(3.5, 10.25, 30.0, 50.5), angle=5.0),
    dict(crop=(-4000.0, -9000.0, 64 * 40.0, 64 * 72.0)),           # 64x minification, the footprint wholly outside the frame
]


@pytest.mark.parametrize("kw", WARP_TABLES, ids=["rot30", "rot-17-flip", "crop-rot5", "outside"])
def test_restated_warp_is_grid_sample(kw):
    frames, masks = U.random_batch(1, 43, 75)
    table = augment_table(1, (43, 75), (40, 72), border="constant", fill=(0, 0, 0), void_label=0, **kw)
    a = unpack_table(table)["a"][0]
    got = U.warp_frame(frames[0], a, 1, (0.0, 0.0, 0.0), 40, 72)
    want = U.torch_warp_zeros(frames[0], a, 40, 72)
    assert float(np.abs(got - want).max()) <= 1e-9
    # labels: equal to grid_sample(nearest) away from pixel edges (the rule floors, torch rounds half to even)
    lab = U.warp_mask(masks[0] + 1, a, 1, 0, 40, 72)
    want_lab, off_edge = U.torch_nearest_zeros(masks[0] + 1, a, 40, 72)
    assert np.array_equal(lab[off_edge], want_lab[off_edge])
    if "crop" in kw and kw["crop"][0] < -1000:
        assert float(np.abs(got).max()) == 0.0 and not lab.any() and not want_lab.any()       # all fill, all void
    else:
        assert off_edge.mean() > 0.9 and lab.any()


def test_restated_reflect101_is_reflect_pad_plus_grid_sample():
    frames, _ = U.random_batch(1, 43, 75)
    table = augment_table(1, (43, 75), (40, 72), angle=20.0, shift=(0.25, 0.2), scale=0.9)
    a = unpack_table(table)["a"][0]
    Ux, Uy = U.source_coords(a, 40, 72)
    pad = 40                                                    # every tap within 40 pixels of the frame (< the smaller side)
    assert Ux.min() >= -(pad - 2) << 16 and Ux.max() <= (75 + pad - 2) << 16 and Uy.min() >= -(pad - 2) << 16 and Uy.max() <= (43 + pad - 2) << 16
    assert Ux.min() < 0 or Uy.min() < 0 or Ux.max() > 75 << 16 or Uy.max() > 43 << 16      # and some do leave it
    got = U.warp_frame(frames[0], a, 0, (0.0, 0.0, 0.0), 40, 72)
    assert float(np.abs(got - U.torch_warp_reflect101(frames[0], a, 40, 72, pad)).max()) <= 1e-9


@pytest.mark.parametrize("shape,ksize", [((43, 75), 3), ((43, 75), 15), ((43, 75), 41), ((21, 24), 41)],
                         ids=["43x75-k3", "43x75-k15", "43x75-k41", "21x24-k41"])
def test_restated_blur_is_reflect_pad_plus_conv2d(shape, ksize):
    frames, _ = U.random_batch(1, *shape)
    w = gaussian_taps(ksize).astype(np.float32)
    r = (ksize - 1) // 2
    v = frames[0].astype(np.float64)
    assert float(np.abs(U.blur(v, r, w) - U.torch_blur(v, r, w)).max()) <= 1e-9


def test_restated_2x_resize_is_interpolate():
    """A 2x reduction samples no pixel outside the frame: F.interpolate(align_corners=False) everywhere.  A 2x enlargement equals it
    away from the outermost output pixels (there interpolate clamps the coordinate, the rule folds by reflect-101)."""
    frames, _ = U.random_batch(1, 12, 20, seed=3)
    src = torch.from_numpy(frames[0].astype(np.float64)).permute(2, 0, 1)[None]
    down = unpack_table(augment_table(1, (12, 20), (6, 10)))["a"][0]
    assert down.tolist() == [131072, 0, 65536, 0, 131072, 65536]
    want = F.interpolate(src, size=(6, 10), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert float(np.abs(U.warp_frame(frames[0], down, 0, (0, 0, 0), 6, 10) - want).max()) <= 1e-9
    up = unpack_table(augment_table(1, (12, 20), (24, 40)))["a"][0]
    assert up.tolist() == [32768, 0, 16384, 0, 32768, 16384]
    want = F.interpolate(src, size=(24, 40), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    got = U.warp_frame(frames[0], up, 0, (0, 0, 0), 24, 40)
    assert float(np.abs(got - want)[1:-1, 1:-1].max()) <= 1e-9


# ------------------------------------------------------------------------------------------------ augment_table
def test_augment_table_exact_cases():
    t = augment_table(2, (43, 75), (43, 75))
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 36) and t.device.type == "cpu"
    f = unpack_table(t)
    for b in range(2):
        a = f["a"][b].tolist()
        assert [a[0], a[1], a[3], a[4]] == [65536, 0, 0, 65536] and plain_translation(a) == (0, 0) and a[2] == a[5] == 32768
    assert f["border"].tolist() == [0, 0] and f["void_label"].tolist() == [255, 255] and f["radius"].tolist() == [0, 0]
    assert f["fill"][0].tolist() == [124.0, 116.0, 104.0] and f["gain"][0] == 1.0 and f["bias"][0] == 0.0 and f["sat"][0] == 1.0
    assert not f["w"].any()
    # an integer crop at the output's size: a pure translation
    a = unpack_table(augment_table(1, (43, 75), (20, 32), crop=(5, 7, 20, 32)))["a"][0].tolist()
    assert [a[0], a[1], a[3], a[4]] == [65536, 0, 0, 65536] and plain_translation(a) == (7 << 16, 5 << 16)
    # the mirror: a0 = -65536 and a translation of W
    a = unpack_table(augment_table(1, (43, 75), (43, 75), flip=True))["a"][0].tolist()
    assert [a[0], a[1], a[3], a[4]] == [-65536, 0, 0, 65536] and plain_translation(a) == (75 << 16, 0)
    # per-frame sequences; a quarter turn about the centre of a square maps the frame onto itself
    t = augment_table(3, (40, 40), (40, 40), angle=[0, 90, 180], flip=[False, True, False], border=["reflect", "constant", "reflect"],
                      gain=[1, 1.5, 0.5], bias=7, ksize=[0, 3, 41], void_label=[255, -100, 3])
    f = unpack_table(t)
    assert f["border"].tolist() == [0, 1, 0] and f["void_label"].tolist() == [255, -100, 3] and f["radius"].tolist() == [0, 1, 20]
    assert f["gain"].tolist() == [1.0, 1.5, 0.5] and f["bias"].tolist() == [7.0, 7.0, 7.0]
    a = f["a"][2].tolist()
    assert [a[0], a[1], a[3], a[4]] == [-65536, 0, 0, -65536] and plain_translation(a) == (40 << 16, 40 << 16)
    # taps: the sigma rule, normalised
    for ksize in (3, 5, 15, 41):
        r = (ksize - 1) // 2
        w = unpack_table(augment_table(1, (64, 64), (64, 64), ksize=ksize))["w"][0]
        assert abs(float(w[0].astype(np.float64) + 2.0 * w[1:r + 1].astype(np.float64).sum()) - 1.0) <= 1e-7 and not w[r + 1:].any()
        sigma = 0.3 * ((ksize - 1) / 2 - 1) + 0.8
        want = np.exp(-np.arange(r + 1) ** 2 / (2 * sigma * sigma))
        assert np.allclose(w[:r + 1] / w[0], want, rtol=1e-6, atol=0)
    assert abs(0.3 * ((41 - 1) / 2 - 1) + 0.8 - 6.5) < 1e-12


def test_augment_table_refuses_bad_values():
    ok = dict(B=2, src=(43, 75), out=(40, 72))
    for bad, msg in ((dict(B=0), "B must be positive"), (dict(src=(0, 75)), "src must be"), (dict(out=(40, 20000)), "out must be"),
                     (dict(out=40), "out must be"), (dict(crop=(0, 0, 0, 10)), "h and w must be positive"),
                     (dict(crop=[(0, 0, 5, 5)] * 3), "crop"), (dict(scale=0), "scale must be positive"),
                     (dict(angle=float("nan")), "angle must be finite"), (dict(shift=(1, 2, 3)), "shift"),
                     (dict(flip=[True]), "flip"), (dict(border="wrap"), "border must be"), (dict(border=["reflect"]), "border must be"),
                     (dict(fill=(1, 2)), "fill"), (dict(void_label=1.5), "void_label"), (dict(gain=float("inf")), "gain must be finite"),
                     (dict(ksize=4), "ksize must be 0 or odd"), (dict(ksize=1), "ksize must be 0 or odd"),
                     (dict(ksize=43), "ksize must be 0 or odd"), (dict(ksize=[3, -3]), "ksize must be 0 or odd"),
                     (dict(out=(40, 16), ksize=41), "must exceed it"), (dict(scale=1e-6), "does not fit Q16")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            augment_table(kw.pop("B"), kw.pop("src"), kw.pop("out"), **kw)


# ------------------------------------------------------------------------------------------------ the reference recipe's draws
def test_reference_draws_are_seeded_and_in_range():
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    t1, t2 = draw_reference_augment(8, (480, 480), (480, 480), g1), draw_reference_augment(8, (480, 480), (480, 480), g2)
    assert torch.equal(t1, t2)
    assert not torch.equal(t1, draw_reference_augment(8, (480, 480), (480, 480), g1))        # the generator has advanced
    N, H, W, OH, OW = 4000, 360, 480, 480, 480
    p = draw_reference_parameters(N, (H, W), (OH, OW), torch.Generator().manual_seed(11))
    table = augment_table(N, (H, W), (OH, OW), **p)
    assert torch.equal(table, draw_reference_augment(N, (H, W), (OH, OW), torch.Generator().manual_seed(11)))
    f = unpack_table(table)
    crop = p["crop"]
    cropped = (crop[:, 2] != H) | (crop[:, 3] != W)
    ssr = (p["angle"] != 0) | (p["scale"] != 1) | (p["shift"] != 0).any(axis=1)
    bright, blurred = p["gain"] != 1, p["ksize"] != 0
    for name, fired, prob in (("crop", cropped, .75), ("shift-scale-rotate", ssr, .25), ("flip", p["flip"], .5),
                              ("brightness", bright, .5), ("blur", blurred, .25)):
        assert abs(float(np.mean(fired)) - prob) <= 0.04, (name, float(np.mean(fired)))
    # ranges
    area, ratio = crop[:, 2] * crop[:, 3] / (H * W), crop[:, 3] / crop[:, 2]
    assert (area[cropped] >= .25 * .98).all() and (area <= 1).all()                      # (sides are rounded to whole pixels)
    assert (ratio[cropped] >= .9 * .99).all() and (ratio[cropped] <= 1.1 * 1.01).all()
    assert (crop[:, 0] >= 0).all() and (crop[:, 1] >= 0).all() and (crop[:, 0] + crop[:, 2] <= H).all() and (crop[:, 1] + crop[:, 3] <= W).all()
    assert (crop == np.floor(crop)).all()
    assert (np.abs(p["shift"]) <= .4).all() and (np.abs(p["angle"]) <= 15).all() and (np.abs(p["scale"] - 1) <= .1).all()
    assert (p["gain"] >= .5).all() and (p["gain"] <= 1.5).all()
    ks = p["ksize"][blurred]
    assert set(ks.tolist()) == set(range(3, 42, 2))                                      # all twenty odd sizes occur
    assert (f["radius"] == (np.maximum(p["ksize"], 1) - 1) // 2).all()
    assert (f["border"] == 0).all() and (f["sat"] == 1).all() and (f["bias"] == 0).all()
    assert ((f["a"][:, 0] * f["a"][:, 4] - f["a"][:, 1] * f["a"][:, 3] < 0) == p["flip"]).all()      # mirrored <=> negative determinant
    # crop-only draws map the output's corners inside the source (up to the Q16 rounding of the coefficients over the frame)
    only = ~ssr
    a = f["a"][only].astype(np.float64)
    tol = 0.5 * (OW + OH + 2)
    for qx in (0, OW):
        for qy in (0, OH):
            ux = a[:, 0] * (qx - .5) + a[:, 1] * (qy - .5) + a[:, 2]
            uy = a[:, 3] * (qx - .5) + a[:, 4] * (qy - .5) + a[:, 5]
            assert (ux >= -tol).all() and (ux <= W * 65536 + tol).all() and (uy >= -tol).all() and (uy <= H * 65536 + tol).all()
    assert only.sum() > 2500


def test_augmenters_with_one_seed_draw_one_sequence():
    class Recorder:
        def __init__(self):
            self.tables = []

        def augment(self, x, y, table, **kw):
            self.tables.append((table, kw))
            return x, y
    x, y = torch.zeros(3, 70, 100, 3, dtype=torch.uint8), torch.zeros(3, 70, 100, dtype=torch.long)
    r1, r2, r3 = Recorder(), Recorder(), Recorder()
    a1, a2, a3 = Augmenter(out=(64, 96), seed=3, labels="pixel"), Augmenter(out=(64, 96), seed=3, labels="pixel"), Augmenter(out=(64, 96), seed=4)
    for _ in range(3):
        a1(r1, x, y), a2(r2, x, y), a3(r3, x, y)
    assert all(torch.equal(p[0], q[0]) for p, q in zip(r1.tables, r2.tables))
    assert not torch.equal(r1.tables[0][0], r1.tables[1][0]) and not torch.equal(r1.tables[0][0], r3.tables[0][0])
    assert r1.tables[0][1] == dict(out=(64, 96), out_kind="f32", labels="pixel") and r3.tables[0][1]["labels"] == "patch"
    assert tuple(r1.tables[0][0].shape) == (3, 36)
    for bad in (dict(labels="both"), dict(out_kind="f16"), dict(out=(0, 5))):
        with pytest.raises(ValueError):
            Augmenter(**bad)


# ------------------------------------------------------------------------------------------------ host refusals of the op
FAKE = 256


def op(**kw):
    a = dict(frames=FAKE, masks=FAKE, mask_kind=0, B=2, H=43, W=75, table=FAKE, max_radius=0, OH=40, OW=72, out_kind=1, out=FAKE,
             pixel_labels=FAKE, patch_labels=FAKE, patch=8, scratch=None)
    a.update(kw)
    return capi.lib().dinoseg_op_augment(a["frames"], a["masks"], a["mask_kind"], a["B"], a["H"], a["W"], a["table"], a["max_radius"],
                                         a["OH"], a["OW"], a["out_kind"], a["out"], a["pixel_labels"], a["patch_labels"], a["patch"],
                                         a["scratch"], None)


def test_augment_op_refuses_bad_arguments_without_gpu():
    """Every refusal happens on the host (-1 and a message) before anything is enqueued; the fake pointers are never dereferenced."""
    def refused(msg, **change):
        assert op(**change) == -1
        assert msg in capi.last_error(), capi.last_error()

    refused("augment: null pointer (frames)", frames=None)
    refused("augment: null pointer (table)", table=None)
    refused("augment: null pointer (out)", out=None)
    refused("augment: mask kind 2 (0 = uint8, 1 = int64)", mask_kind=2)
    refused("augment: mask kind -1", mask_kind=-1)
    refused("augment: output kind 2", out_kind=2)
    refused("augment: bad argument (B=0", B=0)
    refused("augment: bad argument (B=2, source 0 x 75", H=0)
    refused("augment: bad argument (B=2, source 43 x -1", W=-1)
    refused("augment: bad argument (B=2, source 43 x 75, output 0 x 72", OH=0)
    refused("augment: bad argument (B=2, source 43 x 75, output 40 x 0", OW=0)
    refused("a side is above 16384", H=16385)
    refused("a side is above 16384", OW=16392)
    refused("augment: max_radius -1 (0 <= max_radius <= 20)", max_radius=-1)
    refused("augment: max_radius 21 (0 <= max_radius <= 20)", max_radius=21, scratch=FAKE)
    refused("augment: output 20 x 72 does not exceed max_radius 20", OH=20, patch_labels=None, max_radius=20, scratch=FAKE)
    refused("augment: output 40 x 7 does not exceed max_radius 7", OW=7, patch_labels=None, max_radius=7, scratch=FAKE)
    refused("augment: a label output without masks", masks=None)
    refused("augment: a label output without masks", masks=None, pixel_labels=None)
    refused("augment: a label output without masks", masks=None, patch_labels=None)
    refused("augment: patch 12 (8 or 16)", patch=12)
    refused("augment: output 40 x 72 is not a multiple of the patch (16)", patch=16)
    refused("augment: output 44 x 72 is not a multiple of the patch (8)", OH=44)
    refused("augment: null pointer (scratch is required when max_radius > 0)", max_radius=1)
    refused("augment: the destination is not 16-byte aligned", out=FAKE + 8)
    refused("augment: the destination is not 16-byte aligned", out=FAKE + 4, out_kind=0)
    # accepted shapes pass every check but the one provoked: no masks and no labels, a patch that is ignored without patch labels,
    # the smallest output of radius 20, sides of 16384
    for fine in (dict(masks=None, pixel_labels=None, patch_labels=None), dict(patch_labels=None, patch=12),
                 dict(OH=21, OW=24, patch_labels=None, max_radius=20, scratch=FAKE), dict(H=16384, W=16384, OH=16384, OW=16384)):
        assert op(**fine, table=None) == -1 and "null pointer (table)" in capi.last_error()


# ------------------------------------------------------------------------------------------------ the class methods
def test_augment_methods_have_no_cpu_path_and_check_their_arguments_first(tmp_path):
    m = DINOSeg(head="linear", n_blocks=1, write_path=str(tmp_path), max_epochs=1)
    assert m.device.type == "cpu"
    x = torch.zeros(2, 70, 100, 3, dtype=torch.uint8)
    y = torch.zeros(2, 70, 100, dtype=torch.long)
    table = augment_table(2, (70, 100), (64, 96), ksize=[0, 5])
    for kw in (dict(), dict(out_kind="u8", labels="patch")):
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            m.augment(x, y, table, out=(64, 96), **kw)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.augment(x, None, augment_table(2, (70, 100), (70, 100)))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.fit(train_dataloader=[(x, y)], val_dataloader=[(x, y)], augment=Augmenter(out=(64, 96), seed=1, labels="pixel"))
    # ValueError before any device use
    aug = lambda *a, **k: m.augment(*a, **k)
    with pytest.raises(ValueError, match="expected uint8"):
        aug(x.float(), y, table, out=(64, 96))
    with pytest.raises(ValueError, match="expected uint8"):
        aug(x.permute(0, 3, 1, 2), y, table, out=(64, 96))
    with pytest.raises(ValueError, match="expected an integer mask"):
        aug(x, y.float(), table, out=(64, 96))
    with pytest.raises(ValueError, match="expected an integer mask"):
        aug(x, y[:, :64], table, out=(64, 96))
    with pytest.raises(ValueError, match="expected an integer mask"):
        aug(x, y[:1], table, out=(64, 96))
    with pytest.raises(ValueError, match="out_kind must be"):
        aug(x, y, table, out=(64, 96), out_kind="bf16")
    with pytest.raises(ValueError, match="labels must be"):
        aug(x, y, table, out=(64, 96), labels="both")
    with pytest.raises(ValueError, match="multiple of the patch"):
        aug(x, y, augment_table(2, (70, 100), (70, 100)), labels="patch")
    with pytest.raises(ValueError, match="out must be"):
        aug(x, y, table, out=(64, 96, 3))
    with pytest.raises(ValueError, match="frame sides must be in 1..16384"):
        aug(x, y, table, out=(0, 96))
    with pytest.raises(ValueError, match=r"int32 \[B, 36\]"):
        aug(x, y, table.float(), out=(64, 96))
    with pytest.raises(ValueError, match=r"int32 \[B, 36\]"):
        aug(x, y, table[:, :35], out=(64, 96))
    with pytest.raises(ValueError, match="3 rows for 2 frames"):
        aug(x, y, augment_table(3, (70, 100), (64, 96)), out=(64, 96))
    bad = table.clone()
    bad[1, 14] = 21
    with pytest.raises(ValueError, match="radius outside 0..20"):
        aug(x, y, bad, out=(64, 96))
    bad = table.clone()
    bad[0, 6] = 2
    with pytest.raises(ValueError, match="border must be 0"):
        aug(x, y, bad, out=(64, 96))
    bad = table.clone()
    bad[0, 11] = 0x7FC00000                                     # gain = NaN
    with pytest.raises(ValueError, match="non-finite"):
        aug(x, y, bad, out=(64, 96))
    with pytest.raises(ValueError, match="radius 20 needs output sides above it"):
        aug(x[:, :16], y[:, :16], augment_table(2, (16, 100), (32, 96), ksize=41), out=(16, 96))
    assert dino_amd.Augmenter is Augmenter and "augment_table" in dino_amd.__all__


def test_fit_passes_train_batches_alone_through_the_hook(monkeypatch, tmp_path):
    """fit(augment=...): every train batch of both phases goes through the hook before its step, validation and test batches do
    not; with None the history equals that of a hook that returns its inputs.  The steps are stand-ins (no device)."""
    import types

    from dino_amd import ViTConfig
    from dino_amd import dinoseg as dinoseg_mod
    cfg = ViTConfig(embed_dim=128, num_heads=2, n_blocks=1, n_classes=7, head="linear")
    m = DINOSeg(arch=cfg, head="linear", n_blocks=1, n_classes=7, max_epochs=1, write_path=str(tmp_path), pretrain_on_sim=True)
    seen = {"train": [], "eval": []}
    cm = torch.eye(7, dtype=torch.int64)

    def train_step(batch, batch_idx=0, **kw):
        seen["train"].append(batch[0])
        return {"loss": batch[0].float().mean(), "pred": torch.zeros(batch[1].numel(), dtype=torch.int32), "gt": batch[1].reshape(-1).long(),
                "probs": None}

    def eval_step(batch, batch_idx=0, **kw):
        seen["eval"].append(batch[0])
        return {"confusion": cm}
    for name in ("fused_training_step", "fused_training_step_dense"):
        monkeypatch.setattr(m, name, train_step)
    for name in ("validation_step", "validation_step_dense", "test_step"):
        monkeypatch.setattr(m, name, eval_step)
    monkeypatch.setattr(m, "fused_adam_step", lambda *a, **k: None)
    monkeypatch.setattr(m, "check_labels", lambda: None)
    monkeypatch.setattr(dinoseg_mod.capi, "lib", lambda: types.SimpleNamespace(dinoseg_op_confusion=lambda *a: 0))
    monkeypatch.setattr(dinoseg_mod.capi, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(m, "_stream", lambda: None)
    x = torch.full((2, 64, 64, 3), 10, dtype=torch.uint8)
    y = torch.zeros(2, 64, 64, dtype=torch.long)
    calls = []

    def hook(model, xb, yb):
        calls.append(model)
        return xb + 1, yb
    loaders = dict(train_dataloader=[(x, y)] * 2, val_dataloader=[(x, y)], test_dataloader=[(x, y)], sim_dataloader=[(x, y)] * 3)
    out = m.fit(augment=hook, **loaders)
    assert len(calls) == 5 and all(c is m for c in calls)
    assert len(seen["train"]) == 5 and all(int(t[0, 0, 0, 0]) == 11 for t in seen["train"])
    assert len(seen["eval"]) == 3 and all(int(t[0, 0, 0, 0]) == 10 for t in seen["eval"])
    assert out["history"][0]["train_loss"] == 11.0
    plain = m.fit(**loaders)
    stub = m.fit(augment=lambda model, xb, yb: (xb, yb), **loaders)
    assert plain["history"] == stub["history"] and plain["sim_history"] == stub["sim_history"] and plain["test"] == stub["test"]
    assert plain["history"][0]["train_loss"] == 10.0
