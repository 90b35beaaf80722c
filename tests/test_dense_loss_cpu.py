"""Pixel-resolution training loss without a GPU: the C-ABI's host-side refusals (nothing is launched, the fake pointers are never
dereferenced), the scratch-size contract, the CPU-model refusals and fit()'s routing of patch labels."""
import ctypes
import types

import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi
from dino_amd import dinoseg as dinoseg_mod

# the shapes tests/test_dense_loss_gpu.py runs the op at: (B, hp, wp, C, OH, OW)
GPU_SHAPES = [
    (2, 4, 4, 2, 64, 64), (3, 1, 1, 5, 8, 8), (2, 8, 16, 33, 100, 131), (1, 6, 9, 150, 48, 72), (1, 5, 7, 256, 40, 61),
    (2, 7, 5, 7, 7, 5), (2, 15, 20, 21, 120, 160), (2, 3, 5, 150, 95, 97), (1, 60, 80, 7, 480, 640),
]


def test_header_table_and_library_agree_on_the_new_entries():
    new = {"dinoseg_op_upsample_nll_scratch_bytes", "dinoseg_op_upsample_nll", "dinoseg_train_step_dense_hw"}
    assert new <= set(capi.header_symbols()) and new <= set(capi.SIGNATURES)
    lib = capi.lib()
    for s in new:
        assert hasattr(lib, s), s


def test_op_refuses_bad_arguments_without_gpu():
    lib = capi.lib()
    fake = 256
    op = lib.dinoseg_op_upsample_nll

    def call(logp=fake, B=1, hp=4, wp=4, C=7, OH=32, OW=32, labels=fake, ignore=255, loss=fake, scratch=fake):
        return op(logp, B, hp, wp, C, OH, OW, labels, ignore, loss, None, None, None, scratch, None)
    for kw in ({"logp": None}, {"labels": None}, {"loss": None}, {"scratch": None}):
        assert call(**kw) == -1
        assert "upsample_nll: null pointer" in capi.last_error(), kw
    for C in (0, 257):
        assert call(C=C) == -1
        assert "upsample_nll: bad argument (B=1 hp=4 wp=4 C=%d OH=32 OW=32" % C in capi.last_error()
    assert call(OH=3) == -1
    assert "upsample_nll: output 3x32 is smaller than the input grid 4x4" in capi.last_error()
    assert call(OW=3) == -1
    assert "upsample_nll: output 32x3 is smaller than the input grid 4x4" in capi.last_error()
    for kw in ({"B": 0}, {"hp": 0}, {"wp": -4}, {"OH": 0}, {"OW": -1}):
        assert call(**kw) == -1
        assert "upsample_nll: bad argument" in capi.last_error(), kw
    for ignore in (0, 3, 6):
        assert call(ignore=ignore) == -1
        assert "upsample_nll: ignore_index %d is a class" % ignore in capi.last_error()
    assert lib.dinoseg_op_upsample_nll_scratch_bytes(1, 4, 4, 7, 3, 32) == -1
    assert "upsample_nll_scratch_bytes: output 3x32 is smaller" in capi.last_error()


def test_step_refuses_bad_arguments_without_gpu():
    lib = capi.lib()
    fake = 256
    step = lib.dinoseg_train_step_dense_hw
    h = ctypes.c_void_p()
    cfg = capi.Config(384, 6, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.BF16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        for args in ((None, fake, 0, 1, 64, 64, 64, 64, fake, 255, fake), (h, None, 0, 1, 64, 64, 64, 64, fake, 255, fake),
                     (h, fake, 0, 1, 64, 64, 64, 64, None, 255, fake), (h, fake, 0, 1, 64, 64, 64, 64, fake, 255, None),
                     (h, fake, 0, 0, 64, 64, 64, 64, fake, 255, fake)):
            assert step(*args, None, None) == -1
            assert "dinoseg_train_step_dense_hw: bad argument" in capi.last_error()
        assert step(h, fake, 0, 1, 60, 64, 64, 64, fake, 255, fake, None, None) == -1
        assert "Resolution should be a multiple of 8." in capi.last_error()
        for OH, OW in ((7, 64), (64, 7)):
            assert step(h, fake, 0, 1, 64, 64, OH, OW, fake, 255, fake, None, None) == -1
            assert "dinoseg_train_step_dense_hw: output %dx%d is smaller than the input grid 8x8" % (OH, OW) in capi.last_error()
        assert step(h, fake, 0, 1, 64, 64, 0, 64, fake, 255, fake, None, None) == -1
        assert "dinoseg_train_step_dense_hw: bad argument (B=1 hp=8 wp=8 C=7 OH=0 OW=64" in capi.last_error()
        assert step(h, fake, 0, 1, 64, 64, 64, 64, fake, 6, fake, None, None) == -1
        assert "dinoseg_train_step_dense_hw: ignore_index 6 is a class" in capi.last_error()
        # every argument check passed: the forward's own state error (weights never packed), still nothing launched
        assert step(h, fake, 0, 1, 64, 64, 64, 64, fake, 255, fake, None, None) == -3
        assert "weights not packed" in capi.last_error()
    finally:
        assert lib.dinoseg_destroy(h) == 0


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=["%dx%dx%dx%d-%dx%d" % s for s in GPU_SHAPES])
def test_scratch_is_at_most_8_bytes_per_pixel_plus_64k(shape):
    B, hp, wp, C, OH, OW = shape
    n = capi.lib().dinoseg_op_upsample_nll_scratch_bytes(B, hp, wp, C, OH, OW)
    assert 4 * B * OH * OW <= n <= 8 * B * OH * OW + 65536
    assert n < B * C * OH * OW * 4 or C <= 2, "never the size of a [B, C, OH, OW] tensor"


def test_cpu_model_has_no_dense_steps():
    m = DINOSeg(head="linear", n_blocks=1, arch=ViTConfig(n_blocks=1, head="linear"))
    x = torch.zeros(1, 3, 64, 64)
    y = torch.zeros(1, 64, 64, dtype=torch.long)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.fused_training_step_dense((x, y))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.training_step_dense((x, y))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        dino_amd.dense_nll_loss(torch.zeros(64, 7), y, grid=(8, 8))


def test_fit_routes_patch_labels_to_the_patch_steps(monkeypatch, tmp_path):
    """2-D labels: fit() calls fused_training_step / validation_step / test_step as before; 3-D labels: the dense steps.  The steps
    are stand-ins that count their calls (no device)."""
    cfg = ViTConfig(embed_dim=128, num_heads=2, n_blocks=1, n_classes=7, head="linear")
    m = DINOSeg(arch=cfg, head="linear", n_blocks=1, n_classes=7, max_epochs=1, write_path=str(tmp_path))
    calls = {}

    def stand_in(name, out):
        def f(batch, batch_idx=0, **kw):
            calls[name] = calls.get(name, 0) + 1
            return out(batch)
        monkeypatch.setattr(m, name, f)
    cm = torch.eye(7, dtype=torch.int64)
    train_out = lambda b: {"loss": torch.tensor(1.0), "pred": torch.zeros(b[1].numel(), dtype=torch.int32),
                           "gt": b[1].reshape(-1).long(), "probs": None}
    for name in ("fused_training_step", "fused_training_step_dense"):
        stand_in(name, train_out)
    for name in ("validation_step", "validation_step_dense", "test_step"):
        stand_in(name, lambda b: {"confusion": cm})
    monkeypatch.setattr(m, "fused_adam_step", lambda *a, **k: None)
    monkeypatch.setattr(m, "check_labels", lambda: None)
    monkeypatch.setattr(dinoseg_mod.capi, "lib", lambda: types.SimpleNamespace(dinoseg_op_confusion=lambda *a: 0))
    monkeypatch.setattr(dinoseg_mod.capi, "stream_ptr", lambda *a: None)
    monkeypatch.setattr(m, "_stream", lambda: None)
    x = torch.zeros(2, 3, 64, 64)
    patch = [(x, torch.zeros(2, 64, dtype=torch.long))] * 2
    out = m.fit(train_dataloader=patch, val_dataloader=patch[:1], test_dataloader=patch[:1])
    assert calls == {"fused_training_step": 2, "validation_step": 1, "test_step": 1}
    assert out["history"][0]["train_loss"] == 1.0 and "val_acc" in out["history"][0]
    calls.clear()
    pixel = [(x, torch.zeros(2, 64, 64, dtype=torch.long))] * 2
    m.fit(train_dataloader=pixel, val_dataloader=pixel[:1], test_dataloader=pixel[:1])
    assert calls == {"fused_training_step_dense": 2, "validation_step_dense": 2}
