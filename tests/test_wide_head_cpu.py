"""CPU tests of segmentation heads with more than 32 classes (up to 256: ADE20K 150, COCO-Stuff 171 / 182): the C-ABI accepts
the class count, the Python module keeps the reference's head shapes (pl_torch_modules.py:108-138) and checkpoints round-trip."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.ckpt import save_checkpoint


@pytest.mark.parametrize("head", [capi.HEAD_MLP, capi.HEAD_LINEAR])
def test_create_accepts_up_to_256_classes(head):
    lib = capi.lib()
    h = ctypes.c_void_p()
    for C in (33, 150, 256):
        cfg = capi.Config(384, 6, 12, 8, 4, C, head, 28, 1e-6, capi.FP16X3)
        assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, capi.last_error()
        # the argmax-only forward keeps the log-probabilities in the workspace: it is sized for them at every class count
        assert lib.dinoseg_workspace_bytes(h, 1, 64) >= 64 * C * 4
        assert lib.dinoseg_destroy(h) == 0
    cfg = capi.Config(384, 6, 12, 8, 4, 257, head, 28, 1e-6, capi.FP16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert "unsupported config" in capi.last_error()


@pytest.mark.parametrize("head", ["linear", "mlp"])
def test_head_shapes_at_150_classes(head):
    m = DINOSeg(head=head, n_blocks=1, n_classes=150)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("clf.")}
    if head == "mlp":
        assert shapes == {"clf.layer_1.weight": (200, 384), "clf.layer_1.bias": (200,),
                          "clf.layer_2.weight": (100, 200), "clf.layer_2.bias": (100,),
                          "clf.layer_3.weight": (150, 100), "clf.layer_3.bias": (150,)}
    else:
        assert shapes == {"clf.layer_1.weight": (150, 384), "clf.layer_1.bias": (150,)}
    assert m.n_classes == 150


@pytest.mark.parametrize("head", ["linear", "mlp"])
def test_checkpoint_round_trip_at_150_classes(tmp_path, head):
    sd = procedural_state_dict(ViTConfig(n_blocks=1, n_classes=150, head=head))
    m = DINOSeg(head=head, n_blocks=1, n_classes=150)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    path = os.path.join(tmp_path, "wide.ckpt")
    save_checkpoint(m, path, epoch=1)
    m2 = DINOSeg.load_from_checkpoint(path)
    assert m2.n_classes == 150 and m2.head == head
    for k, v in m2.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
