"""The architecture matrix of tests/arch_util.py without a GPU: dinoseg_create takes every config, its name-and-shape table is
tensor_shapes(cfg), the workspace query answers, a checkpoint round-trips; and what create refuses, it refuses with a message before
any device call.  The oracle side of the GPU tests' bars is checked here too: enough patches of every config have the top-2 margin
the argmax comparison of the parity modes needs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, ViTConfig, capi
from dino_amd.ckpt import save_checkpoint
from dino_amd.weights import synthetic_labels, tensor_shapes
from tests import arch_util as A


def _create(cfg, precision="bf16x3"):
    h = ctypes.c_void_p()
    native = A.native_config(cfg, precision) if isinstance(cfg, ViTConfig) else cfg
    return capi.lib().dinoseg_create(ctypes.byref(native), ctypes.byref(h)), h


def test_matrix_is_the_one_the_gpu_tests_expect():
    assert A.TAGS == ["W256", "W512", "W640r2", "W896r1", "W1024p16", "Sr1", "Sr3", "Sr8", "Br2", "T2", "L0", "C1"]
    for tag, cfg in A.ARCH.items():
        assert cfg.num_heads * 64 == cfg.embed_dim, tag
        assert A.n_patches(cfg) + 1 == (65 if cfg.patch == 8 else 37), tag
        assert A.frames(tag).shape == (2, A.side(cfg), A.side(cfg), 3)
    assert {c.embed_dim for c in A.ARCH.values()} == {128, 256, 384, 512, 640, 768, 896, 1024}
    assert {c.mlp_ratio for c in A.ARCH.values()} == {1, 2, 3, 4, 8}
    assert A.ARCH["L0"].n_blocks == 0 and A.ARCH["C1"].n_classes == 1 and A.ARCH["T2"].hidden == 256
    assert A.ARCH["W640r2"].hidden < 3 * 640 and A.ARCH["W896r1"].hidden == 896 and A.ARCH["W1024p16"].hidden == 4096


@pytest.mark.parametrize("precision", list(A.PRECISIONS))
@pytest.mark.parametrize("tag", A.TAGS)
def test_handle_creates_and_sizes_its_workspace(tag, precision):
    cfg = A.ARCH[tag]
    lib = capi.lib()
    rc, h = _create(cfg, precision)
    assert rc == 0, capi.last_error()
    try:
        r = A.side(cfg)
        w = [lib.dinoseg_workspace_bytes(h, b, r) for b in (1, 2, 3)]
        # (at least the fp32 residual rows and one 16-bit copy of them)
        assert w[0] >= (A.n_patches(cfg) + 1) * cfg.embed_dim * 6
        assert w[0] < w[1] < w[2]
        assert lib.dinoseg_workspace_bytes(h, 1, r + cfg.patch // 2) == -1
    finally:
        assert lib.dinoseg_destroy(h) == 0


@pytest.mark.parametrize("tag", A.TAGS)
def test_native_name_and_shape_table(tag):
    """As test_host_cpu.py's table test: a host pointer gets as far as "is not a device pointer" only when the name and the shape were
    accepted; every key names a gradient slot; a block key past the depth is unknown."""
    cfg = A.ARCH[tag]
    lib = capi.lib()
    rc, h = _create(cfg)
    assert rc == 0, capi.last_error()
    buf = (ctypes.c_float * 4)()
    try:
        shapes = tensor_shapes(cfg)
        assert len(shapes) == 6 + 12 * cfg.n_blocks + (6 if cfg.head == "mlp" else 2)
        for name, shape in shapes.items():
            key = name.encode()
            good = (ctypes.c_int64 * len(shape))(*shape)
            assert lib.dinoseg_bind_weight(h, key, ctypes.addressof(buf), good, len(shape)) == -1, name
            assert "is not a device pointer" in capi.last_error(), (name, capi.last_error())
            bad = (ctypes.c_int64 * len(shape))(*shape[:-1], shape[-1] + 1)
            assert lib.dinoseg_bind_weight(h, key, ctypes.addressof(buf), bad, len(shape)) == -1, name
            assert "shape mismatch" in capi.last_error(), (name, capi.last_error())
            assert lib.dinoseg_bind_grad(h, key, None) == 0, name
        past = f"dino.blocks.{cfg.n_blocks}.norm1.weight".encode()
        assert lib.dinoseg_bind_grad(h, past, None) == -1 and "unexpected key" in capi.last_error()
        assert lib.dinoseg_bind_weight(h, past, ctypes.addressof(buf), (ctypes.c_int64 * 1)(cfg.embed_dim), 1) == -1
        assert "unexpected key" in capi.last_error()
        assert lib.dinoseg_grad_stages(h) == cfg.n_blocks + 2
    finally:
        assert lib.dinoseg_destroy(h) == 0


@pytest.mark.parametrize("tag", A.TAGS)
def test_checkpoint_round_trip(tmp_path, tag):
    cfg = A.ARCH[tag]
    sd = A.state(tag)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, arch=cfg)
    assert m.cfg == cfg
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(tensor_shapes(cfg))
    m.load_state_dict({k: A.tensor(v) for k, v in sd.items()}, strict=True)
    path = os.path.join(tmp_path, tag + ".ckpt")
    save_checkpoint(m, path, epoch=1)
    m2 = DINOSeg.load_from_checkpoint(path)
    assert m2.cfg == cfg
    for k, v in m2.state_dict().items():
        assert torch.equal(v, A.tensor(sd[k])), k


REFUSED = [
    ("embed_dim 192", dict(embed_dim=192, num_heads=3)),
    ("embed_dim 1152", dict(embed_dim=1152, num_heads=18)),
    ("heads * 64 != embed_dim", dict(embed_dim=384, num_heads=4)),
    ("heads * 64 != embed_dim (12 heads at 1024)", dict(embed_dim=1024, num_heads=12)),
    ("mlp_ratio 0", dict(mlp_ratio=0)),
    ("0 classes", dict(n_classes=0)),
    ("257 classes", dict(n_classes=257)),
]


@pytest.mark.parametrize("head", ["mlp", "linear"])
@pytest.mark.parametrize("what,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_refuses_with_a_message(what, kw, head):
    """Each of these fails in dinoseg_create itself: the checks come before the handle exists, so nothing reaches a device call (this
    test runs where there is no device)."""
    cfg = ViTConfig(n_blocks=2, head=head, **kw)
    lib = capi.lib()
    lib.dinoseg_set_option(b"no_such_option", 0)            # (leaves another message behind: the next one must be create's own)
    rc, h = _create(cfg)
    assert rc == -1 and not h.value, what
    msg = capi.last_error()
    assert "dinoseg_create: unsupported config" in msg, (what, msg)
    for shown, field in (("embed_dim", "embed_dim"), ("heads", "num_heads"), ("mlp_ratio", "mlp_ratio"), ("classes", "n_classes")):
        assert f"{shown}={getattr(cfg, field)} " in msg.replace(";", " "), (what, field, msg)


@pytest.mark.parametrize("tag", A.TAGS)
def test_oracle_margins_leave_enough_patches_to_compare(tag):
    """The parity modes' argmax is compared on the patches whose reference top-2 margin exceeds 2e-3 (twice the log-prob bar): at least
    95 % of every config's patches."""
    margin = A.oracle_margin(tag)
    assert margin.shape == (A.B * A.n_patches(A.ARCH[tag]),)
    assert float((margin > 2e-3).float().mean()) >= 0.95


@pytest.mark.parametrize("tag", A.TAGS)
def test_step_labels_ignore_only_the_patches_at_a_relu_kink(tag):
    """The fine-tune labels are synthetic_labels(seed 8) with -100 exactly on kink_patches(tag): none for the linear heads, and at least
    three quarters of the patches keep their label everywhere."""
    cfg = A.ARCH[tag]
    y, kink = A.labels(tag), A.kink_patches(tag)
    assert y.shape == (A.B, A.n_patches(cfg)) and kink.shape == (y.size,)
    assert np.array_equal(y.reshape(-1) == -100, kink)
    assert np.array_equal(y.reshape(-1)[~kink], synthetic_labels(A.B, A.n_patches(cfg), cfg.n_classes, seed=A.LABEL_SEED).reshape(-1)[~kink])
    assert ((y >= 0) & (y < cfg.n_classes))[y != -100].all()
    assert kink.mean() <= 0.25
    if cfg.head == "linear":
        assert not kink.any()
