"""CPU tests of patch-16 backbones (ViT-S/16, ViT-B/16): the constructor keeps the config's patch size and position grid (and
takes ``patch_size=``), shapes and messages follow the patch size, checkpoints are recognised by their tensors, the C-ABI
accepts patch 8 and 16 only, and the g16 fixtures -- captured from the reference's VisionTransformer(patch_size=16)
(tools/gen_golden_p16.py) -- equal the CPU oracle with ``patch=16`` on square frames."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.ckpt import read_checkpoint, save_checkpoint
from dino_amd.weights import synthetic_frames, tensor_shapes
from oracle import dinoseg_oracle as O

MIN_MARGIN = 2e-3       # twice the parity bar of 1e-3: the GPU tests demand zero flips


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


# --------------------------------------------------------------------------- constructor
def test_presets_are_exported():
    assert dino_amd.VIT_S16 == ViTConfig(patch=16, pos_grid=14)
    assert dino_amd.VIT_B16 == ViTConfig(embed_dim=768, num_heads=12, patch=16, pos_grid=14)
    assert {"VIT_S16", "VIT_B16"} <= set(dino_amd.__all__)
    assert dino_amd.VIT_S8.patch == 8 and dino_amd.VIT_S8.pos_grid == 28


@pytest.mark.parametrize("kw", [dict(patch_size=16), dict(arch=dino_amd.VIT_S16), dict(arch=ViTConfig(patch=16, pos_grid=14)),
                                dict(arch="vit_small", patch_size=16), dict(arch=dino_amd.VIT_S16, patch_size=16)])
def test_patch16_constructor_gives_the_patch16_state_dict(kw):
    m = DINOSeg(head="mlp", n_blocks=2, **kw)
    cfg = ViTConfig(n_blocks=2, patch=16, pos_grid=14)
    assert m.cfg == cfg and m.patch_size == 16
    got = _shapes(m)
    assert got == dict(tensor_shapes(cfg))
    assert got["dino.patch_embed.proj.weight"] == (384, 3, 16, 16) and got["dino.pos_embed"] == (1, 197, 384)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}, strict=True)


def test_vit_base_16_and_the_patch8_default():
    m = DINOSeg(head="linear", n_blocks=1, n_classes=150, arch="vit_base", patch_size=16)
    cfg = ViTConfig(embed_dim=768, num_heads=12, n_blocks=1, n_classes=150, head="linear", patch=16, pos_grid=14)
    assert m.cfg == cfg and _shapes(m) == dict(tensor_shapes(cfg))
    assert _shapes(DINOSeg(head="mlp", n_blocks=1, arch=dino_amd.VIT_B16))["dino.pos_embed"] == (1, 197, 768)
    for kw in (dict(), dict(patch_size=8), dict(arch=dino_amd.VIT_S8), dict(arch=dino_amd.VIT_S8, patch_size=8)):
        m8 = DINOSeg(head="mlp", n_blocks=1, **kw)
        assert m8.cfg == ViTConfig(n_blocks=1) and m8.patch_size == 8
        assert _shapes(m8)["dino.patch_embed.proj.weight"] == (384, 3, 8, 8) and _shapes(m8)["dino.pos_embed"] == (1, 785, 384)
    # a ViTConfig keeps a position grid of its own
    assert _shapes(DINOSeg(n_blocks=1, arch=ViTConfig(patch=16, pos_grid=30)))["dino.pos_embed"] == (1, 901, 384)


def test_contradictory_or_unsupported_patch_size_raises():
    with pytest.raises(ValueError, match="contradicts"):
        DINOSeg(n_blocks=1, arch=dino_amd.VIT_S16, patch_size=8)
    with pytest.raises(ValueError, match="contradicts"):
        DINOSeg(n_blocks=1, arch=dino_amd.VIT_B8, patch_size=16)
    for p in (12, 32, 4):
        with pytest.raises(ValueError, match="8 or 16"):
            DINOSeg(n_blocks=1, patch_size=p)
        with pytest.raises(ValueError, match="8 or 16"):
            DINOSeg(n_blocks=1, arch=ViTConfig(patch=p, pos_grid=14))
    with pytest.raises(TypeError):
        DINOSeg(None, None, None, "mlp", 1, 1, 1e-6, torch.optim.AdamW, True, 200, 10, False, 7, False, None, True, False, "vit",
                "vit_small", 16)           # patch_size is keyword-only, as arch is


# --------------------------------------------------------------------------- shapes and messages
def test_set_resolution_names_the_patch_size():
    m = DINOSeg(head="mlp", n_blocks=1, patch_size=16)
    with pytest.raises(ValueError, match=r"^Resolution should be a multiple of 16\.$"):
        m.set_resolution(488)
    m.set_resolution(224)
    assert m.resolution == 224 and m.transforms.resolution == 224
    m8 = DINOSeg(head="mlp", n_blocks=1)
    m8.set_resolution(488)                                              # a multiple of 8
    with pytest.raises(ValueError, match=r"^Resolution should be a multiple of 8\.$"):
        m8.set_resolution(250)


def test_batches_need_multiples_of_16_and_reach_the_device_check():
    m = DINOSeg(head="mlp", n_blocks=1, patch_size=16)
    for bad in (torch.zeros((1, 3, 240, 328)), torch.zeros((1, 248, 320, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="Resolution should be a multiple of 16."):
            m._prep_batch(bad)
    x, kind, B, H, W = m._prep_batch(torch.zeros((2, 240, 320, 3), dtype=torch.uint8))
    assert (kind, B, H, W) == (capi.INPUT_U8_HWC, 2, 240, 320)
    x = torch.zeros((1, 3, 240, 320))
    y = torch.zeros((1, 15 * 20), dtype=torch.int64)
    u8 = torch.zeros((2, 240, 320, 3), dtype=torch.uint8)
    calls = [lambda: m(x), lambda: m.dino(x), lambda: m.features(u8), lambda: m.get_last_selfattention(x),
             lambda: m.forward_mask(x, torch.ones((2, 15, 20))), lambda: m.validation_step((x, y)),
             lambda: m.training_step((x, y)), lambda: m.fused_training_step((x, y)), lambda: m.forward_frames(u8),
             lambda: m.predict(np.zeros((480, 480, 3), np.uint8))]
    for call in calls:
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            call()


# --------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("arch,D", [("vit_small", 384), ("vit_base", 768)])
def test_patch16_checkpoint_round_trip(tmp_path, arch, D):
    cfg = ViTConfig(embed_dim=D, num_heads=D // 64, n_blocks=2, patch=16, pos_grid=14)
    sd = procedural_state_dict(cfg)
    m = DINOSeg(data_path="d", write_path="w", head="mlp", n_blocks=2, optimizer=torch.optim.Adam, lr=1e-3, arch=arch, patch_size=16)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    path = os.path.join(tmp_path, "p16.ckpt")
    save_checkpoint(m, path, epoch=3)
    m2 = DINOSeg.load_from_checkpoint(path)
    assert m2.cfg == cfg and m2.patch_size == 16
    for k, v in m2.state_dict().items():
        assert torch.equal(v, torch.from_numpy(sd[k])), k
    # recognised without hyper-parameters: patch size, position grid, width, depth and head all come from the tensors
    ck = read_checkpoint(path)
    bare = os.path.join(tmp_path, "bare.ckpt")
    torch.save({"state_dict": ck["state_dict"]}, bare)
    m3 = DINOSeg.load_from_checkpoint(bare)
    assert m3.cfg == cfg and _shapes(m3) == dict(tensor_shapes(cfg))


def test_patch8_checkpoint_schema_is_unchanged(tmp_path):
    sd = procedural_state_dict(ViTConfig(n_blocks=1))
    m = DINOSeg(head="mlp", n_blocks=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    path = os.path.join(tmp_path, "p8.ckpt")
    save_checkpoint(m, path)
    ck = read_checkpoint(path)
    assert sorted(ck) == ["epoch", "global_step", "hyper_parameters", "pytorch-lightning_version", "state_dict"]
    assert sorted(ck["hyper_parameters"]) == sorted(
        ["class_names", "head", "n_blocks", "batch_size", "lr", "optimizer", "freeze_backbone", "max_epochs", "patience", "grayscale",
         "n_classes", "pretrain_on_sim", "augmented", "random_init", "backbone", "data_path", "write_path", "comet_logger"])
    assert DINOSeg.load_from_checkpoint(path).cfg == ViTConfig(n_blocks=1)
    # a stored grid other than 224 / patch is recognised too
    cfg = ViTConfig(n_blocks=1, patch=16, pos_grid=30)
    odd = os.path.join(tmp_path, "g30.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}}, odd)
    assert DINOSeg.load_from_checkpoint(odd).cfg == cfg
    # ... and keeps the MLP width the tensors have
    cfg = ViTConfig(n_blocks=1, patch=8, pos_grid=30, mlp_ratio=2)
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg).items()}}, odd)
    assert DINOSeg.load_from_checkpoint(odd).cfg == cfg


# --------------------------------------------------------------------------- C-ABI
def _create(patch, pos_grid=14, D=384):
    h = ctypes.c_void_p()
    cfg = capi.Config(D, D // 64, 2, patch, 4, 7, capi.HEAD_MLP, pos_grid, 1e-6, capi.FP16X3)
    return capi.lib().dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)), h


def test_create_accepts_patch_8_and_16_only():
    lib = capi.lib()
    for p, g in ((8, 28), (16, 14)):
        rc, h = _create(p, g)
        assert rc == 0, capi.last_error()
        assert lib.dinoseg_destroy(h) == 0
    for p in (12, 32, 0, 4):
        rc, _ = _create(p)
        assert rc == -1
        assert "unsupported config" in capi.last_error() and f"patch={p}" in capi.last_error() and "8 or 16" in capi.last_error()


def test_patch16_handle_checks_frames_against_16():
    lib = capi.lib()
    rc, h = _create(16)
    assert rc == 0
    rc8, h8 = _create(8, 28)
    assert rc8 == 0
    try:
        for H, W in ((488, 480), (480, 488), (8, 480), (0, 320)):
            assert lib.dinoseg_workspace_bytes_hw(h, 1, H, W) == -1
            assert capi.last_error() == "Resolution should be a multiple of 16."
            assert lib.dinoseg_prepare_resolution_hw(h, H, W, None) == -1
            assert capi.last_error() == "Resolution should be a multiple of 16."
            with pytest.raises(ValueError, match=r"^Resolution should be a multiple of 16\.$"):
                capi.check(lib.dinoseg_forward_hw(h, ctypes.c_void_p(16), capi.INPUT_U8_HWC, 1, H, W, None, None, -1, None, None))
            with pytest.raises(ValueError, match=r"^Resolution should be a multiple of 16\.$"):
                capi.check(lib.dinoseg_train_forward_hw(h, ctypes.c_void_p(16), capi.INPUT_U8_HWC, 1, H, W, None, None))
        assert lib.dinoseg_workspace_bytes_hw(h8, 1, 488, 480) > 0            # a multiple of 8 is a frame of the patch-8 handle
        assert lib.dinoseg_workspace_bytes(h8, 1, 250) == -1
        assert capi.last_error() == "Resolution should be a multiple of 8."
        # 480 x 480: 901 tokens instead of 3601 -- the workspace follows the token count
        w16, w8 = lib.dinoseg_workspace_bytes(h, 1, 480), lib.dinoseg_workspace_bytes(h8, 1, 480)
        assert 901 * 384 * 4 < w16 < w8 / 3
        # equal token counts: only the buffer that hosts the gather matrix differs -- two planes of [900, 768] at patch 16 are
        # larger than the LayerNorm planes [901, 384] it shares the buffer with (at patch 8 the [900, 192] matrix is the smaller)
        assert w16 - lib.dinoseg_workspace_bytes(h8, 1, 240) == 2 * 900 * 768 * 2 - 2 * 901 * 384 * 2
        # 64 x 128 at patch 16: 4 x 8 patches, 33 tokens
        assert lib.dinoseg_forward_mask_hw(h, ctypes.c_void_p(16), capi.INPUT_F32_CHW, 64, 128, ctypes.c_void_p(16), 33,
                                           ctypes.c_void_p(16), None, None) == -1
        assert "must be smaller than the token count 33" in capi.last_error()
    finally:
        assert lib.dinoseg_destroy(h) == 0 and lib.dinoseg_destroy(h8) == 0


def test_patch_gather_p_entry_checks_its_arguments():
    lib = capi.lib()
    assert "dinoseg_op_patch_gather_p" in capi.header_symbols() and hasattr(lib, "dinoseg_op_patch_gather_p")
    fake = ctypes.c_void_p(256)     # never dereferenced: every call below is refused on the host
    assert lib.dinoseg_op_patch_gather_p(fake, capi.INPUT_U8_HWC, 1, 64, 64, 12, fake, 0, 1, None) == -1
    assert "patch=12 must be 8 or 16" in capi.last_error()
    assert lib.dinoseg_op_patch_gather_p(fake, capi.INPUT_U8_HWC, 1, 64, 72, 16, fake, 0, 1, None) == -1
    assert capi.last_error() == "Resolution should be a multiple of 16."
    assert lib.dinoseg_op_patch_gather_p(fake, capi.INPUT_U8_HWC, 1, 64, 68, 8, fake, 0, 1, None) == -1
    assert capi.last_error() == "Resolution should be a multiple of 8."
    assert lib.dinoseg_op_patch_gather_p(fake, capi.INPUT_U8_HWC, 1, 64, 64, 16, fake, 16 * 768 - 1, 2, None) == -1
    assert "bad argument" in capi.last_error()
    assert lib.dinoseg_op_patch_gather_p(None, capi.INPUT_U8_HWC, 1, 64, 64, 16, fake, 0, 1, None) == -1
    # patch 16 reads and writes 16 bytes at a time: a frame or output pointer off that alignment is refused, not read
    off = ctypes.c_void_p(256 + 8)
    for x, out, plane, planes in ((off, fake, 0, 1), (fake, off, 0, 1), (fake, fake, 16 * 768 + 4, 2)):
        assert lib.dinoseg_op_patch_gather_p(x, capi.INPUT_U8_HWC, 1, 64, 64, 16, out, plane, planes, None) == -1
        assert "16-byte aligned" in capi.last_error()
    assert lib.dinoseg_op_patch_gather_p(fake, 7, 1, 64, 64, 16, fake, 0, 1, None) == -1


def test_create_under_address_sanitizer():
    """The host build under AddressSanitizer (`make -C dino_amd/csrc asan`, as tests/test_host_cpu.py runs it) accepts patch = 16 in
    dinoseg_create, refuses 12 and 32, and checks frames against the handle's patch size.  Build container only."""
    import shutil
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "dino_amd", "csrc")
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no toolchain")
    subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "asan"], check=True, capture_output=True)
    rt = subprocess.run(["make", "-s", "-C", csrc, "asan-runtime"], check=True, capture_output=True, text=True).stdout.strip()
    lib = os.path.join(root, "dino_amd", "lib", "libdinoseg_hip_asan.so")
    assert os.path.exists(rt) and os.path.exists(lib)
    env = dict(os.environ, LD_PRELOAD=rt, DINOSEG_LIB=lib, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "create_accepts or checks_frames_against_16 or checks_its_arguments"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2000:]
    assert "3 passed" in r.stdout


# --------------------------------------------------------------------------- fixtures against the oracle
def _oracle_logp(cfg, B, H, seed):
    W = O.to_torch(procedural_state_dict(cfg))
    with torch.no_grad():
        return O.dinoseg_forward(O.preprocess(synthetic_frames(B, H, seed=seed)), W, cfg.num_heads, 16)


SQUARE = [("g16_p16_vits16_L3", "480x480|", ViTConfig(n_blocks=3, patch=16, pos_grid=14)),
          ("g16_p16_vits16_L3", "224x224|", ViTConfig(n_blocks=3, patch=16, pos_grid=14)),
          ("g16_p16_vits16_L12_480x480", "", ViTConfig(n_blocks=12, patch=16, pos_grid=14)),
          ("g16_p16_vits16_L1_linear150_224x224", "", ViTConfig(n_blocks=1, head="linear", n_classes=150, patch=16, pos_grid=14))]


@pytest.mark.parametrize("name,pre,cfg", SQUARE, ids=[n + "-" + p for n, p, _ in SQUARE])
def test_oracle_with_patch16_equals_every_square_fixture(golden_dir, name, pre, cfg):
    g = _load(golden_dir, name)
    B, H, W = (int(v) for v in g[pre + "shape"])
    assert H == W
    lp = _oracle_logp(cfg, B, H, int(g[pre + "seed"]))
    assert lp.shape == (B * (H // 16) ** 2, cfg.n_classes)
    err = float((lp - torch.from_numpy(g[pre + "logp"])).abs().max())
    print(f"{name} {pre} oracle vs reference: {err:.3e}")
    assert err <= 1e-4
    assert np.array_equal(lp.argmax(1).numpy(), g[pre + "argmax"])


def test_every_forward_fixture_has_the_margin_the_parity_bar_needs(golden_dir):
    g = _load(golden_dir, "g16_p16_vits16_L3")
    for tag, rows in (("480x480", 2 * 900), ("480x640", 1200), ("224x224", 196), ("64x128", 32)):
        assert g[f"{tag}|logp"].shape == (rows, 7)
        assert float(g[f"{tag}|margin"].min()) >= MIN_MARGIN, tag
    for name, shape in (("g16_p16_vits16_L12_480x480", (900, 7)), ("g16_p16_vitb16_L2_240x320", (300, 7)),
                        ("g16_p16_vits16_L1_linear150_224x224", (196, 150))):
        g = _load(golden_dir, name)
        assert g["logp"].shape == shape and float(g["margin"].min()) >= MIN_MARGIN, name


def test_fixture_sizes(golden_dir):
    files = [f for f in os.listdir(golden_dir) if f.startswith("g16_p16_")]
    assert len(files) == 7
    sizes = [os.path.getsize(os.path.join(golden_dir, f)) for f in files]
    assert max(sizes) < 256 * 1024 and sum(sizes) < 1024 * 1024


def test_backbone_fixture_matches_the_oracle(golden_dir):
    """64 x 128 is a rectangle, which the square oracle does not take; its position rows do (the square grids), and 14 x 14 is the
    stored grid itself."""
    g = _load(golden_dir, "g16_p16_backbone_64x128")
    cfg = ViTConfig(n_blocks=3, patch=16, pos_grid=14)
    pe = torch.from_numpy(procedural_state_dict(cfg)["dino.pos_embed"])
    assert np.array_equal(g["pos|14x14"], pe[0, :, :8].numpy())
    got = O.resample_pos_embed(pe, 30)
    assert float((got[0, :, :8] - torch.from_numpy(g["pos|30x30"])).abs().max()) <= 2e-6
    assert g["tokens"].shape == (1, 33, 384) and g["attn"].shape == (6, 33, 33) and g["inter2"].shape == (2, 1, 33, 384)
    assert g["mask_emb"].shape == (3, 384) and g["mask_attn"].shape == (1, 6, 3, 33)

