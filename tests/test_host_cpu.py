"""CPU tests of the host side: C-ABI library loads and exports every declared symbol, the DINOSeg mirror
keeps the reference's surface (state_dict keys, ValueError text, checkpoint round trip) and fails loudly
without a GPU (no CPU fallback)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.ckpt import read_checkpoint, save_checkpoint
from dino_amd.weights import synthetic_frames, tensor_shapes


def test_library_exports_every_header_symbol():
    lib = capi.lib()
    declared = capi.header_symbols()
    assert len(declared) >= 17
    assert set(declared) == set(capi.SIGNATURES), "capi.SIGNATURES must mirror include/dinoseg.h"
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.dinoseg_version() >= 100


def test_backward_op_entries_refuse_bad_shapes_without_gpu():
    """The stand-alone backward entries check their shapes before they touch the device (no pointer is dereferenced)."""
    lib = capi.lib()
    fake = 256      # never dereferenced: every call below is refused on the host
    # gemm_tn multiplies whole 128-column tiles of X
    assert lib.dinoseg_op_gemm_tn(fake, 0, 64, fake, 0, 128, 33, 7, 100, 1, 1, fake, fake, 100, 100, None, None) == -1
    assert "gemm_tn: bad shape M=33 N=7 Kc=100 ksplit=1 planes=1" in capi.last_error()
    assert lib.dinoseg_op_gemm_tn(fake, 0, 64, fake, 0, 128, 33, 7, 128, 1, 0, fake, fake, 128, 128, None, None) == -1
    assert "gemm_tn: bad shape" in capi.last_error()
    assert lib.dinoseg_op_gemm_tn(fake, 0, 64, fake, 0, 128, 33, 7, 128, 1, 1, fake, fake, 99, 100, None, None) == -1
    assert "bad output columns (k_cols=100 Kc=128 ldw=99)" in capi.last_error()
    assert lib.dinoseg_op_gemm_tn(fake, 0, 64, fake, 0, 128, 33, 7, 128, 1, 1, None, fake, 128, 128, None, None) == -1
    assert "dinoseg_op_gemm_tn: part is required" in capi.last_error()
    # the wide log-softmax backward stores column pairs: an odd d-logits width is refused
    assert lib.dinoseg_op_nll_loss_grad(fake, None, fake, 4, 33, None, None, None, fake, 4 * 65, 65, None) == -1
    assert "nll_loss: d logits planes need an even width >= C (C=33 ldz=65)" in capi.last_error()
    assert lib.dinoseg_op_nll_loss_grad(fake, fake, fake, 4, 7, fake, fake, fake, fake, 4 * 64, 64, None) == -1
    assert "needs exactly one of labels" in capi.last_error()
    # the backward GEMM takes the backward epilogues only; the activation derivatives need their saved operand
    assert lib.dinoseg_op_gemm_bwd(fake, 0, 64, fake, 0, 33, 128, 64, 1, 2, None, 0, fake, 0, 128, fake, 0, None) == -1
    assert "epi 2 is not a backward epilogue" in capi.last_error()
    assert lib.dinoseg_op_gemm_bwd(fake, 0, 64, fake, 0, 33, 128, 64, 1, 8, None, 0, fake, 0, 128, None, 0, None) == -1
    assert "epi 8 needs aux_in" in capi.last_error()
    assert lib.dinoseg_op_gemm_bwd(fake, 0, 64, fake, 0, 33, 100, 64, 1, 6, None, 0, fake, 0, 128, None, 0, None) == -1
    assert "gemm: unsupported shape M=33 N=100 K=64" in capi.last_error()
    # the narrow-layer route: the transposed planes must hold round_up(N, 128) x m_pad
    assert lib.dinoseg_op_wgrad_nt(None, fake, 0, 384, fake, 0, 192, 100, 384, 192, 1, 0, 0, 1, fake, fake, 384 * 64, 128,
                                   None, fake, None, None) == -1
    assert "dinoseg_op_wgrad_nt: bad argument (M=100 N=384 K=192 m_pad=128 ksplit=1)" in capi.last_error()
    assert lib.dinoseg_op_pos_resample_bwd_hw(fake, 28, 384, 0, 60, fake, fake, None) == -1
    assert "bad shape g=28 D=384 oh=0 ow=60" in capi.last_error()


def test_attention_backward_entry_refuses_bad_shapes_without_gpu():
    """dinoseg_op_attention_bwd: npad must be a multiple of 64 and at least ntok, planes 1 or 2 -- refused before any launch."""
    lib = capi.lib()
    fake = 256      # never dereferenced: every call below is refused on the host

    def call(ntok, npad, planes):
        return lib.dinoseg_op_attention_bwd(fake, fake, fake, 2 * npad * 64, fake, fake, ntok * 128, fake, fake, fake, ntok * 384, 1, 2, ntok,
                                            npad, planes, None)
    assert call(65, 100, 1) == -1
    assert "attention_bwd: npad=100 must be a multiple of 64 and >= ntok=65" in capi.last_error()
    assert call(65, 64, 2) == -1
    assert "attention_bwd: npad=64 must be a multiple of 64 and >= ntok=65" in capi.last_error()
    for planes in (0, 3):
        assert call(65, 128, planes) == -1
        assert "attention_bwd: planes must be 1 or 2" in capi.last_error()


def test_helper_op_entries_refuse_bad_arguments_without_gpu():
    """The stand-alone entries of the helper kernels refuse null pointers and negative sizes on the host, with a message."""
    lib = capi.lib()
    fake = 256      # never dereferenced: every call below is refused on the host
    assert lib.dinoseg_op_attn_probs(fake, None, 0, 1, 1, 2, 16, 64, fake, None) == -1
    assert "dinoseg_op_attn_probs: null pointer" in capi.last_error()
    assert lib.dinoseg_op_attn_probs(fake, fake, 0, 1, 1, 2, -16, 64, fake, None) == -1
    assert "dinoseg_op_attn_probs: bad argument (planes=1 B=1 heads=2 ntok=-16 npad=64" in capi.last_error()
    assert lib.dinoseg_op_attn_probs(fake, fake, 100, 2, 1, 2, 16, 64, fake, None) == -1      # a lo plane inside the hi plane
    assert "qkv_plane=100" in capi.last_error()
    assert lib.dinoseg_op_cls_mask_attn(fake, fake, fake, 0, 1, 2, 65, 128, None, 3, fake, 0, None, None) == -1
    assert "dinoseg_op_cls_mask_attn: null pointer" in capi.last_error()
    assert lib.dinoseg_op_cls_mask_attn(fake, fake, fake, 0, 1, 2, 65, 64, fake, 3, fake, 0, None, None) == -1      # npad < ntok
    assert "dinoseg_op_cls_mask_attn: bad argument (planes=1 heads=2 ntok=65 npad=64 n_masks=3" in capi.last_error()
    assert lib.dinoseg_op_cls_mask_attn(fake, fake, fake, 0, 1, 2, 15361, 15424, fake, 1, fake, 0, None, None) == -1
    assert "cls_mask_attn: 15361 tokens exceed the LDS score buffer" in capi.last_error()
    assert lib.dinoseg_op_cls_rows(fake, fake, None, 1, 2, 128, None) == -1
    assert "dinoseg_op_cls_rows: null pointer" in capi.last_error()
    assert lib.dinoseg_op_cls_rows(fake, fake, fake, -1, 2, 128, None) == -1
    assert "dinoseg_op_cls_rows: bad shape B=-1 ntok=2 D=128" in capi.last_error()
    assert lib.dinoseg_op_broadcast_row0(None, 128, 3, None) == -1
    assert "dinoseg_op_broadcast_row0: null pointer" in capi.last_error()
    assert lib.dinoseg_op_broadcast_row0(fake, 128, -3, None) == -1
    assert "dinoseg_op_broadcast_row0: bad shape D=128 n=-3" in capi.last_error()
    assert lib.dinoseg_op_broadcast_row0(fake, 128, 0, None) == 0            # no rows to fill: legal, nothing is launched
    assert lib.dinoseg_op_batch_sum_rows(fake, 2, 3, 128, None, None) == -1
    assert "dinoseg_op_batch_sum_rows: null pointer" in capi.last_error()
    assert lib.dinoseg_op_batch_sum_rows(fake, 2, -3, 128, fake, None) == -1
    assert "dinoseg_op_batch_sum_rows: bad shape B=2 ntok=-3 D=128" in capi.last_error()
    one = lambda v: (ctypes.c_int32 * 1)(v)
    ptr1, plane1 = (ctypes.c_void_p * 1)(fake), (ctypes.c_int64 * 1)(0)
    assert lib.dinoseg_op_multi_pack(-1, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert "dinoseg_op_multi_pack: bad argument" in capi.last_error()
    assert lib.dinoseg_op_multi_pack(1, ptr1, ptr1, plane1, one(-4), one(4), one(64), one(64), one(1), one(0), one(0), None) == -1
    assert "dinoseg_op_multi_pack: bad job 0 (rows=-4 cols=4 rows_pad=64 cols_pad=64 planes=1" in capi.last_error()
    assert lib.dinoseg_op_multi_pack(1, ptr1, (ctypes.c_void_p * 1)(None), plane1, one(4), one(4), one(64), one(64), one(1), one(0), one(0), None) == -1
    assert "dinoseg_op_multi_pack: null pointer at job 0" in capi.last_error()
    assert lib.dinoseg_op_multi_pack(0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert lib.dinoseg_op_multi_pack(1, (ctypes.c_void_p * 1)(None), (ctypes.c_void_p * 1)(None), plane1, one(0), one(0), one(0), one(0), one(1),
                                     one(0), one(0), None) == 0              # an empty job: legal, nothing is launched
    assert lib.dinoseg_op_multi_zero(1, (ctypes.c_void_p * 1)(None), (ctypes.c_int64 * 1)(4), None) == -1
    assert "dinoseg_op_multi_zero: null pointer or negative size at tensor 0" in capi.last_error()
    assert lib.dinoseg_op_multi_zero(1, ptr1, (ctypes.c_int64 * 1)(-4), None) == -1
    assert "dinoseg_op_multi_zero: null pointer or negative size at tensor 0" in capi.last_error()
    assert lib.dinoseg_op_multi_zero(-1, None, None, None) == -1
    assert "dinoseg_op_multi_zero: bad argument" in capi.last_error()
    assert lib.dinoseg_op_multi_zero(1, ptr1, (ctypes.c_int64 * 1)(0), None) == 0           # an empty tensor: legal
    assert lib.dinoseg_op_multi_zero(0, None, None, None) == 0


def test_handle_lifecycle_and_errors_without_gpu():
    lib = capi.lib()
    h = ctypes.c_void_p()
    bad = capi.Config(100, 2, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.BF16)
    assert lib.dinoseg_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    assert "unsupported config" in capi.last_error()
    cfg = capi.Config(384, 6, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, capi.BF16X3)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.dinoseg_workspace_bytes(h, 1, 480) > 3601 * 384 * 4
    assert lib.dinoseg_workspace_bytes(h, 1, 250) == -1
    assert lib.dinoseg_prepare_resolution(h, 250, None) == -1
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        capi.check(-1)
    # strict binding: unknown key and wrong shape are rejected
    buf = (ctypes.c_float * 4)()
    shape = (ctypes.c_int64 * 1)(4)
    assert lib.dinoseg_bind_weight(h, b"dino.nope", ctypes.addressof(buf), shape, 1) == -1
    assert lib.dinoseg_bind_weight(h, b"dino.norm.weight", ctypes.addressof(buf), shape, 1) == -1
    assert lib.dinoseg_refresh_weights(h, None) == -3          # missing keys
    assert "missing key" in capi.last_error()
    assert lib.dinoseg_state_generation(h) == 0                # nothing allocated yet
    assert lib.dinoseg_destroy(h) == 0
    # the four precisions (include/dinoseg.h) create a handle; anything else is refused; the process-wide switches validate their values
    for prec in (capi.BF16, capi.BF16X3, capi.FP16, capi.FP16X3):
        cfg = capi.Config(384, 6, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, prec)
        assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and lib.dinoseg_destroy(h) == 0
    cfg = capi.Config(384, 6, 1, 8, 4, 7, capi.HEAD_MLP, 28, 1e-6, 4)
    assert lib.dinoseg_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    with dino_amd.options():
        assert lib.dinoseg_set_option(b"op_fmt", 2) == -1 and "op_fmt" in capi.last_error()
        assert lib.dinoseg_set_option(b"op_fmt", 0) == 0 and lib.dinoseg_set_option(b"mlp_variant", 1) == 0
        assert lib.dinoseg_set_option(b"no_such_option", 1) == -1
    assert set(dino_amd.dinoseg._PRECISIONS) == {"bf16", "bf16x3", "fp16", "fp16x3"}
    with pytest.raises(ValueError, match="precision"):
        DINOSeg(precision="fp32")


# Every key of dinoseg_set_option with its default: the one place outside dino_amd/csrc/kernels.h (struct Options) where the defaults
# stand.  Everything else reads them (dino_amd.get_option) or restores what it found (dino_amd.options).
KERNELS_H_DEFAULTS = {
    "gemm_ln": 1, "gemm_big": 1, "gemm_dbg": 0, "attn_dbg": 0, "mlp_fused": 1, "mlp_fused_min_rows": 12000, "mlp_fused3_min_rows": 10000,
    "mlp_stagger": 0, "mlp_grid": 0, "qkv_fused": 0, "mlp_fused4": 0, "qkv_fused4": 1, "qkv_fused3": 1, "gemm_rs": 3,
    "gemm_rs_min_rows": 24000, "gemm_rs_ln": 1, "proj_fused": 1, "streams": 2, "split_min": 8, "route_ab": 0, "fp16_patch_planes": 1,
    "op_v_bf16": 0, "op_fmt": 0, "deterministic": 0, "train_streams": 2, "splitk_tiles": 512, "attn_variant": 66571,       # bits 0, 1, 3, 10 and 16
    "mlp_variant": 0,
}
OPTION_FLAGS = ("op_v_bf16", "deterministic", "gemm_rs_ln", "qkv_fused3", "qkv_fused4", "mlp_fused4")      # stored as 0 / 1


def _get(key):
    """(return code, value) of dinoseg_get_option; the value starts as a sentinel"""
    out = ctypes.c_int32(-77)
    return capi.lib().dinoseg_get_option(key, ctypes.byref(out)), out.value


def test_option_get_reads_what_set_stored():
    """dinoseg_get_option returns the stored, normalised value of every key."""
    lib = capi.lib()
    before = {k: dino_amd.get_option(k) for k in dino_amd.option_names()}
    with dino_amd.options():
        for name in dino_amd.option_names():
            key = name.encode()
            for v in ((0, 1) if name == "op_fmt" else (0, 1, 2, 1000, -3)):
                assert lib.dinoseg_set_option(key, v) == 0, (name, v)
                want = {"mlp_variant": 0, "gemm_rs": v & 7, "split_min": max(v, 2), "fp16_patch_planes": 1 if v == 1 else 2}.get(
                    name, int(v != 0) if name in OPTION_FLAGS else v)
                assert _get(key) == (0, want), (name, v)
        for name, v, want in (("deterministic", 5, 1), ("split_min", 1, 2), ("gemm_rs", 15, 7), ("fp16_patch_planes", 3, 2),
                              ("mlp_variant", 9, 0)):
            assert lib.dinoseg_set_option(name.encode(), v) == 0 and _get(name.encode()) == (0, want), name
        assert lib.dinoseg_set_option(b"op_fmt", 1) == 0
        assert lib.dinoseg_set_option(b"op_fmt", 2) == -1 and "op_fmt" in capi.last_error()
        assert _get(b"op_fmt") == (0, 1)                      # a refused value stores nothing
    assert {k: dino_amd.get_option(k) for k in dino_amd.option_names()} == before


def test_option_get_refusals():
    lib = capi.lib()
    assert _get(b"no_such_option") == (-1, -77)               # the output is untouched
    assert "dinoseg_get_option: unknown key 'no_such_option'" in capi.last_error()
    assert _get(None) == (-1, -77)
    assert "dinoseg_get_option: null argument" in capi.last_error()
    assert lib.dinoseg_get_option(b"streams", None) == -1
    assert "dinoseg_get_option: null argument" in capi.last_error()
    with pytest.raises(capi.DinosegError, match="no_such_option"):
        dino_amd.get_option("no_such_option")


def test_option_enumeration():
    """dinoseg_option_name walks the table: 28 unique names, NULL on both sides, each accepted by get and set and documented."""
    lib = capi.lib()
    names = dino_amd.option_names()
    assert len(names) == 28 and len(set(names)) == 28
    assert lib.dinoseg_option_name(-1) is None and lib.dinoseg_option_name(len(names)) is None
    assert [lib.dinoseg_option_name(i).decode() for i in range(len(names))] == names
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    comment = text[text.index("/* Process-wide switches."):text.index("int dinoseg_set_option(")]
    for name in names:
        rc, value = _get(name.encode())
        assert rc == 0 and lib.dinoseg_set_option(name.encode(), value) == 0, name
        assert f'"{name}"' in comment, f"include/dinoseg.h: the dinoseg_set_option comment does not name {name}"


def test_option_defaults_in_a_fresh_process():
    """A process that has set nothing reads KERNELS_H_DEFAULTS, key by key (a changed default in kernels.h is an edit of that table)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import json, dino_amd; print(json.dumps({k: dino_amd.get_option(k) for k in dino_amd.option_names()}))"
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(KERNELS_H_DEFAULTS) == 28 and got == KERNELS_H_DEFAULTS


def test_option_scope_restores_every_key():
    """dino_amd.options: after a normal body, after a body that raises, after a bare set_option of a key it was not given, nested on
    one key, and when one of its own values is refused."""
    state = lambda: {k: dino_amd.get_option(k) for k in dino_amd.option_names()}
    outside = state()
    with dino_amd.options(streams=1):
        before = state()
        with dino_amd.options(streams=3, deterministic=1):
            assert (dino_amd.get_option("streams"), dino_amd.get_option("deterministic")) == (3, 1)
        assert state() == before
        with pytest.raises(KeyError):
            with dino_amd.options(gemm_ln=0):
                assert dino_amd.get_option("gemm_ln") == 0
                raise KeyError("body")
        assert state() == before
        with dino_amd.options(gemm_ln=2):
            dino_amd.set_option("mlp_fused", 0)
            dino_amd.set_option("gemm_ln", 0)
        assert state() == before
        with dino_amd.options(split_min=4):
            with dino_amd.options(split_min=6):
                assert dino_amd.get_option("split_min") == 6
            assert dino_amd.get_option("split_min") == 4
        assert state() == before
        with pytest.raises(capi.DinosegError, match="op_fmt"):
            with dino_amd.options(gemm_big=0, op_fmt=2, gemm_ln=0):
                raise AssertionError("the body must not run")
        assert state() == before
    assert state() == outside


def test_native_name_and_shape_table_matches_tensor_shapes():
    """The library's own name / shape table (what dinoseg_bind_weight and dinoseg_bind_grad accept) against
    dino_amd.weights.tensor_shapes, key by key, without a GPU: a host pointer gets as far as "is not a device pointer" only when the
    name and the shape were accepted; the last dimension + 1 is a shape mismatch; every key names a gradient slot, NULL unbinds it;
    an unknown key is refused by both."""
    lib = capi.lib()
    configs = [ViTConfig(n_blocks=2),                                                                # ViT-S/8, MLP head, C = 7
               ViTConfig(embed_dim=768, num_heads=12, mlp_ratio=6, n_blocks=2, head="linear", n_classes=150),
               ViTConfig(embed_dim=128, num_heads=2, n_blocks=2),                                    # the suite's TINY
               ViTConfig(patch=16, pos_grid=14, n_blocks=1, n_classes=40)]
    buf = (ctypes.c_float * 4)()
    for cfg in configs:
        h = ctypes.c_void_p()
        native = capi.Config(cfg.embed_dim, cfg.num_heads, cfg.n_blocks, cfg.patch, cfg.mlp_ratio, cfg.n_classes,
                             capi.HEAD_MLP if cfg.head == "mlp" else capi.HEAD_LINEAR, cfg.pos_grid, cfg.ln_eps, capi.BF16X3)
        assert lib.dinoseg_create(ctypes.byref(native), ctypes.byref(h)) == 0
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
            assert lib.dinoseg_bind_grad(h, b"dino.nope", None) == -1
            assert "unexpected key" in capi.last_error()
            assert lib.dinoseg_bind_weight(h, b"dino.nope", ctypes.addressof(buf), (ctypes.c_int64 * 1)(4), 1) == -1
            assert "unexpected key" in capi.last_error()
        finally:
            assert lib.dinoseg_destroy(h) == 0


def test_state_dict_keys_match_reference_schema():
    for head, L in (("mlp", 3), ("linear", 1)):
        m = DINOSeg(head=head, n_blocks=L)
        want = tensor_shapes(ViTConfig(n_blocks=L, head=head))
        got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert got == dict(want)
    assert len(DINOSeg(head="mlp", n_blocks=3).state_dict()) == 48      # 48 tensors for L=3
    assert sum(v.numel() for v in DINOSeg(head="mlp", n_blocks=3).state_dict().values()) == 5797903
    # an arch given as a ViTConfig keeps its MLP width (the native handle is created from self.cfg)
    wide = ViTConfig(embed_dim=768, num_heads=12, mlp_ratio=6, n_blocks=2)
    m = DINOSeg(head="mlp", n_blocks=2, arch=wide)
    assert m.cfg.mlp_ratio == 6
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(tensor_shapes(wide))


def test_set_resolution_and_no_cpu_fallback():
    m = DINOSeg(head="mlp", n_blocks=1)
    with pytest.raises(ValueError, match="Resolution should be a multiple of 8."):
        m.set_resolution(250)
    m.set_resolution(240)
    assert m.resolution == 240 and m.transforms.resolution == 240
    assert m.device.type == "cpu"
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.predict(np.zeros((240, 240, 3), np.uint8))


def test_transforms_match_oracle_preprocess():
    from oracle import dinoseg_oracle as O
    fr = synthetic_frames(1, 64, seed=2)
    t = dino_amd.get_transforms(64)(image=fr[0])["image"]
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 64, 64)
    assert torch.equal(t, O.preprocess(fr)[0])
    big = dino_amd.get_transforms(32).resize(fr[0])
    assert big.shape == (32, 32, 3) and big.dtype == np.uint8


def test_checkpoint_round_trip(tmp_path):
    sd = procedural_state_dict(ViTConfig(n_blocks=2))
    m = DINOSeg(data_path="d", write_path="w", head="mlp", n_blocks=2, optimizer=torch.optim.Adam, lr=1e-3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    path = os.path.join(tmp_path, "two_block.ckpt")
    save_checkpoint(m, path, epoch=3)
    ck = read_checkpoint(path)
    assert ck["pytorch-lightning_version"] == "1.5.10" and ck["hyper_parameters"]["n_blocks"] == 2
    m2 = DINOSeg.load_from_checkpoint(path)
    assert m2.n_blocks == 2 and m2.head == "mlp" and m2.optimizer is torch.optim.Adam and m2.lr == 1e-3
    for k, v in m2.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
    with pytest.raises(RuntimeError):        # strict load, as the reference
        m2.load_state_dict({"dino.cls_token": torch.zeros(1, 1, 384)}, strict=True)


def test_checkpoint_with_unimportable_hyperparameters(tmp_path):
    """PL checkpoints pickle objects of packages that are absent here (comet logger...): they must not block loading."""
    import pickle
    import types
    fake = types.ModuleType("comet_like_pkg")

    class Logger:
        def __init__(self):
            self.key = "secret"
    Logger.__module__ = "comet_like_pkg"
    Logger.__qualname__ = "Logger"
    fake.Logger = Logger
    import sys
    sys.modules["comet_like_pkg"] = fake
    sd = procedural_state_dict(ViTConfig(n_blocks=1))
    path = os.path.join(tmp_path, "pl.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()},
                "hyper_parameters": {"head": "mlp", "n_blocks": 1, "comet_logger": Logger(), "data_path": "x",
                                     "write_path": "y", "optimizer": torch.optim.AdamW}}, path, pickle_module=pickle)
    del sys.modules["comet_like_pkg"]
    m = DINOSeg.load_from_checkpoint(path)
    assert m.n_blocks == 1 and m.comet_logger is None and m.optimizer is torch.optim.AdamW


def test_resize_mirror_matches_scalar_restatement():
    """dino_amd.preprocess (host mirror of cv2.INTER_LINEAR on uint8) against the pixel-at-a-time restatement in oracle/:
    upscale, downscale, the exact-2x INTER_AREA switch, 1-pixel sources and a known 2x ramp (taps 0.25 / 0.75)."""
    from dino_amd.preprocess import resize_linear_u8
    from oracle.resize_oracle import resize_linear_u8 as ref
    rng = np.random.default_rng(0)
    for sh, sw, dh, dw in [(5, 7, 8, 8), (12, 16, 8, 8), (16, 16, 8, 8), (3, 3, 16, 16), (1, 1, 4, 4), (48, 64, 40, 40), (9, 4, 16, 24)]:
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        assert np.array_equal(resize_linear_u8(img, dh, dw), ref(img, dh, dw)), (sh, sw, dh, dw)
    ramp = np.tile(np.array([0, 16, 32, 48], dtype=np.uint8)[None, :, None], (2, 1, 3))
    assert resize_linear_u8(ramp, 2, 8)[0, :, 0].tolist() == [0, 4, 12, 20, 28, 36, 44, 48]
    const = np.full((10, 13, 3), 200, np.uint8)
    assert np.unique(resize_linear_u8(const, 16, 16)).tolist() == [200]
    same = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    assert resize_linear_u8(same, 8, 8) is not None and np.array_equal(resize_linear_u8(same, 8, 8), same)


def test_fast_signature_sees_every_kind_of_weight_change():
    """The cheap per-call check of DINOSeg._sync_weights (no state_dict walk) must notice everything the full signature does:
    in-place updates, optimizer steps, load_state_dict, replaced Parameters / sub-modules, added entries, invalidate_weights()."""
    import copy
    import pickle
    m = DINOSeg(head="mlp", n_blocks=2)
    assert m._fast_signature() is None                       # nothing indexed before the first bind
    m._fast_index = m._build_fast_index()
    base = m._fast_signature()
    assert base is not None and m._fast_signature() == base  # stable while nothing changes
    with torch.no_grad():
        m.clf.layer_3.bias.add_(1.0)
    assert m._fast_signature() != base
    base = m._fast_signature()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    assert m._fast_signature() != base
    base = m._fast_signature()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(m.cfg).items()})
    assert m._fast_signature() != base
    base = m._fast_signature()
    m.dino.norm.bias.data = torch.ones_like(m.dino.norm.bias)          # new storage, same Parameter, version unchanged
    assert m._fast_signature() != base
    m._fast_index = m._build_fast_index()
    base = m._fast_signature()
    m.clf.layer_1.bias = torch.nn.Parameter(torch.zeros(200))          # replaced Parameter object
    assert m._fast_signature() is None
    m._fast_index = m._build_fast_index()
    m.dino.blocks[1] = copy.deepcopy(m.dino.blocks[0])                 # replaced sub-module
    assert m._fast_signature() is None
    m._fast_index = m._build_fast_index()
    m.clf.register_buffer("extra", torch.zeros(1))                     # added entry
    assert m._fast_signature() is None
    m._fast_index = m._build_fast_index()
    base = m._fast_signature()
    m.invalidate_weights()
    assert m._fast_signature() != base
    m2 = pickle.loads(pickle.dumps(m))                                  # the index is process state: not pickled
    assert "_fast_index" not in m2.__dict__ and m2._fast_signature() is None


def test_resize_restatement_against_an_independent_bilinear():
    """cv2 is not in this image (oracle/resize_oracle.py: parity unpinned), so the restatement is held against an INDEPENDENT
    implementation of the same sampling rule: torch's float64 bilinear (align_corners=False = cv2's (dx + 0.5) * scale - 0.5 with edge
    clamping, no antialiasing; 'area' for the exact-2x case, where cv2 switches to INTER_AREA).  cv2's uint8 path rounds its taps to
    11 bits and truncates intermediate sums, so the two may differ by one grey level, never by more."""
    import torch.nn.functional as F
    from dino_amd.preprocess import resize_linear_u8
    rng = np.random.default_rng(1)
    for sh, sw, dh, dw in [(5, 7, 8, 8), (12, 16, 8, 8), (3, 3, 16, 16), (48, 64, 40, 40), (9, 4, 16, 24), (300, 400, 240, 240),
                           (480, 640, 480, 480), (16, 16, 8, 8), (96, 128, 48, 64)]:
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        x = torch.from_numpy(img).permute(2, 0, 1)[None].double()
        if sh == 2 * dh and sw == 2 * dw:
            ref = F.interpolate(x, size=(dh, dw), mode="area")
        else:
            ref = F.interpolate(x, size=(dh, dw), mode="bilinear", align_corners=False, antialias=False)
        ref = ref[0].permute(1, 2, 0).numpy()
        got = resize_linear_u8(img, dh, dw).astype(np.float64)
        d = got - ref
        assert np.abs(d).max() <= 1.0 + 1e-9, (sh, sw, dh, dw, np.abs(d).max())
        # (rounding to a grey level: mean |d| about 0.25; cv2's vertical pass truncates twice -- ((b0 * (S0 >> 4)) >> 16) + ... -- which
        #  shows as a bias of up to about +-0.1 grey levels against exact arithmetic, by the tap values)
        assert abs(d.mean()) < 0.2 and np.abs(d).mean() < 0.3, (sh, sw, dh, dw, d.mean(), np.abs(d).mean())


def test_host_side_under_address_sanitizer():
    """SURVEY.md section 5 (sanitizers): the host side of the C-ABI library built with -fsanitize=address (`make -C dino_amd/csrc asan`:
    device code objects as usual, every host function instrumented) runs this file's C-ABI tests -- symbol table, handle lifecycle,
    refused arguments, strict binding, option validation -- in a child process with the ASan runtime preloaded.  Build container only
    (needs hipcc; the GPU box never runs a sanitizer build)."""
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
    syms = subprocess.run(["nm", "-D", lib], capture_output=True, text=True).stdout
    assert "__asan_init" in syms, "the library is not instrumented"
    env = dict(os.environ, LD_PRELOAD=rt, DINOSEG_LIB=lib, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "exports or lifecycle or no_cpu_fallback"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2000:]
    assert "3 passed" in r.stdout


def test_generated_attention_bodies_are_current():
    """dino_amd/csrc/attention_za_gen.inc is what tools/gen_attn_asm.py writes (the generator re-derives every body -- register map,
    pipeline order, counted LDS waits, with its own consistency assertions at every label -- and compares with the committed file)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_attn_asm.py"), "--check"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
