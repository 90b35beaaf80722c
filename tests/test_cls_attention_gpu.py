"""The CLS attention maps on the GPU (-m gpu): dinoseg_op_cls_attention alone against an fp64 softmax of the operands it saw and
against the exact restatements of tests/attention_util.py, then DINOSeg.cls_attention against the reference's golden rows, against
get_last_selfattention of the same model in every precision, and against the CPU oracle at 480 x 480.

Bars.  Probabilities: the suite's rule for the helper kernels (tests/test_helper_ops_gpu.py): 4 x the error of the same formula in
float32 on the CPU + 2^-23, errors as max |err| / max |ref|, one `helper_ops` line per case.  The threshold and the enlargement are
exact: `keep` must equal the integer rule applied to the kernel's OWN grid-size probabilities at every patch, and every enlarged
output must be the nearest gather of the grid-size one bit for bit.  The model: 2e-4, the bar test_g10_last_selfattention and
test_side_paths_at_480 hold the same numbers to."""
import dataclasses

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames
from oracle import dinoseg_oracle as O
from tests import attention_util as U
from tests import test_helper_ops_gpu as H
from tests.gpu_util import untouched

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
LOG2E = H.LOG2E
THRESHOLDS = (0.1, 0.6, 0.9)
GUARD8 = 0xAB                           # guard pattern of the uint8 outputs
TINY = ViTConfig(embed_dim=128, num_heads=2, n_blocks=2)


class Operands:
    """Q (pre-scaled, log2 domain) and K planes [planes, G * npad, 64] with NaN in the pad rows, as test_attn_probs builds them, and
    the fp64 values the kernel sees"""

    def __init__(self, B, heads, hp, wp, planes, fmt, seed, edit=None):
        self.B, self.heads, self.hp, self.wp, self.planes, self.fmt = B, heads, hp, wp, planes, fmt
        self.G, self.ntok = B * heads, hp * wp + 1
        self.npad = (self.ntok + 63) // 64 * 64
        g_ = np.random.default_rng(seed)
        G, ntok = self.G, self.ntok
        Q = 1.5 * H.rng_normal(g_, (G, ntok, 64)) + H.ramp(64, 0.004)[None, None, :] + (H.ramp(ntok, 1.0) % 13 / 40)[None, :, None]
        K = 1.5 * H.rng_normal(g_, (G, ntok, 64)) - H.ramp(64, 0.003)[None, None, :] + H.ramp(G, 0.05)[:, None, None]
        if edit:
            edit(Q, K)
        self.qp, self.q64 = H._qkv_planes(Q * (0.125 * LOG2E), self.npad, planes, fmt)
        self.kp, self.k64 = H._qkv_planes(K, self.npad, planes, fmt)

    def run(self, OH, OW, threshold=None, want_attn=True, offset=0):
        """-> (attn fp32 [G, OH, OW] or None, keep uint8 [G, OH, OW] or None); guards checked.  offset: the outputs start that many
        elements into their allocations (off the 16-byte / 4-byte boundaries of the vector stores)"""
        n = self.G * OH * OW
        attn = torch.full((offset + n + 64,), float("nan"), device="cuda") if want_attn else None
        keep = torch.full((offset + n + 64,), GUARD8, dtype=torch.uint8, device="cuda") if threshold is not None else None
        with H.op_fmt(self.fmt):
            capi.check(capi.lib().dinoseg_op_cls_attention(
                self.qp.data_ptr(), self.kp.data_ptr(), self.G * self.npad * 64, self.planes, self.B, self.heads, self.ntok, self.npad,
                self.hp, self.wp, OH, OW, 0.0 if threshold is None else threshold,
                None if attn is None else attn.data_ptr() + 4 * offset, None if keep is None else keep.data_ptr() + offset, S()))
            torch.cuda.synchronize()
        if attn is not None:
            assert untouched(attn[:offset]) and untouched(attn[offset + n:]), "attn_out: exactly B x heads x OH x OW floats are written"
            attn = attn[offset:offset + n].reshape(self.G, OH, OW)
            assert bool(torch.isfinite(attn).all())
        if keep is not None:
            assert bool((keep[:offset] == GUARD8).all()) and bool((keep[offset + n:] == GUARD8).all()), "keep_out: exactly B x heads x OH x OW bytes"
            keep = keep[offset:offset + n].reshape(self.G, OH, OW)
            assert bool((keep <= 1).all())
        return attn, keep

    def reference(self):
        """the patches' probabilities [G, hp, wp]: fp64 on the device, and the same formula in float32 on the CPU"""
        def f(q, k):
            s = (k @ q[:, 0, :, None])[:, :, 0]                 # [G, ntok]: the CLS query against every key
            return H._softmax2(s)[:, 1:].reshape(self.G, self.hp, self.wp)
        r32 = f(self.q64.float().cpu(), self.k64.float().cpu())
        assert r32.dtype == torch.float32
        return f(self.q64, self.k64), r32


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


# (B, heads, hp, wp, planes, fmt, OH, OW): the smallest grid; odd grids at non-integer ratios; 65 tokens in npad 128; 257 and 197
# tokens with B > 1; 1025 tokens = one key beyond a full round of the workgroup's 1024 threads; the working grids 60 x 60 / 60 x 80 raw
# and at pixel resolution in both formats; 16 642 tokens = the first size whose scores need more than 64 KiB of LDS.  OW 1, 5, 11, 14,
# 129: one pixel per lane; the others: four
CASES = [
    (1, 1, 1, 1, 1, "bf16", 1, 1),
    (1, 1, 1, 1, 2, "fp16", 8, 8),
    (1, 2, 3, 5, 2, "bf16", 3, 5),
    (1, 2, 3, 5, 2, "bf16", 7, 11),
    (1, 2, 8, 8, 1, "fp16", 64, 64),
    (2, 3, 16, 16, 1, "fp16", 16, 16),
    (2, 3, 14, 14, 2, "bf16", 14, 14),
    (2, 3, 14, 14, 1, "bf16", 112, 112),
    (1, 2, 32, 32, 2, "fp16", 32, 32),
    (1, 2, 60, 60, 1, "fp16", 480, 480),
    (1, 2, 60, 60, 2, "bf16", 60, 60),
    (1, 2, 60, 80, 2, "fp16", 60, 80),
    (1, 2, 60, 80, 1, "bf16", 480, 640),
    (1, 1, 129, 129, 1, "fp16", 129, 129),
]


@pytest.mark.parametrize("B,heads,hp,wp,planes,fmt,OH,OW", CASES)
def test_op_probabilities_threshold_and_enlargement(cuda, B, heads, hp, wp, planes, fmt, OH, OW):
    ops = Operands(B, heads, hp, wp, planes, fmt, seed=6000 + hp * wp + planes + heads)
    case = f"B={B} heads={heads} {hp}x{wp} planes={planes} {fmt} -> {OH}x{OW}"
    a, _ = ops.run(hp, wp)
    ref, r32 = ops.reference()
    err = H.relerr(a, ref)
    assert err <= H.report("cls_attention", case, "probabilities", err, H.relerr(r32.cuda(), ref), H.ULP32)
    a2, _ = ops.run(hp, wp)
    assert same_bits(a, a2), "two runs give the same bits"
    a_np = a.cpu().numpy()
    keeps = {}
    for thr in THRESHOLDS:
        ak, k = ops.run(hp, wp, threshold=thr)
        assert same_bits(a, ak), "attn_out is the same with and without keep_out"
        want = U.keep_rule(a_np.reshape(ops.G, -1), thr).reshape(ops.G, hp, wp)
        got = k.cpu().numpy()
        assert np.array_equal(got, want), f"threshold {thr}: {int((got != want).sum())} patches differ from the integer rule"
        _, k_only = ops.run(hp, wp, threshold=thr, want_attn=False)
        assert torch.equal(k, k_only), "keep_out is the same with and without attn_out"
        keeps[thr] = got
    _, k2 = ops.run(hp, wp, threshold=0.6)
    assert np.array_equal(k2.cpu().numpy(), keeps[0.6]), "two runs give the same keep"
    if (OH, OW) != (hp, wp):
        want_a = torch.from_numpy(U.nearest_gather(a_np, OH, OW))
        for thr in THRESHOLDS:
            ae, ke = ops.run(OH, OW, threshold=thr)
            assert same_bits(ae.cpu(), want_a), "the enlarged attn is the nearest gather of the grid-size attn"
            assert np.array_equal(ke.cpu().numpy(), U.nearest_gather(keeps[thr], OH, OW)), f"the enlarged keep at {thr}"
        ae, _ = ops.run(OH, OW)
        assert same_bits(ae.cpu(), want_a)


def test_op_outputs_off_the_vector_boundaries(cuda):
    """OW % 4 == 0 with outputs one element into their allocations: the one-pixel-per-lane stores, the same bits"""
    ops = Operands(1, 2, 8, 8, 1, "fp16", seed=6100)
    a, k = ops.run(64, 64, threshold=0.6)
    a1, k1 = ops.run(64, 64, threshold=0.6, offset=1)
    assert same_bits(a, a1) and torch.equal(k, k1)


def test_op_one_late_key_dominates(cuda):
    hp, wp = 14, 14
    ntok = hp * wp + 1

    def spike(Q, K):
        K[:, ntok - 3] = Q[:, 0] * 4.0
    ops = Operands(2, 3, hp, wp, 1, "bf16", seed=6200, edit=spike)
    a, k = ops.run(hp, wp, threshold=0.1)
    flat = a.reshape(ops.G, -1)
    assert float(flat[:, ntok - 4].min()) > 0.99
    want = np.zeros((ops.G, ntok - 1), dtype=np.uint8)
    want[:, ntok - 4] = 1
    assert np.array_equal(k.reshape(ops.G, -1).cpu().numpy(), want), "at threshold 0.1 the dominating patch alone is kept"
    assert np.array_equal(want, U.keep_rule(flat.cpu().numpy(), 0.1))


def test_op_the_cls_key_dominates(cuda):
    """the patches share under 1 % of the mass: keep is decided on the patches' own total, not on 1"""
    hp, wp = 16, 16

    def cls_key(Q, K):
        K[:, 0] = Q[:, 0] * 0.8             # (in fp64 the patches of the two heads share 8.8e-6 and 1.0e-3 of the mass)
    ops = Operands(1, 2, hp, wp, 2, "fp16", seed=6300, edit=cls_key)
    ref, r32 = ops.reference()
    for thr in THRESHOLDS:
        a, k = ops.run(hp, wp, threshold=thr)
        flat = a.reshape(ops.G, -1)
        assert float(flat.sum(dim=1).max()) < 0.01
        got = k.reshape(ops.G, -1).cpu().numpy()
        assert np.array_equal(got, U.keep_rule(flat.cpu().numpy(), thr))
        assert 0 < int(got.sum()) < got.size
    err = H.relerr(a, ref)
    assert err <= H.report("cls_attention", "the CLS key dominates", "probabilities", err, H.relerr(r32.cuda(), ref), H.ULP32)


def test_op_duplicated_keys_tie(cuda):
    hp, wp = 16, 16
    rows = (7, 100, 256)                    # tokens: lanes of different groups, of different waves

    def dup(Q, K):
        K[:, rows[1]] = K[:, rows[0]]
        K[:, rows[2]] = K[:, rows[0]]
    ops = Operands(1, 2, hp, wp, 1, "fp16", seed=6400, edit=dup)
    seen = set()
    for thr in THRESHOLDS + (0.3, 0.5, 0.75, 0.97):
        a, k = ops.run(hp, wp, threshold=thr)
        flat, kf = a.reshape(ops.G, -1), k.reshape(ops.G, -1)
        for g in range(ops.G):
            p = [flat[g, r - 1] for r in rows]
            assert same_bits(p[0], p[1]) and same_bits(p[0], p[2]), "duplicated keys get bit-equal probabilities"
            kk = {int(kf[g, r - 1]) for r in rows}
            assert len(kk) == 1, f"threshold {thr}: a tied group is kept or dropped whole"
            seen |= kk
        assert np.array_equal(kf.cpu().numpy(), U.keep_rule(flat.cpu().numpy(), thr))
    assert seen == {0, 1}, "the thresholds put the group on both sides of the cut"


# ------------------------------------------------------------------------------------------------ the model
def build(cfg, precision):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0"), sd


def test_model_golden_rows(cuda, golden_dir):
    """the rows test_g10_last_selfattention compares, through cls_attention"""
    g = np.load(f"{golden_dir}/g10_last_selfattention.npz")
    m, _ = build(TINY, "bf16x3")
    x = O.preprocess(synthetic_frames(1, 64, seed=101)).cuda()
    a, keep = m.cls_attention(x, size=(8, 8))
    assert keep is None and tuple(a.shape) == (1, 2, 8, 8) and a.dtype == torch.float32
    e1 = float((a[0].cpu().reshape(2, 64) - torch.from_numpy(g["tiny_r64_full"][0, :, 0, 1:])).abs().max())
    m, _ = build(ViTConfig(n_blocks=3), "bf16x3")
    x = O.preprocess(synthetic_frames(1, 96, seed=102)).cuda()
    a = m.dino.cls_attention(x, size=(12, 12))[0]
    assert tuple(a.shape) == (1, 6, 12, 12)
    e2 = float((a[0].cpu().reshape(6, 144) - torch.from_numpy(g["vits8_L3_r96_cls_rows"][:, 1:])).abs().max())
    print(f"cls_attention golden rows: tiny {e1:.3e} vits8 L3 {e2:.3e}")
    assert e1 <= 2e-4 and e2 <= 2e-4


@pytest.mark.parametrize("precision,cfg", [(p, ViTConfig(n_blocks=2)) for p in ("bf16x3", "fp16x3", "fp16", "bf16")] +
                         [("fp16x3", dataclasses.replace(dino_amd.VIT_S16, n_blocks=1))],
                         ids=["bf16x3", "fp16x3", "fp16", "bf16", "patch16-fp16x3"])
def test_model_every_precision_matches_last_selfattention(cuda, precision, cfg):
    m, _ = build(cfg, precision)
    frames = synthetic_frames(2, 64, seed=640, w=128)
    x = O.preprocess(frames).cuda()
    hp, wp = 64 // cfg.patch, 128 // cfg.patch
    a = m.cls_attention(x, size=(hp, wp))[0]
    assert tuple(a.shape) == (2, cfg.num_heads, hp, wp)
    ref = m.get_last_selfattention(x)[:, :, 0, 1:].reshape(2, cfg.num_heads, hp, wp)
    e = float((a - ref).abs().max())
    a8 = m.cls_attention(torch.from_numpy(frames).cuda(), size=(hp, wp))[0]
    e8 = float((a8 - a).abs().max())
    print(f"cls_attention [{precision} patch {cfg.patch}] against get_last_selfattention {e:.3e}; uint8 against fp32 frames {e8:.3e}")
    assert e <= 2e-4 and e8 <= 2e-4


def test_model_at_480_against_the_oracle(cuda):
    o = H._oracle_480()
    cfg = o["cfg"]
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision="bf16x3", arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in o["sd"].items()}, strict=True)
    m.to("cuda:0")
    a = m.cls_attention(o["x"].cuda(), size=(60, 60))[0]
    assert tuple(a.shape) == (1, cfg.num_heads, 60, 60)
    e = float((a[0].cpu().reshape(cfg.num_heads, 3600) - o["attn"][0][:, 0, 1:]).abs().max())
    print(f"cls_attention 480x480 against the oracle's CLS row {e:.3e}")
    assert e <= 2e-4


def test_model_threshold_at_the_default_size(cuda):
    m, _ = build(ViTConfig(n_blocks=2), "fp16x3")
    B, Hf, Wf = 2, 64, 128
    frames = torch.from_numpy(synthetic_frames(B, Hf, seed=641, w=Wf)).cuda()
    a0, none = m.cls_attention(frames)
    a, keep = m.cls_attention(frames, threshold=0.6)
    assert none is None and keep.dtype == torch.uint8 and a.dtype == torch.float32
    assert tuple(a.shape) == tuple(keep.shape) == (B, 6, Hf, Wf)
    assert same_bits(a, a0), "attn is the same with and without a threshold"
    grid = m.cls_attention(frames, size=(8, 16))[0].cpu().numpy()
    assert np.array_equal(a.cpu().numpy().view(np.int32), U.nearest_gather(grid, Hf, Wf).view(np.int32))
    want = U.keep_rule(grid.reshape(B, 6, -1), 0.6).reshape(B, 6, 8, 16)
    assert np.array_equal(keep.cpu().numpy(), U.nearest_gather(want, Hf, Wf)), "keep is the integer rule on the grid, gathered, at every pixel"
    assert 0 < int(want.sum()) < want.size


def test_model_launch_is_timed_as_attention(cuda):
    """3 blocks: two attention launches of the blocks in front and the CLS launch count as `attention`; the forward stops there (one
    LayerNorm1 + qkv per block, no third projection / MLP, no head), and profiling changes no bit"""
    m, _ = build(ViTConfig(n_blocks=3), "fp16")
    frames = torch.from_numpy(synthetic_frames(2, 64, seed=642)).cuda()
    a0, k0 = m.cls_attention(frames, threshold=0.6)
    m.profile(2)
    try:
        a, k = m.cls_attention(frames, threshold=0.6)
        torch.cuda.synchronize()
        prof = m.profile_read()
    finally:
        m.profile(0)
    counts = {name: n for name, (_, n) in prof.items() if n}
    assert counts["attention"] == 3 and prof["attention"][0] > 0.0, counts
    assert "head" not in counts, counts
    assert same_bits(a, a0) and torch.equal(k, k0)
