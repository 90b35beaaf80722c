"""The image-guided iterative refinement on the device: dinoseg_op_refine_seed and dinoseg_op_refine_iterate against the fp64
restatement of the rule (tests/refine_util.py), the cases that must agree bit for bit, the edge-following property, containment,
the refusals, and the model-level methods against the operators applied to the forward's own log-probs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import VIT_S8, synthetic_frames
from tests import refine_util as R

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
DEFAULT = R.DEFAULT_DILATIONS

# (B, C, OH, OW, dilations)
CASES = [
    (1, 1, 1, 1, (1,)),                 # every tap is the pixel itself
    (2, 5, 8, 8, (1, 2)),
    (2, 9, 37, 61, DEFAULT),            # the largest dilation exceeds half the frame: it clamps on both sides
    (2, 3, 100, 131, DEFAULT),          # ragged tiles, halos crossing tile borders
    (1, 33, 40, 72, (1, 3, 24)),
    (1, 256, 24, 40, (2, 24)),          # the class limit, class passes
    (1, 7, 480, 640, DEFAULT),          # the robot camera's frame: in one test only
]
SMALL = [0, 1, 2, 3, 4, 5]
LABEL_EXCLUDED_CAP = 2e-3
PASSES = 3                              # the teacher-forced pass is the third
# one seed per case.  The undecided share of the fp64 restatement ALONE is 0 .. 1.4e-3 for these; on the small frames one pixel is
# 3e-4 .. 1e-3 of them, and the first seeds of cases 4 and 5 (204, 205) gave 2.4e-3 and 2.1e-3: they were changed, the cap was not.
SEEDS = [200, 201, 202, 203, 214, 215, 206]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """(state fp32 [B, C, OH, OW] = softmax(2 randn), (noise guide, block guide)) of case i, read-only"""
    B, C, OH, OW, _ = CASES[i]
    rng = np.random.default_rng(SEEDS[i])
    state = R.make_state(rng, B, C, OH, OW)
    guides = R.make_guides(rng, B, OH, OW)
    for a in (state,) + guides:
        a.setflags(write=False)
    return state, guides


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def dil_array(dil):
    return (ctypes.c_int32 * len(dil))(*dil)


def new_scratch(B, C, OH, OW):
    n = capi.lib().dinoseg_refine_scratch_bytes(B, C, OH, OW)
    assert n == 2 * B * C * OH * OW * 4
    return torch.full((2, B, C, OH, OW), float("nan"), dtype=torch.float32, device="cuda")


def seed_op(seed, kind, B, C, OH, OW, hp=0, wp=0, gain=1.0, scratch=None):
    scratch = new_scratch(B, C, OH, OW) if scratch is None else scratch
    capi.check(capi.lib().dinoseg_op_refine_seed(seed.data_ptr(), kind, B, C, OH, OW, hp, wp, gain, scratch.data_ptr(), S()))
    return scratch


def iterate(guide, scratch, dil, sigma=0.1, iters=1, want_labels=True, want_dense=True):
    """device tensors in, (labels or None, dense or None) out; reads half 0 of scratch"""
    _, B, C, OH, OW = scratch.shape
    labels = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda") if want_labels else None
    dense = torch.empty((B, C, OH, OW), dtype=torch.float32, device="cuda") if want_dense else None
    capi.check(capi.lib().dinoseg_op_refine_iterate(guide.data_ptr(), scratch.data_ptr(), B, C, OH, OW, dil_array(dil), len(dil), sigma, iters,
                                                    capi.ptr(labels), capi.ptr(dense), S()))
    return labels, dense


def from_state(state, guide, dil, sigma=0.1, iters=1, **kw):
    """`iters` passes from a state tensor [B, C, OH, OW] on the device (copied into half 0 of a fresh scratch)"""
    scratch = new_scratch(*state.shape)
    scratch[0].copy_(state)
    return iterate(guide, scratch, dil, sigma, iters, **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("g", [0, 1], ids=["noise", "blocks"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_passes_against_fp64_restatement(cuda, i, g):
    """(a) One teacher-forced pass, the last of n: the device's state after n passes against the fp64 pass of the device's OWN state
    after n - 1, inside pass_bars at every element.  (b) The labels of the first pass equal the fp64 first maximum wherever the fp64
    top-2 margin exceeds twice the bar, with at most 2e-3 of the pixels excluded: a condition on the fp64 side alone, which the seeds
    (SEEDS) were chosen to meet.  (Measured on an MI355X, noise / blocks guide per case: the worst share of the pass bar 0.000 / 0.000,
    0.010 / 0.007, 0.013 / 0.009, 0.021 / 0.022, 0.011 / 0.006, 0.007 / 0.005, 0.019 / 0.020 -- the bar is a worst case in max |e_t|,
    38 .. 50 on these guides; undecided pixels 0 / 0, 0 / 0, 4.4e-4 / 1.3e-3, 1.9e-4 / 6.1e-4, 6.9e-4 / 1.0e-3, 0 / 0, 4.1e-4 / 1.4e-3;
    no decided label different.)"""
    B, C, OH, OW, dil = CASES[i]
    state, guides = inputs(i)
    guide = guides[g]
    st, gd = dev(state), dev(guide)
    labels1, _ = from_state(st, gd, dil, iters=1, want_dense=False)
    _, before = from_state(st, gd, dil, iters=PASSES - 1)
    labels, dense = from_state(st, gd, dil, iters=PASSES)
    w, W, E = R.weights_ref(guide, dil)
    own = before.cpu().numpy()
    bar = R.pass_bars(own, E, dil)
    err = np.abs(dense.cpu().numpy().astype(np.float64) - R.pass_ref(own, w, W, dil))
    share = float((err / np.maximum(bar, 1e-300)).max())
    want, margin = R.labels_of(R.pass_ref(state, w, W, dil))
    decided = margin > 2.0 * R.pass_bars(state, E, dil)[:, 0]
    excluded = 1.0 - float(decided.mean())
    wrong = int((labels1.cpu().numpy()[decided] != want[decided]).sum())
    print(f"refine {CASES[i]} guide {g}: worst share of the pass bar {share:.3f} (max E {float(E.max()):.1f}); "
          f"{excluded:.2e} of the pixels undecided, {wrong} decided labels differ")
    assert bool((err <= bar).all())
    assert excluded <= LABEL_EXCLUDED_CAP
    assert wrong == 0
    assert np.array_equal(labels.cpu().numpy(), np.where(dense.cpu().numpy().max(1) > 0, dense.cpu().numpy().argmax(1), -1))


@pytest.mark.parametrize("i", SMALL)
def test_constant_guide_is_the_float32_mean_bit_for_bit(cuda, i):
    B, C, OH, OW, dil = CASES[i]
    state, _ = inputs(i)
    guide = dev(np.full((B, OH, OW, 3), 93, dtype=np.uint8))
    for n in (1, 3):
        _, dense = from_state(dev(state), guide, dil, iters=n)
        want = R.pass_f32_constant(state, dil, n)
        assert np.array_equal(dense.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("i", SMALL)
def test_chained_calls_repeated_runs_and_labels_only_agree_bit_for_bit(cuda, i):
    B, C, OH, OW, dil = CASES[i]
    state, guides = inputs(i)
    st, guide = dev(state), dev(guides[1])
    labels4, dense4 = from_state(st, guide, dil, iters=4)
    cur = st
    for _ in range(4):
        lab, cur = from_state(cur, guide, dil, iters=1)
    assert torch.equal(bits(cur), bits(dense4)) and torch.equal(lab, labels4)
    again_l, again_d = from_state(st, guide, dil, iters=4)
    assert torch.equal(again_l, labels4) and torch.equal(bits(again_d), bits(dense4))
    only_l, _ = from_state(st, guide, dil, iters=4, want_dense=False)
    _, only_d = from_state(st, guide, dil, iters=4, want_labels=False)
    assert torch.equal(only_l, labels4) and torch.equal(bits(only_d), bits(dense4))


@pytest.mark.parametrize("i", SMALL)
def test_label_seed_is_exact_and_zero_passes_label_it(cuda, i):
    B, C, OH, OW, dil = CASES[i]
    rng = np.random.default_rng(300 + i)
    lab = rng.integers(0, C, size=(B, OH, OW)).astype(np.int32)
    void = rng.random((B, OH, OW)) < 0.2
    lab[void] = np.where(rng.random(int(void.sum())) < 0.5, 255 if C <= 255 else 256, -100)
    scratch = seed_op(dev(lab), 0, B, C, OH, OW)
    want = R.seed_labels_ref(lab, C)
    assert np.array_equal(scratch[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool(torch.isnan(scratch[1]).all())                          # the seed goes into half 0 alone
    labels, dense = iterate(dev(inputs(i)[1][0]), scratch, dil, iters=0)
    assert np.array_equal(labels.cpu().numpy(), np.where((lab >= 0) & (lab < C), lab, -1))
    assert np.array_equal(dense.cpu().numpy(), want)
    # an all-void seed: no mass anywhere, -1 everywhere after any number of passes
    scratch = seed_op(dev(np.full((B, OH, OW), -100, dtype=np.int32)), 0, B, C, OH, OW)
    labels, dense = iterate(dev(inputs(i)[1][0]), scratch, dil, iters=2)
    assert bool((labels == -1).all()) and not bool(dense.any())


# (B, hp, wp, C, OH, OW, gain)
SCORE_SEEDS = [(1, 1, 1, 1, 1, 1, 1.0), (2, 4, 5, 9, 37, 61, 1.0), (2, 8, 16, 33, 100, 131, 0.5), (1, 3, 5, 256, 24, 40, 3.0),
               (2, 12, 16, 21, 12, 16, 1.0), (1, 60, 80, 7, 480, 640, 1.0)]


@pytest.mark.parametrize("shape", SCORE_SEEDS, ids=str)
def test_scores_seed_against_fp64_and_the_upsamples_own_values(cuda, shape):
    """The seed inside seed_bar of the fp64 softmax of the exact bilinear values; and, teacher-forced, inside the (tighter) bar of the
    fp64 softmax of dinoseg_op_upsample_argmax's dense values -- the kernel walks the same strip with the same code, and a softmax
    cannot be inverted to read the enlargement back bit for bit, so the second comparison stands in for that.  (Measured on an
    MI355X: at most 0.008 of the bar, 0.026 of the teacher-forced one.)"""
    B, hp, wp, C, OH, OW, gain = shape
    rng = np.random.default_rng(17)
    z = 3.0 * rng.standard_normal((B, hp * wp, C))
    scores = (z - z.max(-1, keepdims=True) - np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True))).astype(np.float32)
    sc = dev(scores)
    scratch = seed_op(sc, 1, B, C, OH, OW, hp, wp, gain)
    got = scratch[0].cpu().numpy().astype(np.float64)
    vmax = float(np.abs(scores).max())
    bar = R.seed_bar(C, vmax, gain)
    err = float(np.abs(got - R.seed_scores_ref(scores, hp, wp, OH, OW, gain)).max())
    dense = torch.empty((B, C, OH, OW), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(sc.data_ptr(), B, hp, wp, C, OH, OW, None, dense.data_ptr(), S()))
    bar_tf = R.seed_bar(C, vmax, gain, teacher_forced=True)
    err_tf = float(np.abs(got - R.softmax_ref(dense.cpu().numpy(), gain)).max())
    print(f"scores seed {shape}: err / bar = {err / bar:.3f}; teacher-forced {err_tf / bar_tf:.3f}")
    assert err <= bar and err_tf <= bar_tf
    assert float(np.abs(got.sum(1) - 1.0).max()) <= (C + 8) * R.U
    assert bool(torch.isnan(scratch[1]).all())
    # with one class the seed is exactly 1 everywhere; iters = 0 labels are the first maximum of the seed
    labels, _ = iterate(dev(np.zeros((B, OH, OW, 3), dtype=np.uint8)), scratch, (1,), iters=0)
    assert np.array_equal(labels.cpu().numpy(), scratch[0].cpu().numpy().argmax(1))


@pytest.mark.parametrize("e", [19, 21, 24, 29])
def test_labels_follow_the_guides_edge_on_the_device(cuda, e):
    seed, guide, want = R.edge_case(e)
    scratch = seed_op(dev(seed), 0, 1, 2, 48, 64)
    labels, _ = iterate(dev(guide), scratch, DEFAULT, iters=10)
    assert np.array_equal(labels.cpu().numpy(), want)


class Fenced:
    """a tensor of `shape` inside a larger flat buffer of sentinels"""

    def __init__(self, shape, dtype, sentinel, pad=4096):
        n = int(np.prod(shape))
        self.flat = torch.full((pad + n + pad,), sentinel, dtype=dtype, device="cuda")
        self.view = self.flat[pad:pad + n].view(shape)
        self.pad, self.n, self.sentinel = pad, n, sentinel

    def intact(self):
        f = self.flat
        outside = torch.cat([f[:self.pad], f[self.pad + self.n:]])
        return bool(torch.isnan(outside).all()) if f.is_floating_point() else bool((outside == self.sentinel).all())

    def untouched(self):
        f = self.view
        return bool(torch.isnan(f).all()) if f.is_floating_point() else bool((f == self.sentinel).all())


@pytest.mark.parametrize("i", [3, 2, 0])
def test_launches_write_only_their_outputs(cuda, i):
    B, C, OH, OW, dil = CASES[i]
    state, guides = inputs(i)
    guide = dev(guides[0])
    guide0 = guide.clone()
    rng = np.random.default_rng(9)
    hp, wp = max(OH // 8, 1), max(OW // 8, 1)
    scores = dev(rng.standard_normal((B, hp * wp, C)).astype(np.float32))
    scores0 = scores.clone()
    scratch = Fenced((2, B, C, OH, OW), torch.float32, float("nan"))
    labels = Fenced((B, OH, OW), torch.int32, -7777)
    dense = Fenced((B, C, OH, OW), torch.float32, float("nan"))
    lib = capi.lib()
    capi.check(lib.dinoseg_op_refine_seed(scores.data_ptr(), 1, B, C, OH, OW, hp, wp, 1.0, scratch.view.data_ptr(), S()))
    torch.cuda.synchronize()
    assert scratch.intact() and bool(torch.isnan(scratch.view[1]).all()) and not bool(torch.isnan(scratch.view[0]).any())
    seeded = scratch.view[0].clone()
    capi.check(lib.dinoseg_op_refine_iterate(guide.data_ptr(), scratch.view.data_ptr(), B, C, OH, OW, dil_array(dil), len(dil), 0.1, 3,
                                             labels.view.data_ptr(), dense.view.data_ptr(), S()))
    torch.cuda.synchronize()
    assert scratch.intact() and labels.intact() and dense.intact()
    assert torch.equal(guide, guide0) and torch.equal(scores, scores0)
    assert not bool(torch.isnan(dense.view).any()) and not bool((labels.view == -7777).any())
    want_l, want_d = from_state(seeded, guide, dil, iters=3)
    assert torch.equal(labels.view, want_l) and torch.equal(bits(dense.view), bits(want_d))


def test_every_refusal_returns_minus_one_and_launches_nothing(cuda):
    B, C, OH, OW = 2, 3, 16, 24
    lib = capi.lib()
    guide = torch.zeros((B, OH, OW, 3), dtype=torch.uint8, device="cuda")
    lab = torch.zeros((B, OH, OW), dtype=torch.int32, device="cuda")
    scores = torch.zeros((B, 6, C), dtype=torch.float32, device="cuda")
    scratch = Fenced((2, B, C, OH, OW), torch.float32, float("nan"))
    labels = Fenced((B, OH, OW), torch.int32, -7777)
    dense = Fenced((B, C, OH, OW), torch.float32, float("nan"))
    sp, lp, dp, gp = scratch.view.data_ptr(), labels.view.data_ptr(), dense.view.data_ptr(), guide.data_ptr()
    big = 1 << 14

    def seed(seed_ptr=lab.data_ptr(), kind=0, B=B, C=C, OH=OH, OW=OW, hp=2, wp=3, gain=1.0, scratch_ptr=sp):
        return lib.dinoseg_op_refine_seed(seed_ptr, kind, B, C, OH, OW, hp, wp, gain, scratch_ptr, S())

    def it(guide_ptr=gp, scratch_ptr=sp, B=B, C=C, OH=OH, OW=OW, dil=(1, 2), n_dil=None, sigma=0.1, iters=1, l=lp, d=dp):
        arr = None if dil is None else dil_array(dil)
        return lib.dinoseg_op_refine_iterate(guide_ptr, scratch_ptr, B, C, OH, OW, arr, len(dil) if n_dil is None else n_dil, sigma, iters, l, d, S())

    sc = scores.data_ptr()
    refusals = [
        ("seed null", lambda: seed(seed_ptr=None)), ("seed scratch null", lambda: seed(scratch_ptr=None)),
        ("seed kind", lambda: seed(kind=2)), ("seed kind negative", lambda: seed(kind=-1)),
        ("seed B", lambda: seed(B=0)), ("seed C 0", lambda: seed(C=0)), ("seed C 257", lambda: seed(C=257)),
        ("seed OH 0", lambda: seed(OH=0)), ("seed OW above 2^14", lambda: seed(OW=big + 1)),
        ("scores gain 0", lambda: seed(sc, 1, gain=0.0)), ("scores gain negative", lambda: seed(sc, 1, gain=-2.0)),
        ("scores gain nan", lambda: seed(sc, 1, gain=float("nan"))), ("scores gain inf", lambda: seed(sc, 1, gain=float("inf"))),
        ("scores gain above fp32", lambda: seed(sc, 1, gain=1e39)),
        ("scores grid above the frame", lambda: seed(sc, 1, hp=17, wp=3)), ("scores grid 0", lambda: seed(sc, 1, hp=0, wp=3)),
        ("iterate guide null", lambda: it(guide_ptr=None)), ("iterate scratch null", lambda: it(scratch_ptr=None)),
        ("iterate no output", lambda: it(l=None, d=None)), ("iterate dilations null", lambda: it(dil=None, n_dil=2)),
        ("iterate B", lambda: it(B=0)), ("iterate C 0", lambda: it(C=0)), ("iterate C 257", lambda: it(C=257)),
        ("iterate OH 0", lambda: it(OH=0)), ("iterate OH above 2^14", lambda: it(OH=big + 1)),
        ("iterate n_dil 0", lambda: it(n_dil=0)), ("iterate n_dil 7", lambda: it(dil=(1, 2, 3, 4, 5, 6, 7))),
        ("iterate dilation 0", lambda: it(dil=(0, 2))), ("iterate dilation 25", lambda: it(dil=(1, 25))),
        ("iterate descending", lambda: it(dil=(2, 1))), ("iterate repeated", lambda: it(dil=(2, 2))),
        ("iterate sigma small", lambda: it(sigma=5e-4)), ("iterate sigma large", lambda: it(sigma=2e3)),
        ("iterate sigma nan", lambda: it(sigma=float("nan"))), ("iterate iters negative", lambda: it(iters=-1)),
        ("iterate iters 65", lambda: it(iters=65)),
    ]
    for name, call in refusals:
        assert call() == -1, name
        msg = capi.last_error()
        assert msg.startswith("dinoseg_op_refine_seed" if name.startswith(("seed", "scores")) else "dinoseg_op_refine_iterate"), (name, msg)
    assert lib.dinoseg_refine_scratch_bytes(0, C, OH, OW) == -1 and lib.dinoseg_refine_scratch_bytes(B, 257, OH, OW) == -1
    assert lib.dinoseg_refine_scratch_bytes(B, C, OH, big + 1) == -1
    assert lib.dinoseg_refine_scratch_bytes(1, 256, big, big) == 2 * 256 * big * big * 4
    torch.cuda.synchronize()
    assert scratch.intact() and labels.intact() and dense.intact()
    assert scratch.untouched() and labels.untouched() and dense.untouched()


# ------------------------------------------------------------------------------------------------ model level
def build(cfg, precision):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


def by_hand(lp, guide, hp, wp, gain=1.0, iters=10, dil=DEFAULT, sigma=0.1):
    """the two operators applied to log-probs [B, n, C]: what the methods must reproduce bit for bit"""
    B, OH, OW, _ = guide.shape
    scratch = seed_op(lp.contiguous(), 1, B, lp.shape[-1], OH, OW, hp, wp, gain)
    return iterate(guide, scratch, dil, sigma, iters)


def resized(frames, OH, OW):
    B, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    out = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device="cuda")
    for b in range(B):
        capi.check(capi.lib().dinoseg_op_resize_u8(frames[b].data_ptr(), H, W, out[b].data_ptr(), OH, OW, S()))
    return out


@pytest.mark.parametrize("arch", ["tiny", "vits8"])
def test_segment_refined_is_the_operators_on_the_forwards_log_probs(cuda, arch):
    cfg = ViTConfig(n_blocks=2) if arch == "tiny" else VIT_S8
    m = build(cfg, "fp16")
    B, H, W = 2, 64, 128
    hp, wp = H // 8, W // 8
    frames = torch.from_numpy(synthetic_frames(B, H, seed=61, w=W)).cuda()
    lp = m.forward_frames(frames)[0].reshape(B, -1, m.cfg.n_classes)
    want_l, want_d = by_hand(lp, frames, hp, wp)
    labels, probs = m.segment_refined(frames)
    assert probs is None and labels.dtype == torch.int32 and labels.shape == (B, H, W)
    assert torch.equal(labels, want_l)
    labels, probs = m.segment_refined(frames, want_probs=True)
    assert torch.equal(labels, want_l) and torch.equal(bits(probs), bits(want_d))
    # refine() from the same log-probs: the same bits again
    labels, probs = m.refine(lp, frames, grid=(hp, wp), want_probs=True)
    assert torch.equal(labels, want_l) and torch.equal(bits(probs), bits(want_d))
    # another size and other parameters: the guide is the frames resized by dinoseg_op_resize_u8
    guide = resized(frames, 100, 131)
    want_l, want_d = by_hand(lp, guide, hp, wp, 2.0, 3, (1, 3, 9), 0.2)
    labels, probs = m.segment_refined(frames, size=(100, 131), gain=2.0, iters=3, dilations=(1, 3, 9), sigma=0.2, want_probs=True)
    assert torch.equal(labels, want_l) and torch.equal(bits(probs), bits(want_d))
    # an explicit guide, with uint8 and with fp32 frames
    other = dev(R.make_guides(np.random.default_rng(5), B, 75, 101)[1])
    want_l, _ = by_hand(lp, other, hp, wp, iters=2)
    assert torch.equal(m.segment_refined(frames, guide=other, iters=2)[0], want_l)
    from oracle import dinoseg_oracle as O
    x32 = O.preprocess(frames.cpu().numpy()).cuda()
    with torch.no_grad():
        lp32 = m(x32).reshape(B, -1, m.cfg.n_classes)
    want32, _ = by_hand(lp32, other, hp, wp, iters=2)
    assert torch.equal(m.segment_refined(x32, guide=other, iters=2)[0], want32)


def test_refine_accepts_the_labels_of_cluster_and_discover_all(cuda):
    m = build(ViTConfig(n_blocks=2), "fp16")
    B, H, W = 2, 64, 128
    frames = torch.from_numpy(synthetic_frames(B, H, seed=62, w=W)).cuda()
    for coarse, n in ((m.cluster(frames, 4, iters=3).labels, 4), (m.discover_all(frames, max_objects=2).labels, 3)):
        labels, probs = m.refine(coarse, frames, n_classes=n, iters=4, want_probs=True)
        scratch = seed_op(coarse.contiguous(), 0, B, n, H, W)
        want_l, want_d = iterate(frames, scratch, DEFAULT, iters=4)
        assert torch.equal(labels, want_l) and torch.equal(bits(probs), bits(want_d))
        assert int(labels.min()) >= 0 and int(labels.max()) < n          # every pixel of a full seed keeps mass
        zero_l, _ = m.refine(coarse, frames, n_classes=n, iters=0)
        assert torch.equal(zero_l, coarse)


def test_segment_refined_behind_the_two_stream_split(cuda):
    """A batch of at least split_min frames: both half-batches run on their streams before the launches on the caller's."""
    m = build(ViTConfig(n_blocks=2), "fp16")
    B = 8
    frames = torch.from_numpy(synthetic_frames(B, 64, seed=49, w=96)).cuda()
    lp = m.forward_frames(frames)[0].reshape(B, -1, m.cfg.n_classes)
    want_l, want_d = by_hand(lp, frames, 8, 12, iters=3)
    for _ in range(2):
        labels, probs = m.segment_refined(frames, iters=3, want_probs=True)
        assert torch.equal(labels, want_l) and torch.equal(bits(probs), bits(want_d))
