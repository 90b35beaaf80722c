"""The refinement's rule without a device: the int64 / fp64 restatement (tests/refine_util.py) against a plain torch statement of the
same rule, what a pass conserves, the edge-following property in fp64, and every refusal of ``dense_plan.refine_plan``."""
import numpy as np
import pytest
import torch

from dino_amd.dense_plan import refine_params, refine_plan
from tests import refine_util as R


@pytest.mark.parametrize("case", [((1, 2, 4, 8, 12, 24), 0.1, 2, 3, 37, 61), ((1, 3), 0.05, 1, 5, 9, 7), ((2, 24), 0.5, 1, 2, 24, 40),
                                  ((1,), 0.1, 2, 1, 1, 1)], ids=str)
def test_restatement_agrees_with_a_plain_torch_statement(case):
    dil, sigma, B, C, OH, OW = case
    rng = np.random.default_rng(3)
    P = R.make_state(rng, B, C, OH, OW)
    for guide in R.make_guides(rng, B, OH, OW) + (np.full((B, OH, OW, 3), 77, dtype=np.uint8),):
        for iters in (1, 3):
            got = R.refine_ref(P, guide, dil, sigma, iters)
            want = R.torch_plain(P, guide, dil, sigma, iters)
            assert float(np.abs(got - want).max()) <= 1e-12


def test_a_pass_conserves_the_sum_over_classes():
    rng = np.random.default_rng(4)
    B, C, OH, OW = 2, 7, 40, 53
    P = R.make_state(rng, B, C, OH, OW).astype(np.float64)
    P /= P.sum(1, keepdims=True)
    for guide in R.make_guides(rng, B, OH, OW):
        w, W, _ = R.weights_ref(guide)
        assert float(w.max(0).min()) == 1.0 and float(W.min()) >= 1.0       # the largest weight is exactly 1
        Q = P
        for _ in range(3):
            Q = R.pass_ref(Q, w, W)
            assert float(np.abs(Q.sum(1) - 1.0).max()) <= 1e-12
            assert float(Q.min()) >= 0.0


def test_constant_guide_pass_in_float32_is_the_plain_mean():
    rng = np.random.default_rng(5)
    P = R.make_state(rng, 1, 3, 20, 31)
    guide = np.full((1, 20, 31, 3), 128, dtype=np.uint8)
    w, W, E = R.weights_ref(guide, (1, 2, 4))
    assert float(w.min()) == 1.0 and float(W.max()) == 24.0 and float(E.max()) == 0.0
    got = R.pass_f32_constant(P, (1, 2, 4), 2)
    assert got.dtype == np.float32
    assert float(np.abs(got - R.refine_ref(P, guide, (1, 2, 4), 0.1, 2)).max()) <= 2 * (2 * 24 + 8) * R.U


@pytest.mark.parametrize("e,min_margin", [(19, 0.846), (21, 0.862), (24, 1.000), (29, 0.855)])
def test_labels_follow_the_guides_edge_in_fp64(e, min_margin):
    """After 10 passes the labels equal the guide's edge at EVERY pixel, with the smallest top-2 margin the issue states (to its three
    decimals).  Not tested at one pass: there the flat guide gives an exact 15-to-15 tap tie."""
    seed, guide, want = R.edge_case(e)
    assert int((seed != want).sum()) == (0 if e == 24 else 144)
    P = R.refine_ref(R.seed_labels_ref(seed, 2), guide, iters=10)
    lab, margin = R.labels_of(P)
    assert np.array_equal(lab, want)
    assert abs(float(margin.min()) - min_margin) <= 1e-3


@pytest.mark.parametrize("e,floor", [(19, 0.63), (21, 0.35), (29, 0.15)])
def test_labels_follow_a_noisy_guides_edge_in_fp64(e, floor):
    """Uniform noise of +-6 on the guide: still exact.  The margins depend on the noise drawn; this draw's are asserted positive, the
    issue's figures for its own draw were 0.63 / 0.35 / 0.15."""
    seed, guide, want = R.edge_case(e, noise=6, seed=e)
    lab, margin = R.labels_of(R.refine_ref(R.seed_labels_ref(seed, 2), guide, iters=10))
    print(f"edge {e}: smallest margin {float(margin.min()):.3f} (the issue's draw: {floor})")
    assert np.array_equal(lab, want)
    assert float(margin.min()) > 0.05


def test_void_pixels_take_what_their_neighbours_give():
    seed, guide, want = R.edge_case(21)
    seed = np.array(seed)
    seed[0, 10:20, 5:15] = 255
    seed[0, 30:35, 40:50] = -100
    P0 = R.seed_labels_ref(seed, 2)
    assert float(P0[0, :, 12, 7].sum()) == 0.0
    lab, _ = R.labels_of(R.refine_ref(P0, guide, iters=10))
    assert np.array_equal(lab, want)
    lab0, _ = R.labels_of(R.refine_ref(np.zeros_like(P0), guide, iters=2))
    assert bool((lab0 == -1).all())


def test_bars_scale_with_the_operation_counts():
    rng = np.random.default_rng(6)
    P = R.make_state(rng, 1, 3, 16, 16)
    E = np.zeros((1, 16, 16))
    flat = R.pass_bars(P, E, (1, 2))
    assert float(flat.max()) <= (2 * 16 + 8) * R.U * float(P.max()) * (1 + 1e-9)
    assert float(R.pass_bars(P, E + 10.0, (1, 2)).max()) > float(flat.max())
    assert flat.shape == (1, 1, 16, 16)


# ------------------------------------------------------------------------------------------------ refine_plan
def _guide(B=2, OH=24, OW=40):
    return torch.zeros((B, OH, OW, 3), dtype=torch.uint8)


def test_refine_plan_accepts_both_seed_kinds():
    g = _guide()
    plan = refine_plan(torch.zeros((2, 24, 40), dtype=torch.int64), g, n_classes=5)
    assert plan == (0, 2, 5, 24, 40, 0, 0, 1.0, 10, (1, 2, 4, 8, 12, 24), 0.1)
    plan = refine_plan(torch.zeros((2, 15, 7)), g, grid=(3, 5), gain=2.0, iters=0, dilations=[1, 3], sigma=1.0)
    assert plan == (1, 2, 7, 24, 40, 3, 5, 2.0, 0, (1, 3), 1.0)
    assert refine_plan(torch.zeros((2, 15, 7)), g, n_classes=7, grid=(3, 5))[2] == 7
    assert refine_plan(torch.zeros((2, 24, 40), dtype=torch.uint8), g, n_classes=256)[2] == 256


REFUSALS = [
    ("guide dtype", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), torch.zeros((2, 24, 40, 3)), n_classes=2)),
    ("guide shape", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), torch.zeros((2, 3, 24, 40), dtype=torch.uint8), n_classes=2)),
    ("guide none", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), None, n_classes=2)),
    ("empty batch", lambda: refine_plan(torch.zeros((0, 24, 40), dtype=torch.int32), _guide(0), n_classes=2)),
    ("empty frame", lambda: refine_plan(torch.zeros((2, 0, 40), dtype=torch.int32), _guide(2, 0, 40), n_classes=2)),
    ("guide too large", lambda: refine_plan(torch.zeros((1, 1, 16385), dtype=torch.int32), _guide(1, 1, 16385), n_classes=2)),
    ("seed not a tensor", lambda: refine_plan(np.zeros((2, 24, 40), dtype=np.int32), _guide(), n_classes=2)),
    ("seed dtype", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.float16), _guide(), n_classes=2)),
    ("labels at another size", lambda: refine_plan(torch.zeros((2, 24, 41), dtype=torch.int32), _guide(), n_classes=2)),
    ("labels at another batch", lambda: refine_plan(torch.zeros((3, 24, 40), dtype=torch.int32), _guide(), n_classes=2)),
    ("labels rank", lambda: refine_plan(torch.zeros((2, 1, 24, 40), dtype=torch.int32), _guide(), n_classes=2)),
    ("labels without n_classes", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide())),
    ("labels with grid", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=2, grid=(3, 5))),
    ("n_classes 0", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=0)),
    ("n_classes 257", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=257)),
    ("n_classes float", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=2.0)),
    ("scores without grid", lambda: refine_plan(torch.zeros((2, 15, 7)), _guide())),
    ("scores rank", lambda: refine_plan(torch.zeros((2, 3, 5, 7)), _guide(), grid=(3, 5))),
    ("scores at another batch", lambda: refine_plan(torch.zeros((1, 15, 7)), _guide(), grid=(3, 5))),
    ("grid does not hold the rows", lambda: refine_plan(torch.zeros((2, 15, 7)), _guide(), grid=(4, 4))),
    ("grid not positive", lambda: refine_plan(torch.zeros((2, 0, 7)), _guide(), grid=(0, 5))),
    ("grid not a pair", lambda: refine_plan(torch.zeros((2, 15, 7)), _guide(), grid="3x5")),
    ("grid above the guide", lambda: refine_plan(torch.zeros((2, 25 * 5, 7)), _guide(), grid=(25, 5))),
    ("scores with too many classes", lambda: refine_plan(torch.zeros((2, 15, 257)), _guide(), grid=(3, 5))),
    ("scores n_classes mismatch", lambda: refine_plan(torch.zeros((2, 15, 7)), _guide(), n_classes=6, grid=(3, 5))),
    ("gain 0", lambda: refine_params(gain=0.0)),
    ("gain negative", lambda: refine_params(gain=-1.0)),
    ("gain inf", lambda: refine_params(gain=float("inf"))),
    ("gain nan", lambda: refine_params(gain=float("nan"))),
    ("gain overflows fp32", lambda: refine_params(gain=1e39)),
    ("gain underflows fp32", lambda: refine_params(gain=1e-50)),
    ("gain text", lambda: refine_params(gain="big")),
    ("sigma small", lambda: refine_params(sigma=5e-4)),
    ("sigma large", lambda: refine_params(sigma=1001.0)),
    ("sigma nan", lambda: refine_params(sigma=float("nan"))),
    ("iters negative", lambda: refine_params(iters=-1)),
    ("iters 65", lambda: refine_params(iters=65)),
    ("iters float", lambda: refine_params(iters=3.0)),
    ("iters bool", lambda: refine_params(iters=True)),
    ("no dilations", lambda: refine_params(dilations=())),
    ("seven dilations", lambda: refine_params(dilations=(1, 2, 3, 4, 5, 6, 7))),
    ("dilation 0", lambda: refine_params(dilations=(0, 1))),
    ("dilation 25", lambda: refine_params(dilations=(1, 25))),
    ("dilation float", lambda: refine_params(dilations=(1, 2.0))),
    ("dilations descending", lambda: refine_params(dilations=(2, 1))),
    ("dilations repeated", lambda: refine_params(dilations=(1, 1))),
    ("dilations not a sequence", lambda: refine_params(dilations=3)),
    ("through refine_plan", lambda: refine_plan(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=2, iters=65)),
]


@pytest.mark.parametrize("name,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refine_plan_refuses(name, call):
    with pytest.raises(ValueError):
        call()


def test_refine_and_segment_refined_refuse_before_any_device_use():
    """Every ValueError is raised by the plan layer: the methods never reach _require_gpu with a bad argument."""
    from dino_amd import DINOSeg, ViTConfig
    cfg = ViTConfig(n_blocks=1)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, arch=cfg)
    with pytest.raises(ValueError):
        m.refine(torch.zeros((2, 24, 40), dtype=torch.int32), _guide())
    with pytest.raises(ValueError):
        m.refine(torch.zeros((2, 24, 40), dtype=torch.int32), _guide(), n_classes=3, dilations=(4, 2))
    with pytest.raises(ValueError):
        m.segment_refined(torch.zeros((1, 3, 64, 64)))                      # fp32 frames carry no guide
    with pytest.raises(ValueError):
        m.segment_refined(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), iters=100)
    with pytest.raises(ValueError):
        m.segment_refined(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), guide=_guide(1, 32, 32), size=(33, 32))
