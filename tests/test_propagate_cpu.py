"""Label propagation without a device: the host restatement (tests/propagate_util.py) against the matrix form of the DINO script in
torch fp64, the context schedule, the seed rule by hand, the plan layer's refusals, and the library's host-only entries."""
import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, LabelPropagator, capi, context_frames
from dino_amd.dense_plan import propagate_plan
from tests import propagate_util as P


def script_matrix_form(ft, fctx, segs, hp, wp, R, k, tau):
    """eval_video_segmentation's label_propagation in torch fp64: exp(bmm / tau) times the neighbourhood mask, topk over all context
    candidates (dim 0), zero below the k-th, renormalise, segs @ aff.  -> V [n, C]"""
    n = hp * wp
    q = torch.from_numpy(P.unit_rows(ft))                               # [n, D]
    keys = torch.from_numpy(P.unit_rows(fctx))                          # [n_ctx, n, D]
    aff = torch.exp(torch.bmm(keys, q.T.expand(keys.shape[0], -1, -1)) / tau)      # [n_ctx, n keys, n queries]
    r, c = torch.div(torch.arange(n), wp, rounding_mode="floor"), torch.arange(n) % wp
    mask = ((r[:, None] - r[None, :]).abs() <= R) & ((c[:, None] - c[None, :]).abs() <= R)
    aff = (aff * mask[None].to(aff.dtype)).reshape(-1, n)               # [n_ctx n, n]
    kth = torch.topk(aff, k=min(k, aff.shape[0]), dim=0).values[-1]
    aff = torch.where(aff < kth[None], torch.zeros_like(aff), aff)
    aff = aff / aff.sum(dim=0, keepdim=True)
    flat = torch.from_numpy(np.asarray(segs, dtype=np.float64)).reshape(-1, segs.shape[-1])       # [n_ctx n, C]
    return (flat.T @ aff).T.numpy()


@pytest.mark.parametrize("hp,wp,n_ctx,R,k", [(4, 5, 1, 1, 5), (4, 5, 2, 2, 3), (6, 6, 3, 2, 5), (6, 6, 1, 0, 5), (6, 6, 2, 12, 1)])
def test_host_rule_is_the_scripts_matrix_form(hp, wp, n_ctx, R, k):
    tok_t, tok_c, segs = P.make_case(40 + hp + n_ctx, hp, wp, 32, 4, n_ctx)
    ft, fctx = tok_t[0, 1:], tok_c[:, 1:]
    _, wn, V, ranked = P.propagate_host(ft, fctx, segs, hp, wp, R, k, 0.1)
    head = ranked[0][:, :k + 1]
    with np.errstate(invalid="ignore"):                                 # (-inf - -inf beyond the count)
        assert np.all(np.diff(head, axis=1)[np.isfinite(head[:, 1:])] < 0), "ties in a random case"
    # the rule rounds a = log2(e) / tau to fp32 once, so the script runs at the temperature that a stands for: exp(s / tau') = 2^(s a)
    want = script_matrix_form(ft, fctx, segs, hp, wp, R, k, P.LOG2E / P.scale_a(0.1))
    assert np.abs(V - want).max() <= 1e-12
    assert np.abs(wn.sum(axis=1) - 1.0).max() <= 1e-12


def test_context_schedules():
    for f in (context_frames, P.context_frames):
        assert f(1, 7) == [0]
        assert f(2, 7) == [0, 1]
        assert f(9, 7) == [0, 2, 3, 4, 5, 6, 7, 8]
        assert f(3, 1) == [0, 2]
        assert f(5, 0) == [0]
    for t in range(1, 40):
        for nc in (0, 1, 7, 15):
            assert context_frames(t, nc) == P.context_frames(t, nc)
            assert len(context_frames(t, nc)) == 1 + min(t - 1, nc) <= 16
    with pytest.raises(ValueError):
        context_frames(0, 7)
    with pytest.raises(ValueError):
        context_frames(3, 16)


def test_seed_rule_by_hand():
    # a 2 x 3 grid under 4 x 6 labels: every cell is 2 x 2 pixels; 255 and -100 are void
    y = np.array([[0, 0, 1, 2, 255, 255],
                  [0, 1, 1, 2, 255, 0],
                  [2, 2, -100, 1, 3, 3],
                  [2, 2, 1, 1, 3, 7]], dtype=np.int64)
    seg = P.label_cells_host(y, 2, 3, 4)
    want = np.array([[0.75, 0.25, 0, 0], [0, 0.5, 0.5, 0], [0.25, 0, 0, 0],
                     [0, 0, 1, 0], [0, 0.75, 0, 0], [0, 0, 0, 0.75]], dtype=np.float32)
    assert seg.dtype == np.float32 and np.array_equal(seg, want)
    # a fractional ratio: 5 x 7 labels, pixel (y, x) -> cell ((2 y) // 5, (3 x) // 7): rows 0-2 | 3-4, columns 0-2 | 3-4 | 5-6
    y = np.arange(35, dtype=np.int64).reshape(5, 7) % 3
    seg = P.label_cells_host(y, 2, 3, 3)
    cell0 = y[0:3, 0:3].reshape(-1)
    assert np.array_equal(seg[0], np.array([(cell0 == c).sum() for c in range(3)], dtype=np.float32) / np.float32(9))
    cell5 = y[3:5, 5:7].reshape(-1)
    assert np.array_equal(seg[5], np.array([(cell5 == c).sum() for c in range(3)], dtype=np.float32) / np.float32(4))


def test_plan_refusals_need_no_device():
    p = 8
    clip = torch.zeros((3, 40, 56, 3), dtype=torch.uint8)
    y = torch.zeros((40, 56), dtype=torch.int64)
    ok = propagate_plan(p, clip, y, n_classes=4)
    assert (ok.T, ok.hp, ok.wp, ok.C, ok.seed, ok.OH, ok.OW) == (3, 5, 7, 4, "labels", 40, 56)
    assert (ok.n_context, ok.radius, ok.topk, ok.temperature, ok.chunk) == (7, 12, 5, 0.1, 32)
    assert propagate_plan(p, clip, y, n_classes=4, radius=None).radius == 7
    soft = propagate_plan(p, clip.permute(0, 3, 1, 2).float(), torch.zeros((35, 9)))
    assert (soft.seed, soft.C, soft.kind) == ("soft", 9, capi.INPUT_F32_CHW)
    assert propagate_plan(p, clip, torch.zeros((5, 7), dtype=torch.uint8), n_classes=2, size=(5, 7)).OH == 5
    bad = [
        dict(frames=torch.zeros((3, 40, 56), dtype=torch.uint8)),                       # layout
        dict(frames=torch.zeros((3, 41, 56, 3), dtype=torch.uint8)),                    # not a patch multiple
        dict(frames=torch.zeros((0, 40, 56, 3), dtype=torch.uint8)),                    # empty clip
        dict(frames=np.zeros((3, 40, 56, 3), dtype=np.uint8)),                          # not a tensor
        dict(n_classes=None), dict(n_classes=0), dict(n_classes=257), dict(n_classes=2.0),
        dict(first=torch.zeros((4, 7), dtype=torch.int64)),                             # labels smaller than the grid
        dict(first=torch.zeros((1, 40, 56), dtype=torch.int64)),                        # labels with a batch
        dict(first=torch.zeros((40, 56), dtype=torch.bool)),
        dict(first=None),
        dict(first=torch.zeros((34, 4))),                                               # a soft seed with the wrong n
        dict(first=torch.zeros((35, 257))), dict(first=torch.zeros((35, 0))),
        dict(first=torch.zeros((35, 5))),                                               # ... whose C contradicts n_classes = 4
        dict(n_context=-1), dict(n_context=16), dict(n_context=1.5),
        dict(radius=-1), dict(radius=2.5),
        dict(topk=0), dict(topk=17), dict(topk=True),
        dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
        dict(temperature="hot"),
        dict(size=(4, 56)), dict(size=(40, 6)), dict(size=40),
        dict(chunk=0),
    ]
    for kw in bad:
        args = dict(frames=clip, first=y, n_classes=4)
        args.update(kw)
        with pytest.raises(ValueError):
            propagate_plan(p, **args)
    # the model's calls refuse the same things before they ask for a GPU; a valid call on a CPU model reaches "no CPU path"
    m = DINOSeg(head="linear", n_blocks=1)
    for kw in (dict(topk=0), dict(n_classes=None), dict(n_blocks=2), dict(temperature=0.0)):
        args = dict(first=y, n_classes=4)
        args.update(kw)
        with pytest.raises(ValueError):
            m.propagate(clip, **args)
        with pytest.raises(ValueError):
            LabelPropagator(m, clip[0], **args)
    with pytest.raises(ValueError):
        LabelPropagator(m, clip, y, n_classes=4)                                        # a batch of three is not one frame
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.propagate(clip, y, n_classes=4)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        LabelPropagator(m, clip[0], y, n_classes=4)


def test_symbols_and_scratch_entry():
    lib = capi.lib()
    names = ("dinoseg_op_normalize_tokens", "dinoseg_op_label_cells", "dinoseg_op_propagate", "dinoseg_propagate_scratch_bytes")
    declared = capi.header_symbols()
    for name in names:
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name)
    f = lib.dinoseg_propagate_scratch_bytes
    assert f(60, 80, 8, 5) == 8 * 8 * 4800 * 5                       # scores and indices, [n_ctx][n][k] each
    assert f(1, 1, 1, 1) == 8
    assert f(60, 60, 16, 16) == 8 * 16 * 3600 * 16
    assert f(60, 80, 8, 5) < 4 * 4800 * 4800                            # far below ONE fp32 [n, n] slice of the affinity
    for bad in ((0, 80, 8, 5), (60, -1, 8, 5), (60, 80, 0, 5), (60, 80, 17, 5), (60, 80, 8, 0), (60, 80, 8, 17), (5000, 80, 8, 5)):
        assert f(*bad) == -1
