"""Label propagation on the device: dinoseg_op_normalize_tokens, dinoseg_op_label_cells and dinoseg_op_propagate through the C-ABI
against the fp64 restatement of the rule (tests/propagate_util.py) -- decided and undecided queries, exact ties, pure motion, the seed
rule, run-to-run identity, containment, refusals -- and DINOSeg.propagate / LabelPropagator against the operators applied by hand."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, LabelPropagator, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames
from tests import arch_util as A
from tests import propagate_util as P

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
TAU = 0.1
UNDECIDED_CAP = 0.04

# (hp, wp, D, C, n_ctx, R, k)
CASES = [
    (1, 1, 64, 2, 1, 0, 1),             # one cell
    (5, 7, 64, 3, 1, 2, 5),             # window clipped on every side
    (9, 11, 64, 7, 2, 12, 5),           # radius wider than the grid
    (3, 4, 192, 5, 2, 0, 5),            # two candidates for k = 5
    (20, 24, 64, 21, 8, 3, 5),          # interior tiles, full context
    (20, 24, 384, 150, 8, 12, 5),       # ViT-S width, wide C
    (12, 16, 768, 256, 3, 12, 1),       # ViT-B width, class limit, k = 1
    (60, 80, 384, 7, 2, 12, 5),         # the camera's grid, once
]
SEEDS = [200, 201, 202, 203, 204, 205, 206, 207]                       # one seed per case


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def normalize(tokens):
    """tokens: device fp32 [B, 1 + n, D] -> planes fp16 [B, 2, n, D]"""
    B, n1, D = tokens.shape
    planes = torch.empty((B, 2, n1 - 1, D), dtype=torch.float16, device="cuda")
    capi.check(capi.lib().dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n1 - 1, D, planes.data_ptr(), S()))
    return planes


def scratch_bytes(hp, wp, n_ctx, k):
    nbytes = capi.lib().dinoseg_propagate_scratch_bytes(hp, wp, n_ctx, k)
    assert nbytes == 8 * n_ctx * hp * wp * k
    return nbytes


def table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def run_propagate(tq, ctx_planes, ctx_segs, hp, wp, R, k, tau=TAU, debug=True, out=None):
    """device tensors in: tq [2, n, D], lists of context planes and segs -> (seg_out [n, C], topk_idx [n, k], topk_w [n, k])"""
    n, D, C = hp * wp, tq.shape[-1], ctx_segs[0].shape[-1]
    if out is None:
        seg = torch.empty((n, C), dtype=torch.float32, device="cuda")
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda") if debug else None
        w = torch.empty((n, k), dtype=torch.float32, device="cuda") if debug else None
        scratch = torch.empty((scratch_bytes(hp, wp, len(ctx_planes), k),), dtype=torch.uint8, device="cuda")
    else:
        seg, idx, w, scratch = out
    capi.check(capi.lib().dinoseg_op_propagate(tq.data_ptr(), table(ctx_planes), table(ctx_segs), len(ctx_planes), hp, wp, D, C, R, k,
                                               tau, seg.data_ptr(), capi.ptr(idx), capi.ptr(w), scratch.data_ptr(), S()))
    return seg, idx, w


def label_cells(y, hp, wp, C):
    kind = 0 if y.dtype == torch.uint8 else 1
    seg = torch.empty((hp * wp, C), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_label_cells(y.data_ptr(), kind, y.shape[0], y.shape[1], hp, wp, C, seg.data_ptr(), S()))
    return seg


@functools.lru_cache(maxsize=None)
def inputs(i):
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    arrays = P.make_case(SEEDS[i], hp, wp, D, C, n_ctx)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(i):
    """the fp64 restatement of a case, computed once"""
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    tok_t, tok_c, segs = inputs(i)
    return P.propagate_host(tok_t[0, 1:], tok_c[:, 1:], segs, hp, wp, R, k, TAU)


def device_case(i):
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    tok_t, tok_c, segs = inputs(i)
    tq = normalize(dev(tok_t))[0]
    cp = normalize(dev(tok_c))
    sg = dev(segs)
    return tq, [cp[c] for c in range(n_ctx)], [sg[c] for c in range(n_ctx)]


def by_key(g, v):
    """rows of v reordered by ascending g (a selection as a set with its values)"""
    order = np.argsort(g, axis=1, kind="stable")
    return np.take_along_axis(g, order, axis=1), np.take_along_axis(v, order, axis=1)


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: "x".join(str(v) for v in CASES[i]))
def test_operator_against_fp64_restatement(cuda, i):
    """Scores bar E(D) = (D + 16) 2^-24, values bar (4 E / tau + (16 + 2k) 2^-24) max|seg|.  Decided queries (fp64 gap at the cut
    above 2E, or no more candidates than k): the selection is the host's as a set, w / W within 4E / tau, seg_out within the values
    bar.  Undecided queries: every selected score >= s_cut - 2E and every unselected one <= s_cut + 2E in fp64, seg_out within the
    bar of the value formed from the device's own selection.  At most 4 % of a case's queries are undecided.  (Measured on an
    MI355X: undecided 0, 0, 0, 0, 0.21 %, 1.67 %, 1.04 %, 1.40 % of the queries in case order; weights and values at 0.001 of their
    bars at most.)"""
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    tok_t, tok_c, segs = inputs(i)
    ft, fctx = tok_t[0, 1:], tok_c[:, 1:]
    g_host, w_host, V_host, ranked = reference(i)
    E, bar = P.score_bar(D), P.value_bar(D, k, TAU, float(np.abs(segs).max()))
    seg, idx, w = (t.cpu().numpy() for t in run_propagate(*device_case(i), hp, wp, R, k))
    idx = idx.astype(np.int64)
    dec = P.decided(ranked, k, E)
    share = 1.0 - float(dec.mean())
    # every device selection is K' distinct candidates, -1 beyond
    kept = np.minimum(ranked[2], k)
    assert np.array_equal((idx >= 0).sum(axis=1), kept)
    assert np.all((idx >= 0) == (np.arange(k)[None, :] < kept[:, None]))
    assert np.all((w > 0) == (idx >= 0))
    # decided queries
    gd, wd = by_key(idx[dec], w[dec].astype(np.float64))
    gh, wh = by_key(g_host[dec], w_host[dec])
    assert np.array_equal(gd, gh), "a decided query's selection differs from the host's"
    w_err = float(np.abs(wd - wh).max())
    v_err = float(np.abs(seg[dec].astype(np.float64) - V_host[dec]).max())
    # undecided queries: the device's selection is one the bar allows, and its value follows from it
    und = np.flatnonzero(~dec)
    u_err = 0.0
    if und.size:
        s_sel = P.scores_of(ft[und], fctx, idx[und])
        s_rank, g_rank, _ = ranked
        cut = s_rank[und, k - 1]
        assert np.all(s_sel >= cut[:, None] - 2.0 * E), "an undecided query selected a score below the cut's band"
        for row, q in enumerate(und):
            cand = g_rank[q][g_rank[q] >= 0]
            assert len(set(idx[q])) == k and set(idx[q]) <= set(cand)
            rest = ~np.isin(g_rank[q], idx[q]) & (g_rank[q] >= 0)
            assert np.all(s_rank[q][rest] <= cut[row] + 2.0 * E), "an undecided query left out a score above the cut's band"
        _, V_dev = P.weights_and_value(s_sel, idx[und], segs, TAU)
        u_err = float(np.abs(seg[und].astype(np.float64) - V_dev).max())
    print(f"propagate {CASES[i]}: undecided {share:.4f} of the queries; weights {w_err / (4 * E / TAU):.3f} of their bar, values "
          f"{v_err / bar:.3f} (decided) and {u_err / bar:.3f} (undecided) of theirs (bar {bar:.3e})")
    assert share <= UNDECIDED_CAP
    assert w_err <= 4.0 * E / TAU
    assert v_err <= bar and u_err <= bar


@pytest.mark.parametrize("hp,wp,D,C,R", [(5, 7, 64, 3, 2), (20, 24, 64, 21, 3)])
def test_exact_ties_go_to_the_lower_index(cuda, hp, wp, D, C, R):
    """Context = the same planes twice: twins score bit-equal, so the order inside a pair is the index alone.  Where the first four
    distinct values are more than 2E apart, the k = 5 selection is the host's: two pairs, then the third value's frame-0 copy without
    its twin."""
    k, n = 5, hp * wp
    tok_t, tok_c, segs = P.make_case(300 + hp, hp, wp, D, C, 2)
    tok_c = np.stack([tok_c[0], tok_c[0]])
    g_host, _, V_host, ranked = P.propagate_host(tok_t[0, 1:], tok_c[:, 1:], segs, hp, wp, R, k, TAU)
    tq, cp, sg = normalize(dev(tok_t))[0], normalize(dev(tok_c[:1]))[0], dev(segs)
    seg, idx, w = (t.cpu().numpy() for t in run_propagate(tq, [cp, cp], [sg[0], sg[1]], hp, wp, R, k))
    s = ranked[0]
    assert np.all(ranked[2] >= 8) and np.array_equal(s[:, 0:8:2], s[:, 1:8:2])          # the host's twins tie exactly too
    E = P.score_bar(D)
    clear = np.all(s[:, 0:6:2] - s[:, 2:8:2] > 2.0 * E, axis=1)                          # v1 > v2 > v3 > v4 beyond the bar
    assert clear.mean() > 0.5
    idx = idx.astype(np.int64)[clear]
    assert np.array_equal(idx, g_host[clear]), "with clear gaps even the rank order is the host's"
    assert np.all(idx[:, 0] + n == idx[:, 1]) and np.all(idx[:, 2] + n == idx[:, 3])     # pairs: frame 0's copy first
    assert np.all(idx[:, 4] < n) and not np.any(idx[:, :4] == idx[:, 4:5] + n)           # the third value: its twin is out
    wb = w[clear].view(np.uint32)
    assert np.array_equal(wb[:, 0], wb[:, 1]) and np.array_equal(wb[:, 2], wb[:, 3])     # bit-equal scores, bit-equal weights
    bar = P.value_bar(D, k, TAU, float(np.abs(segs).max()))
    assert np.abs(seg[clear].astype(np.float64) - V_host[clear]).max() <= bar


def test_pure_motion_moves_the_labels_bit_for_bit(cuda):
    """The target's features are the context grid shifted by (2, -3) cells (new cells random); R = 4, k = 1, one context frame:
    seg_t is the shifted seg_0 bit for bit wherever the source cell is inside the grid."""
    hp, wp, D, C = 20, 24, 64, 21
    tok_t, tok_c, segs = P.make_case(310, hp, wp, D, C, 1)
    r, c = np.divmod(np.arange(hp * wp), wp)
    sr, sc = r - 2, c + 3                                               # target cell (r, c) shows what was at (r - 2, c + 3)
    inside = (sr >= 0) & (sr < hp) & (sc >= 0) & (sc < wp)
    src = (sr * wp + sc)[inside]
    tok_t = tok_t.copy()
    tok_t[0, 1:][inside] = tok_c[0, 1:][src]
    tq, cp, sg = normalize(dev(tok_t))[0], normalize(dev(tok_c))[0], dev(segs)
    seg, idx, w = (t.cpu().numpy() for t in run_propagate(tq, [cp], [sg[0]], hp, wp, 4, 1))
    assert inside.sum() == (hp - 2) * (wp - 3)
    assert np.array_equal(idx[inside, 0], src)
    assert np.array_equal(seg[inside].view(np.uint32), segs[0][src].view(np.uint32))
    assert np.all(w == 1.0)


@pytest.mark.parametrize("hp,wp,OH,OW,C", [(5, 7, 40, 56, 5), (10, 10, 37, 37, 5), (6, 9, 48, 33, 150), (60, 80, 480, 640, 7)])
def test_label_cells_equal_the_integer_rule(cuda, hp, wp, OH, OW, C):
    rng = np.random.default_rng(320 + hp)
    y = rng.integers(0, C, (OH, OW)).astype(np.int64)
    y[rng.random((OH, OW)) < 0.1] = 255
    y8 = y.astype(np.uint8)
    if C <= 255:
        assert np.array_equal(label_cells(dev(y8), hp, wp, C).cpu().numpy(), P.label_cells_host(y8, hp, wp, C))
    y[rng.random((OH, OW)) < 0.05] = -100
    y[0, 0], y[-1, -1] = C, -1                                          # the first labels outside [0, C) on either side
    got = label_cells(dev(y), hp, wp, C).cpu().numpy()
    assert np.array_equal(got, P.label_cells_host(y, hp, wp, C))
    assert got.sum(axis=1).max() <= 1.0 + 1e-6 and got.sum(axis=1).min() < 1.0


def test_two_runs_are_bit_identical(cuda):
    i = 4
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    a = [t.cpu() for t in run_propagate(*device_case(i), hp, wp, R, k)]
    b = [t.cpu() for t in run_propagate(*device_case(i), hp, wp, R, k)]
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    c = run_propagate(*device_case(i), hp, wp, R, k, debug=False)[0].cpu()
    assert torch.equal(c.view(torch.int32), a[0].view(torch.int32))     # the debug outputs change nothing


class Guarded:
    """`nbytes` of device memory between two guard bands of 4 KiB, everything filled with 0xA5"""
    BAND = 4096

    def __init__(self, nbytes, dtype, shape):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * self.BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.raw[self.BAND:self.BAND + nbytes].view(dtype).view(shape)

    def data_ptr(self):
        return self.view.data_ptr()

    def bands_intact(self):
        return bool((self.raw[:self.BAND] == 0xA5).all()) and bool((self.raw[self.BAND + self.nbytes:] == 0xA5).all())


@pytest.mark.parametrize("i", [1, 3, 4])
def test_outputs_and_scratch_stay_between_their_guard_bands(cuda, i):
    hp, wp, D, C, n_ctx, R, k = CASES[i]
    n = hp * wp
    tok_t, tok_c, segs = inputs(i)
    planes = Guarded(n_ctx * 2 * n * D * 2, torch.float16, (n_ctx, 2, n, D))
    tok = dev(tok_c)
    capi.check(capi.lib().dinoseg_op_normalize_tokens(tok.data_ptr(), n_ctx, n, D, planes.data_ptr(), S()))
    tq, cp, sg = device_case(i)
    assert planes.bands_intact() and torch.equal(planes.view, torch.stack(cp))
    seg = Guarded(n * C * 4, torch.float32, (n, C))
    idx = Guarded(n * k * 4, torch.int32, (n, k))
    w = Guarded(n * k * 4, torch.float32, (n, k))
    scratch = Guarded(scratch_bytes(hp, wp, n_ctx, k), torch.uint8, (-1,))
    run_propagate(tq, cp, sg, hp, wp, R, k, out=(seg.view, idx.view, w.view, scratch.view))
    torch.cuda.synchronize()
    for g in (seg, idx, w, scratch):
        assert g.bands_intact()
    want = run_propagate(tq, cp, sg, hp, wp, R, k)
    assert torch.equal(seg.view, want[0]) and torch.equal(idx.view, want[1]) and torch.equal(w.view, want[2])
    OH, OW = hp * 8 - 3, wp * 8 + 5
    cells = Guarded(n * C * 4, torch.float32, (n, C))
    y = dev(np.random.default_rng(i).integers(0, C, (OH, OW)).astype(np.int64))
    capi.check(capi.lib().dinoseg_op_label_cells(y.data_ptr(), 1, OH, OW, hp, wp, C, cells.data_ptr(), S()))
    torch.cuda.synchronize()
    assert cells.bands_intact() and torch.equal(cells.view, label_cells(y, hp, wp, C))


def test_refusals_return_minus_one_without_launching(cuda):
    hp, wp, D, C, n_ctx, R, k = 5, 7, 64, 3, 2, 2, 5
    n = hp * wp
    lib = capi.lib()
    tok = torch.randn((n_ctx, n + 1, D), device="cuda")
    planes = normalize(tok)
    segs = torch.rand((n_ctx, n, C), device="cuda")
    out = torch.full((n, C), -7.0, device="cuda")
    scratch = torch.full((scratch_bytes(hp, wp, n_ctx, k),), 0xA5, dtype=torch.uint8, device="cuda")
    cp, cs = table([planes[0], planes[1]]), table([segs[0], segs[1]])
    good = dict(tq=planes[0].data_ptr(), cp=cp, cs=cs, n_ctx=n_ctx, hp=hp, wp=wp, D=D, C=C, R=R, k=k, tau=TAU, out=out.data_ptr(),
                scratch=scratch.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.dinoseg_op_propagate(a["tq"], a["cp"], a["cs"], a["n_ctx"], a["hp"], a["wp"], a["D"], a["C"], a["R"], a["k"], a["tau"],
                                        a["out"], None, None, a["scratch"], S())

    null_entry = (ctypes.c_void_p * 2)(planes[0].data_ptr(), None)
    bad = [dict(tq=None), dict(cp=None), dict(cs=None), dict(out=None), dict(scratch=None), dict(cp=null_entry), dict(cs=null_entry),
           dict(C=0), dict(C=257), dict(k=0), dict(k=17), dict(n_ctx=0), dict(n_ctx=17), dict(R=-1), dict(tau=0.0), dict(tau=-0.1),
           dict(tau=float("nan")), dict(tau=float("inf")), dict(hp=0), dict(wp=-3), dict(D=0), dict(D=-64), dict(D=96)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "dinoseg_op_propagate" in capi.last_error(), kw
    tokp, plp = tok.data_ptr(), planes.data_ptr()
    for args in ((None, 1, n, D, plp), (tokp, 1, n, D, None), (tokp, 0, n, D, plp), (tokp, 1, 0, D, plp), (tokp, 1, n, 0, plp),
                 (tokp, 1, n, 100, plp)):
        assert lib.dinoseg_op_normalize_tokens(*args, S()) == -1
        assert "dinoseg_op_normalize_tokens" in capi.last_error()
    y = torch.zeros((40, 56), dtype=torch.int64, device="cuda")
    cells = torch.full((n, C), -7.0, device="cuda")
    yp, sp = y.data_ptr(), cells.data_ptr()
    for args in ((None, 1, 40, 56, hp, wp, C, sp), (yp, 1, 40, 56, hp, wp, C, None), (yp, 2, 40, 56, hp, wp, C, sp),
                 (yp, 1, 4, 56, hp, wp, C, sp), (yp, 1, 40, 6, hp, wp, C, sp), (yp, 1, 40, 56, 0, wp, C, sp),
                 (yp, 1, 40, 56, hp, wp, 0, sp), (yp, 1, 40, 56, hp, wp, 257, sp)):
        assert lib.dinoseg_op_label_cells(*args, S()) == -1
        assert "dinoseg_op_label_cells" in capi.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((cells == -7.0).all()) and bool((scratch == 0xA5).all())
    assert call() == 0                                                  # ... and the good call runs
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())


# ------------------------------------------------------------------------------------------------ model level
def build(cfg, precision="fp16"):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def model(patch):
    return build(A.ARCH["T2"] if patch == 8 else ViTConfig(n_blocks=1, patch=16, pos_grid=14))


def clip(T, H, W, seed):
    """a clip that drifts: one wide synthetic frame, cropped at a moving column"""
    wide = synthetic_frames(1, H, seed=seed, w=W + 4 * T)[0]
    return torch.from_numpy(np.stack([wide[:, 4 * t:4 * t + W] for t in range(T)])).cuda()


def by_hand(m, frames, first, n_classes, n_context, R, k, tau, chunk, size):
    """The operators applied by hand to features() of the same chunks: (labels [T, OH, OW], seg [T, n, C])"""
    p = m.cfg.patch
    T, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    hp, wp = H // p, W // p
    tokens = torch.cat([m.features(frames[c:c + chunk]) for c in range(0, T, chunk)])
    planes = normalize(tokens)
    if first.is_floating_point():
        segs = [first.cuda().float().contiguous()]
    else:
        segs = [label_cells(first.cuda(), hp, wp, n_classes)]
    for t in range(1, T):
        ctx = P.context_frames(t, n_context)
        segs.append(run_propagate(planes[t], [planes[c] for c in ctx], [segs[c] for c in ctx], hp, wp, R, k, tau, debug=False)[0])
    seg = torch.stack(segs)
    OH, OW = size
    labels = torch.empty((T, OH, OW), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(seg.data_ptr(), T, hp, wp, seg.shape[-1], OH, OW, labels.data_ptr(), None, S()))
    return labels, seg


def pixel_seed(H, W, C, seed):
    rng = np.random.default_rng(seed)
    y = (np.add.outer(np.arange(H) // 9, np.arange(W) // 13) % C).astype(np.int64)
    y[rng.random((H, W)) < 0.05] = 255
    return torch.from_numpy(y)


@pytest.mark.parametrize("patch,H,W", [(8, 40, 56), (16, 64, 64)])
def test_propagate_is_the_operators_by_hand_and_the_stream_is_propagate(cuda, patch, H, W):
    m = model(patch)
    T, C = 5, 6
    frames = clip(T, H, W, seed=330 + patch)
    first = pixel_seed(H, W, C, 331)
    kw = dict(n_classes=C, n_context=2, radius=2, topk=3, temperature=0.2)
    want_l, want_s = by_hand(m, frames, first, C, 2, 2, 3, 0.2, 2, (H, W))
    labels, seg = m.propagate(frames, first, chunk=2, want_seg=True, **kw)
    assert labels.dtype == torch.int32 and labels.shape == (T, H, W) and seg.shape == (T, (H // patch) * (W // patch), C)
    assert torch.equal(labels, want_l) and torch.equal(seg, want_s)
    labels2, none = m.propagate(frames, first, chunk=2, **kw)
    assert none is None and torch.equal(labels2, want_l)
    # the streaming form, frame by frame, against propagate(chunk=1)
    l1, s1 = m.propagate(frames, first, chunk=1, want_seg=True, **kw)
    stream = LabelPropagator(m, frames[0], first, want_seg=True, **kw)
    assert torch.equal(stream.labels0, l1[0]) and torch.equal(stream.seg0, s1[0])
    for t in range(1, T):
        lt, st = stream.step(frames[t])
        assert lt.shape == (H, W) and torch.equal(lt, l1[t]) and torch.equal(st, s1[t])
    with pytest.raises(ValueError):
        stream.step(frames[1][:, :-patch])


def test_identical_frames_keep_the_seed_and_both_seed_kinds_run(cuda):
    m = model(8)
    H, W, T = 40, 56, 4
    one = clip(1, H, W, seed=340)
    frames = one.expand(T, -1, -1, -1).contiguous()
    # a soft seed from the model's own head
    soft = torch.exp(m.forward_frames(one)[0])
    labels, seg = m.propagate(frames, soft, topk=1, want_seg=True, size=(H + 3, W + 5))
    assert labels.shape == (T, H + 3, W + 5) and seg.shape == (T, 35, m.cfg.n_classes)
    for t in range(T):
        assert torch.equal(seg[t], soft) and torch.equal(labels[t], labels[0])
    # an integer seed with void pixels, at a size of its own
    first = pixel_seed(2 * H, 2 * W + 1, 4, 341)
    labels, seg = m.propagate(frames, first, n_classes=4, topk=1, radius=None, want_seg=True)
    assert torch.equal(seg[0], label_cells(first.cuda(), 5, 7, 4))
    for t in range(T):
        assert torch.equal(seg[t], seg[0]) and torch.equal(labels[t], labels[0])
    # fp32 frames take the same path
    x = frames.permute(0, 3, 1, 2).float().div(255.0).contiguous()
    labels_f, _ = m.propagate(x, first, n_classes=4, topk=1)
    assert labels_f.shape == (T, H, W) and all(torch.equal(labels_f[t], labels_f[0]) for t in range(T))


@pytest.mark.parametrize("n_context", [1, 7])
def test_long_clips_follow_the_context_schedule(cuda, n_context):
    m = model(8)
    T, H, W, C = 10, 40, 56, 3
    frames = clip(T, H, W, seed=350)
    first = pixel_seed(H, W, C, 351)
    want_l, want_s = by_hand(m, frames, first, C, n_context, 12, 5, 0.1, 32, (H, W))
    labels, seg = m.propagate(frames, first, n_classes=C, n_context=n_context, want_seg=True)
    assert torch.equal(seg, want_s) and torch.equal(labels, want_l)
