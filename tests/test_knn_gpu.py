"""k-NN label retrieval on the device: dinoseg_op_knn_labels through the C-ABI against the fp64 restatement of the rule
(tests/knn_util.py) -- decided and undecided queries, split invariance, exact ties, exact integer probes, self-retrieval, dead rows,
batching, containment, refusals -- and DINOSeg.segment_knn / MemoryBank against the operators applied by hand."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, KnnResult, MemoryBank, capi, procedural_state_dict, sample_indices
from dino_amd.weights import VIT_S8, synthetic_frames
from tests import arch_util as A
from tests import knn_util as K
from tests import pair_probe_util as PP
from tests import propagate_util as P
from tests.test_propagate_gpu import by_key, dev, normalize, run_propagate

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
TAU = K.TAU
UNDECIDED_CAP = 0.04


def scratch_bytes(N, M, k, splits):
    nbytes = capi.lib().dinoseg_knn_scratch_bytes(N, M, k, splits)
    assert nbytes == 8 * (splits or capi.lib().dinoseg_knn_splits(N, M, k)) * N * k
    return nbytes


def run_knn(qp, bp, M, labels, C, k, tau=TAU, splits=0, debug=True, out=None):
    """device tensors in: query planes [B, 2, n, D], bank planes [2, bank_rows, D], labels soft fp32 [bank_rows, C] or hard uint8
    [bank_rows] -> (seg_out [N, C], topk_idx [N, k], topk_w [N, k], scratch)"""
    B, _, n, D = qp.shape
    N, rows, kind = B * n, bp.shape[1], K.HARD if labels.dtype == torch.uint8 else K.SOFT
    if out is None:
        seg = torch.empty((N, C), dtype=torch.float32, device="cuda")
        idx = torch.empty((N, k), dtype=torch.int32, device="cuda") if debug else None
        w = torch.empty((N, k), dtype=torch.float32, device="cuda") if debug else None
        scratch = torch.empty((scratch_bytes(N, M, k, splits),), dtype=torch.uint8, device="cuda")
    else:
        seg, idx, w, scratch = out
    capi.check(capi.lib().dinoseg_op_knn_labels(qp.data_ptr(), B, n, bp.data_ptr(), M, rows, labels.data_ptr(), kind, D, C, k, tau,
                                                splits, seg.data_ptr(), capi.ptr(idx), capi.ptr(w), scratch.data_ptr(), S()))
    return seg, idx, w, scratch


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3]))


@functools.lru_cache(maxsize=None)
def device_case(i):
    """a case on the device: (query planes, bank planes, labels), normalised there"""
    tok_q, tok_b, labels = K.make_case(i)
    return normalize(dev(tok_q)), normalize(dev(tok_b))[0], dev(labels)


@functools.lru_cache(maxsize=None)
def reference(i):
    """the fp64 restatement of a case from the device's own planes (the rule's defined rows), computed once"""
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    qp, bp, labels = device_case(i)
    return K.knn_host(qp.cpu().numpy(), bp.cpu().numpy(), M, labels.cpu().numpy(), kind, C, k, TAU)


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.case_id)
def test_operator_against_fp64_restatement(cuda, i):
    """Propagate's bars.  Scores within E(D) = (D + 16) 2^-24 (read from the scratch of a one-range run).  Decided queries (fp64 gap
    at the cut above 2E, or M <= k): the selection is the host's as a set, w / W within 4E / tau, seg_out within the values bar
    (4E / tau + (16 + 2k) 2^-24) max|labels|.  Undecided queries: every selected score >= s_cut - 2E and every unselected one <=
    s_cut + 2E in fp64, seg_out within the bar of the value formed from the device's own selection.  At most 4 % of a case's queries
    are undecided.  The reference reads the device's own planes: the rule defines its rows as (hi + lo) 2^-10.  (Measured on an
    MI355X: undecided 0, 0, 0, 0, 1.77 %, 0.52 %, 1.69 % of the queries in case order; scores at 0.019 of their bar at most, weights
    and values at 0.001 of theirs.)"""
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    qp, bp, labels = device_case(i)
    q, bank = K.query_rows(qp.cpu().numpy()), K.plane_rows(bp.cpu().numpy())
    lab = labels.cpu().numpy()
    g_host, w_host, V_host, ranked = reference(i)
    lmax = float(np.abs(lab).max()) if kind == K.SOFT else 1.0
    E, bar = P.score_bar(D), P.value_bar(D, k, TAU, lmax)
    seg, idx, w = (t.cpu().numpy() for t in run_knn(qp, bp, M, labels, C, k)[:3])
    idx = idx.astype(np.int64)
    # the scores: a one-range run leaves every query's merged list in the scratch, [N][k] scores then [N][k] rows
    seg1, idx1, w1, scratch = run_knn(qp, bp, M, labels, C, k, splits=1)
    assert np.array_equal(seg1.cpu().numpy().view(np.uint32), seg.view(np.uint32)) and np.array_equal(idx1.cpu().numpy(), idx)
    N = B * n
    cand_s = scratch[:4 * N * k].view(torch.float32).view(N, k).cpu().numpy().astype(np.float64)
    cand_g = scratch[4 * N * k:].view(torch.int32).view(N, k).cpu().numpy().astype(np.int64)
    assert np.array_equal(cand_g, idx)
    s_dev = K.scores_of(q, bank, idx)
    assert np.all(np.isneginf(cand_s[idx < 0]))
    s_err = float(np.abs(cand_s[idx >= 0] - s_dev[idx >= 0]).max())
    dec = P.decided(ranked, k, E)
    share = 1.0 - float(dec.mean())
    # every device selection is K' distinct live rows in rank order, -1 beyond
    kept = min(k, M)
    assert np.all(idx[:, :kept] >= 0) and np.all(idx[:, :kept] < M) and np.all(idx[:, kept:] == -1)
    assert np.all((w > 0) == (idx >= 0))
    assert all(len(set(row[:kept])) == kept for row in idx[:: max(1, N // 64)])
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
        s_rank, g_rank, _ = ranked
        cut = s_rank[und, k - 1]
        assert np.all(s_dev[und] >= cut[:, None] - 2.0 * E), "an undecided query selected a score below the cut's band"
        for row, qi in enumerate(und):
            assert len(set(idx[qi])) == k
            rest = ~np.isin(g_rank[qi], idx[qi])
            assert np.all(s_rank[qi][rest] <= cut[row] + 2.0 * E), "an undecided query left out a score above the cut's band"
        _, V_dev = P.weights_and_value(s_dev[und], idx[und], K.label_rows(lab, kind, C)[None], TAU)
        u_err = float(np.abs(seg[und].astype(np.float64) - V_dev).max())
    print(f"knn {K.CASES[i]}: undecided {share:.4f} of the queries; scores {s_err / E:.3f} of their bar, weights "
          f"{w_err / (4 * E / TAU):.3f}, values {v_err / bar:.3f} (decided) and {u_err / bar:.3f} (undecided) of theirs (bar {bar:.3e})")
    assert s_err <= E
    assert share <= UNDECIDED_CAP
    assert w_err <= 4.0 * E / TAU
    assert v_err <= bar and u_err <= bar


@pytest.mark.parametrize("i", [4, 5, 6], ids=K.case_id)
def test_every_number_of_splits_gives_the_same_bits(cuda, i):
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    qp, bp, labels = device_case(i)
    cap = K.split_cap(M, k)
    assert cap >= 5 and capi.lib().dinoseg_knn_splits(B * n, M, k) == K.library_splits(B * n, M, k)
    own = run_knn(qp, bp, M, labels, C, k)
    for splits in (1, 2, 5, cap):
        assert same_bits(run_knn(qp, bp, M, labels, C, k, splits=splits), own), splits


@pytest.mark.parametrize("k", [1, 4])
def test_exact_ties_go_to_the_lower_row(cuda, k):
    """The bank holds the same m rows twice, M = 2 m: twins score bit-equal, so the order inside a pair is the row index alone."""
    m, n, D, C = 100, 70, 64, 4
    rng = np.random.default_rng(410)
    qp = normalize(dev(rng.standard_normal((1, n + 1, D)).astype(np.float32)))
    half = normalize(dev(rng.standard_normal((1, m + 1, D)).astype(np.float32)))[0]
    bp = torch.cat([half, half], dim=1).contiguous()
    labels = dev(rng.random((2 * m, C)).astype(np.float32))
    # the host ranks the m distinct rows; a pair is then (g, g + m) with one score (two columns of a BLAS product need not agree bitwise)
    s, g, _ = K.ranked(K.query_rows(qp.cpu().numpy()), K.plane_rows(half.cpu().numpy()), m)
    g_host = np.stack([g[:, :3], g[:, :3] + m], axis=2).reshape(n, 6)[:, :k]
    _, V_host = P.weights_and_value(np.repeat(s[:, :3], 2, axis=1)[:, :k], g_host, labels.cpu().numpy()[None], TAU)
    clear = np.all(s[:, 0:2] - s[:, 1:3] > 2.0 * P.score_bar(D), axis=1)                 # v1 > v2 > v3 beyond the bar
    assert clear.mean() > 0.5
    for splits in (1, 4):                                               # (4 key blocks: at 4 ranges most twins meet in the merge)
        seg, idx, w, _ = (t.cpu().numpy() for t in run_knn(qp, bp, 2 * m, labels, C, k, splits=splits))
        idx = idx.astype(np.int64)
        assert np.all(idx[:, 0::2] < m), "a pair's upper row came first"
        if k == 4:
            assert np.all(idx[:, 0] + m == idx[:, 1]) and np.all(idx[:, 2] + m == idx[:, 3])
            wb = w.view(np.uint32)
            assert np.array_equal(wb[:, 0], wb[:, 1]) and np.array_equal(wb[:, 2], wb[:, 3])
        assert np.array_equal(idx[clear], g_host[clear]), "with clear gaps even the rank order is the host's"
        bar = P.value_bar(D, k, TAU, 1.0)
        assert np.abs(seg[clear].astype(np.float64) - V_host[clear]).max() <= bar


@pytest.mark.parametrize("splits", [1, None], ids=["one", "cap"])
@pytest.mark.parametrize("n_ctx,k", [(1, 1), (2, 5), (3, 16)])
def test_whole_frame_propagation_is_knn_over_the_context_rows(cuda, n_ctx, k, splits):
    """With the whole frame as neighbourhood, dinoseg_op_propagate is dinoseg_op_knn_labels over the context frames' rows laid end to
    end: g = ci n + cell is the bank row, the stacked segs are the soft labels, and order, weights and gather are one piece of code
    (csrc/select_common.h).  seg_out, topk_idx and topk_w agree as bits, at one range and at the most the bank allows.  9 x 11 cells:
    a ragged second query tile here, ragged 8 x 8 tiles there, two key blocks per frame.  Context frame 1 is a copy of frame 0, so
    every query meets exact ties, which both break towards the lower index."""
    hp, wp, D, C, R = 9, 11, 64, 7, 12
    n = hp * wp
    M = n_ctx * n
    rng = np.random.default_rng(470 + n_ctx)
    tok_c = rng.standard_normal((n_ctx, n + 1, D)).astype(np.float32)
    if n_ctx >= 2:
        tok_c[1] = tok_c[0]
    tq = normalize(dev(rng.standard_normal((1, n + 1, D)).astype(np.float32)))       # [1, 2, n, D]: knn's query planes as they are
    cp = normalize(dev(tok_c))                                                       # [n_ctx, 2, n, D]
    segs = dev(rng.random((n_ctx, n, C)).astype(np.float32))
    bank = cp.permute(1, 0, 2, 3).reshape(2, M, D).contiguous()                      # the hi planes of all frames, then the lo planes
    want = run_propagate(tq[0], [cp[c] for c in range(n_ctx)], [segs[c] for c in range(n_ctx)], hp, wp, R, k, tau=TAU)
    got = run_knn(tq, bank, M, segs.view(M, C), C, k, tau=TAU, splits=splits or K.split_cap(M, k))
    for name, a, b in zip(("seg_out", "topk_idx", "topk_w"), got[:3], want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    if n_ctx >= 2:                                                      # the ties were met: a twin follows its lower copy at once
        idx = got[1].cpu().numpy()
        assert not np.any((idx[:, 0] >= n) & (idx[:, 0] < 2 * n))
        low = idx[:, 0] < n
        assert low.any() and np.array_equal(idx[low, 1], idx[low, 0] + n)


def test_integer_planes_select_and_score_exactly(cuda):
    """Planes of small integers (tests/pair_probe_util.py): every fp32 partial sum is exact, so the scores and the selection --
    with the many exact ties that integer scores have -- compare without a tolerance.  The first ten queries have their best row
    planted at the first and last row of each of the three ranges and at rows 63 / 64 of a key block."""
    B, n, M, rows, D, C, k, mmax = 2, 50, 700, 704, 64, 3, 5, 4
    assert PP.exact_ok(D, mmax)
    N = B * n
    qh, ql = PP.int_planes(420, (N, D), mmax, 0.5)
    kh, kl = PP.int_planes(421, (rows, D), mmax, 0.5)
    ranges = K.split_ranges(M, 3)
    assert ranges == [(0, 192), (192, 448), (448, 700)]
    spots = [0, 191, 192, 447, 448, 699, 63, 64, 255, 256]
    for j, g in enumerate(spots):
        kh[g] = kl[g] = mmax * np.sign(qh[j])
    Sint = PP.int_scores(qh, ql, kh[:M], kl[:M])
    want_s, want_g = PP.rank_rows(PP.f32_of(Sint, 0).astype(np.float64), np.broadcast_to(np.arange(M), (N, M)))
    assert np.array_equal(want_g[:len(spots), 0], spots) and np.all(want_s[:len(spots), 0] > want_s[:len(spots), 1])
    assert (want_s[:, k - 1] == want_s[:, k]).mean() > 0.05, "the probe should put exact ties at the cut"
    qp = dev(PP.stack_planes(qh.reshape(B, n, D), ql.reshape(B, n, D), 0))
    bp = dev(PP.stack_planes(kh, kl, 0))
    labels = dev(np.random.default_rng(422).random((rows, C)).astype(np.float32))
    for splits in (1, 3, K.split_cap(M, k)):
        seg, idx, w, scratch = run_knn(qp, bp, M, labels, C, k, splits=splits)
        assert np.array_equal(idx.cpu().numpy(), want_g[:, :k]), splits
        if splits == 1:
            cand_s = scratch[:4 * N * k].view(torch.float32).view(N, k).cpu().numpy()
            assert np.array_equal(cand_s.view(np.uint32), want_s[:, :k].astype(np.float32).view(np.uint32))
    # splits = 3: what each range left in the scratch is that range's own exact top k
    seg, idx, w, scratch = run_knn(qp, bp, M, labels, C, k, splits=3)
    cand_g = scratch[4 * 3 * N * k:].view(torch.int32).view(3, N, k).cpu().numpy()
    for s, (a, b) in enumerate(ranges):
        _, g_s = PP.rank_rows(PP.f32_of(Sint[:, a:b], 0).astype(np.float64), np.broadcast_to(np.arange(a, b), (N, b - a)))
        assert np.array_equal(cand_g[s], g_s[:, :k]), s


@pytest.mark.parametrize("kind", [K.SOFT, K.HARD])
def test_a_bank_retrieves_itself(cuda, kind):
    """The bank as its own query set with k = 1: topk_idx[q] = q, w = W = 1, and seg_out is the bank's soft rows bit for bit; in
    the hard kind the one-hot of the label, all zero for a void row."""
    M, D, C = 300, 64, 9
    rng = np.random.default_rng(430)
    bp = normalize(dev(rng.standard_normal((1, M + 1, D)).astype(np.float32)))
    if kind == K.SOFT:
        lab = rng.random((M, C)).astype(np.float32)
    else:
        lab = rng.integers(0, C, M).astype(np.uint8)
        lab[::7] = K.VOID
    seg, idx, w, _ = (t.cpu().numpy() for t in run_knn(bp, bp[0], M, dev(lab), C, 1))
    assert np.array_equal(idx[:, 0], np.arange(M)) and np.all(w == 1.0)
    want = lab if kind == K.SOFT else K.label_rows(lab, kind, C).astype(np.float32)
    assert np.array_equal(seg.view(np.uint32), want.view(np.uint32))
    if kind == K.HARD:
        assert np.all(seg[::7] == 0.0) and np.all(seg.sum(axis=1)[lab < C] == 1.0)


@pytest.mark.parametrize("i", [1, 3, 5], ids=K.case_id)
def test_dead_rows_change_no_bit(cuda, i):
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    assert rows > M
    qp, bp, labels = device_case(i)
    want = run_knn(qp, bp, M, labels, C, k)
    bp2, lab2 = bp.clone(), labels.clone()
    bp2[:, M:] = float("nan")
    if kind == K.SOFT:
        lab2[M:] = float("nan")
    else:
        lab2[M:] = (lab2[M:].to(torch.int32) * 37 + 11).to(torch.uint8)
    assert same_bits(run_knn(qp, bp2, M, lab2, C, k), want)


@pytest.mark.parametrize("i", [2, 4], ids=K.case_id)
def test_frames_batch_and_runs_repeat_bit_for_bit(cuda, i):
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    assert B > 1
    qp, bp, labels = device_case(i)
    a = run_knn(qp, bp, M, labels, C, k)
    assert same_bits(run_knn(qp, bp, M, labels, C, k), a)
    assert torch.equal(run_knn(qp, bp, M, labels, C, k, debug=False)[0].view(torch.int32), a[0].view(torch.int32))
    for b in range(B):
        one = run_knn(qp[b:b + 1].contiguous(), bp, M, labels, C, k)
        assert same_bits(one, [t[b * n:(b + 1) * n] for t in a[:3]]), b


class Guarded:
    """`nbytes` of device memory between two guard bands of 4 KiB, everything filled with 0xA5"""
    BAND = 4096

    def __init__(self, nbytes, dtype, shape):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * self.BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.raw[self.BAND:self.BAND + nbytes].view(dtype).view(shape)

    def bands_intact(self):
        return bool((self.raw[:self.BAND] == 0xA5).all()) and bool((self.raw[self.BAND + self.nbytes:] == 0xA5).all())


@pytest.mark.parametrize("i", [1, 2, 3], ids=K.case_id)
def test_outputs_and_scratch_stay_between_their_guard_bands(cuda, i):
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    N = B * n
    qp, bp, labels = device_case(i)
    for splits in (0, K.split_cap(M, k)):
        seg = Guarded(N * C * 4, torch.float32, (N, C))
        idx = Guarded(N * k * 4, torch.int32, (N, k))
        w = Guarded(N * k * 4, torch.float32, (N, k))
        scratch = Guarded(scratch_bytes(N, M, k, splits), torch.uint8, (-1,))
        run_knn(qp, bp, M, labels, C, k, splits=splits, out=(seg.view, idx.view, w.view, scratch.view))
        torch.cuda.synchronize()
        for g in (seg, idx, w, scratch):
            assert g.bands_intact()
        assert same_bits((seg.view, idx.view, w.view), run_knn(qp, bp, M, labels, C, k))


def test_refusals_return_minus_one_without_launching(cuda):
    B, n, M, rows, D, C, k = 1, 35, 130, 192, 64, 3, 5
    lib = capi.lib()
    qp = normalize(torch.randn((B, n + 1, D), device="cuda"))
    bp = normalize(torch.randn((1, rows + 1, D), device="cuda"))[0]
    soft = torch.rand((rows, C), device="cuda")
    out = torch.full((B * n, C), -7.0, device="cuda")
    idx = torch.full((B * n, k), -7, dtype=torch.int32, device="cuda")
    scratch = torch.full((scratch_bytes(B * n, M, k, 2),), 0xA5, dtype=torch.uint8, device="cuda")
    good = dict(qp=qp.data_ptr(), B=B, n=n, bp=bp.data_ptr(), M=M, rows=rows, lab=soft.data_ptr(), kind=0, D=D, C=C, k=k, tau=TAU,
                splits=2, out=out.data_ptr(), scratch=scratch.data_ptr())

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.dinoseg_op_knn_labels(a["qp"], a["B"], a["n"], a["bp"], a["M"], a["rows"], a["lab"], a["kind"], a["D"], a["C"], a["k"],
                                         a["tau"], a["splits"], a["out"], idx.data_ptr(), None, a["scratch"], S())

    bad = [dict(qp=None), dict(bp=None), dict(lab=None), dict(out=None), dict(scratch=None),
           dict(C=0), dict(C=257), dict(k=0), dict(k=17), dict(splits=-1), dict(splits=4), dict(splits=17), dict(kind=-1), dict(kind=2),
           dict(D=0), dict(D=-64), dict(D=96), dict(D=8256), dict(M=0), dict(M=-5), dict(M=rows + 1), dict(rows=(1 << 24) + 1, M=1 << 24),
           dict(rows=0, M=0), dict(tau=0.0), dict(tau=-0.1), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=1e-40),
           dict(B=0), dict(n=0), dict(B=-1), dict(B=1 << 20, n=1 << 20), dict(B=128, n=1 << 24), dict(n=(1 << 24) + 1),
           dict(qp=qp.data_ptr() + 8), dict(bp=bp.data_ptr() + 2)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "dinoseg_op_knn_labels" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((idx == -7).all()) and bool((scratch == 0xA5).all())
    assert call() == 0                                                  # ... and the good call runs
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not bool((idx == -7).any())


# ------------------------------------------------------------------------------------------------ model level
def build(cfg, precision="fp16"):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def model(arch):
    return build(A.ARCH["T2"] if arch == "tiny" else VIT_S8)


H, W = 64, 128


def frames_of(B, seed, fp32):
    x = torch.from_numpy(synthetic_frames(B, H, seed=seed, w=W)).cuda()
    return x.permute(0, 3, 1, 2).float().div(255.0).contiguous() if fp32 else x


def pixel_labels(B, OH, OW, C, seed):
    rng = np.random.default_rng(seed)
    y = np.stack([(np.add.outer(np.arange(OH) // 9, np.arange(OW) // 13 + b) % C) for b in range(B)]).astype(np.int64)
    y[rng.random((B, OH, OW)) < 0.05] = 255
    y[rng.random((B, OH, OW)) < 0.02] = -100
    return torch.from_numpy(y)


def label_cells(y, hp, wp, C):
    kind = 0 if y.dtype == torch.uint8 else 1
    seg = torch.empty((hp * wp, C), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_label_cells(y.data_ptr(), kind, y.shape[0], y.shape[1], hp, wp, C, seg.data_ptr(), S()))
    return seg


def enlarge(seg, B, hp, wp, OH, OW):
    labels = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(seg.data_ptr(), B, hp, wp, seg.shape[-1], OH, OW, labels.data_ptr(), None, S()))
    return labels


@pytest.mark.parametrize("fp32", [False, True], ids=["uint8", "fp32"])
@pytest.mark.parametrize("arch", ["tiny", "vits8"])
def test_segment_knn_is_the_operators_by_hand(cuda, arch, fp32):
    m = model(arch)
    p, C, k = m.cfg.patch, 5, 3
    hp, wp = H // p, W // p
    n = hp * wp
    bank = MemoryBank(m, C, 3 * n)
    assert bank.add(frames_of(2, 440, fp32), pixel_labels(2, H, W, C, 441)) == 2 * n and bank.size == 2 * n
    x = frames_of(3, 442, fp32)
    got = m.segment_knn(x, bank, topk=k, temperature=0.2, chunk=2, size=(H + 3, W - 5), want_seg=True, want_idx=True)
    assert isinstance(got, KnnResult) and got.labels.dtype == torch.int32 and got.labels.shape == (3, H + 3, W - 5)
    assert got.seg.shape == (3, n, C) and got.idx.shape == (3, n, k) and got.idx.dtype == torch.int32
    # by hand: features, normalise, the operator, the enlargement
    planes = normalize(m.features(x))
    seg, idx, _, _ = run_knn(planes, bank.planes, bank.size, bank.labels, C, k, tau=0.2)
    assert torch.equal(got.seg.view(-1, C), seg) and torch.equal(got.idx.view(-1, k), idx)
    assert torch.equal(got.labels, enlarge(seg, 3, hp, wp, H + 3, W - 5))
    # chunk = 1 (the camera's form) equals chunk = 32; without the optional outputs the labels are the same
    for chunk in (1, 32):
        other = m.segment_knn(x, bank, topk=k, temperature=0.2, chunk=chunk, size=(H + 3, W - 5))
        assert other.seg is None and other.idx is None and torch.equal(other.labels, got.labels)
    one = m.segment_knn(x[1:2], bank, topk=k, temperature=0.2, size=(H + 3, W - 5), want_seg=True)
    assert torch.equal(one.labels[0], got.labels[1]) and torch.equal(one.seg[0], got.seg[1])
    # refusals come before any launch
    for kw in (dict(topk=0), dict(topk=17), dict(temperature=0.0), dict(size=(1, 1)), dict(chunk=0), dict(n_blocks=1)):
        with pytest.raises(ValueError):
            m.segment_knn(x, bank, **kw)
    with pytest.raises(ValueError):
        m.segment_knn(x, MemoryBank(m, C, 10))                          # an empty bank


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("arch", ["tiny", "vits8"])
def test_a_frame_retrieves_its_own_labels(cuda, arch, hard):
    """A bank built from one frame and its pixel labels, queried with that frame at topk = 1: every cell finds itself, so the
    result is label_cells + the enlargement of those labels at every pixel (in the hard kind, of their first maximum's one-hot)."""
    m = model(arch)
    p, C = m.cfg.patch, 4
    hp, wp = H // p, W // p
    x = frames_of(1, 450, False)
    y = pixel_labels(1, 2 * H, 2 * W + 1, C, 451)
    bank = MemoryBank(m, C, hp * wp, hard=hard)
    bank.add(x, y)
    got = m.segment_knn(x, bank, topk=1, want_seg=True, want_idx=True)
    assert torch.equal(got.idx.view(-1), torch.arange(hp * wp, dtype=torch.int32, device="cuda"))
    cells = label_cells(y[0].cuda(), hp, wp, C)
    if hard:
        top = cells.max(dim=1, keepdim=True).values
        first = torch.where(cells == top, torch.arange(C, device="cuda"), C).min(dim=1).values
        want = torch.where(top[:, 0] > 0, first, 255)
        assert torch.equal(bank.labels.to(torch.int64), want)                            # the first maximum, 255 where all zero
        cells = (want[:, None] == torch.arange(C, device="cuda")[None, :]).float()
    assert torch.equal(got.seg[0], cells)
    assert torch.equal(got.labels, enlarge(cells, 1, hp, wp, H, W))


def test_memory_bank_add_sample_overflow_and_state(cuda):
    m = model("tiny")
    p, C, per = m.cfg.patch, 6, 20
    hp, wp = H // p, W // p
    n = hp * wp
    x, y = frames_of(3, 460, False), pixel_labels(3, H, W, C, 461)
    bank = MemoryBank(m, C, 2 * n + per + 1, hard=True)
    full = MemoryBank(m, C, 3 * n)
    assert full.add(x, y) == 3 * n
    # per_frame = m keeps exactly the rows of sample_indices, frame i of the bank drawing from seed + i
    assert bank.add(x[:2], y[:2].to(torch.uint8), per_frame=per, seed=7) == 2 * per
    assert bank.add(x[2:], y[2:], per_frame=per, seed=7) == per and bank.size == 3 * per and bank.frames == 3
    for b in range(3):
        keep = sample_indices(n, per, 7 + b).cuda()
        at = slice(b * per, (b + 1) * per)
        assert torch.equal(bank.planes[:, at], full.planes[:, b * n:(b + 1) * n][:, keep])
        rows = full.labels[b * n:(b + 1) * n][keep]
        top = rows.max(dim=1).values
        first = torch.tensor([int(torch.nonzero(r == t)[0]) if t > 0 else 255 for r, t in zip(rows.cpu(), top.cpu())])
        assert torch.equal(bank.labels[at].cpu().to(torch.int64), first)                 # hard = the first maximum of the soft row
    assert bool((full.labels.sum(dim=1) < 1.0).any())                   # (void pixels: shares that do not add up to one)
    # overflow raises and adds nothing
    before = (bank.size, bank.frames, bank.planes.clone(), bank.labels.clone())
    with pytest.raises(ValueError):
        bank.add(x, y)
    assert (bank.size, bank.frames) == before[:2] and torch.equal(bank.planes, before[2]) and torch.equal(bank.labels, before[3])
    # the state round-trips bit for bit
    state = bank.state_dict()
    assert set(state) >= {"planes", "labels", "size", "n_classes", "hard", "n_blocks"}
    other = MemoryBank(m, C, bank.capacity, hard=True)
    other.load_state_dict(state)
    assert other.size == bank.size and other.frames == bank.frames
    assert torch.equal(other.planes.view(torch.int16), bank.planes.view(torch.int16)) and torch.equal(other.labels, bank.labels)
    q = frames_of(1, 462, False)
    assert torch.equal(m.segment_knn(q, other, topk=4).labels, m.segment_knn(q, bank, topk=4).labels)
    with pytest.raises(ValueError):
        MemoryBank(m, C, bank.capacity).load_state_dict(state)          # a soft bank does not take a hard one's state
    bank.clear()
    assert bank.size == 0 and bank.frames == 0
    with pytest.raises(ValueError):
        m.segment_knn(q, bank)
