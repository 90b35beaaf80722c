"""Exact probes of the split-plane pair walk on the device (tests/pair_probe_util.py): dinoseg_op_kmeans_assign, dinoseg_op_kmeans_update,
dinoseg_op_ncut_graph, dinoseg_op_ncut_graph_split and dinoseg_op_propagate on planes of small integers times a power of two, where
every product and every fp32 partial sum is exact and the int64 reference is the only right answer.  Scores, graph bits, topk_idx,
assign / best / moved / objective, partial sums and counts are compared WITHOUT a tolerance; the one bar of this file is the derived
bar of propagate's weights and values (pair_probe_util.prop_ref).  Every launch writes between guard bands into memory preset to 0xA5,
as the operators' own tests do."""
import functools

import numpy as np
import pytest
import torch

from tests import kmeans_util as KM
from tests import ncut_util as NC
from tests import pair_probe_util as PP
from tests import test_kmeans_gpu as TK
from tests import test_ncut_gpu as TN
from tests import test_ncut_split_gpu as TS
from tests import test_propagate_gpu as TP

pytestmark = pytest.mark.gpu
Guarded = TK.Guarded


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ident(case):
    return "x".join(str(v) for v in case)


def intact(*guarded):
    torch.cuda.synchronize()
    return all(g.bands_intact() for g in guarded)


# ---- kmeans ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PP.KM_CASES)), ids=lambda i: ident(PP.KM_CASES[i]))
def test_kmeans_assign_on_integer_planes_is_exact(cuda, i):
    """scores bit for bit; assign the first maximum, ties included (copies of centroids in other lanes, waves and blocks tie at every
    point); best the selected score's bits; moved exact; objective exact: sum |S_best| < 2^24 (asserted), so every partial sum of the
    tiles' xor trees and of the records launch is an integer below 2^24 times the scale."""
    case = PP.kmeans_case(i)
    ref = PP.kmeans_ref(case)
    B, n, D, K = case["shape"]
    N = B * n
    assert ref["obj_abs"] < 2 ** 24
    planes, cpl = dev(PP.stack_planes(*case["points"], case["e"])), dev(PP.stack_planes(*case["cent"], case["e"]))
    scratch = Guarded(KM.scratch_bytes(B, n, K, D), torch.uint8, (-1,))
    a, best = Guarded(N * 4, torch.int32, (N,)), Guarded(N * 4, torch.float32, (N,))
    scores = Guarded(N * K * 4, torch.float32, (N, K))
    obj, moved = Guarded(4, torch.float32, (1,)), Guarded(4, torch.int32, (1,))
    TK.km_assign(planes, cpl, scratch.view, prev=dev(ref["prev"]), out=(a.view, best.view, scores.view, obj.view, moved.view))
    assert intact(scratch, a, best, scores, obj, moved)
    flat = np.concatenate([scores.view.cpu().numpy().ravel(), np.full(64, np.nan, dtype=np.float32)])
    bad = PP.kmeans_failures(ref, flat, a.view.cpu().numpy(), best.view.cpu().numpy())
    assert not bad, bad
    assert int(moved.view) == ref["moved"]
    assert PP.same_bits(obj.view.cpu().numpy(), np.array([ref["objective"]]))
    # no previous assignment: every point moved; no scores wanted: the same selection
    a2, best2, none, obj2, moved2 = TK.km_assign(planes, cpl, scratch.view)
    assert none is None and int(moved2) == N
    assert torch.equal(a2, a.view) and torch.equal(best2.view(torch.int32), best.view.view(torch.int32))
    assert torch.equal(obj2.view(torch.int32), obj.view.view(torch.int32))
    ties = int(((ref["S"] == ref["S"].max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    print(f"kmeans probe {case['shape']}: {N * K} scores exact, {ties} of {N} points tie at their maximum, moved {ref['moved']}")


@pytest.mark.parametrize("i", range(len(PP.KM_UPDATE_CASES)), ids=lambda i: ident(PP.KM_UPDATE_CASES[i]))
def test_kmeans_update_partial_sums_on_integer_planes_are_exact(cuda, i):
    """x = (hi + lo) 2^-10 is an integer times 2^(e - 10) and a range's sum of |x[d]| stays below 2^24 of them (asserted): every order
    of the partial launch's additions gives the int64 sum.  The second case's ranges hold 1032 points: more than one list of 1024."""
    c = PP.kmeans_update_case(i)
    B, n, D, K = c["shape"]
    N = B * n
    assert c["sum_abs"] < 2 ** 24
    planes, a = dev(PP.stack_planes(*c["points"], c["e"])), dev(c["assign"])
    scratch = Guarded(KM.scratch_bytes(B, n, K, D), torch.uint8, (-1,))
    cent, cpl = torch.zeros((K, D), device="cuda"), torch.zeros((2, K, D), dtype=torch.float16, device="cuda")
    c2, p2 = Guarded(K * D * 4, torch.float32, (K, D)), Guarded(2 * K * D * 2, torch.float16, (2, K, D))
    counts = Guarded(K * 4, torch.int32, (K,))
    TK.km_update(planes, a, cent, cpl, scratch.view, out=(c2.view, p2.view, counts.view))
    assert intact(scratch, c2, p2, counts)
    raw = scratch.view.cpu().numpy()
    R = c["R"]
    assert (R, c["L"]) == KM.ranges_of(N, K)
    psum = raw[:4 * R * K * D].view(np.float32).reshape(R, K, D)
    pcount = raw[4 * R * K * D:4 * R * K * (D + 1)].view(np.int32).reshape(R, K)
    assert PP.same_bits(psum, c["psum"]), "a range's partial sum is not the int64 sum"
    assert np.array_equal(pcount, c["pcount"])
    m_d, n_d = KM.scratch_sums(raw, N, K, D)
    assert np.array_equal(m_d.astype(np.float64), c["psum"].astype(np.float64).sum(axis=0)) and np.array_equal(n_d, c["pcount"].sum(axis=0))
    assert np.array_equal(counts.view.cpu().numpy(), c["pcount"].sum(axis=0))


# ---- the 1-bit graph ---------------------------------------------------------------------------------------------------------------
ENTRIES = {"one": TN.nc_graph, "split": TS.split_graph}


def run_graphs(planes_list, taus):
    """one launch per (planes, tau) and entry into slices of two guarded arrays -> {entry: (bits bool [T, B, n, 64 W], degree [T, B, n])},
    after asserting that the split entry wrote the same words and degrees as the one-workgroup entry"""
    T = len(taus)
    B, _, n, D = planes_list[0].shape
    W = NC.words_of(n)
    got, raw = {}, {}
    for name, entry in ENTRIES.items():
        graph, degree = Guarded(T * B * n * W * 8, torch.int64, (T, B, n, W)), Guarded(T * B * n * 4, torch.int32, (T, B, n))
        for t in range(T):
            entry(planes_list[t], taus[t], out=(graph.view[t], degree.view[t]))
        assert intact(graph, degree)
        words = graph.view.cpu().numpy().view(np.uint64)
        bits = np.stack([np.stack([np.concatenate(NC.unpack_words(words[t, b], n), axis=1) for b in range(B)]) for t in range(T)])
        got[name], raw[name] = (bits, degree.view.cpu().numpy()), (graph.view, degree.view)
    assert torch.equal(raw["one"][0], raw["split"][0]) and torch.equal(raw["one"][1], raw["split"][1]), "the split entry differs"
    return got


@pytest.mark.parametrize("i", range(len(PP.NC_CASES)), ids=lambda i: ident(PP.NC_CASES[i]))
def test_threshold_sweep_reads_every_score_back_exactly(cuda, i):
    """One launch per half-integer threshold of the window (tests/test_pair_probes_cpu.py holds that every off-diagonal pair lies inside
    it): a pair's number of set bits is its integer score, so every bit at every threshold is the reference's; the graph is symmetric at
    every threshold, the degree the popcount, pad bits zero, the split entry the same words."""
    case = PP.ncut_case(i)
    ref = PP.ncut_ref(case)
    B, hp, wp, D = case["shape"]
    n = hp * wp
    planes = dev(PP.stack_planes(*case["planes"], case["e"]))
    taus = PP.sweep_taus(ref["t0"], ref["t1"], case["e"])
    assert len(taus) <= PP.MAX_SWEEP
    ts = list(range(ref["t0"], ref["t1"] + 1))
    for name, (bits, degree) in run_graphs([planes] * len(taus), taus).items():
        for b in range(B):
            bad = PP.graph_failures(ref["S"][b], ts, bits[:, b])
            assert not bad, (name, b, bad)
            assert np.array_equal(bits[:, b, :, :n].sum(axis=0), ref["counts"][b]), "a pair's count of set bits is not its score"
        assert np.array_equal(degree, bits.sum(axis=3)), "the degree is not the popcount"
    print(f"graph sweep {case['shape']}: {len(taus)} thresholds, {B * n * n} scores read back exactly, both entries")


@pytest.mark.parametrize("i", range(len(PP.NC_CASES)), ids=lambda i: ident(PP.NC_CASES[i]))
def test_indicator_frames_give_every_bit(cuda, i):
    """hi = one-hot at u(i), lo = one-hot at w(i), tau at half the product: bit = [u_i = u_j] or [u_i = w_j] or [w_i = u_j], and a pair that
    meets in lo . lo alone reads 0.  Over the phases every column of D decides some pair through each term alone (held on the CPU)."""
    B, hp, wp, D = PP.NC_CASES[i]
    n = hp * wp
    launches = -(-PP.indicator_phases(n, D) // B)
    maps = [[PP.indicator_maps(n, D, l * B + b) for b in range(B)] for l in range(launches)]
    planes = [dev(np.stack([PP.indicator_planes(u, w, D) for u, w in frames])) for frames in maps]
    for name, (bits, degree) in run_graphs(planes, [PP.IND_TAU] * launches).items():
        for l in range(launches):
            for b in range(B):
                bad = PP.indicator_failures(*maps[l][b], bits[l, b])
                assert not bad, (name, l, b, bad)
        assert np.array_equal(degree, bits.sum(axis=3))
    print(f"graph indicators {PP.NC_CASES[i]}: {launches} launches of {B} frames, both entries")


# ---- propagate ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prop(i):
    """a case and its reference, computed once"""
    case = PP.prop_case(i)
    return case, PP.prop_ref(case)


@pytest.mark.parametrize("i", range(len(PP.PR_CASES)), ids=lambda i: ident(PP.PR_CASES[i]))
def test_propagate_on_integer_planes_ranks_exactly(cuda, i):
    """topk_idx is the reference's IN RANK ORDER at every query (integer scores tie often: every tie goes to the lower global index), -1
    exactly beyond the candidates.  Weights and seg_out against fp64 formed from the exact scores, within the bar derived from the merge
    launch's instruction sequence (pair_probe_util.prop_ref states it term by term): d = s - s0 exact; x = fl(d a), |x| U; w =
    v_exp_f32(x), one ulp and |x| U ln 2 from x; W a sum of k terms, (k - 1) U; inv = 1 / W, U; w inv, U: weights within
    rw / (1 - rw) (w / W), rw = 2 (xmax U ln 2 + 2 U) + (k + 1) U; k fused multiply-adds and the product with inv: values within
    rv / (1 - rv) sum_i (w_i / W) |seg_i|, rv = 2 (xmax U ln 2 + 2 U) + (2 k + 1) U; 2^-126 per flushed weight.  No E term: the scores
    are exact.  The scale 2^e = 2^8 makes one integer step of a score 0.625 tau: the weights are not all 1 (asserted from the
    reference).  (Measured on an MI355X: weights 0.20 .. 0.30 of their bar, values 0.16 .. 0.26; 0 at k = 1.)"""
    case, ref = prop(i)
    hp, wp, D, C, n_ctx, R, k = case["shape"]
    n = hp * wp
    assert min(prop(j)[1]["x_min"] for j in range(len(PP.PR_CASES))) < -1.0       # some (s - s0) / tau is below -1
    assert k == 1 or ref["x_min"] < -1.0
    tq, cp, sg = dev(PP.stack_planes(*case["target"], case["e"])), dev(PP.stack_planes(*case["ctx"], case["e"])), dev(case["segs"])
    seg, idx, w = Guarded(n * C * 4, torch.float32, (n, C)), Guarded(n * k * 4, torch.int32, (n, k)), Guarded(n * k * 4, torch.float32, (n, k))
    scratch = Guarded(TP.scratch_bytes(hp, wp, n_ctx, k), torch.uint8, (-1,))
    TP.run_propagate(tq, [cp[c] for c in range(n_ctx)], [sg[c] for c in range(n_ctx)], hp, wp, R, k, tau=PP.PR_TAU,
                     out=(seg.view, idx.view, w.view, scratch.view))
    assert intact(seg, idx, w, scratch)
    bad = PP.topk_failures(ref, idx.view.cpu().numpy())
    assert not bad, bad
    wd, vd = w.view.cpu().numpy().astype(np.float64), seg.view.cpu().numpy().astype(np.float64)
    assert np.all(wd[ref["g"] < 0] == 0.0)
    share_w = float((np.abs(wd - ref["wn"]) / ref["bar_w"]).max())
    share_v = float((np.abs(vd - ref["V"]) / ref["bar_v"]).max())
    ties = int((ref["s"][:, :-1] == ref["s"][:, 1:]).any(axis=1).sum()) if k > 1 else 0
    print(f"propagate probe {case['shape']}: ranks exact at {n} queries ({ties} with a tie inside their selection); weights at most "
          f"{share_w:.3f} of their bar, values {share_v:.3f} of theirs; (s - s0) / tau down to {ref['x_min']:.2f}")
    assert share_w <= 1.0 and share_v <= 1.0
