"""k-NN label retrieval without a device: the host restatement (tests/knn_util.py) against the plain matrix form in fp64, the
bank's split ranges and the library's host-only entries, the plan layer's refusals, and the share of undecided queries of every
device case from the host alone."""
import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, KnnResult, MemoryBank, capi
from dino_amd.dense_plan import bank_add_plan, knn_plan
from tests import knn_util as K
from tests import propagate_util as P


def matrix_form(q, bank, rows, k, tau):
    """Q @ Bank.T, a stable sort, softmax over the kept scores, @ labels -> V [N, C]"""
    s = q @ bank.T
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    z = np.take_along_axis(s, order, axis=1) / tau
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return np.einsum("qk,qkc->qc", e / e.sum(axis=1, keepdims=True), rows[order])


@pytest.mark.parametrize("B,n,M,rows,D,C,k,kind", [(1, 20, 30, 30, 64, 4, 5, K.SOFT), (2, 13, 50, 64, 64, 6, 3, K.HARD),
                                                   (1, 9, 3, 8, 128, 3, 5, K.SOFT), (1, 17, 70, 70, 64, 5, 1, K.HARD)])
def test_host_rule_is_the_matrix_form(B, n, M, rows, D, C, k, kind):
    rng = np.random.default_rng(50 + n)
    qp = K.split_rows(rng.standard_normal((B, n, D)))
    bp = K.split_rows(rng.standard_normal((rows, D)))
    labels = rng.random((rows, C)).astype(np.float32) if kind == K.SOFT else rng.integers(0, C + 2, rows).astype(np.uint8)
    g, wn, V, ranked = K.knn_host(qp, bp, M, labels, kind, C, k, K.TAU)
    assert np.all(np.diff(ranked[0][:, :k + 1], axis=1) < 0), "ties in a random case"
    kk = min(k, M)
    assert np.all(g[:, :kk] >= 0) and np.all(g[:, :kk] < M) and np.all(g[:, kk:] == -1)
    # the rule rounds a = log2(e) / tau to fp32 once, so the matrix form runs at the temperature that a stands for
    want = matrix_form(K.query_rows(qp), K.plane_rows(bp)[:M], K.label_rows(labels, kind, C)[:M], k, P.LOG2E / P.scale_a(K.TAU))
    assert np.abs(V - want).max() <= 1e-12
    assert np.abs(wn.sum(axis=1) - 1.0).max() <= 1e-12
    if kind == K.HARD:
        assert (labels[:M] >= C).any() and np.all(V.sum(axis=1) <= 1.0 + 1e-12)        # void rows add to no class


def test_planes_carry_the_unit_rows():
    f = np.random.default_rng(51).standard_normal((40, 384))
    planes = K.split_rows(f)
    assert planes.dtype == np.float16 and planes.shape == (2, 40, 384)
    assert np.abs(K.plane_rows(planes) - P.unit_rows(f)).max() <= 2.0 ** -24


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129, 1000])
def test_split_ranges_tile_the_bank(M):
    lib = capi.lib()
    for k in (1, 5, 16):
        cap = K.split_cap(M, k)
        assert cap == min(16, 256 // k, -(-M // 64)) >= 1
        for S in range(1, cap + 1):
            ranges = K.split_ranges(M, S)
            assert ranges[0][0] == 0 and ranges[-1][1] == M
            for (a, b), (a2, _) in zip(ranges, ranges[1:] + [(M, M)]):
                assert a < b == a2 and a % 64 == 0                      # never empty, contiguous, whole key blocks
            assert all(b % 64 == 0 for _, b in ranges[:-1])
            assert lib.dinoseg_knn_scratch_bytes(100, M, k, S) == 8 * S * 100 * k
        assert lib.dinoseg_knn_scratch_bytes(100, M, k, cap + 1) == -1
        for N in (1, 64, 100, 4800, 40000):
            S = lib.dinoseg_knn_splits(N, M, k)
            assert S == K.library_splits(N, M, k) and 1 <= S <= cap
            assert lib.dinoseg_knn_scratch_bytes(N, M, k, 0) == 8 * S * N * k


def test_symbols_and_host_entries():
    lib = capi.lib()
    declared = capi.header_symbols()
    for name in ("dinoseg_op_knn_labels", "dinoseg_knn_scratch_bytes", "dinoseg_knn_splits"):
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name)
    f, g = lib.dinoseg_knn_scratch_bytes, lib.dinoseg_knn_splits
    assert g(4800, 100000, 5) == 7 and g(3600, 1000000, 10) == 9 and g(64, 1 << 24, 16) == 16 and g(1 << 20, 1 << 20, 1) == 1
    assert g(64, 255, 1) == 1 and g(64, 256, 1) == 1 and g(64, 512, 1) == 2            # ranges of at least 4 key blocks
    assert f(4800, 100000, 5, 0) == 8 * 7 * 4800 * 5 < 4 * 4800 * 100000 // 100        # far below the [N, M] fp32 score matrix
    assert f(1, 1, 1, 0) == f(1, 1, 1, 1) == 8
    for bad in ((0, 10, 5), (-1, 10, 5), (10, 0, 5), (10, (1 << 24) + 1, 5), (10, 10, 0), (10, 10, 17), ((1 << 31) - 255, 10, 5)):
        assert g(*bad) == -1 and f(*bad, 0) == -1
    assert f(10, 1000, 5, -1) == -1 and f(10, 1000, 5, 17) == -1 and f(10, 1000, 16, 16) == 8 * 16 * 10 * 16
    assert f(10, 1000, 16, 0) > 0 and f(10, 2000, 16, 17) == -1 and f(10, 64, 5, 2) == -1


def test_knn_plan_refusals_need_no_device():
    p, D = 8, 384
    x = torch.zeros((3, 40, 56, 3), dtype=torch.uint8)
    good = dict(x=x, bank_size=100, bank_dim=D, bank_classes=7, bank_blocks=0)
    ok = knn_plan(p, D, **good)
    assert (ok.B, ok.hp, ok.wp, ok.M, ok.C, ok.OH, ok.OW, ok.kind) == (3, 5, 7, 100, 7, 40, 56, capi.INPUT_U8_HWC)
    assert (ok.topk, ok.temperature, ok.chunk, ok.n_blocks) == (10, 0.1, 32, 0)
    f32 = knn_plan(p, D, **dict(good, x=x.permute(0, 3, 1, 2).float(), bank_blocks=2, n_blocks=2, size=(5, 7)))
    assert (f32.kind, f32.n_blocks, f32.OH, f32.OW) == (capi.INPUT_F32_CHW, 2, 5, 7)
    bad = [
        dict(x=torch.zeros((3, 40, 56), dtype=torch.uint8)),                            # layout
        dict(x=torch.zeros((3, 41, 56, 3), dtype=torch.uint8)),                         # not a patch multiple
        dict(x=torch.zeros((0, 40, 56, 3), dtype=torch.uint8)),                         # empty batch
        dict(x=np.zeros((3, 40, 56, 3), dtype=np.uint8)),                               # not a tensor
        dict(topk=0), dict(topk=17), dict(topk=True), dict(topk=2.0),
        dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
        dict(temperature="hot"),
        dict(size=(4, 56)), dict(size=(40, 6)), dict(size=40),
        dict(chunk=0), dict(chunk=1.5),
        dict(bank_size=0),                                                              # an empty bank
        dict(bank_dim=768),                                                             # another model's rows
        dict(n_blocks=1),                                                               # features after another number of blocks
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            knn_plan(p, D, **dict(good, **kw))
    y = torch.zeros((3, 40, 56), dtype=torch.int64)
    a = bank_add_plan(p, x, y)
    assert (a.B, a.hp, a.wp, a.OH, a.OW, a.mask_kind, a.per_frame, a.rows) == (3, 5, 7, 40, 56, 1, 35, 105)
    assert bank_add_plan(p, x, y.to(torch.uint8), per_frame=10, room=30).rows == 30
    for kw in (dict(labels=y[:2]), dict(labels=y[0]), dict(labels=y.float()), dict(labels=y.bool()), dict(labels=None),
               dict(labels=y[:, :4]), dict(per_frame=0), dict(per_frame=36), dict(per_frame=2.0), dict(seed=0.5), dict(room=104),
               dict(frames=torch.zeros((3, 44, 56, 3), dtype=torch.uint8)), dict(frames=None)):
        with pytest.raises(ValueError):
            bank_add_plan(p, **dict(dict(frames=x, labels=y), **kw))
    # the model's calls refuse the same things before they ask for a GPU; a valid bank on a CPU model reaches "no CPU path"
    m = DINOSeg(head="linear", n_blocks=1)
    for args in ((0, 10), (257, 10), (4, 0), (4, (1 << 24) + 1), (4, 10, False, 2), (4.0, 10),
                 (256, 10, True)):                                                      # a hard bank's 255 is void
        with pytest.raises(ValueError):
            MemoryBank(m, *args)
    with pytest.raises(ValueError):
        m.segment_knn(x, None)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        MemoryBank(m, 4, 10)
    assert KnnResult._fields == ("labels", "seg", "idx")


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.case_id)
def test_device_cases_leave_few_queries_undecided(i):
    """A query is undecided when its fp64 gap at the cut is <= 2E, E = (D + 16) 2^-24.  The device test caps the share at 4 %; the
    host's reference alone must stay at half of that, so that the cap has room to spare."""
    B, n, M, rows, D, C, k, kind = K.CASES[i]
    qp, bp = K.host_planes(i)
    dec = P.decided(K.ranked(K.query_rows(qp), K.plane_rows(bp), M), k, P.score_bar(D))
    share = 1.0 - float(dec.mean())
    print(f"knn {K.CASES[i]}: undecided {share:.4f} of the queries on the host")
    assert share <= 0.02
