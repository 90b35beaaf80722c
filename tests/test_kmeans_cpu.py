"""Spherical k-means without a device: the host restatement (tests/kmeans_util.py) against the plain matrix form in torch fp64, kept
empty clusters, exact ties, the seeded sample, the plan layer's refusals, and the library's host-only entry."""
import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import ClusterResult, DINOSeg, capi
from dino_amd.dense_plan import kmeans_plan, sample_indices
from tests import kmeans_util as KM


def matrix_form(X, C0, iters):
    """the usual script in torch fp64: X @ C.T, argmax, index_add_, normalize -- with an empty cluster left where it is"""
    X, C = torch.from_numpy(X), torch.from_numpy(np.array(C0))
    for _ in range(iters):
        a = (X @ C.T).argmax(dim=1)
        m = torch.zeros_like(C).index_add_(0, a, X)
        n = torch.bincount(a, minlength=C.shape[0])
        C = torch.where((n > 0)[:, None], torch.nn.functional.normalize(m, dim=1, eps=1e-300), C)
    S = X @ C.T
    return S.argmax(dim=1).numpy(), C.numpy(), S.max(dim=1).values.sum().item()


@pytest.mark.parametrize("N,D,K,iters", [(40, 16, 3, 4), (200, 32, 7, 6), (64, 64, 1, 2), (300, 24, 12, 0)])
def test_host_rule_is_the_plain_matrix_form(N, D, K, iters):
    rng = np.random.default_rng(7 + N)
    X = KM.unit_rows(rng.standard_normal((N, D)))
    C0 = X[rng.permutation(N)[:K]]
    a, C, counts, objective, moved = KM.lloyd_host(X, C0, iters)
    # no near-tie anywhere on the way: the two forms cannot part over an argmax
    Ct = np.array(C0)
    for _ in range(iters + 1):
        at, _, gap, _ = KM.assign_host(X, Ct)
        assert gap.min() > 1e-9, "a near-tie in a random case"
        Ct = KM.update_host(X, at, Ct)[0]
    a2, C2, obj2 = matrix_form(X, C0, iters)
    assert np.array_equal(a, a2)
    assert np.abs(C - C2).max() <= 1e-12
    assert abs(objective[-1] - obj2) <= 1e-12 * N
    assert objective.shape == (iters + 1,) and moved.shape == (iters + 1,) and moved[0] == N
    assert np.all(np.diff(objective) >= -1e-12), "Lloyd's objective does not decrease"
    assert counts.sum() == (N if iters else 0)
    assert np.abs(np.sqrt((C * C).sum(-1)) - 1.0).max() <= 1e-12


def test_an_empty_cluster_keeps_its_centroid():
    rng = np.random.default_rng(11)
    X = KM.unit_rows(rng.standard_normal((50, 16)) + np.array([4.0] + [0.0] * 15))       # everything near +e0
    far = KM.unit_rows(np.array([[-1.0] + [0.0] * 15]))                                   # a centroid nobody chooses
    C0 = np.concatenate([X[:2], far])
    a, _, _, _ = KM.assign_host(X, C0)
    assert not np.any(a == 2)
    C, counts, m, _, kept = KM.update_host(X, a, C0)
    assert counts[2] == 0 and kept[2] and not kept[0] and np.array_equal(C[2], C0[2]) and not np.any(m[2])
    a4, C4, counts4, _, _ = KM.lloyd_host(X, C0, 4)
    assert np.array_equal(C4[2], C0[2]) and counts4[2] == 0 and counts4.sum() == 50


def test_a_centroid_supplied_twice_goes_to_the_lower_index():
    rng = np.random.default_rng(12)
    X = KM.unit_rows(rng.standard_normal((80, 16)))
    c = X[:3]
    C0 = np.stack([c[0], c[1], c[0], c[2]])                             # index 2 repeats index 0
    a, _, gap, _ = KM.assign_host(X, C0)
    assert not np.any(a == 2) and np.any(a == 0)
    assert np.all(gap[a == 0] == 0.0)                                   # an exact tie, resolved by the index
    C, counts, _, _, kept = KM.update_host(X, a, C0)
    assert counts[2] == 0 and kept[2] and np.array_equal(C[2], C0[0]) and not np.array_equal(C[0], C0[0])


def test_the_sample_is_reproducible_and_distinct():
    for N, k, seed in ((10, 10, 0), (4800, 64, 3), (115200, 256, 1 << 40), (7, 1, -5)):
        idx = sample_indices(N, k, seed)
        assert idx.dtype == torch.int64 and idx.shape == (k,)
        assert torch.equal(idx, sample_indices(N, k, seed))
        assert torch.equal(idx, torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:k])
        assert len(set(idx.tolist())) == k and 0 <= int(idx.min()) and int(idx.max()) < N
    assert not torch.equal(sample_indices(4800, 64, 3), sample_indices(4800, 64, 4))
    for N, k in ((3, 5), (10, 0)):
        with pytest.raises(ValueError):
            sample_indices(N, k, 0)


def test_planes_split_and_point_values():
    rng = np.random.default_rng(13)
    c = KM.unit_rows(rng.standard_normal((5, 64))).astype(np.float32)
    p = KM.split_planes(c)
    assert p.dtype == np.float16 and p.shape == (2, 5, 64)
    back = KM.plane_values(p)
    assert np.abs(back - c.astype(np.float64)).max() <= 2.0 ** -22     # hi + lo carries 22 significand bits of a component <= 1
    assert np.array_equal(KM.split_planes(back.astype(np.float32)), p)  # a value the planes hold splits into the same planes
    assert KM.points_of(np.stack([p, p])).shape == (10, 64)


def test_plan_refusals_need_no_device():
    p, D = 8, 384
    x = torch.zeros((3, 40, 56, 3), dtype=torch.uint8)
    ok = kmeans_plan(p, D, x, 5)
    assert (ok.B, ok.hp, ok.wp, ok.N, ok.k, ok.iters, ok.init, ok.seed, ok.n_init, ok.OH, ok.OW, ok.chunk) == \
        (3, 5, 7, 105, 5, 10, "sample", 0, 1, 40, 56, 32)
    rows = torch.zeros((5, D))
    f32 = kmeans_plan(p, D, x.permute(0, 3, 1, 2).float(), 5, init=rows, iters=0, size=(5, 7))
    assert (f32.kind, f32.init, f32.iters, f32.OH, f32.OW) == (capi.INPUT_F32_CHW, "rows", 0, 5, 7)
    assert kmeans_plan(p, D, x, 105).k == 105                           # K = N is the most a sample can give
    assert kmeans_plan(p, D, x[:1], 256, init=torch.zeros((256, D))).k == 256            # ... rows may outnumber the points
    assert kmeans_plan(p, D, x, None, 0, rows).k == 5                   # assign_clusters: k is the rows' count
    assert kmeans_plan(16, D, torch.zeros((1, 64, 96, 3), dtype=torch.uint8), 4).N == 24
    bad = [
        dict(x=torch.zeros((3, 40, 56), dtype=torch.uint8)),                            # layout
        dict(x=torch.zeros((3, 41, 56, 3), dtype=torch.uint8)),                         # not a patch multiple
        dict(x=torch.zeros((0, 40, 56, 3), dtype=torch.uint8)),                         # no frame
        dict(x=np.zeros((3, 40, 56, 3), dtype=np.uint8)),                               # not a tensor
        dict(k=0), dict(k=257), dict(k=2.0), dict(k=True), dict(k=None),
        dict(iters=-1), dict(iters=1.5),
        dict(n_init=0), dict(n_init=2.0),
        dict(seed=0.5),
        dict(init="kmeans++"), dict(init=None),
        dict(init=torch.zeros((4, D))),                                                 # rows that contradict k = 5
        dict(init=torch.zeros((5, D + 64))), dict(init=torch.zeros((5, D), dtype=torch.float64)), dict(init=torch.zeros((5,))),
        dict(init=np.zeros((5, D), dtype=np.float32)),
        dict(k=106),                                                                    # K > N with init="sample"
        dict(size=(4, 56)), dict(size=(40, 6)), dict(size=40),
        dict(chunk=0), dict(chunk=1.5),
    ]
    for kw in bad:
        args = dict(x=x, k=5)
        args.update(kw)
        with pytest.raises(ValueError):
            kmeans_plan(p, D, **args)
    with pytest.raises(ValueError):
        kmeans_plan(p, D, x, None, 0, torch.zeros((257, D)))
    # the model's calls refuse the same things before they ask for a GPU; a valid call on a CPU model reaches "no CPU path"
    m = DINOSeg(head="linear", n_blocks=1)
    for kw in (dict(k=0), dict(k=106), dict(iters=-1), dict(n_init=0), dict(n_blocks=2), dict(size=(4, 56)), dict(chunk=0),
               dict(init=torch.zeros((5, 64)))):
        args = dict(k=5)
        args.update(kw)
        with pytest.raises(ValueError):
            m.cluster(x, **args)
    for kw in (dict(centroids=torch.zeros((5, 64))), dict(centroids=torch.zeros((257, D))), dict(centroids="sample"),
               dict(size=(4, 56)), dict(n_blocks=2)):
        args = dict(centroids=rows)
        args.update(kw)
        with pytest.raises(ValueError):
            m.assign_clusters(x, **args)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.cluster(x, 5)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.assign_clusters(x, rows)


def test_symbols_and_scratch_entry():
    lib = capi.lib()
    names = ("dinoseg_op_kmeans_init", "dinoseg_op_kmeans_assign", "dinoseg_op_kmeans_update", "dinoseg_kmeans_scratch_bytes")
    declared = capi.header_symbols()
    for name in names:
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name)
    for name in ("ClusterResult", "sample_indices"):
        assert name in dino_amd.__all__ and hasattr(dino_amd, name)
    assert ClusterResult._fields == ("labels", "centroids", "counts", "objective", "moved", "scores")
    assert callable(DINOSeg.cluster) and callable(DINOSeg.assign_clusters)
    f = lib.dinoseg_kmeans_scratch_bytes
    # 4 R K (D + 1) + 8 ceil(N / 64), R = min(ceil(N / 256), 4096 // K clamped to 16 .. 64)
    assert f(32, 3600, 64, 384) == 4 * 64 * 64 * 385 + 8 * 1800
    assert f(32, 3600, 128, 384) == 4 * 32 * 128 * 385 + 8 * 1800
    assert f(32, 3600, 256, 384) == 4 * 16 * 256 * 385 + 8 * 1800
    assert f(32, 3600, 8, 384) == 4 * 64 * 8 * 385 + 8 * 1800
    assert f(1, 1, 1, 64) == 4 * 65 + 8
    assert f(1, 4800, 21, 384) == 4 * 19 * 21 * 385 + 8 * 75
    assert f(2, 192, 256, 768) == 4 * 2 * 256 * 769 + 8 * 6
    for B, n, K, D in ((32, 3600, 64, 384), (1, 1, 1, 64), (1, 4800, 21, 384), (3, 480, 64, 384), (2, 99, 7, 192), (8, 3600, 256, 384), (8, 3600, 100, 384)):
        assert f(B, n, K, D) == KM.scratch_bytes(B, n, K, D)
    N, K, D = 32 * 3600, 256, 384
    assert f(32, 3600, K, D) < 4 * N * K and f(32, 3600, K, D) < 2 * N * D               # nothing of size N K or N D
    for bad in ((0, 80, 8, 64), (1, -1, 8, 64), (1, 80, 0, 64), (1, 80, 257, 64), (1, 80, 8, 0), (1, 80, 8, 96), (1, 80, 8, 8256),
                (1 << 16, 1 << 15, 8, 64)):
        assert f(*bad) == -1
