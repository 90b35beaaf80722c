"""PCA of patch features without a device: the host restatement (tests/pca_util.py) against the plain matrix form in fp64, pca_solve
on a constructed covariance, the FeaturePCA state, the plan layer's refusals, the library's host-only entries and every C-ABI refusal."""
import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, FeaturePCA, MemoryBank, PCAFitter, ViTConfig, capi, pca_solve
from dino_amd.dense_plan import knn_plan, pca_plan
from tests import pca_util as U


@pytest.mark.parametrize("B,n,D,kind", [(1, 7, 64, None), (2, 35, 64, "random"), (3, 50, 128, "random0")])
def test_host_rule_is_the_matrix_form(B, n, D, kind):
    """The restatement's moments give np.cov of the kept rows, and its projection is (x - mean) @ basis.T, at 1e-12."""
    tokens, keep = U.make_tokens(B, n, D, seed=n), U.make_keep(B, n, kind, seed=n + 1)
    shift = tokens[:, 1:, :].mean(axis=(0, 1)).astype(np.float32)
    c, kept = U.points(tokens, keep, shift)
    s, o, count = U.moments(c, kept)
    assert count == int(kept.sum()) and not c[~kept].any()
    rows = tokens[:, 1:, :].reshape(-1, D)[kept]
    exact = (rows - shift).astype(np.float32).astype(np.float64)         # the rule's points: one fp32 subtraction
    cov = (o - np.outer(s, s) / count) / (count - 1)
    assert np.abs(cov - np.cov(exact, rowvar=False)).max() <= 1e-12 * max(1.0, np.abs(cov).max())
    bar_s, bar_o = U.moment_bars(c, 10)
    assert np.array_equal(bar_o, bar_o.T) and np.all(bar_o >= 26 * U.U * np.abs(o)) and np.all(bar_s >= 26 * U.U * np.abs(s))
    basis = np.linalg.qr(np.random.default_rng(n).standard_normal((D, 5)))[0].T.astype(np.float32)
    y, bar = U.project(tokens, shift, basis)
    want = (tokens[:, 1:, :] - shift).astype(np.float32).astype(np.float64) @ basis.astype(np.float64).T
    assert np.abs(y - want).max() <= 1e-12 and np.all(bar >= 0)
    ys, bars = U.project(tokens, shift, basis, np.full(5, -2.0, np.float32))
    assert np.array_equal(ys, -2.0 * y) and np.array_equal(bars, 2.0 * bar)


def test_colour_rule_against_torch_bilinear():
    """The integer coordinates and the fp64 lerp of pca_util.colour are F.interpolate(align_corners=False) in fp64; clamp and mask."""
    import torch.nn.functional as F
    hp, wp, OH, OW, q = 5, 7, 37, 53, 4
    rng = np.random.default_rng(3)
    comps = rng.standard_normal((2, 1 + hp * wp, q)).astype(np.float32)
    lo, inv = np.array([-1.0, -0.5, 0.0], np.float32), np.array([0.5, 1.0, 2.0], np.float32)
    keep = (rng.random((2, hp * wp)) < 0.5).astype(np.uint8)
    v255, kept, tmax, raw = U.colour(comps, hp, wp, lo, inv, keep, OH, OW)
    t = (torch.from_numpy(comps[:, 1:, :3]).double() - torch.from_numpy(lo).double()) * torch.from_numpy(inv).double()
    ref = F.interpolate(t.view(2, hp, wp, 3).permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert np.abs(raw - ref.numpy()).max() <= 1e-12 and np.array_equal(v255, 255.0 * np.clip(raw, 0.0, 1.0))
    assert tmax == float(t.abs().max()) and kept.shape == (2, OH, OW)
    assert kept[1, 36, 52] == bool(keep[1, hp * wp - 1]) and kept[0, 0, 0] == bool(keep[0, 0]) and kept[0, 8, 0] == bool(keep[0, wp])
    assert U.colour_bar(1.0) == 255.0 * 17.0 * 2.0 ** -24


def test_range_rule_and_scratch_bytes():
    lib = capi.lib()
    for D in (64, 128, 192, 384, 768, 1024):
        for N in (1, 2, 127, 128, 129, 1200, 4800, 9600, 115200, 2 ** 31 - 256):
            R = U.ranges(N, D)
            assert lib.dinoseg_pca_ranges(N, D) == R and 1 <= R <= 64
            L = U.range_len(N, D)
            assert (R - 1) * L < N + L and R * L >= N                   # the ranges cover every row; only trailing ones may be empty
    assert U.ranges(9600, 384) == 64 and U.range_len(9600, 384) == 150 and U.ranges(1200, 1024) == 10 and U.ranges(100, 64) == 1
    for B, n, D in ((1, 1, 64), (2, 35, 64), (3, 480, 384), (1, 1200, 1024), (32, 3600, 384)):
        assert lib.dinoseg_pca_scratch_bytes(B, n, D) == U.scratch_bytes(B, n, D) > 0
        assert U.scratch_bytes(B, n, D) <= 4 * 64 * (4096 * U.pairs(D) + D + 1)              # bounded by D alone, never by N D
    for bad in ((0, 10, 64), (1, 0, 64), (-1, 10, 64), (1, 10, 0), (1, 10, 96), (1, 10, 1088), (1 << 16, 1 << 16, 64)):
        assert lib.dinoseg_pca_scratch_bytes(*bad) == -1 == U.scratch_bytes(*bad)
    assert lib.dinoseg_pca_ranges(0, 64) == -1 and lib.dinoseg_pca_ranges(10, 100) == -1 and lib.dinoseg_pca_ranges(2 ** 31, 64) == -1


def planted(D, eig, seed, count=1000):
    """moments (sum, outer, count, shift) whose covariance is exactly Q diag(eig) Q^T around a mean, and Q"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    cov = (Q * np.asarray(eig)) @ Q.T
    cov = 0.5 * (cov + cov.T)
    shift = rng.standard_normal(D).astype(np.float32)
    mu = rng.standard_normal(D) * 0.01                                   # the mean of the shifted rows
    s = count * mu
    outer = cov * (count - 1) + np.outer(s, s) / count
    return s, outer, count, shift, Q, mu


def test_pca_solve_recovers_a_planted_spectrum_and_fixes_the_signs():
    D, q = 16, 4
    eig = np.array([9.0, 5.0, 2.0, 1.0] + [0.01] * (D - 4))
    s, outer, count, shift, Q, mu = planted(D, eig, seed=5)
    pca = pca_solve(s, outer, count, shift, q, n_blocks=3)
    assert isinstance(pca, FeaturePCA) and (pca.q, pca.dim, pca.rows, pca.n_blocks) == (q, D, count, 3)
    assert pca.mean.dtype == pca.basis.dtype == pca.eigenvalues.dtype == torch.float32
    assert np.abs(pca.eigenvalues.numpy() - eig[:q]).max() <= 1e-5 and abs(pca.total_variance - eig.sum()) <= 1e-9
    assert np.array_equal(pca.mean.numpy(), (shift.astype(np.float64) + s / count).astype(np.float32))
    for j in range(q):
        v, want = pca.basis[j].numpy().astype(np.float64), Q[:, j]
        big = int(np.argmax(np.abs(want)))
        if want[big] < 0:
            want = -want
        assert np.abs(v - want).max() <= 1e-6 and v[int(np.argmax(np.abs(v)))] > 0
    # the same moments with every direction negated (the same covariance) give the same basis: the sign is the rule's, not eigh's
    big = int(np.argmax(np.abs(Q[:, 0])))
    Qn = Q * np.where(Q[big, :] > 0, -1.0, 1.0)                          # now row `big` is negative in every column
    assert Qn[big, 0] < 0
    cov = (Qn * eig) @ Qn.T
    again = pca_solve(s, 0.5 * (cov + cov.T) * (count - 1) + np.outer(s, s) / count, count, shift, q)
    assert np.abs(again.basis.numpy() - pca.basis.numpy()).max() <= 1e-6 and again.basis[0, big] > 0
    # a tie in magnitude: the first entry decides
    o2 = np.zeros((2, 2))
    o2[:] = [[1.0, -1.0], [-1.0, 1.0]]                                   # the leading direction is (1, -1) / sqrt 2 up to sign
    tie = pca_solve(np.zeros(2), o2, 2, None, 1)
    assert tie.basis[0, 0] > 0 and tie.basis[0, 1] < 0 and abs(float(tie.basis[0, 0]) + float(tie.basis[0, 1])) <= 1e-7
    # torch inputs are taken as well
    t = pca_solve(torch.from_numpy(s), torch.from_numpy(outer), torch.tensor([count]), torch.from_numpy(shift), q, 3)
    assert torch.equal(t.basis, pca.basis) and torch.equal(t.mean, pca.mean)


def test_pca_solve_refusals():
    s, outer, count, shift, _, _ = planted(8, np.arange(8, 0, -1.0), seed=6)
    for kw in (dict(count=1), dict(count=0), dict(q=9), dict(q=0), dict(q=2.0), dict(q=True), dict(outer=outer[:4]), dict(shift=shift[:3])):
        args = dict(sum=s, outer=outer, count=count, shift=shift, q=3)
        args.update(kw)
        with pytest.raises(ValueError):
            pca_solve(**args)
    assert pca_solve(s, outer, 2, shift, 8).q == 8


def test_feature_pca_state_round_trip_is_bit_exact():
    s, outer, count, shift, _, _ = planted(64, np.linspace(5.0, 0.1, 64), seed=7)
    pca = pca_solve(s, outer, count, shift, 6, n_blocks=2)
    state = pca.state_dict()
    assert set(state) == {"mean", "basis", "eigenvalues", "total_variance", "rows", "n_blocks"}
    other = FeaturePCA(torch.zeros(3), torch.ones(1, 3), torch.ones(1), 0.0, 2)
    other.load_state_dict(state)
    third = FeaturePCA.from_state_dict(state)
    for o in (other, third):
        for a, b in ((o.mean, pca.mean), (o.basis, pca.basis), (o.eigenvalues, pca.eigenvalues)):
            assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert (o.total_variance, o.rows, o.n_blocks, o.q, o.dim) == (pca.total_variance, count, 2, 6, 64)
    state["mean"][0] = 99.0                                              # the state is a copy
    assert float(pca.mean[0]) != 99.0
    assert np.array_equal(pca.whitening().numpy(), (1.0 / np.sqrt(pca.eigenvalues.numpy().astype(np.float64))).astype(np.float32))
    for bad in (dict(mean=torch.zeros(3, dtype=torch.float64)), dict(basis=torch.ones(2, 4)), dict(eigenvalues=torch.ones(3))):
        with pytest.raises(ValueError):
            FeaturePCA(**dict(dict(mean=torch.zeros(3), basis=torch.ones(2, 3), eigenvalues=torch.ones(2), total_variance=1.0, rows=5), **bad))


def a_pca(D, q, n_blocks=0):
    basis = torch.eye(D)[:q].contiguous()
    return FeaturePCA(torch.zeros(D), basis, torch.ones(q), float(D), 100, n_blocks)


def test_pca_plan_refusals_need_no_device():
    p, D = 8, 384
    x = torch.zeros((3, 40, 56, 3), dtype=torch.uint8)
    n = 35
    keep = torch.ones((3, n), dtype=torch.bool)
    ok = pca_plan(p, D, 12, x, q=3, keep=keep, n_blocks=2, chunk=4)
    assert (ok.kind, ok.B, ok.hp, ok.wp, ok.q, ok.keep, ok.n_blocks, ok.chunk, ok.OH, ok.OW) == (capi.INPUT_U8_HWC, 3, 5, 7, 3, True, 2, 4, 40, 56)
    assert pca_plan(p, D, 12, x).q == 0 and pca_plan(p, D, 12, x, keep=keep.to(torch.uint8)).keep
    proj = pca_plan(p, D, 12, x.permute(0, 3, 1, 2).float(), pca=a_pca(D, 5, 2), n_blocks=None, size=(41, 57), lo=-1, hi=(1.0, 2.0, 3.0),
                    colour=True)
    assert (proj.kind, proj.q, proj.n_blocks, proj.OH, proj.OW, proj.lo, proj.hi) == (capi.INPUT_F32_CHW, 5, 2, 41, 57, (-1.0,) * 3, (1.0, 2.0, 3.0))
    for kw in (dict(q=0), dict(q=257), dict(q=2.0), dict(q=True), dict(keep=keep[:2]), dict(keep=keep[:, :-1]), dict(keep=keep.float()),
               dict(keep=[1] * n), dict(n_blocks=13), dict(n_blocks=-1), dict(chunk=0), dict(x=None), dict(x=torch.zeros((3, 41, 56, 3), dtype=torch.uint8)),
               dict(x=torch.zeros((0, 40, 56, 3), dtype=torch.uint8)), dict(pca="pca"), dict(pca=a_pca(128, 3)), dict(pca=a_pca(D, 3, 1), n_blocks=2),
               dict(pca=a_pca(D, 300)), dict(pca=a_pca(D, 2), colour=True), dict(pca=a_pca(D, 3), colour=True, size=(4, 56)),
               dict(pca=a_pca(D, 3), colour=True, size=(40, 16385)), dict(pca=a_pca(D, 3), colour=True, size=7),
               dict(pca=a_pca(D, 3), lo="low"), dict(pca=a_pca(D, 3), hi=(1.0, 2.0)), dict(pca=a_pca(D, 3), lo=float("nan"))):
        args = dict(x=x, q=3)
        args.update(kw)
        with pytest.raises(ValueError):
            pca_plan(p, D, 12, **args)
    assert pca_plan(p, 128, 12, x, q=128).q == 128
    with pytest.raises(ValueError):
        pca_plan(p, 128, 12, x, q=129)                                   # no more components than the width
    # knn_plan: a projected bank's rows have the projection's width; unprojected banks keep their message
    good = dict(x=x, bank_size=100, bank_classes=7, bank_blocks=0)
    assert knn_plan(p, D, bank_dim=64, project=a_pca(D, 64), **good).M == 100
    with pytest.raises(ValueError, match="holds rows of width 64, the model's embed_dim is 384"):
        knn_plan(p, D, bank_dim=64, **good)
    for kw in (dict(bank_dim=64, project=a_pca(D, 128)), dict(bank_dim=60, project=a_pca(D, 60)), dict(bank_dim=64, project=a_pca(128, 64)),
               dict(bank_dim=64, project=a_pca(D, 64, 1))):
        with pytest.raises(ValueError):
            knn_plan(p, D, **dict(good, **kw))


def test_model_calls_check_first_and_have_no_cpu_path():
    cfg = ViTConfig(embed_dim=128, num_heads=2, n_blocks=2)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, arch=cfg)
    assert m.device.type == "cpu"
    x = torch.zeros((2, 40, 56, 3), dtype=torch.uint8)
    keep = torch.ones((2, 35), dtype=torch.bool)
    pca3, pca64 = a_pca(128, 3), a_pca(128, 64)
    bad = [lambda: m.pca_fit(x, q=0), lambda: m.pca_fit(x, q=129), lambda: m.pca_fit(x, keep=keep[:1]), lambda: m.pca_fit(x, n_blocks=3),
           lambda: m.pca_fit(x, chunk=0), lambda: m.pca_project(x, pca3, n_blocks=1), lambda: m.pca_project(x, a_pca(384, 3)),
           lambda: m.pca_project(x, None), lambda: m.pca_map(x, a_pca(128, 2)), lambda: m.pca_map(x, pca3, size=(4, 56)),
           lambda: m.pca_map(x, pca3, keep=keep[:, :3]), lambda: m.pca_map(x, pca3, lo=(0.0, 1.0)), lambda: PCAFitter(m, n_blocks=3),
           lambda: PCAFitter(m).update(x, keep=keep.float()), lambda: PCAFitter(m).solve(3), lambda: PCAFitter(m).solve(0),
           lambda: MemoryBank(m, 4, 100, project=pca3), lambda: MemoryBank(m, 4, 100, project=a_pca(128, 60)),
           lambda: MemoryBank(m, 4, 100, n_blocks=1, project=pca64), lambda: MemoryBank(m, 4, 100, project=a_pca(384, 64)),
           lambda: MemoryBank(m, 4, 100, project="pca")]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: m.pca_fit(x), lambda: m.pca_fit(x, q=64, keep=keep, n_blocks=1, chunk=1), lambda: m.pca_project(x, pca3),
                 lambda: m.pca_project(x, pca3, whiten=True, n_blocks=0), lambda: m.pca_map(x, pca3),
                 lambda: m.pca_map(x, a_pca(128, 3, 1)), lambda: m.pca_project(x, a_pca(128, 3, 1)), lambda: m.pca_project(x, a_pca(128, 3, 1), n_blocks=1), lambda: PCAFitter(m, 1).update(x, keep),
                 lambda: m.pca_map(x.permute(0, 3, 1, 2).float(), pca3, size=(80, 60), keep=keep, lo=0.0, hi=1.0),
                 lambda: MemoryBank(m, 4, 100, project=pca64)):
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            call()


def test_symbols_are_declared_bound_and_exported():
    lib, declared = capi.lib(), capi.header_symbols()
    for name in ("dinoseg_op_token_moments", "dinoseg_op_pca_project", "dinoseg_op_pca_colour", "dinoseg_pca_scratch_bytes",
                 "dinoseg_pca_ranges"):
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name)
    for name in ("PCAFitter", "FeaturePCA", "pca_solve"):
        assert name in dino_amd.__all__ and hasattr(dino_amd, name)
    for name in ("pca_fit", "pca_project", "pca_map"):
        assert callable(getattr(DINOSeg, name))


def test_every_c_abi_refusal_names_its_entry():
    """Fake (never dereferenced) pointers: every refusal is on the host, returns -1 and names the entry."""
    lib = capi.lib()
    P16 = 0x10000                                                        # a 16-byte aligned fake address

    def moments(**kw):
        a = dict(tokens=P16, keep=None, B=2, n=35, D=64, shift=P16, sum=P16, outer=P16, count=P16, scratch=P16)
        a.update(kw)
        return lib.dinoseg_op_token_moments(a["tokens"], a["keep"], a["B"], a["n"], a["D"], a["shift"], a["sum"], a["outer"], a["count"],
                                            a["scratch"], None)

    def project(**kw):
        a = dict(tokens=P16, B=2, n=35, D=64, mean=P16, basis=P16, scale=None, q=3, out=P16)
        a.update(kw)
        return lib.dinoseg_op_pca_project(a["tokens"], a["B"], a["n"], a["D"], a["mean"], a["basis"], a["scale"], a["q"], a["out"], None)

    def colour(**kw):
        a = dict(comps=P16, B=2, hp=5, wp=7, q=3, lo=P16, inv=P16, keep=None, OH=40, OW=56, rgb=P16)
        a.update(kw)
        return lib.dinoseg_op_pca_colour(a["comps"], a["B"], a["hp"], a["wp"], a["q"], a["lo"], a["inv"], a["keep"], a["OH"], a["OW"], a["rgb"], None)

    cases = [
        (moments, "dinoseg_op_token_moments",
         [dict(tokens=None), dict(sum=None), dict(count=None), dict(scratch=None), dict(D=0), dict(D=-64), dict(D=32), dict(D=96), dict(D=1088),
          dict(D=2048), dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(B=1 << 16, n=1 << 16), dict(B=1, n=(1 << 31) - 255),
          dict(tokens=P16 + 4), dict(shift=P16 + 8), dict(scratch=P16 + 4), dict(sum=P16 + 4), dict(outer=P16 + 4), dict(count=P16 + 4)]),
        (project, "dinoseg_op_pca_project",
         [dict(tokens=None), dict(mean=None), dict(basis=None), dict(out=None), dict(D=0), dict(D=96), dict(D=1088), dict(q=0), dict(q=-1),
          dict(q=257), dict(B=0), dict(n=0), dict(B=1 << 16, n=1 << 16), dict(tokens=P16 + 4), dict(mean=P16 + 8), dict(basis=P16 + 4),
          dict(scale=P16 + 2), dict(out=P16 + 2)]),
        (colour, "dinoseg_op_pca_colour",
         [dict(comps=None), dict(lo=None), dict(inv=None), dict(rgb=None), dict(q=2), dict(q=0), dict(q=257), dict(B=0), dict(hp=0), dict(wp=-1),
          dict(OH=0), dict(OH=4), dict(OW=6), dict(OH=16385), dict(OW=16385), dict(comps=P16 + 2), dict(lo=P16 + 1), dict(inv=P16 + 2)]),
    ]
    for call, name, bad in cases:
        for kw in bad:
            assert call(**kw) == -1, (name, kw)
            assert name in capi.last_error(), (name, kw, capi.last_error())
