"""The split normalized-cut entries on the device: dinoseg_op_ncut_iterate_split and dinoseg_op_ncut_graph_split against the
one-workgroup entries bit for bit at every grid both accept, the smallest grid the old entries refuse (101 x 101) against fp64, guard
bands, refusals, and DINOSeg.ncut(split=...) against ncut() and against the new operators applied by hand."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import NcutResult, capi, ncut_start
from tests import ncut_util as NC
from tests import test_ncut_gpu as T

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
EPS = T.EPS
KEYS = ("z_out", "rho", "fg", "eigvec", "margin", "seed_cell")
BIG = (1, 101, 101, 64)                 # 10 201 cells: the smallest square grid the one-workgroup entries refuse
BIG_SEED = {"normal": 811, "planted": 812}
BOTH_KINDS = [(i, kind, 0.2) for i in range(len(T.CASES)) for kind in ("normal", "planted")]


def scratch_for(B, n):
    nbytes = capi.lib().dinoseg_ncut_split_scratch_bytes(B, n)
    assert nbytes == 24 * B * n
    return torch.empty((nbytes,), dtype=torch.uint8, device="cuda")


def empty_out(B, n, iters):
    out = {k: torch.empty((B, n), dtype=dt, device="cuda") for k, dt in T.OUT_SPECS}
    out["rho"] = torch.empty((B, iters), dtype=torch.float32, device="cuda")
    out["seed_cell"] = torch.empty((B,), dtype=torch.int32, device="cuda")
    return out


def split_iterate(graph, degree, z_in, iters, rows=0, eps=EPS, out=None, scratch=None):
    B, n = degree.shape
    out = out or empty_out(B, n, iters)
    scratch = scratch_for(B, n) if scratch is None else scratch
    capi.check(capi.lib().dinoseg_op_ncut_iterate_split(
        graph.data_ptr(), degree.data_ptr(), B, n, float(eps), z_in.data_ptr(), iters, rows, out["z_out"].data_ptr(),
        out["rho"].data_ptr() if iters else None, out["fg"].data_ptr(), out["eigvec"].data_ptr(), out["margin"].data_ptr(),
        out["seed_cell"].data_ptr(), scratch.data_ptr(), S()))
    return out


def split_graph(planes, tau, out=None):
    B, _, n, D = planes.shape
    W = NC.words_of(n)
    assert capi.lib().dinoseg_ncut_split_graph_bytes(B, n) == 8 * B * n * W
    graph, degree = out or (torch.empty((B, n, W), dtype=torch.int64, device="cuda"), torch.empty((B, n), dtype=torch.int32, device="cuda"))
    capi.check(capi.lib().dinoseg_op_ncut_graph_split(planes.data_ptr(), B, n, D, float(tau), graph.data_ptr(), degree.data_ptr(), S()))
    return graph, degree


def assert_same(got, want, what=""):
    for k in KEYS:
        assert torch.equal(T.bits_of(got[k]), T.bits_of(want[k])), f"{k} {what}"


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("p", BOTH_KINDS, ids=T.pid)
def test_split_is_the_one_workgroup_launch_bit_for_bit(cuda, p):
    """Every case of tests/test_ncut_gpu.py (1 .. 4800 cells, one or two frames, both kinds of input): the split graph entry gives the
    graph and the degree of dinoseg_op_ncut_graph, and for iters in {0, 1, 4} and rows_per_group in {0, 1, 7, 32, 33, n} the split
    iterate entry gives z_out, rho, fg, eigvec, margin and seed_cell of dinoseg_op_ncut_iterate, bit for bit."""
    i, kind, tau = p
    B, hp, wp, D = T.CASES[i]
    n = hp * wp
    graph, degree, _, _ = T.device_graph(p)
    g2, d2 = split_graph(T.device_points(i, kind)[0], tau)
    assert torch.equal(g2, graph) and torch.equal(d2, degree)
    scratch = scratch_for(B, n)
    for iters in (0, 1, 4):
        want = T.nc_iterate(graph, degree, T.start_for(B, n), iters)
        for rows in (0, 1, 7, 32, 33, n):
            got = split_iterate(graph, degree, T.start_for(B, n), iters, rows, scratch=scratch)
            assert_same(got, want, f"iters {iters} rows {rows}")


# ------------------------------------------------------------------------------------------------ 2. above the old limit
class BlockedBits:
    """The bit graph bool [n, n] as the left operand of `@`: the product is formed over blocks of rows in fp64, so NC.one_pass and
    NC.pass_bars apply to it as they stand and no dense n x n fp64 array exists."""
    ROWS = 512

    def __init__(self, bits):
        self.bits = bits

    def __matmul__(self, v):
        return np.concatenate([self.bits[a:a + self.ROWS].astype(np.float64) @ v for a in range(0, self.bits.shape[0], self.ROWS)])


@functools.lru_cache(maxsize=None)
def big_inputs(kind):
    B, hp, wp, D = BIG
    n = hp * wp
    tok, small = (NC.normal_tokens(BIG_SEED[kind], B, n, D), None) if kind == "normal" else NC.planted_tokens(BIG_SEED[kind], B, n, D)
    planes = T.normalize(T.dev(tok))
    graph, degree = split_graph(planes, 0.2)
    return planes, graph, degree, small


@functools.lru_cache(maxsize=None)
def big_bits(kind):
    n = BIG[1] * BIG[2]
    bits, pad = NC.unpack_words(big_inputs(kind)[1][0].cpu().numpy().view(np.uint64), n)
    bits.setflags(write=False)
    return bits, pad


@functools.lru_cache(maxsize=None)
def big_three_passes(kind):
    _, graph, degree, _ = big_inputs(kind)
    return split_iterate(graph, degree, T.start_for(1, BIG[1] * BIG[2]), 3)


@pytest.mark.parametrize("kind", ["normal", "planted"])
def test_graph_above_the_old_limit_against_fp64(cuda, kind):
    """64 seeded sample rows against the fp64 scores of those rows: every pair with |s - tau| > 2 E has the host's bit, the undecided
    share stays under the suite's 4 % cap (for normal rows of width 64 the band 2 E is about 1e-5 wide against a score spread of
    about 0.125: far under 0.1 % are undecided); graph == graph^T; the degree is the popcount; pad bits are zero.  The old entries
    refuse this grid."""
    B, hp, wp, D = BIG
    n, E, tau32 = hp * wp, NC.score_bar(D), float(np.float32(0.2))
    planes, graph, degree, _ = big_inputs(kind)
    assert n > capi.lib().dinoseg_ncut_max_cells() and capi.lib().dinoseg_ncut_graph_bytes(B, n) == -1
    assert capi.lib().dinoseg_op_ncut_graph(planes.data_ptr(), B, n, D, 0.2, graph.data_ptr(), degree.data_ptr(), S()) == -1
    bits, pad = big_bits(kind)
    assert not pad.any()
    X = NC.frame_points(planes.cpu().numpy())[0]
    rows = np.sort(np.random.default_rng(5).choice(n, 64, replace=False))
    Sh = X[rows] @ X.T + 0.0
    decided = np.abs(Sh - tau32) > 2.0 * E
    share = 1.0 - float(decided.mean())
    print(f"ncut split graph 101x101 {kind}: undecided {share:.6f} of the sampled pairs; density {bits.mean():.4f}")
    assert np.array_equal(bits[rows][decided], (Sh > tau32)[decided]), "a decided pair's bit differs from the host's"
    assert share <= T.UNDECIDED_CAP
    assert np.array_equal(bits, bits.T), "the graph is not symmetric"
    assert np.array_equal(degree[0].cpu().numpy(), bits.sum(1))
    assert bits.diagonal().all()


@pytest.mark.parametrize("kind", ["normal", "planted"])
def test_one_teacher_forced_pass_above_the_old_limit_against_fp64(cuda, kind):
    """One call with iters = 1 on the device's graph against NC.one_pass on the same graph over blocks of rows, within NC.pass_bars."""
    n = BIG[1] * BIG[2]
    _, graph, degree, _ = big_inputs(kind)
    bits = BlockedBits(big_bits(kind)[0])
    cnt = degree[0].cpu().numpy().astype(np.int64)
    _, r, u = NC.weights(cnt, n, EPS)
    z = T.start_for(1, n)
    out = split_iterate(graph, degree, z, 1)
    o = NC.one_pass(bits, r, u, EPS, z[0].cpu().numpy().astype(np.float64))
    dz, drho, _ = NC.pass_bars(o, bits, cnt, r, u, EPS)
    assert np.all(np.isfinite(dz))
    err = np.abs(out["z_out"][0].cpu().numpy().astype(np.float64) - o["z"])
    erho = abs(float(out["rho"][0, 0]) - o["rho"])
    print(f"ncut split pass 101x101 {kind}: z' at most {float((err / dz).max()):.3f} of its bar, rho {erho / drho:.3f} of its bar")
    assert np.all(err <= dz)
    assert erho <= drho
    assert abs(np.linalg.norm(out["z_out"][0].cpu().numpy().astype(np.float64)) - 1.0) <= 1e-6


@pytest.mark.parametrize("kind", ["normal", "planted"])
def test_bits_above_the_old_limit_do_not_depend_on_how_they_are_computed(cuda, kind):
    """Two values of rows_per_group, two runs, three chained calls with iters = 1 against one with iters = 3, and z_out in place of
    z_in (iters = 0 included): the same bits every time."""
    B, n = 1, BIG[1] * BIG[2]
    _, graph, degree, _ = big_inputs(kind)
    want = big_three_passes(kind)
    assert_same(split_iterate(graph, degree, T.start_for(B, n), 3), want, "second run")
    for rows in (13, 512):
        assert_same(split_iterate(graph, degree, T.start_for(B, n), 3, rows), want, f"rows {rows}")
    z, rhos = T.start_for(B, n), []
    for _ in range(3):
        out = split_iterate(graph, degree, z, 1)
        z = out["z_out"]
        rhos.append(out["rho"])
    out["rho"] = torch.cat(rhos, dim=1)
    assert_same(out, want, "chained")
    for iters, ref in ((3, want), (0, split_iterate(graph, degree, T.start_for(B, n), 0))):
        z = T.start_for(B, n)
        o = empty_out(B, n, iters)
        o["z_out"] = z
        assert_same(split_iterate(graph, degree, z, iters, out=o), ref, f"in place, iters {iters}")


def test_planted_groups_above_the_old_limit(cuda):
    n = BIG[1] * BIG[2]
    _, graph, degree, small = big_inputs("planted")
    out = split_iterate(graph, degree, T.start_for(1, n), 32)
    assert np.array_equal(out["fg"].cpu().numpy().astype(bool), small)
    assert small[0][int(out["seed_cell"][0])]


# ------------------------------------------------------------------------------------------------ 3. guard bands
@pytest.mark.parametrize("hp,wp", [(5, 7), (5, 13), (101, 101)])
def test_outputs_graph_and_scratch_stay_between_their_guard_bands(cuda, hp, wp):
    B, D, n, W, iters = 2 if hp == 5 else 1, 64, hp * wp, NC.words_of(hp * wp), 3
    planes = T.normalize(T.dev(NC.normal_tokens(830 + n % 7, B, n, D)))
    graph = T.Guarded(B * n * W * 8, torch.int64, (B, n, W))
    degree = T.Guarded(B * n * 4, torch.int32, (B, n))
    split_graph(planes, 0.2, out=(graph.view, degree.view))
    g = {k: T.Guarded(B * n * dt.itemsize, dt, (B, n)) for k, dt in T.OUT_SPECS}
    g["rho"] = T.Guarded(B * iters * 4, torch.float32, (B, iters))
    g["seed_cell"] = T.Guarded(B * 4, torch.int32, (B,))
    scratch = T.Guarded(24 * B * n, torch.uint8, (24 * B * n,))
    for rows in (0, 5):
        split_iterate(graph.view, degree.view, T.start_for(B, n), iters, rows, out={k: v.view for k, v in g.items()}, scratch=scratch.view)
        torch.cuda.synchronize()
        for v in [graph, degree, scratch] + list(g.values()):
            assert v.bands_intact()
    want_g, want_d = split_graph(planes, 0.2)
    assert torch.equal(graph.view, want_g) and torch.equal(degree.view, want_d)
    assert_same({k: v.view for k, v in g.items()}, split_iterate(want_g, want_d, T.start_for(B, n), iters))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_return_minus_one_without_launching(cuda):
    B, hp, wp, D = 2, 5, 7, 64
    n, W, iters = hp * wp, 1, 2
    lib = capi.lib()
    cells = lib.dinoseg_ncut_split_max_cells()
    planes = T.normalize(torch.randn((B, n + 1, D), device="cuda"))
    graph = torch.full((B, n, W + 1), -7, dtype=torch.int64, device="cuda")
    degree = torch.full((B, n), -7, dtype=torch.int32, device="cuda")
    z = T.start_for(B, n)
    z_before = z.clone()
    outs = {k: torch.full((B, n), 9, dtype=dt, device="cuda") for k, dt in T.OUT_SPECS}
    rho = torch.full((B, iters), 9.0, device="cuda")
    seed = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    scratch = torch.full((24 * B * n + 16,), 9, dtype=torch.uint8, device="cuda")
    good = dict(planes=planes.data_ptr(), B=B, n=n, D=D, tau=0.2, graph=graph.data_ptr(), degree=degree.data_ptr(), eps=EPS,
                z_in=z.data_ptr(), iters=iters, rows=0, z_out=outs["z_out"].data_ptr(), rho=rho.data_ptr(), fg=outs["fg"].data_ptr(),
                eigvec=outs["eigvec"].data_ptr(), margin=outs["margin"].data_ptr(), seed=seed.data_ptr(), scratch=scratch.data_ptr())

    def build(**kw):
        g = dict(good)
        g.update(kw)
        return lib.dinoseg_op_ncut_graph_split(g["planes"], g["B"], g["n"], g["D"], g["tau"], g["graph"], g["degree"], S())

    def iterate(**kw):
        g = dict(good)
        g.update(kw)
        return lib.dinoseg_op_ncut_iterate_split(g["graph"], g["degree"], g["B"], g["n"], g["eps"], g["z_in"], g["iters"], g["rows"],
                                                 g["z_out"], g["rho"], g["fg"], g["eigvec"], g["margin"], g["seed"], g["scratch"], S())

    shapes = [dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(n=cells + 1), dict(B=1 << 30, n=4800)]
    for kw in [dict(planes=None), dict(graph=None), dict(degree=None), dict(planes=planes.data_ptr() + 2), dict(graph=graph.data_ptr() + 4),
               dict(degree=degree.data_ptr() + 2), dict(D=0), dict(D=-64), dict(D=96), dict(D=8256), dict(tau=1.0), dict(tau=-1.0),
               dict(tau=float("nan")), dict(tau=float("inf"))] + shapes:
        assert build(**kw) == -1, kw
        assert "dinoseg_op_ncut_graph_split" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert bool((graph == -7).all()) and bool((degree == -7).all())
    assert build() == 0
    torch.cuda.synchronize()
    assert not bool((degree == -7).any()) and bool((graph.view(-1)[B * n * W:] == -7).all())
    # (B = 2^26 frames of 64 cells pass the graph's launch range and exceed the row workgroups' at one row per workgroup)
    for kw in [dict(graph=None), dict(degree=None), dict(z_in=None), dict(z_out=None), dict(fg=None), dict(eigvec=None), dict(seed=None),
               dict(rho=None), dict(scratch=None), dict(graph=graph.data_ptr() + 4), dict(degree=degree.data_ptr() + 2),
               dict(z_in=z.data_ptr() + 2), dict(rho=rho.data_ptr() + 1), dict(margin=outs["margin"].data_ptr() + 2),
               dict(scratch=scratch.data_ptr() + 4), dict(scratch=scratch.data_ptr() + 8), dict(eps=-1e-9), dict(eps=1.0),
               dict(eps=float("nan")), dict(iters=-1), dict(iters=4097), dict(rows=-1), dict(rows=-(1 << 31)),
               dict(B=1 << 26, n=64, rows=1)] + shapes:
        assert iterate(**kw) == -1, kw
        assert "dinoseg_op_ncut_iterate_split" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 9).all()) for v in outs.values()) and bool((rho == 9.0).all()) and bool((seed == 9).all())
    assert bool((scratch == 9).all())
    assert torch.equal(z, z_before)
    assert iterate() == 0 and iterate(margin=None) == 0 and iterate(iters=0, rho=None) == 0 and iterate(rows=1 << 30) == 0
    torch.cuda.synchronize()
    assert not bool((rho == 9.0).any()) and not bool((seed == 9).any())
    assert bool((scratch[24 * B * n:] == 9).all())


# ------------------------------------------------------------------------------------------------ 5. model level
@pytest.mark.parametrize("tag", ["tiny", "vits8"])
def test_ncut_with_split_is_ncut(cuda, tag):
    m = T.model(tag)
    x = T.frames_of(tag, 3, seed=741)
    want = m.ncut(x, iters=12, want_graph=True)
    for s in (True, 16):
        got = m.ncut(x, iters=12, want_graph=True, split=s)
        assert len(got) == 7
        for f, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(T.bits_of(a), T.bits_of(b)), NcutResult._fields[f]
    assert m.ncut(x, iters=12, split=True).graph is None


def test_ncut_with_split_above_the_old_limit_is_the_operators_by_hand(cuda):
    m = T.model("tiny")
    H = 8 * 101
    frames = torch.from_numpy(T.synthetic_frames(1, H, seed=77))
    assert frames.shape == (1, H, H, 3) and frames.dtype == torch.uint8
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="cells"):
        m.ncut(frames, iters=8, want_graph=True)                        # (a host tensor: nothing is copied)
    assert torch.cuda.memory_allocated() == before
    x = frames.cuda()
    res = m.ncut(x, split=True, iters=8, want_graph=True)
    n = 101 * 101
    planes = T.normalize(m.features(x))
    graph, degree = split_graph(planes, float(np.float32(0.2)))
    out = split_iterate(graph, degree, ncut_start(n, 0).cuda().expand(1, n).contiguous(), 8, eps=1e-5)
    two = torch.stack((torch.zeros_like(out["margin"]), out["margin"]), dim=2).contiguous()
    labels = torch.empty((1, H, H), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(two.data_ptr(), 1, 101, 101, 2, H, H, labels.data_ptr(), None, S()))
    want = NcutResult(labels, out["fg"], out["eigvec"], out["seed_cell"], out["rho"], degree, graph.view(torch.uint64))
    assert res.labels.shape == (1, H, H) and res.labels.dtype == torch.int32
    assert int(res.labels.min()) >= 0 and int(res.labels.max()) <= 1
    assert res.graph.shape == (1, n, NC.words_of(n)) and res.rho.shape == (1, 8)
    assert T.same(res, want)
