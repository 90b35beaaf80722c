"""PCA of patch features on the device: dinoseg_op_token_moments, dinoseg_op_pca_project and dinoseg_op_pca_colour through the C-ABI
against the fp64 restatement of their rules (tests/pca_util.py) -- bars, exact symmetry, accumulation, bit-for-bit repeats, masks,
containment, exact integer probes -- and DINOSeg.pca_fit / pca_project / pca_map / PCAFitter / a projected MemoryBank against the
operators applied by hand and against an fp64 PCA (Weyl and Davis-Kahan bounds from the moments' bars, no measured tolerance)."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, FeaturePCA, MemoryBank, PCAFitter, capi, pca_solve, procedural_state_dict
from dino_amd.weights import VIT_S8, synthetic_frames
from tests import arch_util as A
from tests import pca_util as U

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
GUARD = 64


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """a device buffer with GUARD elements of `fill` on either side of the part the library is given"""

    def __init__(self, shape, dtype, fill, zero=False):
        n = int(np.prod(shape))
        self.fill, self.buf = fill, torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if zero:
            self.t.zero_()

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[-GUARD:] == self.fill).all())


class Acc:
    """zeroed accumulators and a scratch of exactly the library's size, all between guard bands"""

    def __init__(self, B, n, D):
        nbytes = capi.lib().dinoseg_pca_scratch_bytes(B, n, D)
        assert nbytes == U.scratch_bytes(B, n, D) and capi.lib().dinoseg_pca_ranges(B * n, D) == U.ranges(B * n, D)
        self.sum, self.outer = Guarded((D,), torch.float64, -7.0, True), Guarded((D, D), torch.float64, -7.0, True)
        self.count, self.scratch = Guarded((1,), torch.int64, -7, True), Guarded((nbytes,), torch.uint8, 0xA5)

    def run(self, tokens, keep, shift, outer=True):
        B, n1, D = tokens.shape
        capi.check(capi.lib().dinoseg_op_token_moments(tokens.data_ptr(), capi.ptr(keep), B, n1 - 1, D, capi.ptr(shift), self.sum.t.data_ptr(),
                                                       self.outer.t.data_ptr() if outer else None, self.count.t.data_ptr(),
                                                       self.scratch.t.data_ptr(), S()))
        return self

    def read(self):
        torch.cuda.synchronize()
        return self.sum.t.cpu().numpy(), self.outer.t.cpu().numpy(), int(self.count.t.item())

    def intact(self):
        return self.sum.intact() and self.outer.intact() and self.count.intact() and self.scratch.intact()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def moment_case(i):
    B, n, D, kind = U.MOMENT_CASES[i]
    tokens, keep = U.make_tokens(B, n, D, seed=100 + i), U.make_keep(B, n, kind, seed=200 + i)
    shift = tokens[:, 1:, :].mean(axis=(0, 1)).astype(np.float32)
    c, kept = U.points(tokens, keep, shift)
    return tokens, keep, shift, U.moments(c, kept), U.moment_bars(c, U.range_len(B * n, D))


# ------------------------------------------------------------------------------------------------ 1. the moments
@pytest.mark.parametrize("i", range(len(U.MOMENT_CASES)), ids=[U.case_id(c) for c in U.MOMENT_CASES])
def test_moments_against_fp64_restatement(cuda, i):
    """Every element of sum and outer within its bar, (L + 16) 2^-24 times the sum of the absolute terms, of the fp64 restatement
    from the same points; outer exactly symmetric; count exact; a second call into the same accumulators within both bars; from
    equal accumulators two runs agree bit for bit; an all-zero keep changes no bit; a null outer gives the same sum bits; the guard
    bands around accumulators and scratch stay intact.  (Measured worst shares of the bars: see the README entry.)"""
    B, n, D, _ = U.MOMENT_CASES[i]
    tokens, keep, shift, (s64, o64, count), (bar_s, bar_o) = moment_case(i)
    tok, kp, sh = dev(tokens), dev(keep), dev(shift)
    acc = Acc(B, n, D).run(tok, kp, sh)
    s, o, cnt = acc.read()
    assert cnt == count
    es, eo = np.abs(s - s64), np.abs(o - o64)
    share_s = float(np.max(es[bar_s > 0] / bar_s[bar_s > 0], initial=0.0))
    share_o = float(np.max(eo[bar_o > 0] / bar_o[bar_o > 0], initial=0.0))
    print(f"moments {U.MOMENT_CASES[i]}: R = {U.ranges(B * n, D)}, L = {U.range_len(B * n, D)}; sum at {share_s:.4f} of its bar, outer at "
          f"{share_o:.4f} of its bar")
    assert np.all(es <= bar_s) and np.all(eo <= bar_o)
    assert np.array_equal(bits(o), bits(o.T)), "outer is not exactly symmetric"
    # bit for bit from equal accumulators
    s2, o2, cnt2 = Acc(B, n, D).run(tok, kp, sh).read()
    assert np.array_equal(bits(s2), bits(s)) and np.array_equal(bits(o2), bits(o)) and cnt2 == cnt
    # a null outer: the same sums and count
    other = Acc(B, n, D).run(tok, kp, sh, outer=False)
    s3, o3, cnt3 = other.read()
    assert np.array_equal(bits(s3), bits(s)) and cnt3 == cnt and not o3.any() and other.intact()
    # a second call adds
    s4, o4, cnt4 = acc.run(tok, kp, sh).read()
    assert cnt4 == 2 * count
    assert np.all(np.abs(s4 - 2 * s64) <= 2 * bar_s) and np.all(np.abs(o4 - 2 * o64) <= 2 * bar_o)
    assert np.array_equal(bits(o4), bits(o4.T))
    # an all-zero keep changes nothing
    s5, o5, cnt5 = acc.run(tok, torch.zeros((B, n), dtype=torch.uint8, device="cuda"), sh).read()
    assert np.array_equal(bits(s5), bits(s4)) and np.array_equal(bits(o5), bits(o4)) and cnt5 == cnt4
    assert acc.intact()


def test_moments_null_shift_is_zero_shift(cuda):
    B, n, D = 2, 35, 64
    tokens, keep = U.make_tokens(B, n, D, seed=31), U.make_keep(B, n, "random", seed=32)
    c, kept = U.points(tokens, keep, None)
    s64, o64, count = U.moments(c, kept)
    bar_s, bar_o = U.moment_bars(c, U.range_len(B * n, D))
    s, o, cnt = Acc(B, n, D).run(dev(tokens), dev(keep), None).read()
    assert cnt == count and np.all(np.abs(s - s64) <= bar_s) and np.all(np.abs(o - o64) <= bar_o)
    z, oz, _ = Acc(B, n, D).run(dev(tokens), dev(keep), torch.zeros((D,), dtype=torch.float32, device="cuda")).read()
    assert np.array_equal(bits(z), bits(s)) and np.array_equal(bits(oz), bits(o))


@pytest.mark.parametrize("B,n,D,masked", [(3, 1365, 128, False), (3, 1365, 128, True), (2, 100, 192, True), (1, 7, 64, False)])
def test_moments_exact_integer_probes(cuda, B, n, D, masked):
    """Integer tokens |x| <= 15 and an integer shift |s| <= 3: every product and partial sum is an integer below 2^24 (N <= 4096), so
    sum and outer must equal the int64 result exactly.  The first and last row of every range, the rows next to the CLS rows and
    columns 31 / 32 / 63 / 64 carry planted values (kept rows all of them); the CLS rows hold 1000, so a dropped row, a counted CLS
    row or a mis-mirrored tile shows as a wrong integer."""
    N, L = B * n, U.range_len(B * n, D)
    rng = np.random.default_rng(B * 1000 + D)
    x = rng.integers(-15, 16, size=(B, 1 + n, D)).astype(np.float32)
    keep = (rng.random((B, n)) < 0.6).astype(np.uint8) if masked else None
    rows = sorted({r for k in range(U.ranges(N, D)) for r in (k * L, min((k + 1) * L, N) - 1) if k * L < N} |
                  {b * n for b in range(B)} | {b * n + n - 1 for b in range(B)})
    flat = x[:, 1:, :].reshape(N, D)
    for j, r in enumerate(rows):
        flat[r] = ((np.arange(D) * 7 + j * 5) % 31) - 15
        flat[r, [c for c in (31, 32, 63, 64) if c < D]] = [v for c, v in zip((31, 32, 63, 64), (15, -14, 13, -15)) if c < D]
        if keep is not None:
            keep.reshape(-1)[r] = 1
    x[:, 1:, :] = flat.reshape(B, n, D)
    x[:, 0, :] = 1000.0
    shift = rng.integers(-3, 4, size=D).astype(np.float32)
    ci = (x[:, 1:, :].reshape(N, D) - shift).astype(np.int64)
    if keep is not None:
        ci[keep.reshape(-1) == 0] = 0
    assert int(np.abs(ci).max()) ** 2 * N < 2 ** 24
    s, o, cnt = Acc(B, n, D).run(dev(x), dev(keep), dev(shift)).read()
    assert cnt == (N if keep is None else int(keep.sum()))
    assert np.array_equal(s, ci.sum(axis=0).astype(np.float64))
    assert np.array_equal(o, (ci.T @ ci).astype(np.float64))


# ------------------------------------------------------------------------------------------------ 2. the projection
def run_project(tokens, mean, basis, scale, q, out=None):
    B, n1, D = tokens.shape
    if out is None:
        out = Guarded((B, n1, q), torch.float32, -7.0)
    capi.check(capi.lib().dinoseg_op_pca_project(tokens.data_ptr(), B, n1 - 1, D, mean.data_ptr(), basis.data_ptr(), capi.ptr(scale), q,
                                                 out.t.data_ptr(), S()))
    return out


def u32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", U.PROJECT_CASES, ids=[U.case_id(c) for c in U.PROJECT_CASES])
def test_project_against_fp64_restatement(cuda, case):
    """Within (D + 16) 2^-24 sum |c basis| of the fp64 restatement; the CLS rows zero; frames one by one equal the batch bit for bit;
    scale equals the unscaled result times scale in fp32, bit for bit; guard bands intact."""
    B, n, D, q = case
    rng = np.random.default_rng(D * 7 + q)
    tokens = U.make_tokens(B, n, D, seed=300 + q)
    mean = tokens[:, 1:, :].mean(axis=(0, 1)).astype(np.float32)
    basis = (rng.standard_normal((q, D)) / np.sqrt(D)).astype(np.float32)
    scale = (rng.random(q) * 4.0 - 2.0).astype(np.float32)
    tok, mn, bs, sc = dev(tokens), dev(mean), dev(basis), dev(scale)
    out = run_project(tok, mn, bs, None, q)
    torch.cuda.synchronize()
    assert out.intact()
    y64, bar = U.project(tokens, mean, basis)
    got = out.t.cpu().numpy()
    assert not got[:, 0, :].any(), "a CLS row of out is not zero"
    err = np.abs(got[:, 1:, :].astype(np.float64) - y64)
    print(f"project {case}: at {float(np.max(err[bar > 0] / bar[bar > 0], initial=0.0)):.4f} of the bar")
    assert np.all(err <= bar)
    # frames one by one
    for b in range(B):
        one = run_project(tok[b:b + 1], mn, bs, None, q)
        assert torch.equal(u32(one.t[0]), u32(out.t[b])) and one.intact()
    # whitening: one more fp32 multiplication
    scaled = run_project(tok, mn, bs, sc, q)
    assert torch.equal(u32(scaled.t[:, 1:]), u32(out.t[:, 1:] * sc)) and not bool(scaled.t[:, 0].any()) and scaled.intact()
    y64s, bars = U.project(tokens, mean, basis, scale)
    assert np.all(np.abs(scaled.t.cpu().numpy()[:, 1:, :].astype(np.float64) - y64s) <= bars)


@pytest.mark.parametrize("case", [(2, 35, 192, 33), (1, 130, 1024, 256), (1, 5, 64, 3)], ids=U.case_id)
def test_project_exact_integer_probes(cuda, case):
    """Integer tokens and mean, basis entries in {-1, 0, 1}: every partial sum is an integer below 2^24, the result is exact."""
    B, n, D, q = case
    rng = np.random.default_rng(q)
    x = rng.integers(-15, 16, size=(B, 1 + n, D)).astype(np.float32)
    x[:, 0, :] = 1000.0
    mean = rng.integers(-3, 4, size=D).astype(np.float32)
    basis = rng.integers(-1, 2, size=(q, D)).astype(np.float32)
    out = run_project(dev(x), dev(mean), dev(basis), None, q)
    torch.cuda.synchronize()
    want = (x[:, 1:, :] - mean).astype(np.int64) @ basis.astype(np.int64).T
    assert np.array_equal(out.t.cpu().numpy()[:, 1:, :].astype(np.int64), want) and out.intact()
    assert np.array_equal(out.t.cpu().numpy()[:, 1:, :], want.astype(np.float32))


# ------------------------------------------------------------------------------------------------ 3. the colour map
def run_colour(comps, hp, wp, lo, inv, keep, OH, OW):
    B, _, q = comps.shape
    rgb = Guarded((B, OH, OW, 3), torch.uint8, 0x5A)
    capi.check(capi.lib().dinoseg_op_pca_colour(comps.data_ptr(), B, hp, wp, q, lo.data_ptr(), inv.data_ptr(), capi.ptr(keep), OH, OW,
                                                rgb.t.data_ptr(), S()))
    return rgb


@pytest.mark.parametrize("masked", [False, True], ids=["all", "keep"])
@pytest.mark.parametrize("case", U.COLOUR_CASES, ids=[U.case_id(c) for c in U.COLOUR_CASES])
def test_colour_against_fp64_restatement(cuda, case, masked):
    """Every byte b of a kept pixel satisfies |b - 255 t64| <= 0.5 + bar with t64 the clamped fp64 value and bar = the bilinear bar
    of the arithmetic times 255 (pca_util.colour_bar); unkept pixels are exactly 0; values below lo and above hi saturate at 0 and
    255; two runs agree bit for bit; guard bands intact.  lo / hi sit inside the data's range so that both clamps are reached."""
    hp, wp, OH, OW, q = case
    B, n = 2, hp * wp
    rng = np.random.default_rng(OH * 31 + OW + q)
    comps = (3.0 * rng.standard_normal((B, 1 + n, q))).astype(np.float32)
    comps[:, 0, :] = np.nan                                           # the CLS rows are not read
    lo = np.array([-2.0, -1.5, -2.5], np.float32)
    inv = (1.0 / (np.array([2.0, 2.5, 1.5], np.float32) - lo)).astype(np.float32)
    keep = (rng.random((B, n)) < 0.7).astype(np.uint8) if masked else None
    args = (dev(comps), hp, wp, dev(lo), dev(inv), dev(keep), OH, OW)
    rgb = run_colour(*args)
    again = run_colour(*args)
    torch.cuda.synchronize()
    assert rgb.intact() and torch.equal(rgb.t, again.t)
    got = rgb.t.cpu().numpy().astype(np.float64)
    want, kept, tmax, raw = U.colour(comps, hp, wp, lo, inv, keep, OH, OW)
    bar = U.colour_bar(tmax)
    assert not got[~kept].any(), "an unkept pixel is not black"
    err = np.abs(got - want)[kept]
    print(f"colour {case} {'keep' if masked else 'all'}: worst |b - 255 t| = {float(err.max(initial=0.0)):.6f} (0.5 + {bar:.2e})")
    assert np.all(err <= 0.5 + bar)
    margin = bar / 255.0
    low, high = kept[..., None] & (raw < -margin), kept[..., None] & (raw > 1.0 + margin)
    assert not got[low].any() and np.all(got[high] == 255.0)
    if n > 1:
        assert low.any() and high.any()


def test_refusals_launch_nothing(cuda):
    """Every refusal of the three entries leaves the outputs untouched; the good calls then run."""
    lib = capi.lib()
    B, n, D, q = 1, 6, 64, 3
    tok = dev(U.make_tokens(B, n, D, seed=1))
    acc = Acc(B, n, D)
    mean, basis = torch.zeros((D,), device="cuda"), torch.ones((q, D), device="cuda")
    out, rgb = Guarded((B, n + 1, q), torch.float32, -7.0), Guarded((B, 8, 8, 3), torch.uint8, 0x5A)
    lo, inv = torch.zeros((3,), device="cuda"), torch.ones((3,), device="cuda")

    def moments(**kw):
        a = dict(tokens=tok.data_ptr(), keep=None, B=B, n=n, D=D, shift=None, sum=acc.sum.t.data_ptr(), outer=acc.outer.t.data_ptr(),
                 count=acc.count.t.data_ptr(), scratch=acc.scratch.t.data_ptr())
        a.update(kw)
        return lib.dinoseg_op_token_moments(a["tokens"], a["keep"], a["B"], a["n"], a["D"], a["shift"], a["sum"], a["outer"], a["count"],
                                            a["scratch"], S())

    def project(**kw):
        a = dict(tokens=tok.data_ptr(), B=B, n=n, D=D, mean=mean.data_ptr(), basis=basis.data_ptr(), q=q, out=out.t.data_ptr())
        a.update(kw)
        return lib.dinoseg_op_pca_project(a["tokens"], a["B"], a["n"], a["D"], a["mean"], a["basis"], None, a["q"], a["out"], S())

    def colour(**kw):
        a = dict(comps=out.t.data_ptr(), hp=2, wp=3, q=q, lo=lo.data_ptr(), rgb=rgb.t.data_ptr(), OH=8, OW=8)
        a.update(kw)
        return lib.dinoseg_op_pca_colour(a["comps"], B, a["hp"], a["wp"], a["q"], a["lo"], inv.data_ptr(), None, a["OH"], a["OW"], a["rgb"], S())

    for kw in (dict(tokens=None), dict(sum=None), dict(count=None), dict(scratch=None), dict(D=0), dict(D=96), dict(D=1088), dict(B=0),
               dict(n=0), dict(B=1 << 16, n=1 << 16), dict(sum=acc.sum.t.data_ptr() + 4), dict(count=acc.count.t.data_ptr() + 4),
               dict(tokens=tok.data_ptr() + 4)):
        assert moments(**kw) == -1 and "dinoseg_op_token_moments" in capi.last_error(), kw
    for kw in (dict(tokens=None), dict(mean=None), dict(basis=None), dict(out=None), dict(D=32), dict(q=0), dict(q=257), dict(B=-1),
               dict(n=0), dict(basis=basis.data_ptr() + 4)):
        assert project(**kw) == -1 and "dinoseg_op_pca_project" in capi.last_error(), kw
    for kw in (dict(comps=None), dict(lo=None), dict(rgb=None), dict(q=2), dict(q=257), dict(hp=0), dict(OH=1), dict(OW=16385),
               dict(lo=lo.data_ptr() + 2)):
        assert colour(**kw) == -1 and "dinoseg_op_pca_colour" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert not bool(acc.sum.t.any()) and not bool(acc.outer.t.any()) and int(acc.count.t.item()) == 0
    assert bool((acc.scratch.t == 0xA5).all()) and bool((out.t == -7.0).all()) and bool((rgb.t == 0x5A).all())
    assert moments() == 0 and project() == 0 and colour() == 0
    torch.cuda.synchronize()
    assert int(acc.count.t.item()) == n and not bool((out.t == -7.0).any()) and not bool((rgb.t == 0x5A).all())
    assert acc.intact() and out.intact() and rgb.intact()


# ------------------------------------------------------------------------------------------------ 4. model level
def build(cfg, precision="fp16"):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def model(arch):
    return build(A.ARCH["T2"] if arch == "tiny" else VIT_S8)


H, W = 64, 128
ARCHS = ["tiny", "vits8"]


def frames_of(B, seed, fp32):
    x = torch.from_numpy(synthetic_frames(B, H, seed=seed, w=W)).cuda()
    return x.permute(0, 3, 1, 2).float().div(255.0).contiguous() if fp32 else x


def keep_of(B, n, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((B, n)) < 0.6).cuda()


def op_moments(tokens, keep, shift, s, o, cnt):
    B, n1, D = tokens.shape
    scratch = torch.empty((capi.lib().dinoseg_pca_scratch_bytes(B, n1 - 1, D),), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().dinoseg_op_token_moments(tokens.data_ptr(), capi.ptr(keep), B, n1 - 1, D, capi.ptr(shift), s.data_ptr(), capi.ptr(o),
                                                   cnt.data_ptr(), scratch.data_ptr(), S()))


def moments_by_hand(chunks):
    """the fitter's sequence of operator calls on (tokens, keep uint8 or None) chunks -> (shift, sum, outer, count)"""
    D = chunks[0][0].shape[2]
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")          # noqa: E731
    s, o, cnt, shift = z(D), z(D, D), z(1, dt=torch.int64), None
    for tokens, keep in chunks:
        if shift is None:
            s0, n0 = z(D), z(1, dt=torch.int64)
            op_moments(tokens, keep, None, s0, None, n0)
            if int(n0.item()) == 0:
                continue
            shift = (s0 / int(n0.item())).to(torch.float32)
        op_moments(tokens, keep, shift, s, o, cnt)
    return shift, s, o, cnt


def same_pca(a, b):
    return all(torch.equal(u32(x), u32(y)) for x, y in ((a.mean, b.mean), (a.basis, b.basis), (a.eigenvalues, b.eigenvalues))) and \
        (a.total_variance, a.rows, a.n_blocks) == (b.total_variance, b.rows, b.n_blocks)


def fit_bars(chunks, shift):
    """Over the fitter's chunks (tokens, keep as numpy): the moments' bars summed over the calls (each call has its own range length),
    each grown by the rounding of the points themselves against the exact x - shift -- |c - (x - shift)| <= 2^-24 |c|, so a product
    moves by at most (2 u + u^2) |c c| <= 3 u |c c| and a term of sum by u |c| -- and the kept rows x as fp64."""
    bar_s = bar_o = 0.0
    rows = []
    for tokens, keep in chunks:
        B, n1, D = tokens.shape
        c, kept = U.points(tokens, keep, shift)
        L = U.range_len(B * (n1 - 1), D)
        bs, bo = U.moment_bars(c, L)
        bar_s, bar_o = bar_s + bs * (L + 17) / (L + 16), bar_o + bo * (L + 19) / (L + 16)
        rows.append(tokens[:, 1:, :].reshape(-1, D)[kept].astype(np.float64))
    return bar_s, bar_o, np.concatenate(rows)


def covariance_bar(x64, shift, bar_s, bar_o):
    """||E||_F for E >= |cov(device moments) - cov(x)| elementwise: cov = (O - s s^T / N) / (N - 1) with |dO| <= bar_o, |ds| <= bar_s"""
    N = x64.shape[0]
    s = np.abs((x64 - shift.astype(np.float64)).sum(axis=0))
    E = (bar_o + (np.outer(bar_s, s) + np.outer(s, bar_s) + np.outer(bar_s, bar_s)) / N) / (N - 1)
    return float(np.linalg.norm(E))


@pytest.mark.parametrize("fp32", [False, True], ids=["uint8", "fp32"])
@pytest.mark.parametrize("arch", ARCHS)
def test_pca_fit_is_one_fitter_and_the_operators_by_hand(cuda, arch, fp32):
    """pca_fit equals a PCAFitter fed the same chunks and the operators + pca_solve by hand, bit for bit in every field; its
    eigenvalues are within ||E||_F of those of an fp64 PCA of the read-back features (Weyl), E the covariance's bar matrix from the
    moments' bars (plus one fp32 rounding of the stored eigenvalue); chunk = 1 against chunk = 32 agree within the two fits' bars."""
    m = model(arch)
    n, q, B = (H // m.cfg.patch) * (W // m.cfg.patch), 4, 5
    x, keep = frames_of(B, 500, fp32), keep_of(B, n, 501)
    pca = m.pca_fit(x, q=q, keep=keep, chunk=2)
    assert isinstance(pca, FeaturePCA) and pca.q == q and pca.dim == m.cfg.embed_dim and pca.rows == int(keep.sum()) and pca.n_blocks == 0
    fitter = PCAFitter(m)
    taken = [fitter.update(x[c0:c0 + 2], keep[c0:c0 + 2]) for c0 in range(0, B, 2)]
    assert taken == [int(keep[c0:c0 + 2].sum()) for c0 in range(0, B, 2)]
    assert same_pca(fitter.solve(q), pca)
    chunks = [(m.features(x[c0:c0 + 2]), keep[c0:c0 + 2].to(torch.uint8).contiguous()) for c0 in range(0, B, 2)]
    shift, s, o, cnt = moments_by_hand(chunks)
    assert same_pca(pca_solve(s.cpu(), o.cpu(), int(cnt.item()), shift.cpu(), q), pca)
    # Weyl, against the fp64 PCA of the features themselves
    host = [(t.cpu().numpy(), k.cpu().numpy()) for t, k in chunks]
    bar_s, bar_o, x64 = fit_bars(host, shift.cpu().numpy())
    e2 = covariance_bar(x64, shift.cpu().numpy(), bar_s, bar_o)
    lam = np.linalg.eigvalsh(np.cov(x64, rowvar=False))[::-1]
    err = np.abs(pca.eigenvalues.numpy().astype(np.float64) - lam[:q])
    print(f"pca_fit {arch}: eigenvalues {lam[:q]}, worst error at {float((err / (e2 + U.U * lam[:q])).max()):.4f} of the Weyl bar")
    assert np.all(err <= e2 + U.U * lam[:q])
    assert abs(pca.total_variance - lam.sum()) <= np.sqrt(m.cfg.embed_dim) * e2
    # chunk = 1 (another shift: the first frame's mean) against chunk = 32
    for chunk in (1, 32):
        other = m.pca_fit(x, q=q, keep=keep, chunk=chunk)
        k8 = keep.to(torch.uint8)
        oc = [(m.features(x[c0:c0 + chunk]).cpu().numpy(), k8[c0:c0 + chunk].cpu().numpy()) for c0 in range(0, B, chunk)]
        osh = PCAFitter(m)
        osh.update(x, keep, chunk)
        bs, bo, _ = fit_bars(oc, osh.shift.cpu().numpy())
        e_other = covariance_bar(x64, osh.shift.cpu().numpy(), bs, bo)
        d = np.abs(other.eigenvalues.numpy().astype(np.float64) - pca.eigenvalues.numpy().astype(np.float64))
        assert np.all(d <= e2 + e_other + 2 * U.U * lam[:q])


def test_planted_directions_within_davis_kahan(cuda):
    """Planted tokens -- three strong orthogonal directions plus small noise around a large common mean -- through the moments
    operator in two chunks and pca_solve: with gap the distance of an eigenvalue to the rest of the fp64 spectrum, first
    gap >= 100 ||E||_F (an input without a clear gap fails as a bad input), then |<v, v64>| >= 1 - (2 ||E||_F / gap)^2
    (Davis-Kahan's sin theta <= 2 ||E|| / gap), v the stored fp32 component normalised in fp64: rounding a unit vector to fp32 moves
    its direction's cosine only in second order."""
    B, n, D, q = 2, 300, 128, 3
    rng = np.random.default_rng(77)
    dirs = np.linalg.qr(rng.standard_normal((D, q)))[0].T
    mean = 3.0 * rng.standard_normal(D)
    coef = rng.standard_normal((B * n, q)) * np.array([8.0, 4.0, 2.0])
    rows = (mean + coef @ dirs + 0.05 * rng.standard_normal((B * n, D))).astype(np.float32)
    tokens = np.full((B, 1 + n, D), 1.0e3, np.float32)
    tokens[:, 1:, :] = rows.reshape(B, n, D)
    chunks = [(dev(tokens[b:b + 1]), None) for b in range(B)]
    shift, s, o, cnt = moments_by_hand(chunks)
    pca = pca_solve(s.cpu(), o.cpu(), int(cnt.item()), shift.cpu(), q)
    bar_s, bar_o, x64 = fit_bars([(tokens[b:b + 1], None) for b in range(B)], shift.cpu().numpy())
    e2 = covariance_bar(x64, shift.cpu().numpy(), bar_s, bar_o)
    lam, vec = np.linalg.eigh(np.cov(x64, rowvar=False))
    lam, vec = lam[::-1], vec[:, ::-1]
    for j in range(q):
        gap = float(np.min(np.abs(np.delete(lam, j) - lam[j])))
        assert gap >= 100.0 * e2, "the planted spectrum has no clear gap: a bad input, not a kernel error"
        v = pca.basis[j].numpy().astype(np.float64)
        cos = abs(float(v @ vec[:, j])) / float(np.linalg.norm(v))
        print(f"planted direction {j}: eigenvalue {lam[j]:.4f}, gap {gap:.4f}, ||E||_F {e2:.3e}, 1 - |<v, v64>| = {1.0 - cos:.3e}")
        assert cos >= 1.0 - (2.0 * e2 / gap) ** 2
        assert abs(float(pca.basis[j].numpy().astype(np.float64) @ dirs[j])) > 0.99             # and it is the planted one
        assert abs(float(pca.eigenvalues[j]) - lam[j]) <= e2 + U.U * lam[j]
        assert float(pca.basis[j][int(pca.basis[j].abs().argmax())]) > 0.0                     # the sign rule


@pytest.mark.parametrize("fp32", [False, True], ids=["uint8", "fp32"])
@pytest.mark.parametrize("arch", ARCHS)
def test_pca_project_and_map_are_the_operators_by_hand(cuda, arch, fp32):
    m = model(arch)
    hp, wp = H // m.cfg.patch, W // m.cfg.patch
    n, B, D = hp * wp, 3, m.cfg.embed_dim
    x = frames_of(B, 510, fp32)
    pca = m.pca_fit(x, q=5)
    mean, basis, white = pca.mean.cuda(), pca.basis.cuda(), pca.whitening().cuda()
    tokens = m.features(x)
    plain, whitened = run_project(tokens, mean, basis, None, 5).t, run_project(tokens, mean, basis, white, 5).t
    got = m.pca_project(x, pca)
    assert got.shape == (B, n, 5) and got.dtype == torch.float32 and torch.equal(u32(got), u32(plain[:, 1:]))
    assert torch.equal(u32(m.pca_project(x, pca, whiten=True, n_blocks=0)), u32(whitened[:, 1:]))
    ev = pca.eigenvalues.numpy().astype(np.float64)
    assert np.array_equal(pca.whitening().numpy(), (1.0 / np.sqrt(ev)).astype(np.float32))
    # the map with the call's own range, with and without a mask, at the frames' size and another
    keep = got[..., 0] > 0                                               # the demo's first stage
    for kp, size in ((None, None), (keep, (H + 5, W - 3))):
        OH, OW = (H, W) if size is None else size
        v = plain[:, 1:, :3]
        if kp is None:
            lo, hi = v.amin(dim=(0, 1)), v.amax(dim=(0, 1))
        else:
            lo = torch.where(kp.unsqueeze(-1), v, float("inf")).amin(dim=(0, 1))
            hi = torch.where(kp.unsqueeze(-1), v, float("-inf")).amax(dim=(0, 1))
        inv = 1.0 / (hi - lo)
        k8 = None if kp is None else kp.to(torch.uint8).contiguous()
        want = run_colour(plain.contiguous(), hp, wp, lo.contiguous(), inv.contiguous(), k8, OH, OW).t
        rgb = m.pca_map(x, pca, size=size, keep=kp)
        assert rgb.dtype == torch.uint8 and rgb.shape == (B, OH, OW, 3) and torch.equal(rgb, want)
    # fixed ranges: a frame alone or inside a batch gives the same bytes; a degenerate range gives a channel of zeros
    fixed = m.pca_map(x, pca, lo=(-1.0, -0.5, -2.0), hi=(1.0, 0.5, -2.0))
    for b in range(B):
        assert torch.equal(m.pca_map(x[b:b + 1], pca, lo=(-1.0, -0.5, -2.0), hi=(1.0, 0.5, -2.0))[0], fixed[b])
    assert not bool(fixed[..., 2].any()) and bool(fixed[..., 0].any())
    # the two-stage recipe runs end to end
    p2 = m.pca_fit(x, keep=keep)
    assert p2.rows == int(keep.sum()) and m.pca_map(x, p2, keep=keep).shape == (B, H, W, 3)
    for call in (lambda: m.pca_project(x, pca, n_blocks=1), lambda: m.pca_map(x, m.pca_fit(x, q=2)), lambda: m.pca_map(x, pca, size=(2, 2)),
                 lambda: m.pca_map(x, pca, keep=keep[:1]), lambda: m.pca_fit(x, q=0), lambda: m.pca_fit(x, q=D + 1)):
        with pytest.raises(ValueError):
            call()


def test_an_intermediate_depth_runs_through_fit_project_and_map(cuda):
    """n_blocks = 1 on the tiny ViT (two blocks): pca_fit, pca_project and pca_map take the features after one block -- the
    operators by hand on features(x, 1), bit for bit -- and differ from the full depth's; a call for another depth is refused."""
    m = model("tiny")
    hp, wp = H // m.cfg.patch, W // m.cfg.patch
    x = frames_of(2, 530, False)
    pca = m.pca_fit(x, q=3, n_blocks=1)
    assert pca.n_blocks == 1
    tokens = m.features(x, 1)
    shift, s, o, cnt = moments_by_hand([(tokens, None)])
    assert same_pca(pca_solve(s.cpu(), o.cpu(), int(cnt.item()), shift.cpu(), 3, 1), pca)
    plain = run_project(tokens, pca.mean.cuda(), pca.basis.cuda(), None, 3).t
    got = m.pca_project(x, pca)
    assert torch.equal(u32(got), u32(plain[:, 1:])) and torch.equal(u32(m.pca_project(x, pca, n_blocks=1)), u32(got))
    v = plain[:, 1:, :3]
    lo, hi = v.amin(dim=(0, 1)), v.amax(dim=(0, 1))
    want = run_colour(plain.contiguous(), hp, wp, lo.contiguous(), (1.0 / (hi - lo)).contiguous(), None, H, W).t
    assert torch.equal(m.pca_map(x, pca), want)
    assert not torch.equal(u32(m.pca_project(x, m.pca_fit(x, q=3))), u32(got))
    with pytest.raises(ValueError):
        m.pca_project(x, pca, n_blocks=0)


def normalize(tokens):
    B, n1, D = tokens.shape
    planes = torch.empty((B, 2, n1 - 1, D), dtype=torch.float16, device="cuda")
    capi.check(capi.lib().dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n1 - 1, D, planes.data_ptr(), S()))
    return planes


def knn_by_hand(planes, bank, C, k, tau):
    B, _, n, D = planes.shape
    N = B * n
    seg = torch.empty((N, C), dtype=torch.float32, device="cuda")
    idx = torch.empty((N, k), dtype=torch.int32, device="cuda")
    scratch = torch.empty((capi.lib().dinoseg_knn_scratch_bytes(N, bank.size, k, 0),), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().dinoseg_op_knn_labels(planes.data_ptr(), B, n, bank.planes.data_ptr(), bank.size, bank.capacity,
                                                bank.labels.data_ptr(), 1 if bank.hard else 0, D, C, k, tau, 0, seg.data_ptr(), idx.data_ptr(),
                                                None, scratch.data_ptr(), S()))
    return seg, idx


def pixel_labels(B, OH, OW, C, seed):
    rng = np.random.default_rng(seed)
    y = np.stack([(np.add.outer(np.arange(OH) // 9, np.arange(OW) // 13 + b) % C) for b in range(B)]).astype(np.int64)
    y[rng.random((B, OH, OW)) < 0.05] = 255
    return torch.from_numpy(y)


def test_projected_bank_is_the_operators_by_hand(cuda):
    """On the tiny ViT (width 128) a bank with project (q = 64): segment_knn equals features, project, normalise and
    dinoseg_op_knn_labels by hand, bit for bit; a frame added to it retrieves its own label_cells labels at every pixel; the state
    carries the projection; a bank without project keeps the path it had (the same call before and after loading a state without a
    projection, and the operators by hand at the model's width)."""
    m = model("tiny")
    hp, wp = H // m.cfg.patch, W // m.cfg.patch
    n, C, k = hp * wp, 5, 3
    xb, yb, x = frames_of(2, 520, False), pixel_labels(2, H, W, C, 521), frames_of(3, 522, True)
    pca = m.pca_fit(torch.cat([xb, frames_of(3, 522, False)]), q=64)
    bank = MemoryBank(m, C, 3 * n, project=pca)
    assert bank.dim == 64 and bank.planes.shape == (2, 3 * n, 64)
    assert bank.add(xb, yb) == 2 * n
    got = m.segment_knn(x, bank, topk=k, temperature=0.2, chunk=2, want_seg=True, want_idx=True)
    mean, basis = pca.mean.cuda(), pca.basis.cuda()
    rows_b = normalize(run_project(m.features(xb), mean, basis, None, 64).t.contiguous())
    assert torch.equal(bank.planes[:, :2 * n].view(torch.int16), rows_b.permute(1, 0, 2, 3).reshape(2, 2 * n, 64).view(torch.int16))
    seg, idx = knn_by_hand(normalize(run_project(m.features(x), mean, basis, None, 64).t.contiguous()), bank, C, k, 0.2)
    assert torch.equal(u32(got.seg.view(-1, C)), u32(seg)) and torch.equal(got.idx.view(-1, k), idx)
    labels = torch.empty((3, H, W), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(seg.data_ptr(), 3, hp, wp, C, H, W, labels.data_ptr(), None, S()))
    assert torch.equal(got.labels, labels)
    # self-retrieval
    own = MemoryBank(m, C, n, project=pca)
    own.add(xb[:1], yb[:1])
    res = m.segment_knn(xb[:1], own, topk=1, want_seg=True, want_idx=True)
    assert torch.equal(res.idx.view(-1), torch.arange(n, dtype=torch.int32, device="cuda"))
    cells = torch.empty((n, C), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_label_cells(yb[0].cuda().data_ptr(), 1, H, W, hp, wp, C, cells.data_ptr(), S()))
    capi.check(capi.lib().dinoseg_op_upsample_argmax(cells.data_ptr(), 1, hp, wp, C, H, W, labels.data_ptr(), None, S()))
    assert torch.equal(res.seg[0], cells) and torch.equal(res.labels[0], labels[0])
    # the state carries the projection bit for bit
    state = bank.state_dict()
    other = MemoryBank(m, C, 3 * n, project=m.pca_fit(xb, q=64))
    other.load_state_dict(state)
    assert same_pca(other.project, pca) and torch.equal(m.segment_knn(x, other, topk=k, temperature=0.2).labels, got.labels)
    for bad in (lambda: MemoryBank(m, C, 3 * n).load_state_dict(state), lambda: MemoryBank(m, C, 3 * n, project=m.pca_fit(xb, q=3)),
                lambda: MemoryBank(m, C, 3 * n, n_blocks=1, project=pca), lambda: m.segment_knn(x, bank, n_blocks=1)):
        with pytest.raises(ValueError):
            bad()
    # without project: the parent's path
    plain = MemoryBank(m, C, 3 * n)
    plain.add(xb, yb)
    before = m.segment_knn(x, plain, topk=k, temperature=0.2, want_seg=True, want_idx=True)
    st = plain.state_dict()
    assert "project" not in st and plain.dim == m.cfg.embed_dim and plain.project is None
    again = MemoryBank(m, C, 3 * n)
    again.load_state_dict(st)
    after = m.segment_knn(x, again, topk=k, temperature=0.2, want_seg=True, want_idx=True)
    seg, idx = knn_by_hand(normalize(m.features(x)), plain, C, k, 0.2)
    for r in (before, after):
        assert torch.equal(u32(r.seg.view(-1, C)), u32(seg)) and torch.equal(r.idx.view(-1, k), idx) and torch.equal(r.labels, before.labels)
    with pytest.raises(ValueError):
        MemoryBank(m, C, 3 * n, project=pca).load_state_dict(st)
