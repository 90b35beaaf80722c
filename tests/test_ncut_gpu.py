"""Normalized cut on the 1-bit patch graph on the device: dinoseg_op_ncut_graph and dinoseg_op_ncut_iterate through the C-ABI against
the fp64 restatement of the rule (tests/ncut_util.py) -- the graph pair by pair, four teacher-forced passes and the result rule with
their bars, the planted partition end to end, run-to-run identity, containment, refusals -- and DINOSeg.ncut against the operators
applied by hand."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, NcutResult, ViTConfig, capi, ncut_start, procedural_state_dict
from dino_amd.weights import synthetic_frames
from tests import arch_util as A
from tests import ncut_util as NC

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
UNDECIDED_CAP = 0.04
PASSES = 4
EPS = 1e-5
START_SEED = 3

# (B, hp, wp, D)
CASES = [
    (1, 1, 1, 64),                      # one cell: nothing is left after the deflation
    (1, 1, 3, 64),
    (1, 5, 7, 64),                      # ragged tile
    (2, 8, 8, 64),                      # exactly one word, two frames
    (1, 5, 13, 64),                     # 65 cells: one bit in the second word
    (2, 9, 11, 192),                    # three D slices, two frames
    (2, 12, 16, 768),                   # ViT-B width, three query tiles
    (1, 20, 24, 384),                   # ViT-S width, a row of words shorter than the eight-word groups of the row sums
    (1, 60, 80, 384),                   # the camera's grid: 75 words per row
]
# every case with both kinds of input at tau = 0.2, and once at tau = 0
PARAMS = [(i, kind, 0.2) for i in range(len(CASES)) for kind in ("normal", "planted")] + [(i, "normal", 0.0) for i in range(len(CASES))]
PLANTED = [(i, "planted", 0.2) for i in range(len(CASES))]


def pid(p):
    return "x".join(str(v) for v in CASES[p[0]]) + f"-{p[1]}-tau{p[2]}"


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def normalize(tokens):
    """tokens: device fp32 [B, 1 + n, D] -> planes fp16 [B, 2, n, D]"""
    B, n1, D = tokens.shape
    planes = torch.empty((B, 2, n1 - 1, D), dtype=torch.float16, device="cuda")
    capi.check(capi.lib().dinoseg_op_normalize_tokens(tokens.data_ptr(), B, n1 - 1, D, planes.data_ptr(), S()))
    return planes


def nc_graph(planes, tau, out=None):
    """-> (graph int64 [B, n, W] holding the uint64 words, degree int32 [B, n])"""
    B, _, n, D = planes.shape
    W = NC.words_of(n)
    assert capi.lib().dinoseg_ncut_graph_bytes(B, n) == 8 * B * n * W
    graph, degree = out or (torch.empty((B, n, W), dtype=torch.int64, device="cuda"), torch.empty((B, n), dtype=torch.int32, device="cuda"))
    capi.check(capi.lib().dinoseg_op_ncut_graph(planes.data_ptr(), B, n, D, float(tau), graph.data_ptr(), degree.data_ptr(), S()))
    return graph, degree


OUT_SPECS = (("z_out", torch.float32), ("fg", torch.uint8), ("eigvec", torch.float32), ("margin", torch.float32))


def nc_iterate(graph, degree, z_in, iters, eps=EPS, out=None):
    """-> dict(z_out fp32 [B, n], rho fp32 [B, iters], fg uint8 [B, n], eigvec fp32 [B, n], margin fp32 [B, n], seed_cell int32 [B])"""
    B, n = degree.shape
    if out is None:
        out = {k: torch.empty((B, n), dtype=dt, device="cuda") for k, dt in OUT_SPECS}
        out["rho"] = torch.empty((B, iters), dtype=torch.float32, device="cuda")
        out["seed_cell"] = torch.empty((B,), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_ncut_iterate(graph.data_ptr(), degree.data_ptr(), B, n, float(eps), z_in.data_ptr(), iters,
                                                  out["z_out"].data_ptr(), out["rho"].data_ptr() if iters else None, out["fg"].data_ptr(),
                                                  out["eigvec"].data_ptr(), out["margin"].data_ptr(), out["seed_cell"].data_ptr(), S()))
    return out


def start_for(B, n):
    return ncut_start(n, START_SEED).cuda().expand(B, n).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(i, kind):
    """(tokens fp32 [B, 1 + n, D], small bool [B, n] or None) of a case, seeded by the case and the kind"""
    B, hp, wp, D = CASES[i]
    n, seed = hp * wp, 600 + 10 * i + (kind == "planted")
    tok, small = (NC.normal_tokens(seed, B, n, D), None) if kind == "normal" else NC.planted_tokens(seed, B, n, D)
    tok.setflags(write=False)
    return tok, small


@functools.lru_cache(maxsize=None)
def device_points(i, kind):
    """(planes on the device, the points they define in fp64 on the host [B, n, D]), computed once per case"""
    planes = normalize(dev(inputs(i, kind)[0]))
    X = NC.frame_points(planes.cpu().numpy())
    X.setflags(write=False)
    return planes, X


@functools.lru_cache(maxsize=4)
def device_graph(p):
    """(graph and degree on the device, the graph as bool [B, n, n] and its pad bits on the host), computed once per parameter set"""
    i, kind, tau = p
    n = CASES[i][1] * CASES[i][2]
    graph, degree = nc_graph(device_points(i, kind)[0], tau)
    words = graph.cpu().numpy().view(np.uint64)
    bits, pad = zip(*(NC.unpack_words(w, n) for w in words))
    return graph, degree, np.stack(bits), np.stack(pad)


def bits_of(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.uint64 else t


@pytest.mark.parametrize("p", PARAMS, ids=pid)
def test_graph_against_fp64_pair_by_pair(cuda, p):
    """Every pair with |s_fp64 - tau| > 2 E has the host's bit (E = (D + 16) 2^-24 is the score's bar; every other pair lies in the
    band, where either bit is right); at most 4 % of a frame's pairs are undecided; graph == graph^T at every pair; the degree is the
    popcount exactly; pad bits are zero."""
    i, kind, tau = p
    B, hp, wp, D = CASES[i]
    n, E, tau32 = hp * wp, NC.score_bar(D), float(np.float32(tau))
    X = device_points(i, kind)[1]
    _, degree, bits, pad = device_graph(p)
    assert not pad.any()
    worst = 0.0
    for b in range(B):
        Sh = NC.scores_host(X[b])
        decided = np.abs(Sh - tau32) > 2.0 * E
        share = 1.0 - float(decided.mean())
        worst = max(worst, share)
        assert np.array_equal(bits[b][decided], (Sh > tau32)[decided]), "a decided pair's bit differs from the host's"
        assert share <= UNDECIDED_CAP
        assert np.array_equal(bits[b], bits[b].T), "the graph is not symmetric"
        assert np.array_equal(degree[b].cpu().numpy(), bits[b].sum(1))
        assert bits[b].diagonal().all()                                 # s_ii = 1 up to E: every cell is its own neighbour
    print(f"ncut graph {pid(p)}: undecided at most {worst:.5f} of the pairs; density {bits.mean():.3f}")


@pytest.mark.parametrize("p", PARAMS, ids=pid)
def test_four_teacher_forced_passes_and_the_result_against_fp64(cuda, p):
    """Four calls with iters = 1 chained through z_out on the DEVICE's graph, each checked against the fp64 restatement applied to
    the same graph and the device's own z_in.  Bars (written before the first device run; tests/ncut_util.py: pass_bars): per row the
    fp32 sum (cnt_i + 16) 2^-24 sum over the set bits of |xv_j| plus the terms' own roundings, carried through r_i into y, rho and p,
    then through the deflation and the normalisation into z'.  A bar of inf (n = 1: nothing is left after the deflation) is checked as
    z' = 0 exactly.  The result rule is checked on the device's own z: fg wherever |v_i - avg| exceeds its bar, seed_cell wherever
    the two largest |v| differ by more than theirs, sigma wherever the seed is decided and clear of the mean, eigvec within its bar.
    iters = 4 in one launch equals the four chained calls bit for bit."""
    i, kind, tau = p
    B, hp, wp, D = CASES[i]
    n = hp * wp
    graph, degree, bits, _ = device_graph(p)
    cnt = degree.cpu().numpy().astype(np.int64)
    z = start_for(B, n)
    worst_z, worst_rho, undecided_fg, rhos, last = 0.0, 0.0, 0, [], None
    bits_f = [bits[b].astype(np.float64) for b in range(B)]
    wts = [NC.weights(cnt[b], n, EPS) for b in range(B)]
    for t in range(PASSES):
        out = nc_iterate(graph, degree, z, 1)
        z_in, z_out, rho = z.cpu().numpy().astype(np.float64), out["z_out"].cpu().numpy().astype(np.float64), out["rho"].cpu().numpy()
        for b in range(B):
            _, r, u = wts[b]
            o = NC.one_pass(bits_f[b], r, u, EPS, z_in[b])
            dz, drho, _ = NC.pass_bars(o, bits_f[b], cnt[b], r, u, EPS)
            if n == 1:
                assert not z_out[b].any() and rho[b, 0] == 0.0
                continue
            assert np.all(np.isfinite(dz)), "the normalisation is undetermined at the bars"
            err = np.abs(z_out[b] - o["z"])
            worst_z = max(worst_z, float((err / dz).max()))
            worst_rho = max(worst_rho, abs(float(rho[b, 0]) - o["rho"]) / drho)
            assert np.all(err <= dz)
            assert abs(float(rho[b, 0]) - o["rho"]) <= drho
            assert abs(np.linalg.norm(z_out[b]) - 1.0) <= 1e-6
        rhos.append(out["rho"])
        z, last = out["z_out"], out
    # the result rule on the device's own z
    z_dev = last["z_out"].cpu().numpy().astype(np.float64)
    for b in range(B):
        _, r, u = wts[b]
        res = NC.result_host(z_dev[b], r)
        dv, davg = NC.result_bars(res)
        fg, eig = last["fg"][b].cpu().numpy().astype(bool), last["eigvec"][b].cpu().numpy().astype(np.float64)
        margin, seed = last["margin"][b].cpu().numpy(), int(last["seed_cell"][b])
        assert np.array_equal(fg, margin > 0) and 0 <= seed < n
        a = np.abs(res["v"])
        order = np.argsort(-a, kind="stable")
        seed_decided = n == 1 or a[order[0]] - a[order[1]] > dv[order[0]] + dv[order[1]]
        if seed_decided:
            assert seed == res["seed"]
        else:
            assert a[seed] >= a[order[0]] - 2.0 * dv[order[0]]
        if seed_decided and abs(res["v"][seed] - res["avg"]) > dv[seed] + davg:
            clear = np.abs(res["v"] - res["avg"]) > dv + davg
            undecided_fg += int((~clear).sum())
            assert np.array_equal(fg[clear], res["fg"][clear])
            assert np.all(np.abs(eig - res["eigvec"]) <= dv)
            assert np.all(np.abs(margin - res["margin"]) <= dv + davg + NC.EPS32 * np.abs(res["margin"]))
        else:
            assert np.all(np.abs(np.abs(eig) - a) <= dv)
    # one launch of four passes
    one = nc_iterate(graph, degree, start_for(B, n), PASSES)
    assert torch.equal(bits_of(one["rho"]), bits_of(torch.cat(rhos, dim=1)))
    for k in ("z_out", "fg", "eigvec", "margin", "seed_cell"):
        assert torch.equal(bits_of(one[k]), bits_of(last[k])), k
    print(f"ncut passes {pid(p)}: z' at most {worst_z:.3f} of its bar, rho {worst_rho:.3f} of its bar; {undecided_fg} cells undecided "
          f"at the result's bar; rho after {PASSES} passes {[round(float(v), 5) for v in one['rho'][:, -1]]}")


def test_zero_passes_is_the_result_rule_on_the_prepared_start(cuda):
    p = (5, "normal", 0.2)
    B, hp, wp, D = CASES[p[0]]
    n = hp * wp
    graph, degree, _, _ = device_graph(p)
    cnt = degree.cpu().numpy().astype(np.int64)
    out = nc_iterate(graph, degree, start_for(B, n), 0)
    again = nc_iterate(graph, degree, out["z_out"], 0)                  # preparing a prepared vector moves it by roundings only
    for b in range(B):
        _, r, u = NC.weights(cnt[b], n, EPS)
        z0 = NC.dn(ncut_start(n, START_SEED).numpy(), u)[0]
        z_dev = out["z_out"][b].cpu().numpy().astype(np.float64)
        assert np.abs(z_dev - z0).max() <= 8.0 * NC.EPS32               # 4 e |z0_i| with |z0_i| <= 1, and u's own rounding
        res = NC.result_host(z_dev, r)
        assert int(out["seed_cell"][b]) == res["seed"]
        assert np.array_equal(out["fg"][b].cpu().numpy().astype(bool), res["fg"])
        assert np.abs(again["z_out"][b].cpu().numpy() - z_dev).max() <= 8.0 * NC.EPS32


@pytest.mark.parametrize("p", PLANTED, ids=pid)
def test_planted_groups_end_to_end(cuda, p):
    """32 passes on the planted inputs: fg is the smaller planted group at EVERY cell, the pixel labels at the patch grid's own size
    are fg, and the last Rayleigh record is within 1e-5 of the second eigenvalue that fp64 eigvalsh finds for the device's graph
    (the gap to the third is about 1: convergence, not luck)."""
    i, kind, tau = p
    B, hp, wp, D = CASES[i]
    n = hp * wp
    small = inputs(i, kind)[1]
    graph, degree, bits, _ = device_graph(p)
    cnt = degree.cpu().numpy().astype(np.int64)
    out = nc_iterate(graph, degree, start_for(B, n), 32)
    fg = out["fg"].cpu().numpy().astype(bool)
    assert np.array_equal(fg, small)
    two = torch.stack((torch.zeros_like(out["margin"]), out["margin"]), dim=2).contiguous()
    labels = torch.empty((B, hp, wp), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(two.data_ptr(), B, hp, wp, 2, hp, wp, labels.data_ptr(), None, S()))
    assert np.array_equal(labels.cpu().numpy().reshape(B, n), fg.astype(np.int32))
    for b in range(B):
        if n < 2:
            assert float(out["rho"][b, -1]) == 0.0                      # one cell: there is no second eigenvalue
            continue
        _, r, u = NC.weights(cnt[b], n, EPS)
        assert small[b][int(out["seed_cell"][b])] and float(out["eigvec"][b, int(out["seed_cell"][b])]) > 0
        M = r[:, None] * (EPS + (1.0 - EPS) * bits[b].astype(np.float64)) * r[None, :]
        lam = np.linalg.eigvalsh(M)
        assert abs(float(out["rho"][b, -1]) - lam[-2]) <= 1e-5
        assert n < 3 or lam[-2] - lam[-3] > 0.4
        print(f"ncut planted {pid(p)} frame {b}: rho {float(out['rho'][b, -1]):.7f}, lambda_2 {lam[-2]:.7f}, lambda_3 "
              f"{lam[-3] if n > 2 else float('nan'):.4f}")


def full_run(p):
    i, kind, tau = p
    B, hp, wp, D = CASES[i]
    graph, degree = nc_graph(device_points(i, kind)[0], tau)
    out = nc_iterate(graph, degree, start_for(B, hp * wp), 6)
    return [graph.cpu(), degree.cpu()] + [bits_of(out[k]).cpu() for k in ("z_out", "rho", "fg", "eigvec", "margin", "seed_cell")]


@pytest.mark.parametrize("p", [(5, "normal", 0.2), (6, "planted", 0.2), (7, "normal", 0.0)], ids=pid)
def test_two_runs_are_bit_identical_and_z_out_may_be_z_in(cuda, p):
    a, b = full_run(p), full_run(p)
    assert len(a) == 8
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    i, kind, tau = p
    B, hp, wp, D = CASES[i]
    graph, degree, _, _ = device_graph(p)
    z = start_for(B, hp * wp)
    out = {k: torch.empty((B, hp * wp), dtype=dt, device="cuda") for k, dt in OUT_SPECS}
    out.update(z_out=z, rho=torch.empty((B, 6), dtype=torch.float32, device="cuda"), seed_cell=torch.empty((B,), dtype=torch.int32, device="cuda"))
    nc_iterate(graph, degree, z, 6, out=out)
    for x, k in zip(a[2:], ("z_out", "rho", "fg", "eigvec", "margin", "seed_cell")):
        assert torch.equal(x, bits_of(out[k]).cpu()), k


class Guarded:
    """`nbytes` of device memory between two guard bands of 4 KiB, everything filled with 0xA5"""
    BAND = 4096

    def __init__(self, nbytes, dtype, shape):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * self.BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.raw[self.BAND:self.BAND + nbytes].view(dtype).view(shape)

    def bands_intact(self):
        return bool((self.raw[:self.BAND] == 0xA5).all()) and bool((self.raw[self.BAND + self.nbytes:] == 0xA5).all())


@pytest.mark.parametrize("i", [1, 2, 3, 4, 5])
def test_outputs_and_the_graph_stay_between_their_guard_bands(cuda, i):
    B, hp, wp, D = CASES[i]
    n, W, iters = hp * wp, NC.words_of(hp * wp), 3
    planes = device_points(i, "normal")[0]
    graph = Guarded(B * n * W * 8, torch.int64, (B, n, W))
    degree = Guarded(B * n * 4, torch.int32, (B, n))
    nc_graph(planes, 0.2, out=(graph.view, degree.view))
    g = {k: Guarded(B * n * dt.itemsize, dt, (B, n)) for k, dt in OUT_SPECS}
    g["rho"] = Guarded(B * iters * 4, torch.float32, (B, iters))
    g["seed_cell"] = Guarded(B * 4, torch.int32, (B,))
    nc_iterate(graph.view, degree.view, start_for(B, n), iters, out={k: v.view for k, v in g.items()})
    torch.cuda.synchronize()
    for v in [graph, degree] + list(g.values()):
        assert v.bands_intact()
    want_g, want_d = nc_graph(planes, 0.2)
    assert torch.equal(graph.view, want_g) and torch.equal(degree.view, want_d)
    want = nc_iterate(want_g, want_d, start_for(B, n), iters)
    for k, v in g.items():
        assert torch.equal(bits_of(v.view), bits_of(want[k])), k


def test_refusals_return_minus_one_without_launching(cuda):
    B, hp, wp, D = 2, 5, 7, 64
    n, W, iters = hp * wp, 1, 2
    lib = capi.lib()
    cells = lib.dinoseg_ncut_max_cells()
    planes = normalize(torch.randn((B, n + 1, D), device="cuda"))
    graph = torch.full((B, n, W + 1), -7, dtype=torch.int64, device="cuda")
    degree = torch.full((B, n), -7, dtype=torch.int32, device="cuda")
    z = start_for(B, n)
    z_before = z.clone()
    outs = {k: torch.full((B, n), 9, dtype=dt, device="cuda") for k, dt in OUT_SPECS}
    rho = torch.full((B, iters), 9.0, device="cuda")
    seed = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    good = dict(planes=planes.data_ptr(), B=B, n=n, D=D, tau=0.2, graph=graph.data_ptr(), degree=degree.data_ptr(), eps=EPS,
                z_in=z.data_ptr(), iters=iters, z_out=outs["z_out"].data_ptr(), rho=rho.data_ptr(), fg=outs["fg"].data_ptr(),
                eigvec=outs["eigvec"].data_ptr(), margin=outs["margin"].data_ptr(), seed=seed.data_ptr())

    def build(**kw):
        g = dict(good)
        g.update(kw)
        return lib.dinoseg_op_ncut_graph(g["planes"], g["B"], g["n"], g["D"], g["tau"], g["graph"], g["degree"], S())

    def iterate(**kw):
        g = dict(good)
        g.update(kw)
        return lib.dinoseg_op_ncut_iterate(g["graph"], g["degree"], g["B"], g["n"], g["eps"], g["z_in"], g["iters"], g["z_out"], g["rho"],
                                           g["fg"], g["eigvec"], g["margin"], g["seed"], S())

    shapes = [dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(n=cells + 1), dict(B=1 << 30, n=4800)]
    for kw in [dict(planes=None), dict(graph=None), dict(degree=None), dict(planes=planes.data_ptr() + 2), dict(graph=graph.data_ptr() + 4),
               dict(degree=degree.data_ptr() + 2), dict(D=0), dict(D=-64), dict(D=96), dict(D=8256), dict(tau=1.0), dict(tau=-1.0),
               dict(tau=float("nan")), dict(tau=float("inf"))] + shapes:
        assert build(**kw) == -1, kw
        assert "dinoseg_op_ncut_graph" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert bool((graph == -7).all()) and bool((degree == -7).all())
    assert build() == 0                                                 # ... and the good call runs, inside its rows
    torch.cuda.synchronize()
    assert not bool((degree == -7).any()) and bool((graph.view(-1)[B * n * W:] == -7).all())
    for kw in [dict(graph=None), dict(degree=None), dict(z_in=None), dict(z_out=None), dict(fg=None), dict(eigvec=None), dict(seed=None),
               dict(rho=None), dict(graph=graph.data_ptr() + 4), dict(degree=degree.data_ptr() + 2), dict(z_in=z.data_ptr() + 2),
               dict(rho=rho.data_ptr() + 1), dict(margin=outs["margin"].data_ptr() + 2), dict(eps=-1e-9), dict(eps=1.0),
               dict(eps=float("nan")), dict(iters=-1), dict(iters=4097)] + shapes:
        assert iterate(**kw) == -1, kw
        assert "dinoseg_op_ncut_iterate" in capi.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((v == 9).all()) for v in outs.values()) and bool((rho == 9.0).all()) and bool((seed == 9).all())
    assert torch.equal(z, z_before)
    assert iterate() == 0 and iterate(margin=None) == 0 and iterate(iters=0, rho=None) == 0
    torch.cuda.synchronize()
    assert not bool((rho == 9.0).any()) and not bool((seed == 9).any())


# ------------------------------------------------------------------------------------------------ model level
def build_model(cfg, precision="fp16"):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def model(tag):
    return build_model(A.ARCH["T2"] if tag == "tiny" else ViTConfig(n_blocks=2))


def frames_of(tag, B, seed):
    H, W = (40, 56) if tag == "tiny" else (64, 128)
    return torch.from_numpy(synthetic_frames(B, H, seed=seed, w=W)).cuda()


def by_hand(m, x, tau, eps, iters, seed, chunk, size):
    """The operators applied by hand to features() of the same chunks -> the fields of NcutResult"""
    p = m.cfg.patch
    B = x.shape[0]
    H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])
    hp, wp = H // p, W // p
    n = hp * wp
    planes = normalize(torch.cat([m.features(x[c:c + chunk]) for c in range(0, B, chunk)]))
    graph, degree = nc_graph(planes, float(np.float32(tau)))
    out = nc_iterate(graph, degree, ncut_start(n, seed).cuda().expand(B, n).contiguous(), iters, eps=eps)
    two = torch.stack((torch.zeros_like(out["margin"]), out["margin"]), dim=2).contiguous()
    OH, OW = size
    labels = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(two.data_ptr(), B, hp, wp, 2, OH, OW, labels.data_ptr(), None, S()))
    return NcutResult(labels, out["fg"], out["eigvec"], out["seed_cell"], out["rho"], degree, graph.view(torch.uint64))


def same(res, want):
    return all(torch.equal(bits_of(g), bits_of(w)) for g, w in zip(res, want) if g is not None)


@pytest.mark.parametrize("tag,tau,iters", [("tiny", 0.2, 8), ("tiny", 0.0, 0), ("vits8", 0.2, 16)])
def test_ncut_is_the_operators_by_hand(cuda, tag, tau, iters):
    m = model(tag)
    x = frames_of(tag, 3, seed=700 + iters)
    B, H, W = x.shape[:3]
    n = (H // 8) * (W // 8)
    want = by_hand(m, x, tau, 1e-4, iters, 9, 32, (H, W))
    res = m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9, want_graph=True)
    assert res.labels.dtype == torch.int32 and res.labels.shape == (B, H, W) and res.fg.shape == (B, n) and res.fg.dtype == torch.uint8
    assert res.eigvec.shape == (B, n) and res.seed_cell.shape == (B,) and res.rho.shape == (B, iters) and res.degree.shape == (B, n)
    assert res.graph.dtype == torch.uint64 and res.graph.shape == (B, n, NC.words_of(n))
    assert int(res.labels.min()) >= 0 and int(res.labels.max()) <= 1
    assert same(res, want)
    plain = m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9)
    assert plain.graph is None and same(plain, want[:6])
    # chunk = 1 is chunk = 32; a two-frame batch is the two single-frame calls: frames are independent
    assert same(m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9, chunk=1), by_hand(m, x, tau, 1e-4, iters, 9, 1, (H, W))[:6])
    if torch.equal(m.features(x[:1]), m.features(x)[:1]):               # (as far as features() itself is independent of the batch)
        assert same(m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9, chunk=1), want[:6])
        pair, singles = m.ncut(x[:2], tau=tau, iters=iters), [m.ncut(x[k:k + 1], tau=tau, iters=iters) for k in range(2)]
        for f in range(6):
            assert torch.equal(bits_of(pair[f]), bits_of(torch.cat([s[f] for s in singles]))), NcutResult._fields[f]
    # another output size; fp32 frames take the same path as uint8 frames
    size = (H + 3, W - 5)
    sized = m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9, size=size)
    assert sized.labels.shape == (B, *size) and torch.equal(sized.labels, by_hand(m, x, tau, 1e-4, iters, 9, 32, size).labels)
    grid = m.ncut(x, tau=tau, eps=1e-4, iters=iters, seed=9, size=(H // 8, W // 8))
    assert torch.equal(grid.labels.view(B, n), res.fg.to(torch.int32))
    from oracle import dinoseg_oracle as O
    x32 = O.preprocess(x.cpu().numpy()).cuda()
    assert same(m.ncut(x32, tau=tau, eps=1e-4, iters=iters, seed=9, want_graph=True), by_hand(m, x32, tau, 1e-4, iters, 9, 32, (H, W)))


def test_two_frames_are_two_single_frame_graphs(cuda):
    """frames are independent at the operators: a two-frame launch is the two one-frame launches"""
    p = (5, "normal", 0.2)
    B, hp, wp, D = CASES[p[0]]
    n = hp * wp
    planes = device_points(p[0], p[1])[0]
    graph, degree, _, _ = device_graph(p)
    both = nc_iterate(graph, degree, start_for(B, n), 5)
    for b in range(B):
        g1, d1 = nc_graph(planes[b:b + 1].contiguous(), 0.2)
        assert torch.equal(g1, graph[b:b + 1]) and torch.equal(d1, degree[b:b + 1])
        one = nc_iterate(g1, d1, start_for(1, n), 5)
        for k, v in one.items():
            assert torch.equal(bits_of(v), bits_of(both[k][b:b + 1])), k


def test_a_grid_above_the_cell_limit_raises_before_any_device_use(cuda):
    m = model("tiny")
    cells = capi.lib().dinoseg_ncut_max_cells()
    assert cells >= 4800
    big = torch.zeros((1, 8 * 101, 8 * 101, 3), dtype=torch.uint8)      # 10 201 cells, a host tensor: nothing is copied
    assert 101 * 101 > cells
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="cells"):
        m.ncut(big)
    assert torch.cuda.memory_allocated() == before
