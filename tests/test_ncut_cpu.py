"""Normalized cut on the 1-bit patch graph without a device: the host restatement (tests/ncut_util.py) against the plain matrix form in
fp64, convergence to eigvalsh's second eigenvalue and the planted partition, the packing of the graph, the seeded start vector, the
plan layer's refusals, and the library's host-only entries."""
import math

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, NcutResult, capi, ncut_start
from dino_amd.dense_plan import NCUT_MAX_CELLS, ncut_plan
from tests import ncut_util as NC


def planted_graph(seed, n, D, tau=0.2):
    """(bits fp64 [n, n], cnt int64 [n], small bool [n]) of one planted frame, from the fp64 unit rows"""
    tok, small = NC.planted_tokens(seed, 1, n, D)
    X = NC.unit_rows(tok[0, 1:])
    bits = NC.scores_host(X) > np.float32(tau)
    return bits.astype(np.float64), bits.sum(1).astype(np.int64), small[0]


@pytest.mark.parametrize("n,D,iters,eps", [(35, 64, 5, 1e-5), (64, 64, 3, 1e-5), (65, 192, 4, 0.0), (150, 64, 6, 1e-3), (1, 64, 2, 1e-5), (12, 64, 0, 1e-5)])
def test_host_rule_is_the_plain_matrix_form(n, D, iters, eps):
    rng = np.random.default_rng(3 + n)
    X = NC.unit_rows(rng.standard_normal((n, D)))
    bits = NC.scores_host(X) > np.float32(0.05)
    bits_f, cnt = bits.astype(np.float64), bits.sum(1)
    assert np.array_equal(bits, bits.T)
    _, r, u = NC.weights(cnt, n, eps)
    start = ncut_start(n, 5).numpy()
    z, rho = NC.iterate_host(bits_f, r, u, eps, start, iters)
    z2, rho2, _ = NC.matrix_form(bits_f, r, u, eps, start, iters)
    assert rho.shape == (iters,) and z.shape == (n,)
    assert np.abs(z - z2).max() <= 1e-12
    assert iters == 0 or np.abs(rho - rho2).max() <= 1e-12
    if n > 1:
        assert abs(np.linalg.norm(z) - 1.0) <= 1e-12 and abs(u @ z) <= 1e-6           # (u holds fp32 values: ||u||^2 = 1 up to that)
    else:
        assert not z.any() and not rho.any()                            # a one-cell grid: nothing is left after the deflation
    res, res2 = NC.result_host(z, r), NC.result_host(z2, r)
    assert res["seed"] == res2["seed"] and res["sigma"] == res2["sigma"] and np.array_equal(res["fg"], res2["fg"])
    assert res["eigvec"][res["seed"]] >= 0.0 and (n == 1 or res["fg"][res["seed"]])


def test_a_complete_graph_has_nothing_left_after_the_deflation():
    n, eps = 20, 1e-5
    bits_f = np.ones((n, n))
    _, r, u = NC.weights(np.full(n, n), n, eps)
    o = NC.one_pass(bits_f, r, u, eps, ncut_start(n, 0).numpy())
    # M = u u^T up to the fp32 roundings that r and u hold (2^-24 each): the deflated space sees eigenvalue 0, the lazy step halves z
    assert abs(o["rho"]) <= 1e-6
    assert np.abs(o["p"] - 0.5 * o["z0"]).max() <= 1e-6
    assert NC.dn(u * 3.0, u)[2] <= 1e-6                                 # u itself is what the deflation removes (u holds fp32 values)
    assert not NC.dn(np.zeros(n), u)[0].any()                           # ||q|| = 0 -> z' = 0


@pytest.mark.parametrize("n,D", [(35, 64), (99, 192), (480, 384), (1200, 64)])
def test_planted_inputs_reach_the_second_eigenvalue_and_the_smaller_group(n, D):
    eps = 1e-5
    bits_f, cnt, small = planted_graph(40 + n, n, D)
    _, r, u = NC.weights(cnt, n, eps)
    z, rho = NC.iterate_host(bits_f, r, u, eps, ncut_start(n, 0).numpy(), 32)
    M = NC.matrix_form(bits_f, r, u, eps, np.ones(n), 0)[2]
    lam = np.linalg.eigvalsh(M)
    assert abs(lam[-1] - 1.0) <= 1e-6                                   # (u holds fp32 values: the top eigenvalue is 1 up to that)
    assert lam[-2] > 0.99 and lam[-3] < 0.6                             # the gap of a planted pair
    assert abs(rho[-1] - lam[-2]) <= 1e-9
    assert np.all(np.diff(rho) >= -1e-12)                               # the Rayleigh record of a power iteration on a PSD matrix rises
    res = NC.result_host(z, r)
    assert np.array_equal(res["fg"], small) and small[res["seed"]]
    assert 0 < small.sum() < n - small.sum()


def test_pack_and_unpack_are_inverse_and_pad_bits_are_zero():
    rng = np.random.default_rng(9)
    for n in (1, 3, 63, 64, 65, 130):
        bits = rng.random((n, n)) < 0.4
        words = NC.pack_bits(bits)
        assert words.dtype == np.dtype("<u8") and words.shape == (n, NC.words_of(n))
        back, pad = NC.unpack_words(words, n)
        assert np.array_equal(back, bits) and not pad.any()
        for i, j in ((0, 0), (n - 1, n - 1), (0, n - 1)):
            assert bool((int(words[i, j // 64]) >> (j % 64)) & 1) == bool(bits[i, j])
        assert np.array_equal([bin(int(w)).count("1") for w in words.reshape(-1)], np.unpackbits(
            words.view(np.uint8).reshape(-1, 8), axis=1).sum(1))


def test_the_start_vector_is_reproducible():
    for n, seed in ((1, 0), (35, 3), (4800, 1 << 40), (7, -5)):
        z = ncut_start(n, seed)
        assert z.dtype == torch.float32 and z.shape == (n,) and z.device.type == "cpu"
        assert torch.equal(z, ncut_start(n, seed))
        assert torch.equal(z, torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32))
    assert not torch.equal(ncut_start(4800, 3), ncut_start(4800, 4))
    for n in (0, -3):
        with pytest.raises(ValueError):
            ncut_start(n, 0)


def test_plan_refusals_need_no_device():
    p = 8
    x = torch.zeros((3, 40, 56, 3), dtype=torch.uint8)
    ok = ncut_plan(p, x)
    assert (ok.B, ok.hp, ok.wp, ok.eps, ok.iters, ok.seed, ok.OH, ok.OW, ok.chunk) == (3, 5, 7, 1e-5, 64, 0, 40, 56, 32)
    assert ok.tau == float(np.float32(0.2))                             # rounded once to fp32, on the host
    f32 = ncut_plan(p, x.permute(0, 3, 1, 2).float(), tau=0.0, eps=0.0, iters=0, size=(5, 7))
    assert (f32.kind, f32.tau, f32.eps, f32.iters, f32.OH, f32.OW) == (capi.INPUT_F32_CHW, 0.0, 0.0, 0, 5, 7)
    assert ncut_plan(p, x, iters=4096).iters == 4096 and ncut_plan(p, x, tau=-0.999).tau < 0
    assert ncut_plan(16, torch.zeros((1, 64, 96, 3), dtype=torch.uint8)).wp == 6
    assert ncut_plan(p, torch.zeros((1, 8 * 80, 8 * 127, 3), dtype=torch.uint8)).hp * 127 == 10160      # the largest grid
    big = torch.zeros((1, 8 * 101, 8 * 101, 3), dtype=torch.uint8)      # 10 201 cells
    bad = [
        dict(x=torch.zeros((3, 40, 56), dtype=torch.uint8)),                            # layout
        dict(x=torch.zeros((3, 41, 56, 3), dtype=torch.uint8)),                         # not a patch multiple
        dict(x=torch.zeros((0, 40, 56, 3), dtype=torch.uint8)),                         # no frame
        dict(x=np.zeros((3, 40, 56, 3), dtype=np.uint8)),                               # not a tensor
        dict(tau=1.0), dict(tau=-1.0), dict(tau=1.5), dict(tau=math.nan), dict(tau=math.inf), dict(tau="0.2"), dict(tau=None),
        dict(eps=-1e-9), dict(eps=1.0), dict(eps=math.nan), dict(eps=None),
        dict(iters=-1), dict(iters=4097), dict(iters=1.5), dict(iters=True),
        dict(seed=0.5),
        dict(size=(4, 56)), dict(size=(40, 6)), dict(size=40),
        dict(chunk=0), dict(chunk=1.5),
        dict(x=big),                                                                    # above dinoseg_ncut_max_cells()
    ]
    for kw in bad:
        args = dict(x=x)
        args.update(kw)
        with pytest.raises(ValueError):
            ncut_plan(p, **args)
    # the model's call refuses the same things before it asks for a GPU; a valid call on a CPU model reaches "no CPU path"
    m = DINOSeg(head="linear", n_blocks=1)
    for kw in (dict(tau=1.0), dict(eps=1.0), dict(iters=-1), dict(iters=4097), dict(n_blocks=2), dict(size=(4, 56)), dict(chunk=0),
               dict(x=big)):
        args = dict(x=x)
        args.update(kw)
        with pytest.raises(ValueError):
            m.ncut(**args)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.ncut(x)


def test_symbols_and_host_entries():
    lib = capi.lib()
    names = ("dinoseg_op_ncut_graph", "dinoseg_op_ncut_iterate", "dinoseg_ncut_graph_bytes", "dinoseg_ncut_max_cells")
    declared = capi.header_symbols()
    for name in names:
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name)
    for name in ("NcutResult", "ncut_start"):
        assert name in dino_amd.__all__ and hasattr(dino_amd, name)
    assert NcutResult._fields == ("labels", "fg", "eigvec", "seed_cell", "rho", "degree", "graph")
    assert callable(DINOSeg.ncut)
    cells = lib.dinoseg_ncut_max_cells()
    assert cells == NCUT_MAX_CELLS and cells >= 4800                    # the 480 x 640 camera fits
    assert 16 * cells <= 160 * 1024 < 16 * (cells + 128)                # four fp32 vectors beside under 2 KiB of fixed use
    assert cells < 14400                                                # 960 x 960 at patch 8 does not fit (the README says so)
    f = lib.dinoseg_ncut_graph_bytes
    assert f(1, 3600) == 3600 * 57 * 8 and f(1, 3600) < 1.7e6           # n^2 bits: 1.6 MB at 60 x 60 cells
    assert f(32, 4800) == 32 * 4800 * 75 * 8
    assert f(1, 1) == 8 and f(2, 64) == 2 * 64 * 8 and f(1, 65) == 65 * 16 and f(1, cells) == cells * NC.words_of(cells) * 8
    for bad in ((0, 80), (1, 0), (1, -1), (-1, 80), (1, cells + 1), (1 << 30, 4800)):
        assert f(*bad) == -1
