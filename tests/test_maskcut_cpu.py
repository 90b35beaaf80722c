"""Multi-object discovery without a device: the restatement of the rule (tests/maskcut_util.py) against the plain matrix form of every
round, the integer properties of the mask, the select step against a flood fill, the planted expectation that the device tests rely on,
maskcut_plan's refusals, and the host-only queries of the library."""
import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, MaskCutResult, capi, ncut_start
from dino_amd.dense_plan import MASKCUT_MAX_OBJECTS, MaskCutPlan, maskcut_plan, ncut_plan
from tests import components_util as CU
from tests import maskcut_util as MC
from tests import ncut_util as NC

NAMES = ("dinoseg_maskcut_scratch_bytes", "dinoseg_op_ncut_mask", "dinoseg_op_maskcut_select", "dinoseg_op_maskcut")
EPS, TAU, ITERS = 1e-5, 0.2, 64
TOKEN_SEEDS, START_SEEDS = (1201, 1202), (0, 1)


def frame(hp, wp, B=1):
    return torch.zeros((B, 8 * hp, 8 * wp, 3), dtype=torch.uint8)


def start(n, seed):
    return ncut_start(n, seed).numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("hp,wp,D", [(1, 3, 64), (5, 7, 64), (5, 13, 64), (9, 11, 192)])
def test_every_round_of_the_restatement_is_the_plain_matrix_form(hp, wp, D):
    """Three rounds on a random graph and on a planted one: the cut of every round (through the packed words, graph &= alive and the
    popcount degree) against the dense W with the dead rows and columns set to eps, within the 1e-12 of the other host tests; the dead
    cells are isolated nodes, the degree is the row count, the graph stays symmetric and only ever loses bits."""
    n = hp * wp
    rects = next((r for h, w, _, r in MC.PLANTED if (h, w) == (hp, wp)), ((0, 0, 1, 1),))
    for tok in (NC.normal_tokens(1100 + n, 1, n, D)[0], MC.planted_rect_tokens(1150 + n, hp, wp, D, rects)):
        bits = MC.host_bits(tok, TAU)
        alive, z0, before = np.ones(n, dtype=bool), start(n, 3), bits
        for t in range(3):
            r = MC.round_host(bits, alive, hp, wp, EPS, z0, 12, 4)
            zm, rhom = MC.matrix_round(bits, alive, EPS, z0, 12)
            assert np.abs(r["z"] - zm).max() <= 1e-12 and np.abs(r["rho"] - rhom).max() <= 1e-12, t
            m = r["masked"]
            assert np.array_equal(m, bits & alive[:, None] & alive[None, :]) and np.array_equal(m, m.T)
            assert np.array_equal(r["degree"], m.sum(1)) and not (m & ~before).any()
            assert not r["cells"][~alive].any() and r["area"] == r["cells"].sum()
            assert np.array_equal(r["alive"], alive & ~r["cells"])
            before, alive = m, r["alive"]


def test_mask_properties_on_packed_words():
    """Masking twice is masking once; masking with a subset after a superset is masking the original with the subset; pad bits stay zero"""
    g = np.random.default_rng(7)
    for n in (1, 35, 64, 65, 130):
        bits = g.random((n, n)) < 0.4
        bits = bits | bits.T
        words = NC.pack_bits(bits)
        a1 = g.random(n) < 0.7
        a2 = a1 & (g.random(n) < 0.5)
        for alive in (np.ones(n, bool), np.zeros(n, bool), a1, np.arange(n) == n - 1, np.arange(n) != n // 2):
            w1, d1 = MC.mask_host(words, MC.pack_alive(alive))
            b1, pad = NC.unpack_words(w1, n)
            assert not pad.any() and np.array_equal(b1, bits & alive[:, None] & alive[None, :]) and np.array_equal(d1, b1.sum(1))
            w2, d2 = MC.mask_host(w1, MC.pack_alive(alive))
            assert np.array_equal(w2, w1) and np.array_equal(d2, d1)
        w12 = MC.mask_host(MC.mask_host(words, MC.pack_alive(a1))[0], MC.pack_alive(a2))
        w02 = MC.mask_host(words, MC.pack_alive(a2))
        assert np.array_equal(w12[0], w02[0]) and np.array_equal(w12[1], w02[1])


def test_select_against_a_flood_fill():
    g = np.random.default_rng(11)
    for hp, wp in ((1, 1), (5, 7), (9, 11)):
        n = hp * wp
        for trial in range(6):
            fg = (g.random(n) < 0.6).astype(np.uint8)
            alive = g.random(n) < 0.8
            cand = MC.candidates_host(fg, alive)
            ids = CU.components_frame(cand.reshape(hp, wp), 4, 0, 1)[0].reshape(-1)
            fill = CU.flood_fill(cand.reshape(hp, wp) - (cand.reshape(hp, wp) == 0), 4, -1)[0].reshape(-1)
            margin = g.standard_normal(n).astype(np.float32)
            for seed in range(n):
                s = MC.select_host(ids, fg, margin, seed, alive, hp, wp)
                want = (fill == fill[seed]) if cand[seed] else np.zeros(n, bool)
                assert s["found"] == int(cand[seed]) and np.array_equal(s["cells"], want)
                assert np.array_equal(s["score"].view(np.float32), np.where(want, margin, -np.abs(margin)))
                if s["found"]:
                    y, x = np.nonzero(want.reshape(hp, wp))
                    assert tuple(s["box"]) == (x.min(), y.min(), x.max() + 1, y.max() + 1) and s["area"] == want.sum()
                else:
                    assert not s["box"].any() and s["area"] == 0 and np.array_equal(s["alive"], alive)


# ------------------------------------------------------------------------------------------------ the planted expectation
@pytest.mark.parametrize("case", MC.PLANTED, ids=lambda c: f"{c[0]}x{c[1]}")
def test_planted_rectangles_are_found_one_per_round_then_nothing(case):
    """What the device test asserts on the planted grids, established here in fp64 (64 passes, tau 0.2, eps 1e-5, two token seeds, the
    start seeds 0 and 1): each of the first G rounds returns exactly one rectangle's cell set, the rounds' rectangles are distinct (in
    an order that may depend on the start seed, so the SET is compared), round G finds nothing with a dead seed and every later round
    repeats it; the labels at the grid's own size are the object map up to the rounds' order."""
    hp, wp, D, rects = case
    n, G = hp * wp, len(rects)
    sets, _ = MC.rect_cells(hp, wp, rects)
    for ts in TOKEN_SEEDS:
        bits = MC.host_bits(MC.planted_rect_tokens(ts, hp, wp, D, rects), TAU)
        for ss in START_SEEDS:
            rounds, count, grid = MC.maskcut_host(bits, hp, wp, EPS, start(n, ss), ITERS, G + 2)
            assert [r["found"] for r in rounds] == [1] * G + [0, 0], (ts, ss)
            assert count == G
            assert MC.found_sets([r["cells"] for r in rounds], [r["found"] for r in rounds]) == MC.rect_sets(hp, wp, rects)
            dead = ~rounds[G]["alive"]
            assert dead[rounds[G]["res"]["seed"]] and np.array_equal(dead, sets.any(0))
            assert np.array_equal(rounds[G + 1]["z"], rounds[G]["z"]) and np.array_equal(rounds[G + 1]["alive"], rounds[G]["alive"])
            for t in range(G):
                assert np.array_equal(grid == t + 1, rounds[t]["cells"])
            assert np.array_equal(grid == 0, ~sets.any(0))


# ------------------------------------------------------------------------------------------------ the plan and the host queries
def test_plan_is_built_on_ncut_plan_and_refuses_what_it_must():
    x = frame(5, 7, B=3)
    p = maskcut_plan(8, x)
    assert isinstance(p, MaskCutPlan) and p.ncut == ncut_plan(8, x, split=True) and (p.max_objects, p.connectivity) == (3, 4)
    p = maskcut_plan(8, x, 16, 0.1, 0.0, 5, 9, (80, 112), 2, 7, 8)
    assert p.ncut == ncut_plan(8, x, 0.1, 0.0, 5, 9, (80, 112), 2, 7) and (p.max_objects, p.connectivity) == (16, 8)
    assert maskcut_plan(8, x, np.int64(1), connectivity=np.int32(8)).max_objects == 1 and MASKCUT_MAX_OBJECTS == 16
    assert maskcut_plan(8, frame(101, 101)).ncut.hp == 101               # above the one-workgroup limit: the split launches take it
    for kw in (dict(max_objects=0), dict(max_objects=17), dict(max_objects=-1), dict(max_objects=2.0), dict(max_objects=True),
               dict(max_objects=None), dict(connectivity=6), dict(connectivity=True), dict(connectivity="4"), dict(connectivity=4.0),
               dict(split=False), dict(split=np.bool_(False)), dict(split=0), dict(split=-3), dict(split="yes"), dict(tau=1.0),
               dict(tau="a"), dict(eps=1.0), dict(eps=-1e-9), dict(iters=-1), dict(iters=4097), dict(seed=0.5), dict(size=(4, 56)),
               dict(size=3), dict(chunk=0), dict(x=frame(202, 202)), dict(x=torch.zeros((1, 41, 56, 3), dtype=torch.uint8)),
               dict(x=np.zeros((1, 40, 56, 3), np.uint8)), dict(x=torch.zeros((0, 40, 56, 3), dtype=torch.uint8))):
        args = dict(patch=8, x=x)
        args.update(kw)
        with pytest.raises(ValueError):
            maskcut_plan(**args)
    with pytest.raises(ValueError, match="split"):
        maskcut_plan(8, x, split=False)


def test_a_cpu_model_reaches_no_cpu_path_only_after_every_value_error():
    m = DINOSeg(head="linear", n_blocks=1)
    x = frame(5, 7, B=2)
    for kw in (dict(max_objects=0), dict(max_objects=17), dict(split=False), dict(connectivity=5), dict(n_blocks=2), dict(tau=-1.0),
               dict(x=frame(202, 202))):
        args = dict(x=x)
        args.update(kw)
        with pytest.raises(ValueError):
            m.discover_all(**args)
    with pytest.raises(capi.DinosegError, match="no CPU path"):
        m.discover_all(x)
    assert MaskCutResult._fields == ("labels", "count", "found", "box", "area", "cells", "seed_cell", "rho", "graph")


def test_symbols_are_declared_bound_and_exported():
    lib, declared = capi.lib(), capi.header_symbols()
    for name in NAMES:
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name), name
    assert len(capi.SIGNATURES["dinoseg_op_maskcut"][1]) == 24 and len(capi.SIGNATURES["dinoseg_op_maskcut_select"][1]) == 16


def test_scratch_query():
    lib = capi.lib()
    q = lib.dinoseg_maskcut_scratch_bytes

    def up(v):
        return (v + 15) // 16 * 16

    for B, hp, wp in ((1, 1, 1), (3, 5, 7), (1, 5, 13), (1, 60, 80), (32, 60, 80), (1, 120, 120)):
        n = hp * wp
        W = NC.words_of(n)
        want = sum(up(v) for v in (lib.dinoseg_ncut_split_scratch_bytes(B, n), lib.dinoseg_components_scratch_bytes(B, hp, wp), 36 * B,
                                   8 * B * W, 4 * B * n, 4 * B * n, 4 * B * n, B * n, 4 * B * n, 4 * B * n, 4 * B, 4 * B * 4096))
        for K in (1, 3, 16):
            assert q(B, hp, wp, K) == want, (B, hp, wp, K)              # (it does not grow with K)
    for bad in ((0, 5, 7, 3), (1, 0, 7, 3), (1, 5, 0, 3), (-1, 5, 7, 3), (1, 5, 7, 0), (1, 5, 7, 17), (1, 5, 7, -1), (1, 202, 202, 3),
                (1, 8193, 1, 3), (1, 1, 8193, 3), (1 << 30, 60, 80, 3)):
        assert q(*bad) == -1, bad
