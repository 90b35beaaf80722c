"""What tests/attention_probe_util.py claims about its own probes, checked without a GPU: the generators' construction, the order
independence of the expectations under an fp32 emulation of both softmax bookkeepings, and the store bound against brute force."""
from fractions import Fraction

import numpy as np
import pytest

from tests import attention_probe_util as P

SHAPES = [(1, 1, 1), (1, 1, 33), (1, 3, 65), (2, 2, 197), (1, 1, 257), (2, 5, 300)]
LONG = (1, 1, 2051)
_cache = {}


def _case(probe, shp, kw, v_fp16=False):
    key = (probe, shp, tuple(sorted(kw.items())), v_fp16)
    if key not in _cache:
        _cache[key] = P.build(probe, *shp, v_fp16=v_fp16, **kw)
    return _cache[key]


@pytest.mark.parametrize("planes,v_fp16", [(1, False), (2, False), (2, True)])
def test_generator_claims(planes, v_fp16):
    cases = P.case_list(SHAPES + [LONG], planes)
    used = set()
    sizes = set()
    best_tiles = set()
    for probe, shp, kw, _ in cases:
        c = _case(probe, shp, kw, v_fp16)
        B, H, ntok = shp
        what = f"{probe} {shp} {kw}"
        used.update(int(d) for d in c.dims)
        nz = np.flatnonzero(np.abs(c.K[:, :, :ntok]).sum(axis=(0, 1, 2)) + np.abs(c.Q[:, :, :ntok]).sum(axis=(0, 1, 2)))
        assert set(nz) <= set(int(d) for d in c.dims), what
        pi, nsel, hit = c.meta["pi"], c.meta["nsel"], c.meta["hit"]
        assert (np.sort(pi, axis=-1) == np.arange(ntok)).all(), f"{what}: pi is not a permutation"
        assert (hit >= 1).all(), f"{what}: a key lies in no query's set"
        V = c.V[:, :, :ntok]
        assert (V != 0).all() and (V == np.round(V)).all(), what
        ctx = c.ctx.reshape(B, ntok, H, 64)
        if probe == "selector":
            assert (nsel == 1).all() and c.pow2.all(), what
            for b in range(B):
                for h in range(H):
                    assert (ctx[b, :, h] == V[b, h, pi[b, h]]).all(), what
            if kw.get("lo") is None:
                assert (c.lse == 0).all(), what
        elif probe == "groups":
            assert ((nsel >= 1) & (nsel <= 4)).all(), what
            sizes.update(int(x) for x in np.unique(nsel))
            assert (c.pow2.reshape(B, ntok, H).transpose(0, 2, 1) == (nsel != 3)).all(), what
            assert (c.den.reshape(B, ntok, H).transpose(0, 2, 1) == nsel * 2 ** P.HMAX).all(), what
        elif probe == "weights":
            ns = len(P.soft_bits(ntok))
            assert (nsel <= 2 ** ns).all() and (c.log2l <= ns * np.log2(1.5) + 1 + 1e-9).all(), what
            if ntok >= 193:
                S = c.Q[0, 0, :ntok] @ c.K[0, 0, :ntok].T
                best = S.argmax(axis=1) // 64
                first_near = (S >= S.max(axis=1, keepdims=True) - P.HMAX).argmax(axis=1) // 64
                late = best[first_near < best]                  # a farther key came in an earlier tile: the reference has to rise
                nt = (ntok + 63) // 64
                best_tiles.update("last" if t == nt - 1 else "middle" for t in late)
                best_tiles.update("first" for t in best if t == 0)
        else:
            assert (c.Q == 0).all() and (nsel == ntok).all() and (c.den == ntok * 2 ** P.HMAX).all(), what
            assert np.allclose(c.lse, np.log2(ntok), rtol=0, atol=1e-12), what
        # operands: exact in one bf16 plane and one fp16 plane, or in two planes with a lo plane that is used and never meets another
        if planes == 1:
            for x in (c.Q, c.K):
                P.exact_planes(x, False, 1), P.exact_planes(x, True, 1)
            P.exact_planes(c.V, False, 1)
        else:
            for fp16 in (False, True):
                lo_q = P.exact_planes(c.Q, fp16, 2)[1] != 0
                lo_k = P.exact_planes(c.K, fp16, 2)[1] != 0
                assert not (lo_q.any(axis=(0, 1, 2)) & lo_k.any(axis=(0, 1, 2))).any(), f"{what}: a lo x lo product"
                if kw.get("lo") == "k":
                    assert (ntok < 8 or lo_k[:, :, :ntok, c.sh_col].any()) and not lo_q.any(), what
                if kw.get("lo") == "q":
                    assert lo_q[:, :, :ntok, c.sh_col].all() and not lo_k.any(), what
            lo_v = P.exact_planes(c.V, v_fp16, 2)[1] != 0
            assert lo_v[:, :, :ntok].all(), what
            assert (P.exact_planes(c.V, v_fp16, 2)[0] != 0).all()
        for sh in P.SHIFTS:                                   # the shifted K stays exact too, and the one-row shift adds no lo plane
            if kw.get("lo") != "q" and probe in ("selector", "weights"):
                _, K, _ = P.shifted(c, sh)
                Q1, K1, _ = P.shifted(c, sh, ntok - 1)
                for fp16 in (False, True):
                    P.exact_planes(K, fp16, planes)
                    if sh in (200, -200, 61, -61):
                        q1, k1 = P.exact_planes(Q1, fp16, planes), P.exact_planes(K1, fp16, planes)
                        assert planes == 1 or not ((q1[1] != 0).any(axis=(0, 1, 2)) & (k1[1] != 0).any(axis=(0, 1, 2))).any(), what
        rows = np.random.default_rng(1).integers(0, B * ntok, 8)           # the fp64 expectations against Fractions
        for r in rows:
            col = int(r * 7 % (H * 64))
            f = P.fraction_ctx(c, int(r), col)
            if c.pow2[r, col // 64]:
                assert Fraction(float(c.ctx[r, col])) == f, what
            else:
                assert abs(Fraction(float(c.ctx[r, col])) - f) <= abs(f) * Fraction(1, 2 ** 52), what
    assert used == set(range(64)), "a head dimension carries no code or offset in any case"
    assert {1, 2, 3, 4} <= sizes
    assert best_tiles == {"first", "middle", "last"}, best_tiles


def test_every_route_uses_every_dimension():
    """a route's cases are case_list over its shapes: the smallest set (the six common shapes) already covers the 64 dimensions"""
    for planes in (1, 2):
        for shapes in (SHAPES, SHAPES + [LONG], SHAPES + [(1, 6, 3601)]):
            used = set()
            for _, _, kw, _ in P.case_list(shapes, planes):
                used.update(int(d) for d in P.case_dims(kw["n"]))
            assert used == set(range(64))


EMU_SHAPES = [(1, 1, 33), (1, 3, 65), (2, 2, 197), (2, 5, 300)]


@pytest.mark.parametrize("planes", [1, 2])
def test_expectations_do_not_depend_on_order(planes):
    """Both bookkeepings in fp32, tile by tile, in natural and reversed order and split over two and three groups: before the final divide
    O and l are, bit for bit, the exact integers times one power of two per row -- whatever the order, the split, the rescale history or
    the shift.  So the expectation is a property of the inputs, and either bookkeeping alone meets the bit-equality condition."""
    for probe, shp, kw, shift_too in P.case_list(EMU_SHAPES, planes):
        c = _case(probe, shp, kw)
        ntok = c.ntok
        b, h = c.B - 1, c.H - 1
        rows = slice(b * ntok, (b + 1) * ntok)
        num, den = c.num[rows, h * 64:(h + 1) * 64].astype(np.float64), c.den[rows, h].astype(np.float64)
        runs = [(0, None)] + ([(s, None) for s in (P.SHIFTS[1:] if kw.get("lo") is None else (60, -61, 200))] +
                              [(200, ntok // 2), (-61, ntok - 1), (-200, 0)] if shift_too else [])
        for shift, one_row in runs:
            Q, K, lse = P.shifted(c, shift, one_row)
            q, k, v = Q[b, h, :ntok], K[b, h], c.V[b, h]
            mrow = np.round(lse[b, h] - c.log2l[b, h])                          # the row's best score
            for emu in (P.emulate_zero_reference, P.emulate_running_reference):
                for order, groups in (("natural", 1), ("reversed", 1), ("natural", 2), ("natural", 3), ("reversed", 3)):
                    o, l, m = emu(q, k, v, ntok, order, groups)
                    what = f"{probe} {shp} {kw} shift {shift} row {one_row} {emu.__name__} {order} {groups}"
                    assert o.dtype == np.float32 and l.dtype == np.float32, what
                    sc = np.ldexp(1.0, (mrow - m.astype(np.float64)).astype(np.int64) - P.HMAX)
                    assert (o.astype(np.float64) == num * sc[:, None]).all(), what
                    assert (l.astype(np.float64) == den * sc).all(), what


@pytest.mark.parametrize("fp16,planes", [(False, 1), (True, 1), (False, 2), (True, 2)])
def test_store_bound_against_brute_force(fp16, planes):
    """10^5 fp32 values, correctly rounded to the store format: the error stays within half_ulp_store and reaches 0.9 of it"""
    g = np.random.default_rng(5 + 2 * planes + fp16)
    x = (np.exp2(g.uniform(-6.0, 6.0, 100000)) * np.where(g.integers(0, 2, 100000) == 0, 1.0, -1.0)).astype(np.float32).astype(np.float64)
    got = P.planes_value(P.rne_planes(x, fp16, planes), fp16)
    ratio = np.abs(got - x) / P.half_ulp_store(x, fp16, planes)
    assert ratio.max() <= 1.0 and ratio.max() >= 0.9, ratio.max()
    assert (P.ctx_bound(x, fp16, planes) <= (2.0 ** -(8, 11, 16, 22)[2 * (planes - 1) + fp16] + 4 * 2.0 ** -24) * np.abs(x) + 2.0 ** -25).all()


def test_lse_bound_sees_one_key():
    """one key more or less in a row of 3601 is hundreds of times the lse bound, on either kind of kernel"""
    lse = np.log2(3601.0)
    for trail in (0, 16):
        assert (np.log2(3601.0) - np.log2(3600.0)) > 50 * P.lse_bound(np.array(lse), np.array(lse), trail)
