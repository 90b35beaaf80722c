"""What tests/attention_bwd_probe_util.py claims about its own probes, checked without a GPU: the construction on the values, the
expectations against an fp64 restatement (torch autograd where lse and O are the forward's, the five formulas elsewhere), the order
independence under an fp32 emulation of the three launches, and -- the point of the exercise -- that the expected bits notice every listed
way in which the kernels could be subtly wrong (mutants of that emulation, on pad rows filled with a real key, large V and query 0)."""
import math

import numpy as np
import pytest
import torch

from tests import attention_probe_util as P
from tests import attention_bwd_probe_util as U

_cache = {}
PARAMS = [pytest.param(planes, *shp, id=f"{planes}pl-{shp[0]}x{shp[1]}x{shp[2]}") for planes in (1, 2) for shp in U.SHAPES]


def _cases(planes, shp):
    """the cases of case_list (numbered over all the shapes) at one shape, built once"""
    out = []
    for probe, s, kw in U.case_list(U.SHAPES, planes):
        if s == shp:
            key = (probe, s, tuple(sorted(kw.items())))
            if key not in _cache:
                _cache[key] = U.build(probe, *s, **kw)
            out.append((f"{probe} {s} {kw}", _cache[key]))
    return out


@pytest.mark.parametrize("planes,B,H,ntok", PARAMS)
def test_builder_claims(planes, B, H, ntok):
    """(1) On the values: operands exact in their planes, V small nonzero integers, dO one or two nonzero integers per (frame, head, query)
    on dimensions that move with all three indices, the pad rows as stated, and on hi + lo planes a lo plane that is needed in some operand
    of each of the five products.  (Integer scores, power-of-two P, dS within the planes and the 24-bit sums are asserted by the builder on
    every case it builds, here and in the GPU test.)"""
    lo_seen = set()
    for what, c in _cases(planes, (B, H, ntok)):
        ops = U.operand_planes(c)                                            # asserts exactness in the planes
        assert ops["lse"].astype(np.float64).tolist() == c.lse.tolist(), what
        V = c.V[:, :, :ntok]
        assert (V != 0).all() and (V == np.round(V)).all() and np.abs(V).max() <= 15, what
        dO = c.dO.reshape(B, ntok, H, 64)
        nzd = (dO != 0).sum(axis=-1)
        zero_rows_allowed = c.probe == "groups"
        assert (nzd <= 2).all() and ((nzd >= 1) | zero_rows_allowed).all() and (dO == np.round(dO)).all(), what
        first = np.where(nzd > 0, (dO != 0).argmax(axis=-1), -1)
        for axis, n in ((0, B), (1, ntok), (2, H)):
            if n > 1 and c.probe != "groups":
                a, b = np.take(first, 0, axis=axis), np.take(first, 1, axis=axis)
                assert (a != b).any(), f"{what}: dO's dimensions do not move with index {axis}"
        # pad rows: a real key that some query weights, large V, query 0
        if c.npad > ntok:
            assert (c.Q[:, :, ntok:] == c.Q[:, :, :1]).all() and (np.abs(c.V[:, :, ntok:]) >= 96 * 256).all(), what
            for b in range(B):
                for h in range(H):
                    same = (c.K[b, h, :ntok] == c.K[b, h, ntok]).all(axis=1)
                    S = c.Q[b, h, :ntok] @ c.K[b, h, ntok]
                    assert same.any() and (c.K[b, h, ntok:] == c.K[b, h, ntok]).all(), what
                    assert c.probe == "count" or (S - c.lse[b, h] > -P.ZERO_FROM).any(), f"{what}: no query weights the pad key"
        if planes == 2:
            lo = {k: (ops[k][1] != 0).any() for k in ("q", "k", "v", "dO", "O")}
            assert not lo["v"] and not (lo["q"] and lo["k"]), what
            nonzero_ds = bool((c.sums["dq"] != 0).any())
            lo_seen |= {("scores", lo["q"] or lo["k"]), ("dP", lo["dO"]), ("dV", lo["dO"]), ("delta", lo["O"] and c.probe not in ("selector", "groups")),
                        ("dQ", c.meta["any_lo_ds"] or (lo["k"] and nonzero_ds)), ("dK", c.meta["any_lo_ds"] or (lo["q"] and nonzero_ds)),
                        ("dQ by K lo", lo["k"] and nonzero_ds), ("dK by Q lo", lo["q"] and nonzero_ds), ("dS lo", c.meta["any_lo_ds"])}
    if planes == 2:
        # (as in the forward util, the per-key lo bit of K is zero for the first keys: one token has none)
        wanted = ("scores", "dP", "dV", "delta", "dQ", "dK", "dK by Q lo", "dS lo") + (("dQ by K lo",) if ntok >= 8 else ())
        missing = [k for k in wanted if (k, True) not in lo_seen]
        assert not missing, f"no case at {(B, H, ntok)} needs a lo plane for {missing}"


def test_cases_use_every_dimension():
    for planes in (1, 2):
        for shapes in (U.SHAPES, U.SHAPES + [U.PRODUCTION]):
            used = set()
            for _, _, kw in U.case_list(shapes, planes):
                used.update(int(d) for d in P.case_dims(kw["n"]))
            assert used == set(range(64))


def _restate(c, autograd):
    """fp64 sums (before 0.125 / ln 2) of dQ, dK, dV as [B, ntok, H, 64] and the magnitudes sum |P| (|dP| + |delta|) |K| ... that scale the
    comparison.  autograd: gradients of softmax(q k^T / 8) v, q = Q~ / (0.125 log2 e), from dO alone (lse and O are not used) -- taken
    with respect to Q~ through the exact fp64 scores and converted by the chain rule.  Otherwise the five formulas on the six operands,
    with the kernels' rounding of dS to the planes where the case asks for it."""
    B, H, ntok = c.B, c.H, c.ntok
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    q, k, v = (t(x[:, :, :ntok]) for x in (c.Q, c.K, c.V))
    dO = t(c.dO).reshape(B, ntok, H, 64).transpose(1, 2)
    O = t(c.O).reshape(B, ntok, H, 64).transpose(1, 2)
    lse = t(c.lse)
    if autograd:
        q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
        ctx = torch.softmax((q @ k.transpose(-1, -2)) * math.log(2.0), dim=-1) @ v
        ctx.backward(dO)
        # d/dq = d/dQ~ * 0.125 log2 e and the kernel's dQ = 0.125 * sum:  sum = d/dQ~ * log2 e;  dK = ln 2 * sum:  sum = d/dK * log2 e
        log2e = 1.0 / math.log(2.0)
        got = (q.grad * log2e, k.grad * log2e, v.grad)
        q, k, v = q.detach(), k.detach(), v.detach()
    Pm = torch.exp2(q @ k.transpose(-1, -2) - lse[..., None]).float().double()        # an fp32 value: 2^-240 and below is 0
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    if not autograd:
        dS = Pm * (dP - delta)
        if c.meta["rounded"]:
            dS = t(U.round_to_planes(dS.numpy(), c.planes))
        got = (dS @ k, dS.transpose(-1, -2) @ q, Pm.transpose(-1, -2) @ dO)
    w = Pm * (dP.abs() + delta.abs())
    mag = (w @ k.abs(), w.transpose(-1, -2) @ q.abs(), Pm.transpose(-1, -2) @ dO.abs())
    back = lambda x: x.transpose(1, 2).numpy()
    return [back(x) for x in got], [back(x) for x in mag]


@pytest.mark.parametrize("planes,B,H,ntok", PARAMS)
def test_expectations_match_fp64(planes, B, H, ntok):
    """(2) The exact sums equal an fp64 restatement to 1e-12 of sum |P| (|dP| + |delta|) |operand| per element (plus 2^-150, half the smallest
    fp32 subnormal: autograd's softmax leaves 2^-256 where the probes have an exact 0)."""
    worst = 0.0
    for what, c in _cases(planes, (B, H, ntok)):
        got, mag = _restate(c, autograd=c.probe in ("selector", "groups"))
        for name, g, m in zip(("dq", "dk", "dv"), got, mag):
            err = np.abs(c.sums[name] - g)
            bound = 1e-12 * m + 2.0 ** -150
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"{what}: {name} differs from fp64 by {float((err / bound).max()):.3g} of the bound"
    print(f"attention_bwd probes {planes} plane(s) {B}x{H}x{ntok}: worst |expectation - fp64| / bound {worst:.3g}")


@pytest.mark.parametrize("planes,B,H,ntok", PARAMS)
def test_emulation_is_bit_equal_in_both_tile_orders(planes, B, H, ntok):
    """(3) The three launches in fp32 numpy, tile by tile, give the expected planes bit for bit with the tiles in natural and in reversed
    order: the expectation is a property of the inputs, not of an accumulation order."""
    n = 0
    for what, c in _cases(planes, (B, H, ntok)):
        for order in ("natural", "reversed"):
            e = U.emulate(c, order)
            assert np.array_equal(e, c.expect), f"{what} {order}: {int((e != c.expect).sum())} elements differ"
            assert not U.mismatches(c, e)[0].any(), f"{what} {order}: the emulation misses the condition the GPU test applies"
            n += e.size
    print(f"attention_bwd probes {planes} plane(s) {B}x{H}x{ntok}: {n} elements compared")


@pytest.mark.parametrize("planes,B,H,ntok", PARAMS)
def test_every_mutant_changes_an_expected_bit(planes, B, H, ntok):
    """(4) Each mutant of the emulation -- key mask off by one either way, a pad query with -lse = 0, the dO row clamp dropped, a key tile
    (dQ) or a query tile (dK, dV) skipped or run twice, dS truncated, the lo plane of dS dropped, two heads' columns swapped, delta
    omitted, 0.125 and ln 2 exchanged -- changes a bit of some probe's output at this shape (for dK on hi + lo planes: leaves its bound).  A condition, not a measurement.  (The lo
    plane of P is identically zero on these probes, P being a power of two: dropping it is not a mutant these inputs can see, and the
    builder asserts that it is zero.)"""
    cases = _cases(planes, (B, H, ntok))
    order = {"pick": 0, "weights": 1, "groups": 2, "count": 3, "selector": 4}
    cases = sorted(cases, key=lambda wc: (order[wc[1].probe], not wc[1].meta["rounded"]))
    killed = {}
    for mut in U.MUTANTS:
        if not U.mutant_applies(mut, B, H, ntok, planes):
            continue
        for what, c in cases:
            if U.mismatches(c, U.emulate(c, "natural", mut))[0].any():             # the condition of the GPU test: dK on two planes by its bound
                killed[mut] = what
                break
        assert mut in killed, f"mutant {mut} survives every probe at {(B, H, ntok)} on {planes} plane(s)"
    assert {"mask+1", "mask-1", "padq", "noclamp", "trunc", "no_delta", "scales"} <= set(killed)
    print(f"attention_bwd probes {planes} plane(s) {B}x{H}x{ntok}: {len(killed)} mutants caught")
