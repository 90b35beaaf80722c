"""Exact per-element probes of the attention forward kernels (-m gpu): attention.hip, attention_z.hip, attention_za.hip through every
dispatch route of tests/test_forward_containment_gpu.py::ATTN_KERNELS.

The inputs of tests/attention_probe_util.py make every intermediate exact in every route's arithmetic, so the expected ctx is an exact
rational whatever the tile order, wave-group split or rescale history: where the row sum is a power of two the stored planes must be THE
round-to-nearest-even planes of it, bit for bit; elsewhere each element lies within the store format's half ulp plus four fp32 roundings;
the log-sum-exp lies within the bound derived there.  A dropped, doubled or mis-weighted key, a wrong key <-> V-row pairing, a misplaced
row or head column, a pad key that leaks or a truncating store changes some output bit.  Each test prints its worst error / bound."""
import numpy as np
import pytest
import torch

from dino_amd import capi, options
from tests import attention_probe_util as P
from tests.test_forward_containment_gpu import ATTN_KERNELS, ATTN_LONG, ATTN_LONG_KERNELS, DT, QSCALE, attn_variant_of, to_planes

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
SHAPES = [(1, 1, 1), (1, 1, 33), (1, 3, 65), (2, 2, 197), (1, 1, 257), (2, 5, 300)]
PRODUCTION = (1, 6, 3601)
DEFAULT_ROUTES = ("split-bf16", "split-fp16", "default-bf16x3", "ref3-fp16x3")
UNSPLIT = 512                        # attn_variant bit 9: keep the unsplit kernel
_cases, _planes = {}, {}


def _route(name):
    """(attn_variant, planes, Q / K / ctx fp16, V fp16, wants an lse, what its reference trails the row maximum by)"""
    _, planes, fmt, v_bf16, want_lse, _, _ = ATTN_KERNELS[name]
    v_fp16 = fmt == "fp16" and planes == 2 and not v_bf16
    running = name.startswith(("ref", "default"))
    return attn_variant_of(name), planes, fmt == "fp16", v_fp16, want_lse, (14 if fmt == "fp16" else 16) if running else 0


def _shapes(name):
    return SHAPES + ([ATTN_LONG] if name in ATTN_LONG_KERNELS else []) + ([PRODUCTION] if name in DEFAULT_ROUTES else [])


def _params():
    return [pytest.param(name, *shp, id=f"{name}-{shp[0]}x{shp[1]}x{shp[2]}") for name in ATTN_KERNELS for shp in _shapes(name)]


def _route_cases(name, shp, probe):
    """the cases of case_list (numbered over ALL the route's shapes, so that its cases use every head dimension) at one shape"""
    _, planes, _, v_fp16, _, _ = _route(name)
    out = []
    for pr, s, kw, shift_too in P.case_list(_shapes(name), planes):
        if pr == probe and s == shp:
            key = (pr, s, tuple(sorted(kw.items())), v_fp16)
            if key not in _cases:
                _cases[key] = P.build(pr, *s, v_fp16=v_fp16, **kw)
            out.append((key, _cases[key], shift_too))
    return out


def _dev(key, x, fp16, planes):
    """device planes of exact operand values [B, H, npad, 64], converted once per (operand, format)"""
    k = (key, fp16, planes)
    if k not in _planes:
        _planes[k] = torch.from_numpy(P.exact_planes(x, fp16, planes).reshape(planes, -1, 64)).cuda()
    return _planes[k]


def _launch(name, B, H, ntok, q, k, v, variant_or=0):
    variant, planes, fp16, v_fp16, want_lse, _ = _route(name)
    npad = (ntok + 63) // 64 * 64
    ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
    lse = torch.full((B * H * ntok,), float("nan"), device="cuda") if want_lse else None
    with options(attn_variant=variant | variant_or, op_fmt=int(fp16), op_v_bf16=ATTN_KERNELS[name][3]):
        capi.check(capi.lib().dinoseg_op_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B * H * npad * 64, ctx.data_ptr(), B * ntok * H * 64,
                                                   lse.data_ptr() if want_lse else None, B, H, ntok, npad, planes, S()))
        torch.cuda.synchronize()
    return ctx.cpu().numpy(), None if lse is None else lse.cpu().numpy().astype(np.float64).reshape(B, H, ntok)


def _run(name, key, c, shift=0, one_row=None):
    """one launch of the route on the case (shifted); split routes also run unsplit and must agree bit for bit.  Returns (ctx planes, lse,
    expected lse)"""
    _, planes, fp16, v_fp16, _, _ = _route(name)
    Q, K, lse_want = (c.Q, c.K, c.lse) if (shift == 0 and one_row is None) else P.shifted(c, shift, one_row)
    q = _dev((key, "q", one_row), Q, fp16, planes)
    k = _dev((key, "k", shift, one_row), K, fp16, planes)
    v = _dev((key, "v"), c.V, v_fp16, planes)
    ctx, lse = _launch(name, c.B, c.H, c.ntok, q, k, v)
    if shift != 0:                                   # the K of every shift is used once: do not keep it
        del _planes[((key, "k", shift, one_row), fp16, planes)]
    if name.startswith("split"):
        ctx1, _ = _launch(name, c.B, c.H, c.ntok, q, k, v, UNSPLIT)
        assert np.array_equal(ctx, ctx1), f"{name}: the key-split kernel and the unsplit kernel differ on an exact probe"
    return ctx, lse, lse_want


def _check(name, c, ctx, lse, lse_want, what):
    """bit equality where the row sum is a power of two, the per-element bound elsewhere, the lse bound; returns the worst error / bound"""
    _, planes, fp16, _, want_lse, trail = _route(name)
    got = P.planes_value(ctx, fp16)
    assert np.isfinite(got).all(), what
    ex = np.repeat(c.pow2, 64, axis=1)
    want_bits = P.rne_planes(np.where(ex, c.ctx, 0.0), fp16, planes)
    bad = (ctx != want_bits).any(axis=0) & ex
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} exact elements differ; first ctx[{r}, {col}] (batch {r // c.ntok} query {r % c.ntok} head {col // 64} "
                             f"d {col % 64}) = {got[r, col]!r}, expected {c.ctx[r, col]!r}")
    ratio = np.where(ex, 0.0, np.abs(got - c.ctx) / P.ctx_bound(c.ctx, fp16, planes))
    worst = float(ratio.max())
    if worst > 1.0:
        r, col = np.unravel_index(ratio.argmax(), ratio.shape)
        raise AssertionError(f"{what}: ctx[{r}, {col}] = {got[r, col]!r}, exact {c.ctx[r, col]!r}: {worst:.2f} of the bound")
    worst_lse = 0.0
    if want_lse:
        rl = np.abs(lse - lse_want) / P.lse_bound(lse_want, c.log2l, trail)
        worst_lse = float(np.nanmax(rl)) if np.isfinite(lse).all() else float("inf")
        if not worst_lse <= 1.0:
            b, h, i = np.unravel_index(np.nanargmax(np.where(np.isfinite(rl), rl, np.inf)), rl.shape)
            raise AssertionError(f"{what}: lse[{b}, {h}, {i}] = {lse[b, h, i]!r}, exact {lse_want[b, h, i]!r}: {worst_lse:.2f} of the bound")
    return worst, worst_lse


def _report(probe, name, shp, worst):
    w = max((x[0] for x in worst), default=0.0), max((x[1] for x in worst), default=0.0)
    print(f"attention probe {probe} {name} {shp[0]}x{shp[1]}x{shp[2]}: worst ctx error / bound {w[0]:.3f}, lse {w[1]:.3f}")


def _probe(probe, name, shp):
    worst = []
    for key, c, _ in _route_cases(name, shp, probe):
        ctx, lse, lse_want = _run(name, key, c)
        worst.append(_check(name, c, ctx, lse, lse_want, f"{probe} {name} {shp} {dict(key[2])}"))
    _report(probe, name, shp, worst)


@pytest.mark.parametrize("name,B,H,ntok", _params())
def test_selector(cuda, name, B, H, ntok):
    """Every query selects exactly one key pi(i), pi a permutation (same tile, reversed, far stride; another offset per (batch, head)):
    ctx row i is V[pi(i)] bit for bit in every plane, lse is the selected key's score."""
    _probe("selector", name, (B, H, ntok))


@pytest.mark.parametrize("name,B,H,ntok", _params())
def test_groups(cuda, name, B, H, ntok):
    """Two don't-care bits per query, rotating over the 12 positions: groups of 4 neighbouring or far keys, of 3, 2 or 1 at the ragged end;
    every key lies in some group.  Sizes 1, 2, 4: the exact mean, bit for bit (rounded to nearest even by the store); size 3: the bound."""
    _probe("groups", name, (B, H, ntok))


@pytest.mark.parametrize("name,B,H,ntok", _params())
def test_weights(cuda, name, B, H, ntok):
    """The high index bits soft: P = 2^-h over neighbours spread over the whole sequence, the best key in the first, a middle or the last
    tile depending on the query (so the running reference rises late, by exact powers of two).  ctx = O / l and lse within the bounds."""
    _probe("weights", name, (B, H, ntok))


@pytest.mark.parametrize("name,B,H,ntok", _params())
def test_count(cuda, name, B, H, ntok):
    """Q = 0: every real key has score 0, l = ntok exactly: lse = log2(ntok) (one key more or less is hundreds of times the bound at 3601
    tokens), ctx = the column means; the pad keys, which carry a real key's code and large V rows, count for nothing."""
    _probe("count", name, (B, H, ntok))


@pytest.mark.parametrize("name,B,H,ntok", _params())
def test_shift(cuda, name, B, H, ntok):
    """The selector and the weights probe with the integer c added to every score, c in {0, +-1, +-59, +-60, +-61, +-126, +-200}: ctx
    carries the bits of the c = 0 run, lse = lse(0) + c.  The zero-reference kernels walk their fast path to both edges of the band
    [2^-60, 2^60] and the two-pass exact recomputation beyond, through scores whose 2^S is infinite or flushed; the others move their
    reference by c.  Then c = 200 / -200 / -61 / 61 on ONE query row -- row 77 (the first 128 rows), 130 (the second), 300 (the third
    128 of a 384-query workgroup) and the last row (299 at 300 tokens: the third 128 as well), each where the sequence has it -- on every
    route, hi + lo ones with their lo planes in place: the workgroup decides the recomputation, the other rows must not notice."""
    shp = (B, H, ntok)
    worst = []
    for probe in ("selector", "weights"):
        for key, c, shift_too in _route_cases(name, shp, probe):
            if not shift_too:
                continue
            base, _, _ = _run(name, key, c)
            runs = [(s, None) for s in P.SHIFTS[1:]]
            runs += [(200, min(ntok - 1, 77)), (-200, min(ntok - 1, 130)), (-61, min(ntok - 1, 300)), (61, ntok - 1)]
            for shift, one_row in runs:
                what = f"shift {shift} row {one_row} {probe} {name} {shp}"
                ctx, lse, lse_want = _run(name, key, c, shift, one_row)
                assert np.array_equal(ctx, base), f"{what}: ctx differs from the unshifted run in {int((ctx != base).sum())} places"
                worst.append(_check(name, c, ctx, lse, lse_want, what))
    _report("shift", name, shp, worst)


@pytest.mark.parametrize("name", ["split-bf16", "split-fp16"])
@pytest.mark.parametrize("B,H,ntok", [s for s in SHAPES + [ATTN_LONG, PRODUCTION] if s[2] >= 193])
def test_split_routes_run_the_key_split_kernel(cuda, name, B, H, ntok):
    """Exact probes hide the summation order, so they cannot show that attn_fwd_zs_kernel ran: an ordinary random draw does.  At every
    shape at which the split applies (two groups from 193 tokens, three from 2048) the route's ctx differs somewhere from the unsplit
    kernel's (attn_variant bit 9): another summation order (test_attention_key_split_for_small_grids holds how far it may go)."""
    _, planes, fp16, _, _, _ = _route(name)
    npad = (ntok + 63) // 64 * 64
    g = np.random.default_rng(ntok)
    draw = lambda sc: torch.from_numpy(g.standard_normal((B * H * npad, 64)).astype(np.float32)) * sc
    dt = DT["fp16" if fp16 else "bf16"]
    q, k, v = to_planes(draw(1.5) * QSCALE, dt, 1).cuda(), to_planes(draw(1.5), dt, 1).cuda(), to_planes(draw(1.0), torch.bfloat16, 1).cuda()
    split, _ = _launch(name, B, H, ntok, q, k, v)
    unsplit, _ = _launch(name, B, H, ntok, q, k, v, UNSPLIT)
    a, b = P.planes_value(split, fp16), P.planes_value(unsplit, fp16)
    assert (a != b).any(), "the key-split kernel was not dispatched"
