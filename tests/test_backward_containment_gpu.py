"""Where the attention backward writes, and what it must not read (-m gpu): the rules of tests/test_forward_containment_gpu.py for
dinoseg_op_attention_bwd (attn_bwd_prep_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel).

The value tests (tests/test_train_gpu.py::test_attention_bwd, tests/test_backward_ops_gpu.py::test_attention_backward_per_block) hand the
entry exactly-sized buffers, the minimal plane strides, zero pad rows and a zeroed scratch.  Here, on the seeded draws of the latter:
  layout    dqkv lies in a Guarded buffer (NaN bands in front, between the planes and behind; the entry has no row stride, ld = cols);
            q / k / v and dO / O are re-laid by strided_planes with finite garbage in the gaps; the scratch is exactly 2 B H npad floats
            between NaN bands and holds NaN itself.  Every guard stays untouched, the scratch payload is fully written (neg_lse finite
            below ntok and -inf from there to npad, neg_delta finite throughout), and dqkv equals, bit for bit, the run on exact sizes,
            minimal strides, zero pad rows and a zeroed scratch -- which meets the fp64 check of test_attention_backward_per_block at that
            test's bars (no tolerance is new).
  pad rows  rows ntok..npad of Q, K and V filled as the forward test fills them (draws like the real rows, V four times larger, one pad key
            per head a multiple of a real query: a log2-domain score near +100): the bits of the zero-pad run, and finite."""
import numpy as np
import pytest
import torch

from dino_amd import capi
from tests.gpu_util import Guarded, pack, seeded, strided_planes, unpack, untouched
from tests.test_backward_ops_gpu import LOG2E, _attn_pair_ref, _pair_grads

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
SHAPES = [(1, 1, 1), (1, 3, 65), (2, 2, 197), (1, 1, 257), (2, 5, 300)]
BAND = 4096                      # floats of NaN on either side of the scratch


def _wide_route_shape():
    """the smallest (B, 8, 449) at which launch_attention_bwd takes the 256-query dQ workgroups (two 128-query ones per CU)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nq = (449 + 127) // 128
    pairs = ((2 * ncu + nq - 1) // nq + 7) // 8 * 8
    assert pairs * nq >= 2 * ncu > (pairs - 8) * nq
    return pairs // 8, 8, 449


def _operands(B, H, ntok, planes):
    """The draws of test_attention_backward_per_block (seed ntok + planes), with zero pad rows and with garbage pad rows, and the forward's
    ctx and lse on them.  Returns ((q, k, v) zero-pad planes, (q, k, v) garbage-pad planes, dO planes, ctx planes, lse)."""
    seed = ntok + planes
    npad = (ntok + 63) // 64 * 64
    npd = npad - ntok
    real = [seeded((B, H, ntok, 64), seed) * (0.125 * LOG2E), seeded((B, H, ntok, 64), seed + 1), seeded((B, H, ntok, 64), seed + 2)]
    pads = [seeded((B, H, npd, 64), 9000 + ntok) * (0.125 * LOG2E), seeded((B, H, npd, 64), 9001 + ntok), seeded((B, H, npd, 64), 9002 + ntok) * 4.0]
    if npd:
        # unmasked, this key would own its query: 0.125 log2(e) * 8.5 |q|^2 is about 100 at |q|^2 = 64, and 2^100 is finite
        pads[1][:, :, npd // 2] = 8.5 * real[0][:, :, min(5, ntok - 1)] / (0.125 * LOG2E)
    sets = []
    for garbage in (False, True):
        out = []
        for x, p in zip(real, pads):
            full = torch.zeros((B, H, npad, 64), device="cuda")
            full[:, :, :ntok] = x
            if garbage:
                full[:, :, ntok:] = p
            out.append(pack(full.reshape(-1, 64), planes))
        sets.append(tuple(out))
    dop = pack(seeded((B * ntok, H * 64), seed + 3, scale=0.1), planes)
    q, k, v = sets[0]
    ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
    lse = torch.zeros((B, H, ntok), device="cuda")
    capi.check(capi.lib().dinoseg_op_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B * H * npad * 64, ctx.data_ptr(), B * ntok * H * 64,
                                               lse.data_ptr(), B, H, ntok, npad, planes, S()))
    return sets[0], sets[1], dop, ctx, lse


def _run(B, H, ntok, planes, qkv, dop, ctx, lse, guarded):
    """one dinoseg_op_attention_bwd.  guarded: every stride larger than minimal, NaN around dqkv and around (and in) the scratch; else exact
    sizes, minimal strides, a zeroed scratch.  Returns (dqkv planes, scratch payload or None, guards untouched)."""
    npad = (ntok + 63) // 64 * 64
    n_scr = 2 * B * H * npad
    dqkv = Guarded(planes, B * ntok, 3 * H * 64, torch.int16, exact=not guarded)
    if guarded:
        keep = [strided_planes(t, gap_rows=5) for t in qkv] + [strided_planes(t, gap_rows=7) for t in (dop, ctx)]
        (qp, kp, vp, dp, op), qkv_plane, o_plane = [x[1] for x in keep], keep[0][2], keep[3][2]
        flat = torch.full((n_scr + 2 * BAND,), float("nan"), device="cuda")
        scratch = flat[BAND:BAND + n_scr]
    else:
        (qp, kp, vp, dp, op) = [t.data_ptr() for t in (*qkv, dop, ctx)]
        qkv_plane, o_plane = B * H * npad * 64, B * ntok * H * 64
        flat = scratch = torch.zeros(n_scr, device="cuda")
    capi.check(capi.lib().dinoseg_op_attention_bwd(qp, kp, vp, qkv_plane, dp, op, o_plane, lse.data_ptr(), scratch.data_ptr(), dqkv.ptr(),
                                                   dqkv.plane, B, H, ntok, npad, planes, S()))
    torch.cuda.synchronize()
    ok = dqkv.guards_untouched() and (not guarded or (untouched(flat[:BAND]) and untouched(flat[BAND + n_scr:])))
    return dqkv.dense(), (scratch.clone() if guarded else None), ok


def _fp64_check(B, H, ntok, planes, qkv, dop, dqkv):
    """test_attention_backward_per_block's check: relative Frobenius error per 64-token block of the first, a middle and the last pair.
    err <= tol * |ref| is that test's e <= tol without the division: at one token the fp64 dQ and dK are exactly zero (the softmax of one
    key is constant) while the kernel subtracts a delta and a dP that it sums in different orders, so there -- and only there -- the
    block is held to tol times the norm of the terms that cancel, 0.125 (|dP| + |delta|) |K| and 0.125 (|dP| + |delta|) |q|."""
    tol = 2e-2 if planes == 1 else 2e-4
    npad = (ntok + 63) // 64 * 64
    qp, kp, vp = qkv
    worst, npairs = 0.0, B * H
    for pair in sorted({0, npairs // 2, npairs - 1}):
        b, h = divmod(pair, H)
        ref = _attn_pair_ref(qp, kp, vp, dop, B, H, ntok, npad, b, h)
        got = _pair_grads(dqkv, B, H, ntok, b, h)
        for name, r, g in zip("qkv", ref, got):
            for t0 in range(0, ntok, 64):
                rb, gb = r[t0:t0 + 64], g[t0:t0 + 64]
                scale = float(rb.norm())
                if scale == 0.0:
                    assert ntok == 1 and name in "qk"
                    rows = lambda p: unpack(p).reshape(B, H, npad, 64)[b, h, :1].double()
                    dO = unpack(dop).reshape(B, ntok, H, 64)[b, :, h].double()
                    dP = (dO @ rows(vp).T).abs()
                    scale = float((2 * dP * 0.125 * (rows(kp) if name == "q" else rows(qp) / (0.125 * LOG2E)).abs()).norm())
                err = float((gb - rb).norm())
                worst = max(worst, err / (tol * scale))
                assert err <= tol * scale, (name, b, h, t0, err, scale)
    return worst


def _cases():
    out = [pytest.param(*shp, planes, id=f"{shp[0]}x{shp[1]}x{shp[2]}-{planes}pl") for shp in SHAPES for planes in (1, 2)]
    return out + [pytest.param(None, None, None, 1, id="8-wave-dq-route-1pl")]


@pytest.mark.parametrize("B,H,ntok,planes", _cases())
def test_attention_backward_containment(cuda, B, H, ntok, planes):
    if B is None:
        B, H, ntok = _wide_route_shape()
    npad = (ntok + 63) // 64 * 64
    zero, garbage, dop, ctx, lse = _operands(B, H, ntok, planes)
    assert npad == ntok or not torch.equal(zero[1], garbage[1])
    d0, _, ok0 = _run(B, H, ntok, planes, zero, dop, ctx, lse, guarded=False)
    d1, scr, ok1 = _run(B, H, ntok, planes, zero, dop, ctx, lse, guarded=True)
    d2, _, ok2 = _run(B, H, ntok, planes, garbage, dop, ctx, lse, guarded=True)
    assert ok0 and ok1 and ok2, "a guard element around dqkv or the scratch was written"
    neg_lse, neg_delta = scr[:B * H * npad].reshape(B * H, npad), scr[B * H * npad:].reshape(B * H, npad)
    assert bool(torch.isfinite(neg_lse[:, :ntok]).all()) and bool((neg_lse[:, ntok:] == float("-inf")).all()), "neg_lse: finite below ntok, -inf above"
    assert bool(torch.isfinite(neg_delta).all()), "neg_delta is not written throughout"
    assert torch.equal(d1, d0), f"{int((d1 != d0).sum())} elements change with the strides and the scratch's contents"
    assert bool(torch.isfinite(unpack(d2)).all()), "dqkv is not finite with garbage pad rows"
    assert torch.equal(d2, d0), f"{int((d2 != d0).sum())} of {d0.numel()} elements change with the pad rows"
    worst = _fp64_check(B, H, ntok, planes, zero, dop, d0)
    print(f"attention_bwd containment {B}x{H}x{ntok} on {planes} plane(s): {d0.numel()} elements bit-equal in three runs, {scr.numel()} scratch floats "
          f"written; worst block error / bound {worst:.3g}")
