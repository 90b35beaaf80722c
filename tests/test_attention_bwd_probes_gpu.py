"""Exact per-element probes of the attention backward (-m gpu): attn_bwd_prep_kernel, attn_bwd_dq_kernel<PLANES, 4 | 8> and
attn_bwd_dkv_kernel<PLANES, 4> through dinoseg_op_attention_bwd, on one and on two planes.

The six operands of tests/attention_bwd_probe_util.py make every intermediate exact in the kernels' arithmetic, so dQ, dK and dV must carry
THE round-to-nearest-even planes of 0.125 * sum, float32(sum) * float32(ln 2) and sum, bit for bit, whatever the tile order or the
register <-> key mapping -- except dK on hi + lo planes, whose lo plane the compiler rounds from the exact product (a contracted multiply
and subtract in the split) and which is therefore held to  half_ulp_store + 2^-23 |x|  of the exact product instead (the util's docstring).
A key dropped or doubled, a query missing from a dK / dV sum, a wrong mask on the ragged last key tile, a pad query that weighs, a wrong dO
row in the last query tile, a truncated dS, a lost lo plane, swapped head columns, a missing delta or a wrong epilogue factor changes some
bit (tests/test_attention_bwd_probes_cpu.py shows that on mutants of an emulation).  The pad rows hold a real key, large V rows and query 0;
the scratch is NaN before the launch; dO and O are followed by NaN rows.  Each test prints the number of elements compared and, on two
planes, dK's worst error / bound."""
import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import capi, options
from tests import attention_bwd_probe_util as U

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
SENT16 = 0x7F7F                      # bf16 sentinel of the output (a large finite value)
NAN16 = 0x7FC1
FORCE_4_WAVE = 64                    # attn_variant bit 6: keep the 128-query dQ workgroups
ALL_SHAPES = U.SHAPES + [U.PRODUCTION]
_cases = {}


def _built(probe, shp, kw):
    key = (probe, shp, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = U.build(probe, *shp, **kw)
    return _cases[key]


def _launch(c, variant=None):
    """one dinoseg_op_attention_bwd on the case's operands; returns the dqkv planes [planes, B * ntok, 3 * H * 64] as int16 numpy"""
    B, H, ntok, npad, planes = c.B, c.H, c.ntok, c.npad, c.planes
    ops = U.operand_planes(c)
    q, k, v = (torch.from_numpy(ops[n]).cuda() for n in ("q", "k", "v"))
    rows = B * ntok + 64                                                 # 64 NaN rows behind dO and O: what an unclamped row would read
    dO, O = (torch.full((planes, rows, H * 64), NAN16, dtype=torch.int16, device="cuda") for _ in range(2))
    dO[:, :B * ntok] = torch.from_numpy(ops["dO"]).cuda()
    O[:, :B * ntok] = torch.from_numpy(ops["O"]).cuda()
    lse = torch.from_numpy(ops["lse"]).cuda()
    scratch = torch.full((2 * B * H * npad,), float("nan"), device="cuda")
    dqkv = torch.full((planes, B * ntok, 3 * H * 64), SENT16, dtype=torch.int16, device="cuda")
    with options(**({} if variant is None else {"attn_variant": variant})):
        capi.check(capi.lib().dinoseg_op_attention_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), B * H * npad * 64, dO.data_ptr(), O.data_ptr(),
                                                       rows * H * 64, lse.data_ptr(), scratch.data_ptr(), dqkv.data_ptr(),
                                                       B * ntok * 3 * H * 64, B, H, ntok, npad, planes, S()))
        torch.cuda.synchronize()
    return dqkv.cpu().numpy()


def _check(c, got, what):
    """U.mismatches: bit equality on every plane (dK on two planes: its bound); the first failing element by (frame, head, row, d).  Returns
    (elements compared, worst dK error / bound)"""
    bad, worst = U.mismatches(c, got)
    if bad.any():
        row, col = (int(x) for x in np.argwhere(bad)[0])
        val = lambda p: float(torch.from_numpy(p[:, row, col].copy()).view(torch.bfloat16).double().sum())
        part, head, d = "QKV"[col // (c.H * 64)], col % (c.H * 64) // 64, col % 64
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first d{part} frame {row // c.ntok} head {head} row {row % c.ntok} "
                             f"d {d}: got {val(got)!r} (bits {got[:, row, col].tolist()}), expected {val(c.expect)!r} "
                             f"(bits {c.expect[:, row, col].tolist()}); worst dK error / bound {worst:.3g}")
    return got.size, worst


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("B,H,ntok", ALL_SHAPES)
@pytest.mark.parametrize("probe", U.PROBES)
def test_probe(cuda, probe, B, H, ntok, planes):
    """selector: dV[pi(q)] = dO[q], dQ = dK = 0 (consistent lse and O: dS = 0).  pick: one nonzero P and dS per query, with a lo plane in K
    or Q~, and with a dS that the split has to round.  groups: consistent sets of 1, 2 and 4 keys.  weights: 64 neighbours at P = 2^-h.
    count: Q~ = 0, every key and every query counts exactly once.  (tests/attention_bwd_probe_util.py)"""
    shp = (B, H, ntok)
    n = cases = 0
    worst = 0.0
    for pr, s, kw in U.case_list(ALL_SHAPES, planes):
        if pr == probe and s == shp:
            c = _built(pr, s, kw)
            m, w = _check(c, _launch(c), f"{probe} {shp} {kw}")
            n, cases, worst = n + m, cases + 1, max(worst, w)
    assert cases >= 1
    print(f"attention_bwd probe {probe} {B}x{H}x{ntok} on {planes} plane(s): {n} elements compared over {cases} case(s), all bit-equal"
          + (f" but dK: worst error / bound {worst:.3f}" if planes == 2 else ""))


def test_probes_on_the_8_wave_dq_route(cuda):
    """The smallest grid at which launch_attention_bwd takes attn_bwd_dq_kernel<1, 8> (256-query workgroups): 128-row workgroups over
    (pairs rounded up to 8) x ceil(ntok / 128) reach two per CU.  449 tokens: a ragged 128-row block AND a ragged 256-row block, 8 key
    tiles with one key in the last.  One lean variant of each probe, bit-equal to the expectation, and again with attn_variant bit 6 (the
    4-wave kernel): bit-identical output."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ntok, H = 449, 8
    nq = (ntok + 127) // 128
    pairs = (2 * ncu + nq - 1) // nq
    pairs = (pairs + 7) // 8 * 8
    B = pairs // H
    assert B * H == pairs and pairs * nq >= 2 * ncu > (pairs - 8) * nq, "not the smallest grid that selects the 8-wave dQ kernel"
    n = 0
    far = U.P.coprime_steps(ntok)[-1]
    for i, probe in enumerate(U.PROBES):
        c = U.build(probe, B, H, ntok, n=i, planes=1, **({} if probe == "count" else dict(s=far[0], t=far[1])))
        d8 = _launch(c)
        n += _check(c, d8, f"{probe} {(B, H, ntok)} on the 8-wave route")[0]
        d4 = _launch(c, variant=dino_amd.get_option("attn_variant") | FORCE_4_WAVE)
        assert np.array_equal(d8, d4), f"{probe}: {int((d8 != d4).sum())} elements differ between the 8-wave and the 4-wave dQ route"
    print(f"attention_bwd probes on the 8-wave dQ route {B}x{H}x{ntok} ({ncu} CUs): {n} elements compared, all bit-equal, twice")
