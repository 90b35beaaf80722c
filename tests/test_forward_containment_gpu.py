"""Where the forward kernels write, and what they must not read (-m gpu).

The value tests of the hot path (tests/test_ops_gpu.py, tests/test_fp16_gpu.py) hand every entry exactly-sized buffers and the minimal
strides (a_plane = M*K, lda = K, out_plane = M*N, ldo = N, qkv_plane = B*H*npad*64, ctx_plane = B*ntok*H*64) and zero pad rows.  Here
every output lies in one flat buffer between guard bands of a full tile of rows (tests/gpu_util.py: Guarded, 384 rows), every stride an
entry takes is larger than the minimal one, and the gaps of the inputs hold finite garbage.  Per case:
  (a) every guard element is untouched;
  (b) the outputs equal, bit for bit, those of the same call on exact sizes and minimal strides (a stride changes no dispatch at these
      sizes: gemm_big's span check only looks at offsets beyond 2^32 bytes);
  (c) the exact-layout outputs meet the fp64 reference of the operator's existing test at that test's bar (no tolerance is new here).
The attention kernels additionally run with finite garbage in the pad rows ntok..npad of Q, K and V -- one pad key per head a multiple of
a real query, a log2-domain score near +100 -- and must give the bits of the run on zero pad rows: the pad rows need not be zero (the
contract of include/dinoseg.h)."""
import math

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import capi, options
from oracle import dinoseg_oracle as O
from tests.gpu_util import Guarded, pack_slabs, seeded, strided_planes, untouched
from tests.test_ops_gpu import _ln_ref, _mlp3_case, _one_plane, _pack_mlp4, _pack_rs, _q1, _split_planes, pack_mlp

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
LOG2E = 1.4426950408889634
QSCALE = 0.125 * LOG2E
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
M_EDGES = [1, 77, 128 * 5 + 33]         # one row; one partial tile; five tiles and a ragged sixth
M_PERSISTENT = 128 * 300 + 19           # more items than workgroups (the persistent kernels), ragged last item


def to_planes(x, dt, planes):
    """fp32 [...] -> int16 planes [planes, ...]: RNE of x, RNE of the remainder (what dinoseg_op_pack writes)"""
    hi = x.to(dt)
    pl = [hi] if planes == 1 else [hi, (x - hi.float()).to(dt)]
    return torch.stack(pl).contiguous().view(torch.int16)


def planes_value(p, dt):
    return p.view(dt).double().sum(dim=0)


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def _ends(M):
    """the rows a host reference is taken on: all of them, or the first and last 256 of a persistent-walk case"""
    return slice(None) if M <= 1024 else torch.cat([torch.arange(256), torch.arange(M - 256, M)]).cuda()


# ------------------------------------------------------------------------------------------------ attention
# name -> (attn_variant, planes, Q / K / ctx format, op_v_bf16, LSE output, ctx bar, lse bar); attn_variant None = the library's default, which
# attn_variant_of() reads.  The bars are those of the kernel's existing
# test: test_attention / test_attention_kernel_variants (1.2e-2 / 6e-3 on one bf16 plane, 1e-4 / 1e-4 on hi + lo planes),
# test_attention_za_is_bit_identical_to_the_compiled_kernel (2e-2), test_attention_za_hi_lo_planes_bit_identical (1e-4 / 5e-3),
# test_attention_key_split_for_small_grids (1.5e-2), test_fp16_gpu.py::test_attention_fp16_qk (1.2e-2: the default route without an LSE,
# i.e. the key-split kernel from 193 tokens on) and ::test_attention_hi_lo_planes_fp16 (1e-5).
ATTN_KERNELS = {}
for _v in range(4):                      # attention.hip: attn_fwd_kernel<PLANES, 4, false, VAR>
    ATTN_KERNELS[f"ref{_v}-bf16"] = (_v, 1, "bf16", 0, True, 1.2e-2, 6e-3)
    ATTN_KERNELS[f"ref{_v}-bf16x3"] = (_v, 2, "bf16", 0, True, 1e-4, 1e-4)
ATTN_KERNELS.update({
    "z128-bf16": (11, 1, "bf16", 0, True, 1.2e-2, 6e-3),                                   # attn_fwd_z_kernel<1, 4, 4>
    "z256-bf16": (11 | 512 | 4096, 1, "bf16", 0, True, 2e-2, 6e-3),                        # attn_fwd_z_kernel<1, 4, 8>
    "za32-bf16": (11 | 512 | 1024 | 2048, 1, "bf16", 0, True, 2e-2, 6e-3),                 # attention_za.hip, 32 queries per wave
    "za64-bf16": (11 | 512 | 1024 | 2048 | 65536, 1, "bf16", 0, True, 2e-2, 6e-3),         # ... 64 queries per wave
    "split-bf16": (None, 1, "bf16", 0, False, 1.5e-2, None),               # attn_fwd_zs_kernel<., 2 / 3> from 193 / 2048 tokens on
    "z-bf16x3": (11 | 16, 2, "bf16", 0, True, 1e-4, 5e-3),                                 # attn_fwd_z_kernel<2, 3, 12>
    "za-bf16x3": (11 | 16 | 1024 | 2048, 2, "bf16", 0, True, 1e-4, 5e-3),                  # attention_za.hip, hi + lo body
    # the default options with an LSE (the training forward): launch_attention keeps attention.hip VAR 3 then, the kernel of ref3-bf16x3,
    # reached here through the default dispatch; the default hi + lo INFERENCE route (no LSE, large grids) is attention_za.hip = za-bf16x3
    "default-bf16x3": (None, 2, "bf16", 0, True, 1e-4, 1e-4),
    "z128-fp16": (11 | 512, 1, "fp16", 0, False, 1.2e-2, None),                            # fp16 Q / K, bf16 V
    "z256-fp16": (11 | 512 | 4096, 1, "fp16", 0, False, 2e-2, None),
    "za32-fp16": (11 | 512 | 1024 | 2048, 1, "fp16", 0, False, 2e-2, None),
    "za64-fp16": (11 | 512 | 1024 | 2048 | 65536, 1, "fp16", 0, False, 2e-2, None),
    "split-fp16": (None, 1, "fp16", 0, False, 1.2e-2, None),
    "z-fp16x3-vbf16": (11 | 16, 2, "fp16", 1, False, 1e-4, None),                          # fp16 hi + lo Q / K / ctx, bf16 hi + lo V
    "za-fp16x3-vbf16": (11 | 16 | 1024 | 2048, 2, "fp16", 1, False, 1e-4, None),
    "ref3-fp16x3": (None, 2, "fp16", 0, False, 1e-5, None),                # attention.hip, every operand fp16 hi + lo
})
ATTN_SHAPES = [(1, 1, 1), (1, 3, 65), (2, 2, 197), (1, 1, 257), (2, 5, 300)]
ATTN_LONG = (1, 1, 2051)       # 33 key tiles with 3 valid keys in the last, a last q-tile with 3 valid rows: the three-group split, 256-query forms
ATTN_LONG_KERNELS = ("z256-bf16", "za32-bf16", "za64-bf16", "split-bf16", "za-bf16x3", "z256-fp16", "za32-fp16", "za64-fp16", "split-fp16",
                     "za-fp16x3-vbf16")
PAD_SHAPES = [(1, 3, 65), (1, 1, 257), (2, 2, 197)]
_attn_cache = {}


def attn_variant_of(name):
    variant = ATTN_KERNELS[name][0]
    return dino_amd.get_option("attn_variant") if variant is None else variant


def _attn_operands(B, H, ntok, planes, fmt, v_bf16):
    """(q, k, v planes with zero pad rows, the same with finite garbage in the pad rows, fp64 ctx reference, fp64 lse reference); seeded,
    built once per operand format and shared"""
    vdt = torch.bfloat16 if (planes == 1 or v_bf16 or fmt == "bf16") else torch.float16
    key = (B, H, ntok, planes, fmt, vdt)
    if key in _attn_cache:
        return _attn_cache[key]
    npad = (ntok + 63) // 64 * 64
    # the real rows are the existing tests' draws (test_attention: seed ntok + planes; test_fp16_gpu.py::test_attention_fp16_qk: seed ntok), so that
    # their bars mean here what they mean there: on one 16-bit plane the bar sits close to the format's own rounding of a peaked row's output
    # (half a bf16 ulp of |ctx| in [2, 4) is 7.8e-3) and is a statement about those draws
    g = np.random.default_rng(ntok if (fmt == "fp16" and planes == 1) else ntok + planes)
    draw = lambda n, sc: torch.from_numpy(g.standard_normal((B, H, n, 64)).astype(np.float32)) * sc
    Q, K, V = draw(ntok, 1.5), draw(ntok, 1.5), draw(ntok, 1.0)
    g = np.random.default_rng(9000 + ntok)
    npd = npad - ntok
    Qp, Kp, Vp = draw(npd, 1.5), draw(npd, 1.5), draw(npd, 4.0)      # pad rows: Q and K like the real rows, V four times larger
    if npd and ntok > 5:
        Kp[:, :, npd // 2] = 4.0 * Q[:, :, 5]          # unmasked, this key would own query 5 (score ~ +100 in the log2 domain, 2^100 is finite)

    def build(x, pad, dt, garbage):
        full = torch.zeros((B, H, npad, 64), dtype=torch.float32)
        full[:, :, :ntok] = x
        if garbage:
            full[:, :, ntok:] = pad
        return to_planes(full.reshape(B * H * npad, 64), dt, planes).cuda()
    sets = [tuple(build(x, p, dt, gb) for x, p, dt in ((Q * QSCALE, Qp * QSCALE, DT[fmt]), (K, Kp, DT[fmt]), (V, Vp, vdt))) for gb in (False, True)]
    q, k, v = sets[0]
    val = lambda p, dt: planes_value(p.cpu(), dt).reshape(B, H, npad, 64)[:, :, :ntok]
    s = (val(q, DT[fmt]) / LOG2E) @ val(k, DT[fmt]).transpose(-1, -2)
    ref = (torch.softmax(s, dim=-1) @ val(v, vdt)).transpose(1, 2).reshape(B * ntok, H * 64)
    ref_lse = torch.logsumexp(s, dim=-1) * LOG2E
    _attn_cache[key] = (sets[0], sets[1], ref, ref_lse)
    return _attn_cache[key]


def _attn_run(name, B, H, ntok, qkv, guarded):
    """one dinoseg_op_attention launch, ctx and lse between guard bands; guarded: every stride larger than minimal, else the exact layout.
    Returns (ctx planes [planes, B*ntok, H*64] int16, lse [B*H*ntok] or None, guards untouched)"""
    _, planes, fmt, v_bf16, want_lse, _, _ = ATTN_KERNELS[name]
    npad = (ntok + 63) // 64 * 64
    ctx = Guarded(planes, B * ntok, H * 64, torch.int16, exact=not guarded)
    lse = Guarded(1, 1, B * H * ntok, torch.float32, band=4096) if want_lse else None
    if guarded:
        keep = [strided_planes(t, gap_rows=5) for t in qkv]          # qkv_plane = (B*H*npad + 5) * 64
        (qp, kp, vp), qkv_plane = [x[1] for x in keep], keep[0][2]
    else:
        (qp, kp, vp), qkv_plane = [t.data_ptr() for t in qkv], B * H * npad * 64
    with options(attn_variant=attn_variant_of(name), op_fmt=int(fmt == "fp16"), op_v_bf16=v_bf16):
        capi.check(capi.lib().dinoseg_op_attention(qp, kp, vp, qkv_plane, ctx.ptr(), ctx.plane, lse.ptr() if lse else None, B, H, ntok, npad,
                                                   planes, S()))
        torch.cuda.synchronize()
    ok = ctx.guards_untouched() and (lse is None or lse.guards_untouched())
    return ctx.dense(), None if lse is None else lse.dense().reshape(-1), ok


def _attn_cases(shapes, every_long=False):
    return [pytest.param(name, *shp, id=f"{name}-{shp[0]}x{shp[1]}x{shp[2]}") for name in ATTN_KERNELS
            for shp in shapes + ([ATTN_LONG] if (every_long or name in ATTN_LONG_KERNELS) else [])]


@pytest.mark.parametrize("name,B,H,ntok", _attn_cases(ATTN_SHAPES))
def test_attention_guarded_layout(cuda, name, B, H, ntok):
    """dinoseg_op_attention with qkv_plane and ctx_plane larger than the minimal strides, ctx and lse between guard bands.

    (c) at (2, 5, 300) is what made attention.hip's one-plane kernels (ref0 .. ref3) sum the probabilities AS ROUNDED to bf16 for P.V: with
    the row sum taken from the unrounded fp32 probabilities they gave max |ctx - fp64| = 1.3708e-2 here against the 1.2e-2 of test_attention /
    test_attention_kernel_variants (an fp64 emulation of that arithmetic reproduces the figure to five digits; the other shapes gave 7.8e-3 ..
    8.5e-3), because 2^-9 sum(p |v|) then comes on top of half a bf16 ulp of |ctx| < 4.  With the sum of the rounded probabilities their
    rounding cancels in the quotient and the emulation gives 8.0e-3; the zero-reference kernels, which always summed them on the matrix
    core, give 1.127e-2."""
    _, planes, fmt, v_bf16, want_lse, bar, lse_bar = ATTN_KERNELS[name]
    zero, _, ref, ref_lse = _attn_operands(B, H, ntok, planes, fmt, v_bf16)
    ctx0, lse0, ok0 = _attn_run(name, B, H, ntok, zero, guarded=False)
    ctx1, lse1, ok1 = _attn_run(name, B, H, ntok, zero, guarded=True)
    assert ok0 and ok1, "a guard element around ctx / lse was written"                                 # (a)
    assert torch.equal(ctx1, ctx0) and (lse0 is None or torch.equal(lse1, lse0))                       # (b)
    got = planes_value(ctx0.cpu(), DT[fmt])                                                             # (c)
    assert torch.isfinite(got).all()
    err = maxerr(got, ref)
    err_lse = maxerr(lse0.cpu().reshape(B, H, ntok), ref_lse) if lse0 is not None else 0.0
    print(f"attention {name} {B}x{H}x{ntok}: ctx {err:.3e} (bar {bar:.1e}) lse {err_lse:.3e}")
    assert err <= bar, err
    assert lse0 is None or err_lse <= lse_bar, err_lse


@pytest.mark.parametrize("name,B,H,ntok", _attn_cases(PAD_SHAPES, every_long=True))
def test_attention_pad_rows_do_not_matter(cuda, name, B, H, ntok):
    """Finite garbage in rows ntok..npad of Q, K and V (K pads drawn like keys, one of them 4 x a real query; V pads four times V's scale):
    ctx and lse carry the bits of the run on zero pad rows, the guards stay untouched.  No value tolerance: a pad key that reaches a row sum
    or a P.V product changes bits."""
    _, planes, fmt, v_bf16, _, _, _ = ATTN_KERNELS[name]
    zero, garbage, _, _ = _attn_operands(B, H, ntok, planes, fmt, v_bf16)
    assert not torch.equal(zero[1], garbage[1])
    ctx0, lse0, ok0 = _attn_run(name, B, H, ntok, zero, guarded=True)
    ctx1, lse1, ok1 = _attn_run(name, B, H, ntok, garbage, guarded=True)
    assert ok0 and ok1, "a guard element around ctx / lse was written"
    diff = ctx0 != ctx1
    assert not bool(diff.any()), f"{float(diff.float().mean()):.4f} of ctx changes with the pad rows"
    assert lse0 is None or torch.equal(lse0, lse1)


# ------------------------------------------------------------------------------------------------ dinoseg_op_gemm
def _gemm_call(Aptr, a_plane, lda, Wp, M, N, K, planes, epi, bias, out_f32, out16, out_plane, ldo):
    capi.check(capi.lib().dinoseg_op_gemm(Aptr, a_plane, lda, Wp.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), out_f32, out16,
                                          out_plane, ldo, S()))


# gemm.hip; gemm.hip at an N gemm_big.hip takes; gemm_big.hip.  The persistent kernel also with more tiles than workgroups: at 38 419 rows
# x 768 columns its 256-row configuration has ceil(151 / 8) * 2 = 38 (panel, column tile) pairs per XCD and the 128-row hi + lo one 76, both
# above the 32 workgroups an XCD of 32 CUs gets (launch_big_cfg), so workgroups walk on to a second tile.  (At N = 384 the one-plane
# configuration has 19 pairs per XCD: one tile per workgroup.)
@pytest.mark.parametrize("N,big,M", [(n, b, m) for n, b in ((256, 0), (384, 0), (384, 2)) for m in M_EDGES] + [(768, 2, M_PERSISTENT)])
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_gemm_guarded_layout(cuda, fmt, planes, N, big, M):
    """dinoseg_op_gemm, every epilogue the format has, with a_plane / lda / out_plane / ldo larger than minimal; the residual epilogue of
    gemm.hip on its 64-row (default at these sizes) and 128-row (route_ab bit 0) tiles.  38 419 rows x 768: the persistent kernel only."""
    K = 128
    dt = DT[fmt]
    A = seeded((M, K), 10 + M) + torch.arange(K, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    W = seeded((N, K), 20 + N) * 0.1 + torch.arange(N, device="cuda", dtype=torch.float32)[:, None] * 1e-3
    bias, X0 = seeded((N,), 3), seeded((M, N), 4)
    Ap, Wp = to_planes(A, dt, planes), to_planes(W, dt, planes)
    keepA, A_ptr, a_plane, lda = strided_planes(Ap, ld=K + 64, gap_rows=3)
    rows = _ends(M)
    Aq, Wq = planes_value(Ap, dt)[rows], planes_value(Wp, dt)
    base = Aq @ Wq.t() + bias.double()                              # fp64 on the operands the kernel sees
    scale = float(base.abs().max())
    exact = (A.double()[rows] @ W.double().t() + bias.double())
    epis = [capi.EPI_RESID, capi.EPI_GELU] + ([capi.EPI_PLAIN] if fmt == "bf16" else []) + ([capi.EPI_RELU] if (fmt == "bf16" or planes == 2) else [])
    for epi in epis:
        for ab in ((0, 1) if (epi == capi.EPI_RESID and big == 0) else (0,)):
            what = f"epi {epi} route_ab {ab}"
            with options(op_fmt=int(fmt == "fp16"), gemm_big=big, route_ab=ab):
                if epi in (capi.EPI_PLAIN, capi.EPI_RESID):
                    e, g = Guarded(1, M, N, torch.float32, exact=True), Guarded(1, M, N, torch.float32)
                    if epi == capi.EPI_RESID:
                        e.fill(X0), g.fill(X0)
                    _gemm_call(Ap.data_ptr(), M * K, K, Wp, M, N, K, planes, epi, bias, e.ptr(), None, 0, 0)
                    _gemm_call(A_ptr, a_plane, lda, Wp, M, N, K, planes, epi, bias, g.ptr(), None, 0, 0)
                    got = e.dense()[0]
                else:
                    e, g = Guarded(planes, M, N, torch.int16, exact=True), Guarded(planes, M, N, torch.int16, ld=N + 64)
                    _gemm_call(Ap.data_ptr(), M * K, K, Wp, M, N, K, planes, epi, bias, None, e.ptr(), e.plane, e.ld)
                    _gemm_call(A_ptr, a_plane, lda, Wp, M, N, K, planes, epi, bias, None, g.ptr(), g.plane, g.ld)
                    got = planes_value(e.dense(), dt)
                torch.cuda.synchronize()
            assert e.guards_untouched() and g.guards_untouched(), what                                 # (a)
            assert torch.equal(g.dense(), e.dense()), what                                             # (b)
            got = got[rows]                                                                            # (c): the bars of the existing tests
            assert torch.isfinite(got).all(), what
            if epi == capi.EPI_PLAIN:            # test_gemm_plain
                assert maxerr(got, base.float()) <= (2e-6 if planes == 1 else 3e-5) * scale * math.sqrt(K / 64), what
                if planes == 2:
                    assert maxerr(got, exact.float()) <= 4e-5 * scale, what
            elif epi == capi.EPI_RESID and fmt == "bf16":         # test_gemm_epilogues
                assert torch.allclose(got, X0[rows] + base.float(), atol=2e-4, rtol=1e-5), what
            elif epi == capi.EPI_RESID and planes == 1:           # test_fp16_gpu.py::test_gemm_resid_and_gelu
                assert maxerr(got - X0[rows], base.float()) <= 3e-6 * scale * max(1.0, (K / 64) ** 0.5), what
            elif epi == capi.EPI_RESID:                           # test_fp16_gpu.py::test_gemm_hi_lo_planes_fp16: against the unsplit operands
                assert maxerr(got - X0[rows], exact.float()) <= 3e-6 * float(exact.abs().max()), what
            elif fmt == "bf16":                                   # test_gemm_epilogues
                want = O.gelu_erf(base.float().cpu()).cuda() if epi == capi.EPI_GELU else torch.relu(base.float())
                assert maxerr(got, want) <= (2.0 ** -8 if planes == 1 else 2.0 ** -15) * float(want.abs().max()) + 2e-4, what
            elif epi == capi.EPI_GELU and planes == 1:            # test_fp16_gpu.py::test_gemm_resid_and_gelu
                want = O.gelu_erf(base.float().cpu()).cuda()
                assert maxerr(got, want) <= 2.0 ** -11 * float(want.abs().max()) + 1e-4, what
            elif epi == capi.EPI_RELU:                            # test_fp16_gpu.py::test_gemm_hi_lo_planes_fp16
                assert maxerr(got, torch.relu(exact.float())) <= 3e-6 * float(exact.abs().max()) + 2.0 ** -24, what
            # (fp16 hi + lo GELU has no value test of its own to take a bar from: (a) and (b) only)
    del keepA


# ------------------------------------------------------------------------------------------------ Q / K / V scatters
def _qkv_guarded(planes, B, H, npad):
    return [Guarded(planes, B * H * npad, 64, torch.int16) for _ in range(3)]


def _qkv_check(bufs, exact, planes, B, H, ntok, npad, what=""):
    """(a) bands, pad rows ntok..npad still the guard pattern, in both layouts; (b) rows < ntok equal the exact-layout call's.  Returns
    the exact-layout q, k, v as [planes, B, H, npad, 64]"""
    dense = []
    for g, e in zip(bufs, exact):
        assert g.guards_untouched() and e.guards_untouched(), what
        got, want = (t.dense().reshape(planes, B, H, npad, 64) for t in (g, e))
        assert untouched(got[:, :, :, ntok:]) and untouched(want[:, :, :, ntok:]), f"{what}: pad rows written"
        assert torch.equal(got[:, :, :, :ntok], want[:, :, :, :ntok]), what
        dense.append(want)
    return dense


def _qkv_exact(planes, B, H, npad):
    return [Guarded(planes, B * H * npad, 64, torch.int16, exact=True) for _ in range(3)]


@pytest.mark.parametrize("B,ntok", [(1, 1), (1, 77), (2, 197), (3, 130)])
@pytest.mark.parametrize("big", [0, 2])
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_qkv_gemm_guarded_layout(cuda, fmt, planes, big, B, ntok):
    """dinoseg_op_qkv_gemm (gemm.hip and gemm_big.hip, EPI_QKV) with a_plane and qkv_plane larger than minimal; q / k / v start as the guard
    pattern, so "pad rows untouched" means still that pattern."""
    H = 6
    D, npad, M = H * 64, (ntok + 63) // 64 * 64, B * ntok
    dt = DT[fmt]
    A, W, bias = seeded((M, D), 5), seeded((3 * D, D), 6) * 0.1, seeded((3 * D,), 7)
    Ap, Wp = to_planes(A, dt, planes), to_planes(W, dt, planes)
    keepA, A_ptr, a_plane, _ = strided_planes(Ap, gap_rows=3)
    bufs, exact = _qkv_guarded(planes, B, H, npad), _qkv_exact(planes, B, H, npad)
    lib = capi.lib()
    with options(op_fmt=int(fmt == "fp16"), gemm_big=big):
        capi.check(lib.dinoseg_op_qkv_gemm(Ap.data_ptr(), M * D, Wp.data_ptr(), 3 * D * D, bias.data_ptr(), B, ntok, npad, H, planes, QSCALE,
                                           *[t.ptr() for t in exact], B * H * npad * 64, S()))
        capi.check(lib.dinoseg_op_qkv_gemm(A_ptr, a_plane, Wp.data_ptr(), 3 * D * D, bias.data_ptr(), B, ntok, npad, H, planes, QSCALE,
                                           *[g.ptr() for g in bufs], bufs[0].plane, S()))
        torch.cuda.synchronize()
    exact = _qkv_check(bufs, exact, planes, B, H, ntok, npad)
    ref = (planes_value(Ap, dt) @ planes_value(Wp, dt).t() + bias.double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    vdt = torch.bfloat16 if (fmt == "bf16" or planes == 1) else dt          # one fp16 plane: V stays bf16
    gq, gk, gv = (planes_value(t, d)[:, :, :ntok] for t, d in zip(exact, (dt, dt, vdt)))
    top = float(ref.abs().max())
    if fmt == "bf16":             # test_qkv_gemm_layout
        tq = tk = tv = (2.0 ** -8 if planes == 1 else 2.0 ** -15) * top + 1e-4
    elif planes == 1:             # test_fp16_gpu.py::test_qkv_layout_q_k_fp16_v_bf16 (its slack for the plain GEMM routes is 1)
        tq = tk = 2.0 ** -11 * top + 1e-4
        tv = 2.0 ** -8 * top + 1e-4
    else:                         # fp16 hi + lo: no value test of its own; the bf16 hi + lo bar holds a fortiori
        tq = tk = tv = 2.0 ** -15 * top + 1e-4
    assert maxerr(gq, ref[0] * QSCALE) <= tq and maxerr(gk, ref[1]) <= tk and maxerr(gv, ref[2]) <= tv
    del keepA


@pytest.mark.parametrize("B,ntok", [(1, 1), (1, 77), (2, 197), (3, 130)])
@pytest.mark.parametrize("fmt,planes", [("bf16", 1), ("bf16", 2), ("fp16", 1)])
def test_ln_gemm_qkv_guarded_layout(cuda, fmt, planes, B, ntok):
    """dinoseg_op_ln_gemm with EPI_QKV (gemm_ln.hip): qkv_plane larger than minimal, guard pattern in the pad rows and behind the last pair."""
    H, K = 6, 384
    D, npad, M = 384, (ntok + 63) // 64 * 64, B * ntok
    dt = DT[fmt]
    X = seeded((M, K), 21) * 2.0 - 0.3
    gam, bet = 1 + 0.2 * seeded((K,), 22), 0.1 * seeded((K,), 23)
    W, bias = seeded((3 * D, K), 24) * 0.1, seeded((3 * D,), 25)
    bufs, exact = _qkv_guarded(planes, B, H, npad), _qkv_exact(planes, B, H, npad)
    with options(op_fmt=int(fmt == "fp16")):
        Wp = pack_slabs(W, planes)
        for ptrs, plane in (([t.ptr() for t in exact], B * H * npad * 64), ([g.ptr() for g in bufs], bufs[0].plane)):
            capi.check(capi.lib().dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), 3 * D * K, bias.data_ptr(), M,
                                                     3 * D, K, planes, 4, None, 0, *ptrs, plane, ntok, npad, H, QSCALE, None, None, S()))
        torch.cuda.synchronize()
    exact = _qkv_check(bufs, exact, planes, B, H, ntok, npad)
    A = to_planes(_ln_ref(X, gam, bet).cuda(), dt, planes)
    ref = (planes_value(A, dt) @ planes_value(to_planes(W, dt, planes), dt).t() + bias.double()).float()
    ref = ref.reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    top = float(ref.abs().max())
    gq, gk, gv = (planes_value(t, d)[:, :, :ntok] for t, d in zip(exact, (dt, dt, torch.bfloat16)))
    if fmt == "bf16":             # test_ln_gemm_qkv_layout
        tq = tv = (2.0 ** -7 if planes == 1 else 2.0 ** -14) * top + 1e-4
    else:                         # test_fp16_gpu.py::test_qkv_layout_q_k_fp16_v_bf16, route ln_gemm
        tq, tv = 2.0 * 2.0 ** -11 * top + 1e-4, 2.0 ** -8 * top + 1e-4
    assert maxerr(gq, ref[0] * QSCALE) <= tq and maxerr(gk, ref[1]) <= tq and maxerr(gv, ref[2]) <= tv


@pytest.mark.parametrize("fmt,planes,M,N", [(f, p, m, n) for f, p in (("bf16", 1), ("bf16", 2)) for m, n in
                                            ((1, 768), (77, 640), (128 * 5 + 33, 768), (M_PERSISTENT, 640))] +
                         [("fp16", 1, 1, 768), ("fp16", 1, 77, 1536), ("fp16", 1, 128 * 5 + 33, 768), ("fp16", 1, M_PERSISTENT, 768)])
def test_ln_gemm_gelu_guarded_layout(cuda, fmt, planes, M, N):
    """dinoseg_op_ln_gemm with EPI_GELU: out_plane larger than minimal for the output and the pre-activation by-product (they share the
    stride); the normalised planes a_out, whose plane stride is M * K by contract, between two guard bands.  N = 640: a partial last column
    tile.  fp16 operands: the output only (the by-products of the training forward have no fp16 form)."""
    K = 384
    dt = DT[fmt]
    byp = fmt == "bf16"
    X = seeded((M, K), 11) * 1.7 + 0.4
    gam, bet = 1 + 0.2 * seeded((K,), 12), 0.1 * seeded((K,), 13)
    W, bias = seeded((N, K), 14) * 0.1, seeded((N,), 15)
    out, pre = Guarded(planes, M, N, torch.int16), Guarded(planes, M, N, torch.int16)
    aout = Guarded(planes, M, K, torch.int16, exact=True)
    e_out, e_pre, e_a = (Guarded(planes, M, n, torch.int16, exact=True) for n in (N, N, K))
    lib = capi.lib()
    with options(op_fmt=int(fmt == "fp16")):
        Wp = pack_slabs(W, planes)
        capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), N * K, bias.data_ptr(), M, N, K, planes,
                                          capi.EPI_GELU, e_out.ptr(), M * N, None, None, None, 0, 0, 0, 6, 0.0, e_a.ptr() if byp else None,
                                          e_pre.ptr() if byp else None, S()))
        capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), N * K, bias.data_ptr(), M, N, K, planes,
                                          capi.EPI_GELU, out.ptr(), out.plane, None, None, None, 0, 0, 0, 6, 0.0,
                                          aout.ptr() if byp else None, pre.ptr() if byp else None, S()))
        torch.cuda.synchronize()
    for t in (out, pre, aout, e_out, e_pre, e_a):
        assert t.guards_untouched()                                                                             # (a)
    e_out, e_pre, e_a = e_out.dense(), e_pre.dense(), e_a.dense()
    assert torch.equal(out.dense(), e_out)                                                                      # (b)
    rows = _ends(M)                                                                                             # (c)
    Wq = planes_value(to_planes(W, dt, planes), dt)
    if not byp:                   # test_fp16_gpu.py::test_ln_gemm_gelu
        assert untouched(pre.flat) and untouched(aout.flat)
        z = (planes_value(to_planes(_ln_ref(X[rows], gam, bet).cuda(), dt, 1), dt) @ Wq.t() + bias.double()).float()
        want = O.gelu_erf(z.cpu()).cuda()
        assert maxerr(planes_value(e_out, dt)[rows], want) <= 2.0 ** -10 * float(want.abs().max()) + 3e-4
        return
    assert torch.equal(pre.dense(), e_pre)
    assert torch.equal(aout.dense(), e_a)
    tol = 2.0 ** -8 if planes == 1 else 2.0 ** -15              # test_ln_gemm_gelu
    got_a = planes_value(e_a, dt)[rows]
    A = _ln_ref(X[rows], gam, bet).cuda()
    assert maxerr(got_a, A) <= tol * float(A.abs().max()) + 1e-5
    z = (got_a @ Wq.t() + bias.double()).float()
    assert maxerr(planes_value(e_pre, dt)[rows], z) <= tol * float(z.abs().max()) + 2e-4
    want = O.gelu_erf(z.cpu()).cuda()
    assert maxerr(planes_value(e_out, dt)[rows], want) <= tol * float(want.abs().max()) + 2e-4


# ------------------------------------------------------------------------------------------------ gemm_rs.hip (embed_dim 768)
def _qkv_rows(bufs, dts, B, H, ntok, npad):
    """q / k / v planes [planes][B, H, npad, 64] -> fp64 [B * ntok, 3 * H * 64] in the column order of the qkv projection"""
    cols = [planes_value(t.reshape(-1, B, H, npad, 64), d)[:, :, :ntok].permute(0, 2, 1, 3).reshape(B * ntok, H * 64) for t, d in zip(bufs, dts)]
    return torch.cat(cols, dim=1)


RS_SHAPES = [(1, 1), (1, 77), (1, 128 * 5 + 33), (103, 373)]          # B x ntok; 103 x 373 = 38 419 rows


@pytest.mark.parametrize("B,ntok", RS_SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_gemm_rs_guarded_layout(cuda, fmt, B, ntok):
    """dinoseg_op_gemm_rs with lda / ldo larger than minimal: the residual epilogue (N = 768, x in place between guard bands), GELU into
    out16 [M][ldo] and the Q / K / V scatter (guard pattern in the pad rows), K = 768."""
    H, D, F_ = 12, 768, 3072
    M, npad, fp16, dt = B * ntok, (ntok + 63) // 64 * 64, fmt == "fp16", DT[fmt]
    lib, rows = capi.lib(), _ends(B * ntok)
    A = seeded((M, D), 201) + torch.arange(D, device="cuda", dtype=torch.float32)[None, :] * 1e-4
    Ap, Aq = _one_plane(A, fp16)
    keepA, A_ptr, _, lda = strided_planes(Ap[None], ld=D + 64, gap_rows=0)
    Aq = Aq.double()[rows]
    Wr, br = seeded((D, D), 202) * 0.05 + torch.arange(D, device="cuda", dtype=torch.float32)[:, None] * 1e-5, seeded((D,), 203)
    W1, b1 = seeded((F_, D), 212) * 0.04 + torch.arange(F_, device="cuda", dtype=torch.float32)[:, None] * 1e-6, seeded((F_,), 213) * 0.5
    Wq_, bq = seeded((3 * D, D), 222) * 0.05, seeded((3 * D,), 223)
    X0 = seeded((M, D), 204) * 2.0
    with options(op_fmt=int(fp16)):
        Wrp, W1p, Wqp = _pack_rs(Wr, 1), _pack_rs(W1, 0), _pack_rs(Wq_, 0)
        # residual
        e_x, g_x = Guarded(1, M, D, torch.float32, exact=True).fill(X0), Guarded(1, M, D, torch.float32).fill(X0)
        for a, ld, x in ((Ap.data_ptr(), D, e_x.ptr()), (A_ptr, lda, g_x.ptr())):
            capi.check(lib.dinoseg_op_gemm_rs(a, ld, Wrp.data_ptr(), br.data_ptr(), M, D, D, capi.EPI_RESID, x, None, 0, None, None, None, 0, 0, 0, 0.0, S()))
        # GELU
        e_h, g_h = Guarded(1, M, F_, torch.int16, exact=True), Guarded(1, M, F_, torch.int16, ld=F_ + 64)
        for a, ld, o, ldo in ((Ap.data_ptr(), D, e_h.ptr(), F_), (A_ptr, lda, g_h.ptr(), g_h.ld)):
            capi.check(lib.dinoseg_op_gemm_rs(a, ld, W1p.data_ptr(), b1.data_ptr(), M, F_, D, capi.EPI_GELU, None, o, ldo, None, None, None, 0, 0, 0, 0.0, S()))
        # Q / K / V
        bufs, exact = _qkv_guarded(1, B, H, npad), _qkv_exact(1, B, H, npad)
        for a, ld, ptrs in ((Ap.data_ptr(), D, [t.ptr() for t in exact]), (A_ptr, lda, [g.ptr() for g in bufs])):
            capi.check(lib.dinoseg_op_gemm_rs(a, ld, Wqp.data_ptr(), bq.data_ptr(), M, 3 * D, D, 4, None, None, 0, *ptrs, ntok, npad, H, QSCALE, S()))
        torch.cuda.synchronize()
    for t in (g_x, g_h, e_x, e_h):
        assert t.guards_untouched()                                                             # (a)
    e_x, e_h = e_x.dense()[0], e_h.dense()
    assert torch.equal(g_x.dense()[0], e_x) and torch.equal(g_h.dense(), e_h)                   # (b)
    exact = _qkv_check(bufs, exact, 1, B, H, ntok, npad)
    q1 = lambda t: _q1(t, fp16).double()
    delta = Aq @ q1(Wr).t() + br.double()                                                       # (c) test_gemm_rs_residual
    assert maxerr(e_x[rows], X0[rows].double() + delta) <= 2e-6 * float(delta.abs().max()) * math.sqrt(D / 64) + 1e-5
    z = Aq @ q1(W1).t() + b1.double()                                                           # test_gemm_rs_gelu
    want = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    got = planes_value(e_h, dt)[rows]
    assert torch.isfinite(got).all()
    assert float(((got - want).abs() - (2.0 ** -11 if fp16 else 2.0 ** -8) * want.abs()).max()) <= 1e-4
    ref = Aq @ q1(Wq_).t() + bq.double()                                                        # test_gemm_rs_qkv_layout
    ref[:, :D] *= QSCALE
    gqkv = _qkv_rows(exact, (dt, dt, torch.bfloat16), B, H, ntok, npad)[rows]
    tol = lambda r, d: (2.0 ** -11 if d == torch.float16 else 2.0 ** -8) * float(r.abs().max()) + 1e-4
    for i, d in enumerate((dt, dt, torch.bfloat16)):
        assert maxerr(gqkv[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D]) <= tol(ref[:, i * D:(i + 1) * D], d), i
    del keepA


@pytest.mark.parametrize("B,ntok", RS_SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_ln_gemm_rs_guarded_layout(cuda, fmt, B, ntok):
    """dinoseg_op_ln_gemm_rs (the LayerNorm inside the launch; it has the GELU and the Q / K / V epilogues): ldo larger than minimal, the
    guard pattern around q / k / v and in their pad rows."""
    H, D, F_ = 12, 768, 3072
    M, npad, fp16, dt = B * ntok, (ntok + 63) // 64 * 64, fmt == "fp16", DT[fmt]
    lib, rows = capi.lib(), _ends(B * ntok)
    X = seeded((M, D), 231) * 1.6 + 0.3 + torch.arange(D, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    X[:, 7] += 25.0
    gam, bet = 1 + 0.2 * seeded((D,), 232), 0.1 * seeded((D,), 233)
    Wq_, bq = seeded((3 * D, D), 234) * 0.05, seeded((3 * D,), 235)
    W1, b1 = seeded((F_, D), 236) * 0.04, seeded((F_,), 237) * 0.5
    with options(op_fmt=int(fp16)):
        fold = {}
        for name, W_, b_ in (("q", Wq_, bq), ("1", W1, b1)):
            wf, bf = torch.empty((W_.numel(),), dtype=torch.int16, device="cuda"), torch.empty((W_.shape[0],), device="cuda")
            capi.check(lib.dinoseg_op_pack_rs_ln(W_.data_ptr(), gam.data_ptr(), bet.data_ptr(), b_.data_ptr(), W_.shape[0], D, wf.data_ptr(), bf.data_ptr(), S()))
            fold[name] = (wf, bf)
        e_h, g_h = Guarded(1, M, F_, torch.int16, exact=True), Guarded(1, M, F_, torch.int16, ld=F_ + 64)
        for o, ldo in ((e_h.ptr(), F_), (g_h.ptr(), g_h.ld)):
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 1e-6, fold["1"][0].data_ptr(), fold["1"][1].data_ptr(), M, F_, D, capi.EPI_GELU, o, ldo,
                                                 None, None, None, 0, 0, 0, 0.0, S()))
        bufs, exact = _qkv_guarded(1, B, H, npad), _qkv_exact(1, B, H, npad)
        for ptrs in ([t.ptr() for t in exact], [g.ptr() for g in bufs]):
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 1e-6, fold["q"][0].data_ptr(), fold["q"][1].data_ptr(), M, 3 * D, D, 4, None, 0, *ptrs,
                                                 ntok, npad, H, QSCALE, S()))
        torch.cuda.synchronize()
    assert g_h.guards_untouched() and e_h.guards_untouched()                                   # (a)
    e_h = e_h.dense()
    assert torch.equal(g_h.dense(), e_h)                                                       # (b)
    exact = _qkv_check(bufs, exact, 1, B, H, ntok, npad)
    # (c) test_ln_gemm_rs: fp64 on the operands the kernel sees
    x64 = X.double()[rows]
    mu = x64.mean(dim=1, keepdim=True)
    xhat = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
    Aq = _q1(xhat.float(), fp16).double()
    ulp = 2.0 ** -10 if fp16 else 2.0 ** -7
    tol = lambda r, e: 3 * e * float(r.abs().max()) + 1e-4
    ref = Aq @ _q1(Wq_ * gam[None, :], fp16).double().t() + fold["q"][1].double()
    ref[:, :D] *= QSCALE
    gqkv = _qkv_rows(exact, (dt, dt, torch.bfloat16), B, H, ntok, npad)[rows]
    for i, e in enumerate((ulp, ulp, 2.0 ** -7)):
        assert maxerr(gqkv[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D]) <= tol(ref[:, i * D:(i + 1) * D], e), i
    z1 = Aq @ _q1(W1 * gam[None, :], fp16).double().t() + fold["1"][1].double()
    want1 = 0.5 * z1 * (1.0 + torch.erf(z1 / math.sqrt(2.0)))
    d1 = (planes_value(e_h, dt)[rows] - want1).abs()
    assert float(d1.max()) <= tol(want1, ulp) and float(d1.mean()) <= 0.25 * ulp * float(want1.abs().mean()) + 1e-5


# ------------------------------------------------------------------------------------------------ the fused projection + MLP launches
def _fused_ref(kind, c, X, ctx_val, fp16):
    """fp64 on the operands the kernel sees, rows of X (and of ctx_val, or None = the MLP half only): (x after the projection, MLP term).
    kind 2: mlp_fused2.hip (one plane, LayerNorm output rounded); 3: mlp_fused3.hip (hi + lo planes); 4: mlp_fused4.hip (one plane,
    (x - mean) rstd rounded, the LayerNorm folded into W1 / b1)"""
    q = (lambda t: _split_planes(t, fp16)[1].double()) if kind == 3 else (lambda t: _q1(t, fp16).double())
    xmid = X.double()
    if ctx_val is not None:
        xmid = xmid + ctx_val.double() @ q(c["Wpr"]).t() + c["bpr"].double()
    if kind == 4:
        mu = xmid.mean(dim=1, keepdim=True)
        xhat = (xmid - mu) / torch.sqrt(((xmid - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
        z = q(xhat.float()) @ q(c["W1"] * c["gam"][None, :]).t() + (c["b1"].double() + c["W1"].double() @ c["bet"].double())
    else:
        z = q(_ln_ref(xmid.float(), c["gam"], c["bet"]).cuda()) @ q(c["W1"]).t() + c["b1"].double()
    g = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))) if kind == 3 else O.gelu_erf(z.float().cpu()).cuda()
    return xmid, q(g.float()) @ q(c["W2"]).t() + c["b2"].double()


FUSED_SHAPES = [(1, 1), (1, 77), (1, 128 * 5 + 33), (103, 373)]       # B x ntok: 1, 77, 673 and 38 419 rows (more items than workgroups)


@pytest.mark.parametrize("B,ntok", FUSED_SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_fused2_guarded_layout(cuda, fmt, B, ntok):
    """mlp_fused2.hip: dinoseg_op_mlp_fused, dinoseg_op_proj_mlp_fused, dinoseg_op_block_tail_fused.  X is updated in place between guard
    bands; q / k / v carry the guard pattern in their pad rows and around them.  (The entries take no strides: ld = 384.)"""
    D_, F_, H = 384, 1536, 6
    M, npad, fp16, dt = B * ntok, (ntok + 63) // 64 * 64, fmt == "fp16", DT[fmt]
    lib, rows = capi.lib(), _ends(B * ntok)
    c = _mlp3_case(M, fp16, 640, tail=True)
    ctx_i, ctx_v = _one_plane(c["ctx"], fp16)
    res = {}
    with options(op_fmt=int(fp16)):
        Wp = pack_mlp(c["W1"], c["W2"])
        Wprp = torch.empty((lib.dinoseg_op_proj_pack_elems(D_),), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_pack_proj(c["Wpr"].data_ptr(), D_, Wprp.data_ptr(), S()))
        Wqp = torch.empty((lib.dinoseg_op_qkv_pack_elems(D_),), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_pack_qkv(c["Wqkv"].data_ptr(), D_, Wqp.data_ptr(), S()))
        p = lambda *names: [c[n].data_ptr() for n in names]
        for guarded in (False, True):
            xs = [Guarded(1, M, D_, torch.float32, exact=not guarded).fill(c["X"]) for _ in range(3)]
            xp = [x.ptr() for x in xs]
            qkv = _qkv_guarded(1, B, H, npad) if guarded else _qkv_exact(1, B, H, npad)
            capi.check(lib.dinoseg_op_mlp_fused(xp[0], *p("gam", "bet"), 1e-6, Wp.data_ptr(), *p("b1", "b2"), M, D_, F_, S()))
            capi.check(lib.dinoseg_op_proj_mlp_fused(xp[1], ctx_i.data_ptr(), Wprp.data_ptr(), *p("bpr", "gam", "bet"), 1e-6, Wp.data_ptr(), *p("b1", "b2"),
                                                     M, D_, F_, S()))
            capi.check(lib.dinoseg_op_block_tail_fused(xp[2], ctx_i.data_ptr(), Wprp.data_ptr(), *p("bpr", "gam", "bet"), 1e-6, Wp.data_ptr(),
                                                       *p("b1", "b2"), Wqp.data_ptr(), *p("bq", "gam1", "bet1"),
                                                       *[t.ptr() for t in qkv], B, ntok, npad, H, QSCALE, D_, F_, S()))
            res[guarded] = (xs, qkv)
        torch.cuda.synchronize()
    (ex, eqkv), (gx, gqkv) = res[False], res[True]
    for e, g in zip(ex, gx):
        assert g.guards_untouched() and e.guards_untouched() and torch.equal(g.dense(), e.dense())          # (a), (b)
    ex = [e.dense()[0] for e in ex]
    eqkv = _qkv_check(gqkv, eqkv, 1, B, H, ntok, npad)
    assert torch.equal(ex[2], ex[1])                        # test_block_tail_fused: the tail leaves X as the launch without it
    bar = 2.0 ** -11 if fp16 else 2.0 ** -9                 # (c) test_mlp_fused / test_proj_mlp_fused / test_fp16_gpu.py::test_proj_mlp_fused
    for i, ctxv in ((0, None), (1, ctx_v[rows])):
        xmid, delta = _fused_ref(2, c, c["X"][rows], ctxv, fp16)
        scale = float(delta.abs().max())
        assert torch.isfinite(ex[i]).all()
        assert maxerr(ex[i][rows], (xmid + delta).float()) <= bar * scale + 1e-3, i
    if not fp16:                                            # test_block_tail_fused (bf16; the fp16 tail has no bar of its own: (a), (b) only)
        A = _q1(_ln_ref(ex[2][rows], c["gam1"], c["bet1"]).cuda(), False).double()
        ref = A @ _q1(c["Wqkv"], False).double().t() + c["bq"].double()
        tol = 2.0 ** -7 * float(ref.float().abs().max()) + 1e-4
        ref[:, :D_] *= QSCALE
        got = _qkv_rows(eqkv, (dt, dt, dt), B, H, ntok, npad)[rows]
        assert maxerr(got, ref) <= tol


@pytest.mark.parametrize("B,ntok", FUSED_SHAPES)
@pytest.mark.parametrize("fmt,v_bf16", [("bf16", 0), ("fp16", 0), ("fp16", 1)])
def test_fused3_guarded_layout(cuda, fmt, v_bf16, B, ntok):
    """mlp_fused3.hip (hi + lo planes): dinoseg_op_proj_mlp_fused3 with and without the projection and dinoseg_op_block_tail_fused3, with
    ctx_plane and qkv_plane larger than minimal and finite garbage between the ctx planes."""
    D_, F_, H = 384, 1536, 6
    M, npad, fp16, dt = B * ntok, (ntok + 63) // 64 * 64, fmt == "fp16", DT[fmt]
    lib, rows = capi.lib(), _ends(B * ntok)
    c = _mlp3_case(M, fp16, 170, tail=True)
    ctx_pl, ctx_v = _split_planes(c["ctx"], fp16)
    keepC, C_ptr, c_plane, _ = strided_planes(ctx_pl, gap_rows=3)
    p = lambda *names: [c[n].data_ptr() for n in names]
    res = {}
    for guarded in (False, True):
        xs = [Guarded(1, M, D_, torch.float32, exact=not guarded).fill(c["X"]) for _ in range(3)]
        xp = [x.ptr() for x in xs]
        qkv = _qkv_guarded(2, B, H, npad) if guarded else _qkv_exact(2, B, H, npad)
        cp, cpl = (C_ptr, c_plane) if guarded else (ctx_pl.data_ptr(), M * D_)
        qpl = qkv[0].plane if guarded else B * H * npad * 64
        capi.check(lib.dinoseg_op_proj_mlp_fused3(xp[0], None, M * D_, c["bpr"].data_ptr(), 1e-6, c["Wp"].data_ptr(), c["b2"].data_ptr(), M, D_, F_, int(fp16), S()))
        capi.check(lib.dinoseg_op_proj_mlp_fused3(xp[1], cp, cpl, c["bpr"].data_ptr(), 1e-6, c["Wp"].data_ptr(), c["b2"].data_ptr(), M, D_, F_, int(fp16), S()))
        capi.check(lib.dinoseg_op_block_tail_fused3(xp[2], cp, cpl, c["bpr"].data_ptr(), 1e-6, c["Wp"].data_ptr(), c["b2"].data_ptr(),
                                                    *[t.ptr() for t in qkv], qpl, B, ntok, npad, H, QSCALE, v_bf16,
                                                    D_, F_, int(fp16), S()))
        res[guarded] = (xs, qkv)
    torch.cuda.synchronize()
    (ex, eqkv), (gx, gqkv) = res[False], res[True]
    for e, g in zip(ex, gx):
        assert g.guards_untouched() and e.guards_untouched() and torch.equal(g.dense(), e.dense())          # (a), (b)
    ex = [e.dense()[0] for e in ex]
    eqkv = _qkv_check(gqkv, eqkv, 2, B, H, ntok, npad)
    assert torch.equal(ex[2], ex[1])                        # test_block_tail_fused_hi_lo_planes
    for i, ctxv in ((0, None), (1, ctx_v[rows])):           # (c) test_proj_mlp_fused_hi_lo_planes
        xmid, delta = _fused_ref(3, c, c["X"][rows], ctxv, fp16)
        scale = float(delta.abs().max())
        assert torch.isfinite(ex[i]).all()
        assert maxerr(ex[i][rows], (xmid + delta).float()) <= (2.0e-5 if fp16 else 6.0e-5) * scale + 1e-5, i
    q2 = lambda t: _split_planes(t, fp16)[1].double()       # test_block_tail_fused_hi_lo_planes
    z = q2(_ln_ref(ex[2][rows], c["gam1"], c["bet1"]).cuda()) @ q2(c["Wqkv"]).t() + c["bq"].double()
    top = float(z.float().abs().max())
    z[:, :D_] *= QSCALE
    vdt = torch.bfloat16 if (v_bf16 or not fp16) else torch.float16
    got = _qkv_rows(eqkv, (dt, dt, vdt), B, H, ntok, npad)[rows]
    tol = (2.0 ** -18 if fp16 else 2.0 ** -14) * top + 2e-5
    for i, t in enumerate((tol, tol, tol if (fp16 and not v_bf16) else 2.0 ** -14 * top + 2e-5)):
        assert maxerr(got[:, i * D_:(i + 1) * D_], z.float()[:, i * D_:(i + 1) * D_]) <= t, i
    del keepC


@pytest.mark.parametrize("B,ntok", FUSED_SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_fused4_guarded_layout(cuda, fmt, B, ntok):
    """mlp_fused4.hip (one wave per SIMD): dinoseg_op_proj_mlp_fused4 and dinoseg_op_block_tail_fused4; X in place between guard bands,
    q / k / v with the guard pattern in their pad rows and around them.  (The entries take no strides.)"""
    D_, F_, H = 384, 1536, 6
    M, npad, fp16, dt = B * ntok, (ntok + 63) // 64 * 64, fmt == "fp16", DT[fmt]
    lib, rows = capi.lib(), _ends(B * ntok)
    c = _mlp3_case(M, fp16, 470, tail=True)
    ctx_i, ctx_v = _one_plane(c["ctx"], fp16)
    Wp = _pack_mlp4(c["Wpr"], c["W1"], c["b1"], c["W2"], c["gam"], c["bet"], fp16, tail=(c["Wqkv"], c["bq"], c["gam1"], c["bet1"]))
    res = {}
    for guarded in (False, True):
        xs = [Guarded(1, M, D_, torch.float32, exact=not guarded).fill(c["X"]) for _ in range(2)]
        xp = [x.ptr() for x in xs]
        qkv = _qkv_guarded(1, B, H, npad) if guarded else _qkv_exact(1, B, H, npad)
        capi.check(lib.dinoseg_op_proj_mlp_fused4(xp[0], ctx_i.data_ptr(), c["bpr"].data_ptr(), 1e-6, Wp.data_ptr(), c["b2"].data_ptr(), M, D_, F_, int(fp16), S()))
        capi.check(lib.dinoseg_op_block_tail_fused4(xp[1], ctx_i.data_ptr(), c["bpr"].data_ptr(), 1e-6, Wp.data_ptr(), c["b2"].data_ptr(),
                                                    *[t.ptr() for t in qkv], B, ntok, npad, H, QSCALE, D_, F_, int(fp16), S()))
        res[guarded] = (xs, qkv)
    torch.cuda.synchronize()
    (ex, eqkv), (gx, gqkv) = res[False], res[True]
    for e, g in zip(ex, gx):
        assert g.guards_untouched() and e.guards_untouched() and torch.equal(g.dense(), e.dense())          # (a), (b)
    ex = [e.dense()[0] for e in ex]
    eqkv = _qkv_check(gqkv, eqkv, 1, B, H, ntok, npad)
    assert torch.equal(ex[1], ex[0])                        # test_block_tail_fused_one_wave
    xmid, delta = _fused_ref(4, c, c["X"][rows], ctx_v[rows], fp16)         # (c) test_proj_mlp_fused_one_wave
    assert torch.isfinite(ex[0]).all()
    assert maxerr(ex[0][rows], (xmid + delta).float()) <= 2.0 ** -9 * float(delta.abs().max()) + 1e-3
    xo = ex[1].double()[rows]                               # test_block_tail_fused_one_wave
    mu = xo.mean(dim=1, keepdim=True)
    xhat = (xo - mu) / torch.sqrt(((xo - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
    z = _q1(xhat.float(), fp16).double() @ _q1(c["Wqkv"] * c["gam1"][None, :], fp16).double().t() + (c["bq"].double() + c["Wqkv"].double() @ c["bet1"].double())
    z = z.float().double()
    z[:, :D_] *= QSCALE
    got = _qkv_rows(eqkv, (dt, dt, torch.bfloat16), B, H, ntok, npad)[rows]
    ulp = 2.0 ** -10 if fp16 else 2.0 ** -7
    for i, e in enumerate((ulp, ulp, 2.0 ** -7)):
        r = z[:, i * D_:(i + 1) * D_]
        assert maxerr(got[:, i * D_:(i + 1) * D_], r) <= 3 * e * float(r.abs().max()) + 1e-4, i
