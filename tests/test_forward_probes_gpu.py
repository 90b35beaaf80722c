"""Stage-by-stage probes of the fused forward kernels mlp_fused2/3/4.hip (every probe), and of the 16-bit epilogues of the stand-alone GEMMs gemm.hip,
gemm_big.hip, gemm_ln.hip, gemm_ln12.hip and gemm_rs.hip with W = 0 (probes 1, 2 and 6 only: the K loop of those kernels adds nothing here).

Which probe reaches which kernel:
  probes 1, 2, 6    mlp_fused2/3/4.hip (FUSED) and the GELU / ReLU epilogues of the eight GEMMS kinds (W = 0, the probe in the bias; probe 6 also
                    through the fc1 product of gemm_ln12.hip, gemm_ln.hip and gemm_rs.hip's LayerNorm route, and the Q / K / V stores of the qkv tails,
                    gemm_ln12.hip and gemm_rs.hip)
  probes 3, 4       mlp_fused2/3/4.hip only
  probe 5           mlp_fused2/3/4.hip and their qkv tails (TAILS) only
The K loops and the scatter epilogues of the stand-alone GEMMs are held per element by tests/test_gemm_probes_gpu.py (probes G1 to G3), with the
builders this file shares with it through tests/probe_util.py.

tests/test_ops_gpu.py and tests/test_fp16_gpu.py hold these launches to one bound scaled by the largest output, on seeded normal data: the
16-bit roundings inside a fused launch sit at points its own fp32 noise moves.  Here every stage but one is made EXACT by the weights
(tests/probe_util.py), so that one stage can be held element by element:

  1. GELU: W1 = 0 and b1 = probe, W2 a 0 / 1 selector, X = 0: the output row IS the stored hidden activation.  Range (clamp at +-8, both
     tails), every hidden unit = every (tile, accumulator element, lane half), rows bit-identical, the value one number of the format.
  2. Store rounding: probes >= 8 (where both GELU forms return x itself) on ties of the output format and next to them.
  3. fc2: h known exactly, operands exact in the format (as hi + lo on two planes), fp64 reference on those operands.
  4. Projection: the MLP switched off (adds b2 only).
  5. LayerNorm + fc1: rows of +-1 (their LayerNorm is the row), block-sparse exact W1, selector W2.
  6. fp16 saturation at +-65504 wherever the source promises it (pack2_sat, split2<FMT, true>, OP_SAT, the Q / K stores of the qkv tails and
     QKV epilogues); the documented limit where it does not.

Bounds.  E_formula is the formula's own error on the probe points (tests/test_gelu_formula_cpu.py: 2.55e-5 fast form, 2.1e-7 erf form),
E_eval the fp32 evaluation noise derived instruction by instruction in probe_util.e_eval_fast / e_eval_erf (U = 2^-24 per rounding,
v_exp_f32 and v_rcp_f32 one ulp), half_ulp what round-to-nearest may lose in the stored format.  A GEMM stage is held to
c U sum |terms| with c = 4 sqrt(n) + 8 (probe_util.sum_bound) against fp64 on the operands the kernel multiplies, the lo x lo products
that the two-plane kernels drop by design taken out of the reference exactly.  Nothing is fitted to an output.

Which GELU a kernel runs, read from the sources: one plane = gelu_fast (gemm.hip:201, gemm_big.hip:370, gemm_ln12.hip:201, gemm_rs.hip
gelu_op, mlp_fused2.hip and mlp_fused4.hip gelu_op), two planes = gelu_erf (gemm.hip, gemm_big.hip, gemm_ln.hip:283; mlp_fused3.hip
restates it as max(x, 0) - |x| P t E / 2).

mlp_fused2.hip and gemm_ln12.hip hand the bias to the accumulator as three 16-bit pieces times a ones fragment: exact for bf16 (3 x 8
bits) and for fp16 down to its subnormal grid, 2^-24 -- an fp16 bias loses at most 2^-25 (pre_err below, times |gelu'| <= 1.13), and
a bias beyond 65504 cannot be given at all: there the saturation probe reaches 76 800 through the fc1 product instead.
"""
import math

import numpy as np
import pytest
import torch

from dino_amd import capi, options
from tests import probe_util as P
from tests.probe_util import GEMMS, NAN16, banded, block_sparse_w1, exact_operand, ln_fc1_case, planes_of, stored, unplane      # (shared with test_gemm_probes_gpu.py)

pytestmark = pytest.mark.gpu

S = capi.stream_ptr
D, F = P.D, P.F
LOG2E = 1.4426950408889634
MS = (33, 77, 129, 673)
FUSED = ("mlp2", "proj2", "mlp3", "proj3", "mlp4", "proj4")
# Does the GELU output of the launch saturate at the fp16 range?  mlp_fused3.hip does (OP_SAT).  mlp_fused2.hip and mlp_fused4.hip pack it with
# the plain pack2<FMT>: an fp16 pre-activation beyond 65504 becomes inf there and 0 x inf = NaN spreads along the row.  The saturating pack was
# built and measured (profiles/fused_gelu_saturation_ab.md: -0.46 % frames/s on the headline, outside the parent's spread) and not kept; the limit
# is stated next to dinoseg_op_mlp_fused in include/dinoseg.h and in DESIGN.md, and these two kernels are probed up to 65504 only.
GELU_SATURATES = {"mlp2": False, "proj2": False, "mlp3": True, "proj3": True, "mlp4": False, "proj4": False}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.float32, device="cuda")


def i16(*shape):
    return torch.zeros(shape, dtype=torch.int16, device="cuda")


def one_plane(x, fp16):
    return x.to(P.tdtype(fp16)).contiguous().view(torch.int16)


def two_planes(x, fp16):
    dt = P.tdtype(fp16)
    hi = x.to(dt)
    return torch.stack([hi, (x - hi.float()).to(dt)]).contiguous().view(torch.int16)


def pre_err(kind, fp16):
    """what the pre-activation may differ from the fp32 bias by (module docstring)"""
    return 2.0 ** -25 if fp16 and kind in ("mlp2", "proj2", "ln_gemm-1") else 0.0


# ------------------------------------------------------------------------------------------------ the fused launches
def run_fused(kind, fp16, X, W1, b1, W2, b2, eps=1e-6, ctx=None, Wpr=None, bpr=None):
    """X += [ctx Wpr^T + bpr;]  X += fc2(gelu(fc1(LayerNorm(X)))) with gamma = 1, beta = 0, through the entry `kind` names; fp32 device tensors in,
    the updated copy of X out.  proj* with ctx = None: a zero ctx, a zero Wproj and a zero bproj."""
    lib = capi.lib()
    M = X.shape[0]
    out = X.clone()
    gam, bet = torch.ones(D, device="cuda"), zeros(D)
    proj = kind.startswith("proj")
    if proj:
        ctx = zeros(M, D) if ctx is None else ctx
        Wpr = zeros(D, D) if Wpr is None else Wpr
        bpr = zeros(D) if bpr is None else bpr
    if kind in ("mlp2", "proj2"):
        with options(op_fmt=fp16):
            Wp = i16(lib.dinoseg_op_mlp_fused_pack_elems(D, F))
            capi.check(lib.dinoseg_op_pack_mlp(W1.data_ptr(), W2.data_ptr(), D, F, Wp.data_ptr(), S()))
            if proj:
                Wq = i16(lib.dinoseg_op_proj_pack_elems(D))
                capi.check(lib.dinoseg_op_pack_proj(Wpr.data_ptr(), D, Wq.data_ptr(), S()))
                c16 = one_plane(ctx, fp16)
                capi.check(lib.dinoseg_op_proj_mlp_fused(out.data_ptr(), c16.data_ptr(), Wq.data_ptr(), bpr.data_ptr(), gam.data_ptr(), bet.data_ptr(), eps,
                                                         Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(), M, D, F, S()))
            else:
                capi.check(lib.dinoseg_op_mlp_fused(out.data_ptr(), gam.data_ptr(), bet.data_ptr(), eps, Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(),
                                                    M, D, F, S()))
            torch.cuda.synchronize()
    elif kind in ("mlp3", "proj3"):
        Wp = i16(lib.dinoseg_op_mlp3_pack_elems(D, F))
        Wz = Wpr if proj else zeros(D, D)
        capi.check(lib.dinoseg_op_pack_mlp3(Wz.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), gam.data_ptr(), bet.data_ptr(), None, None,
                                            None, None, D, F, int(fp16), Wp.data_ptr(), S()))
        c16 = two_planes(ctx, fp16) if proj else None
        bz = bpr if proj else zeros(D)
        capi.check(lib.dinoseg_op_proj_mlp_fused3(out.data_ptr(), c16.data_ptr() if proj else None, M * D, bz.data_ptr(), eps, Wp.data_ptr(),
                                                  b2.data_ptr(), M, D, F, int(fp16), S()))
        torch.cuda.synchronize()
    else:
        Wp = i16(lib.dinoseg_op_mlp4_pack_elems(D, F))
        capi.check(lib.dinoseg_op_pack_mlp4(Wpr.data_ptr() if proj else None, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), gam.data_ptr(),
                                            bet.data_ptr(), None, None, None, None, D, F, int(fp16), Wp.data_ptr(), S()))
        c16 = one_plane(ctx, fp16) if proj else None
        capi.check(lib.dinoseg_op_proj_mlp_fused4(out.data_ptr(), c16.data_ptr() if proj else None, bpr.data_ptr() if proj else None, eps,
                                                  Wp.data_ptr(), b2.data_ptr(), M, D, F, int(fp16), S()))
        torch.cuda.synchronize()
    return out


_SEL = {}


def selector(s):
    if s not in _SEL:
        _SEL[s] = dev(P.selector(s))
    return _SEL[s]


def hidden_through_selectors(kind, fp16, M, b1, W1=None, X=None, eps=1e-6):
    """the stored hidden activation of every row, [M, 1536] fp64 on the host: four launches, W2 = selector s, b2 = 0; out - X is exact in fp32 for
    X = 0 and for X = +-1 with |h| >= 8 in [8, 2^15) (h has at most 22 significant bits)"""
    X = zeros(M, D) if X is None else X
    W1 = zeros(F, D) if W1 is None else W1
    cols = []
    for s in range(4):
        out = run_fused(kind, fp16, X, W1, b1, selector(s), zeros(D), eps=eps)
        cols.append((out.double() - X.double()).cpu())
    return torch.cat(cols, dim=1)


def check_gelu_values(name, h, x, fp16, planes, erf, perr, residual=0.0, fused3=False):
    """h [n] fp64: the stored GELU of the pre-activations x [n] (fp32 values as fp64).  residual: |X| of a row the launch added h to in fp32
    (h was read back as out - X: one more rounding, U (|X| + |h|), and no longer a number of the format).  fused3: the erf form as
    mlp_fused3.hip restates it, with the constants that kernel holds"""
    pts = P.probe_points()
    formula = (P.gelu_erf64_fused3 if fused3 else P.gelu_erf64) if erf else P.gelu_fast64
    e_formula = float(np.abs(formula(pts) - P.gelu_exact(pts)).max())
    ref, f64 = P.gelu_exact(x), formula(x)
    e_eval = (P.e_eval_erf if erf else P.e_eval_fast)(x) + 1.13 * perr + (P.U * (residual + np.abs(ref)) if residual else 0.0)
    assert np.isfinite(h).all(), name
    if not residual:
        assert bool(P.representable(torch.from_numpy(h).float(), fp16, planes).all()), f"{name}: a stored value is not a number of the format"
    err = np.abs(h - ref)
    bound = e_formula + e_eval + P.half_ulp(np.abs(ref) + e_formula + e_eval, fp16, planes)
    # sharper: against the formula the kernel evaluates -- no E_formula
    err_f = np.abs(h - f64)
    bound_f = e_eval + P.half_ulp(np.abs(f64) + e_eval, fp16, planes)
    i, j = int(np.argmax(err - bound)), int(np.argmax(err_f - bound_f))
    print(f"{name}: worst against gelu: x = {x[i]:.6g} |err| {err[i]:.3e} bound {bound[i]:.3e}; against the formula: x = {x[j]:.6g} "
          f"|err| {err_f[j]:.3e} bound {bound_f[j]:.3e}")
    assert (err <= bound).all(), (name, x[i], h[i], ref[i], err[i], bound[i])
    assert (err_f <= bound_f).all(), (name, x[j], h[j], f64[j], err_f[j], bound_f[j])
    big = x >= 8.0
    want = stored(x[big], fp16, planes)
    assert (h[big] == want).all(), (name, x[big][h[big] != want][:4], h[big][h[big] != want][:4])


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", FUSED)
def test_gelu_probe_fused(cuda, kind, fp16):
    """Probe 1 on the three fused kernels, with and without the (zero) projection in front."""
    vecs = P.gelu_probe_vectors()
    planes, erf = planes_of(kind), kind.endswith("3")
    first = None
    for M in MS:
        hs = []
        for v in vecs:
            h = hidden_through_selectors(kind, fp16, M, dev(v))
            assert torch.equal(h, h[0:1].expand_as(h)), f"{kind} M={M}: rows differ from row 0"
            hs.append(h[0].numpy())
        hs = np.stack(hs)
        if first is None:
            first = hs
        assert np.array_equal(first, hs, equal_nan=True), f"{kind}: M={M} differs from M={MS[0]}"
    check_gelu_values(f"{kind}-{'fp16' if fp16 else 'bf16'}", first.reshape(-1), vecs.astype(np.float64).reshape(-1), fp16, planes, erf,
                      pre_err(kind, fp16), fused3=erf)


# ------------------------------------------------------------------------------------------------ the GEMM epilogues
def run_epilogue(kind, fp16, M, bias, epi=capi.EPI_GELU, X=None, W=None):
    """act(A W^T + bias) through the 16-bit epilogue `kind` names, N = 1536: int16 planes [planes, M, N].  Default A = 0, W = 0: the pre-activation
    is the bias.  X / W (ln_gemm*, the saturation probe): fp32 rows for the LayerNorm inside the launch (gamma = 1, beta = 0; eps = 0 with them) and the weight."""
    lib = capi.lib()
    route, planes = kind.split("-")[0], planes_of(kind)
    N = bias.numel()
    out = i16(planes, M, N)
    with options(op_fmt=fp16, gemm_big=P.GEMM_BIG_OPTION.get(route, 1)):
        if route in ("gemm", "gemm_big"):
            K = 64
            A, Wz = i16(planes, M, K), i16(planes, N, K)
            capi.check(lib.dinoseg_op_gemm(A.data_ptr(), M * K, K, Wz.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), None, out.data_ptr(),
                                           M * N, N, S()))
        elif route == "ln_gemm":
            K = D
            eps = 1e-6 if X is None else 0.0          # (zero rows: rstd must stay finite)
            X = zeros(M, K) if X is None else X
            W = zeros(N, K) if W is None else W
            n = lib.dinoseg_op_ln_gemm_slab_elems(N, K, planes)
            assert n > 0
            Wp = i16(n)
            capi.check(lib.dinoseg_op_pack_slabs(W.data_ptr(), N, K, planes, Wp.data_ptr(), S()))
            gam, bet = torch.ones(K, device="cuda"), zeros(K)
            capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), eps, Wp.data_ptr(), N * K, bias.data_ptr(), M, N, K, planes,
                                              epi, out.data_ptr(), M * N, None, None, None, 0, 0, 0, 6, 0.0, None, None, S()))
        elif route == "gemm_rs":
            K = 768
            A, Wp = i16(M, K), i16(N * K)
            capi.check(lib.dinoseg_op_pack_rs(zeros(N, K).data_ptr(), N, K, 0, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_gemm_rs(A.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), M, N, K, epi, None, out.data_ptr(), N, None, None, None,
                                              0, 0, 0, 0.0, S()))
        else:
            K = 768
            eps = 1e-6 if X is None else 0.0
            X = zeros(M, K) if X is None else X
            W = zeros(N, K) if W is None else W
            Wp, bf = i16(N * K), zeros(N)
            gam, bet = torch.ones(K, device="cuda"), zeros(K)
            capi.check(lib.dinoseg_op_pack_rs_ln(W.data_ptr(), gam.data_ptr(), bet.data_ptr(), bias.data_ptr(), N, K, Wp.data_ptr(), bf.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), eps, Wp.data_ptr(), bf.data_ptr(), M, N, K, epi, out.data_ptr(), N, None, None, None,
                                                 0, 0, 0, 0.0, S()))
        torch.cuda.synchronize()
    return out


def epilogue_formats(kind):
    """ln_gemm on two planes is bf16 only (dinoseg_op_ln_gemm)"""
    return (False,) if kind == "ln_gemm-2" else (False, True)


EPI_CASES = [(k, f) for k in GEMMS for f in epilogue_formats(k)]
EPI_IDS = [f"{k}-{'fp16' if f else 'bf16'}" for k, f in EPI_CASES]
# ... with the activation: ReLU where the entry has it (dinoseg_op_gemm; gemm.hip refuses it for one fp16 plane: "the inference epilogues only")
ACT_CASES = [(k, f, e) for k, f in EPI_CASES for e in (capi.EPI_GELU, capi.EPI_RELU)
             if e == capi.EPI_GELU or (k.split("-")[0] in ("gemm", "gemm_big") and (k, f) != ("gemm-1", True))]
ACT_IDS = [f"{k}-{'fp16' if f else 'bf16'}-{'gelu' if e == capi.EPI_GELU else 'relu'}" for k, f, e in ACT_CASES]


@pytest.mark.parametrize("kind,fp16", EPI_CASES, ids=EPI_IDS)
def test_gelu_probe_epilogues(cuda, kind, fp16):
    """Probe 1 on the GELU epilogues: W = 0 and bias = probe in gemm.hip (gemm_big 0), gemm_big.hip (gemm_big 2), gemm_ln12.hip / gemm_ln.hip
    (one / two planes) and gemm_rs.hip, plain and with the LayerNorm inside."""
    vecs = P.gelu_probe_vectors()
    planes = planes_of(kind)
    first = None
    for M in MS:
        hs = []
        for v in vecs:
            o = unplane(run_epilogue(kind, fp16, M, dev(v)), fp16)
            assert np.array_equal(o, np.broadcast_to(o[:, 0:1], o.shape), equal_nan=True), f"{kind} M={M}: rows differ from row 0"
            hs.append(o[:, 0].sum(axis=0))
        hs = np.stack(hs)
        if first is None:
            first = hs
        assert np.array_equal(first, hs, equal_nan=True), f"{kind}: M={M} differs from M={MS[0]}"
    check_gelu_values(f"{kind}-{'fp16' if fp16 else 'bf16'}", first.reshape(-1), vecs.astype(np.float64).reshape(-1), fp16, planes, planes == 2,
                      pre_err(kind, fp16))


# ------------------------------------------------------------------------------------------------ probe 2: store rounding
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", FUSED)
def test_store_rounding_fused(cuda, kind, fp16):
    """The P pack of the fused kernels on ties: from 8 on the GELU returns x itself (test_gelu_formula_cpu.py::test_tails_and_clamp), so the
    stored activation must be RNE(x) bit for bit -- a tie goes to the even neighbour, the fp32 neighbours of a tie go apart -- and on two
    planes hi = RNE(x), lo = RNE(x - hi), whose sum the selector hands out exactly."""
    planes = planes_of(kind)
    vecs = P.tie_probe_vectors(fp16)
    for r, v in enumerate(vecs):
        h = hidden_through_selectors(kind, fp16, 77, dev(v))[0].numpy()
        want = stored(v, fp16, planes)
        bad = h != want
        assert not bad.any(), (kind, fp16, r, int(bad.sum()), v[bad][:4], h[bad][:4], want[bad][:4])


@pytest.mark.parametrize("kind,fp16,epi", ACT_CASES, ids=ACT_IDS)
def test_store_rounding_epilogues(cuda, kind, fp16, epi):
    """... and the 16-bit epilogues, plane by plane: hi = RNE(v), lo = RNE(v - hi).  ReLU where the entry has it (dinoseg_op_gemm)."""
    planes = planes_of(kind)
    for r, v in enumerate(P.tie_probe_vectors(fp16)):
        o = unplane(run_epilogue(kind, fp16, 77, dev(v), epi=epi), fp16)[:, 0]
        hi, lo = P.split(v, fp16)
        assert (o[0] == hi).all(), (kind, fp16, r, "hi", v[o[0] != hi][:4], o[0][o[0] != hi][:4])
        if planes == 2:
            assert (o[1] == lo).all(), (kind, fp16, r, "lo", v[o[1] != lo][:4], o[1][o[1] != lo][:4])


# ------------------------------------------------------------------------------------------------ probe 3: fc2 accumulation
@pytest.mark.parametrize("M", [77, 673, 128 * 300 + 19])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", FUSED)
def test_fc2_accumulation(cuda, kind, fp16, M):
    """Probe 3.  W1 = 0 and b1 exact in [8, 64): h = b1 (the GELU returns x, the pack is exact).  W2 exact in the format, dense and banded; X and b2
    seeded.  Reference: fp64 on those operands without the lo x lo products the two-plane kernel leaves out.  Bound: c U sum |h W2| with
    c = 4 sqrt(F) + 8 for the products, and 4 U (|X| + |b2|) for the residual and the bias on their own: x + b2 is one rounded add and the value
    the sum starts from or ends in (another).  M = 38 419: more items than CUs -- the weight ring runs on across items."""
    planes = planes_of(kind)
    h, h_lo = exact_operand((F,), 301, fp16, planes, 8.0, 64.0, signed=False)
    X = torch.from_numpy(np.random.default_rng(302).standard_normal((M, D)).astype(np.float32)).cuda()
    b2 = np.random.default_rng(303).standard_normal(D).astype(np.float32)
    W2d, W2d_lo = exact_operand((D, F), 304, fp16, planes, 2.0 ** -6, 2.0 ** -4)
    for name, mask in (("dense", np.ones((D, F), dtype=bool)), ("banded", banded((D, F)))):
        W2, W2_lo = W2d * mask, W2d_lo * mask
        got = run_fused(kind, fp16, X, zeros(F, D), dev(h), dev(W2), dev(b2))
        s = (W2 * h[None, :]).sum(axis=1) - (W2_lo * h_lo[None, :]).sum(axis=1)
        sabs = (np.abs(W2) * np.abs(h)[None, :]).sum(axis=1)
        ref = X.double().cpu().numpy() + (s + b2.astype(np.float64))[None, :]
        bound = P.sum_bound(sabs, F)[None, :] + 4.0 * P.U * (np.abs(X.cpu().numpy()) + np.abs(b2)[None, :])
        err = np.abs(got.double().cpu().numpy() - ref)
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        print(f"fc2 {kind} fp16={fp16} M={M} {name}: worst |err| / bound {err[i] / bound[i]:.3f} (|err| {err[i]:.3e}) at {i}")
        assert (err <= bound).all(), (kind, fp16, M, name, i, err[i], bound[i])


# ------------------------------------------------------------------------------------------------ probe 4: the projection
@pytest.mark.parametrize("M", [77, 673, 128 * 300 + 19])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["proj2", "proj3", "proj4"])
def test_projection(cuda, kind, fp16, M):
    """Probe 4.  W1 = 0 and b1 = 0: the hidden activation is gelu(0) = 0 and the MLP adds b2 alone.  out = X + ctx Wproj^T + bproj + b2, per element."""
    planes = planes_of(kind)
    ctx, ctx_lo = exact_operand((M, D), 401, fp16, planes, 0.25, 2.0)
    Wpr, Wpr_lo = exact_operand((D, D), 402, fp16, planes, 2.0 ** -5, 2.0 ** -3)
    g = np.random.default_rng(403)
    X, bpr, b2 = (g.standard_normal(s).astype(np.float32) for s in ((M, D), (D,), (D,)))
    got = run_fused(kind, fp16, dev(X), zeros(F, D), zeros(F), zeros(D, F), dev(b2), ctx=dev(ctx), Wpr=dev(Wpr), bpr=dev(bpr))
    t64 = lambda a: torch.from_numpy(a).cuda()
    s = t64(ctx) @ t64(Wpr).t() - t64(ctx_lo) @ t64(Wpr_lo).t()
    sabs = t64(np.abs(ctx)) @ t64(np.abs(Wpr)).t()
    ref = t64(X.astype(np.float64)) + s + t64((bpr.astype(np.float64) + b2.astype(np.float64)))[None, :]
    bound = (P.sum_bound(sabs.cpu().numpy(), D)
             + 4.0 * P.U * (np.abs(X).astype(np.float64) + (np.abs(bpr).astype(np.float64) + np.abs(b2).astype(np.float64))[None, :]))      # (as probe 3)
    err = (got.double() - ref).abs().cpu().numpy()
    i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    print(f"proj {kind} fp16={fp16} M={M}: worst |err| / bound {err[i] / bound[i]:.3f} (|err| {err[i]:.3e}) at {i}")
    assert (err <= bound).all(), (kind, fp16, M, i, err[i], bound[i])


# ------------------------------------------------------------------------------------------------ probe 5: LayerNorm + fc1
@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", FUSED)
def test_layernorm_fc1(cuda, kind, fp16, eps):
    """Probe 5.  out - X = fmt(z) per hidden unit and row: |h - z| <= half an ulp at |z| + c U (|b1| + sum |W1|).  Every |W1| is at least 1, which
    is more than twice that bound for every element (asserted), so one dropped or duplicated product of fc1 cannot pass.  M = 77, 673: ragged
    last items and row groups."""
    planes = planes_of(kind)
    for M in (77, 673):
        X, W1, b1, z, zerr = ln_fc1_case(M, eps, fp16, planes)
        h = hidden_through_selectors(kind, fp16, M, dev(b1), W1=dev(W1), X=dev(X), eps=eps).numpy()
        bound = P.half_ulp(np.abs(z) + zerr, fp16, planes) + zerr
        assert (2.0 * bound <= np.abs(W1[W1 != 0]).min()).all(), float(bound.max())
        err = np.abs(h - z)
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        print(f"ln+fc1 {kind} fp16={fp16} eps={eps} M={M}: worst |err| / bound {err[i] / bound[i]:.3f} (|err| {err[i]:.3e}) at {i}")
        assert (err <= bound).all(), (kind, fp16, eps, M, i, h[i], z[i], bound[i])
        assert bool(P.representable(torch.from_numpy(h).float(), fp16, planes).all())


# ------------------------------------------------------------------------------------------------ probe 6: fp16 saturation
SAT_Z = 76800.0        # 384 x 200 = 768 x 100: beyond 65504, every partial sum exact in fp32 (multiples of 100 below 2^24)


def sat_probe():
    """pre-activations [1536]: the general probe vector with every seventh unit beyond the fp16 range"""
    v = P.gelu_probe_vectors()[0].copy()
    hot = np.zeros(F, dtype=bool)
    hot[::7] = True
    return v, hot


@pytest.mark.parametrize("kind", FUSED)
def test_fp16_saturation_fused(cuda, kind):
    """mlp_fused3.hip: a pre-activation of 76 800 (reached through the fc1 product: rows of +1 / -1 times 200 x the same signs) must be stored as
    65504, finite in both planes, and must not disturb its neighbours: the selector's 0 x h products of the same row stay 0 only while h is
    finite.  mlp_fused2.hip and mlp_fused4.hip do not saturate (GELU_SATURATES): there the pre-activation is 65504 itself, 384 x 170 + 224, the
    largest they are documented for, and must come back as 65504."""
    planes = planes_of(kind)
    v, hot = sat_probe()
    M = 77
    w, b = (200.0, 0.0) if GELU_SATURATES[kind] else (170.0, 224.0)
    assert (D * w + b > P.FP16_MAX) if GELU_SATURATES[kind] else (D * w + b == P.FP16_MAX)
    pat = P.sign_rows(1, 601)[0]
    X = np.tile(pat, (M, 1))
    W1 = np.zeros((F, D), dtype=np.float32)
    W1[hot] = w * pat[None, :]
    b1 = np.where(hot, b, v).astype(np.float32)
    h = hidden_through_selectors(kind, True, M, dev(b1), W1=dev(W1), X=dev(X), eps=0.0).numpy()
    assert np.isfinite(h).all(), (kind, int((~np.isfinite(h)).sum()))
    assert (h[:, hot] == P.FP16_MAX).all(), (kind, h[0, hot][:4])
    check_gelu_values(f"sat-{kind}", h[0][~hot], v[~hot].astype(np.float64), True, planes, kind.endswith("3"), pre_err(kind, True), residual=1.0,
                      fused3=kind.endswith("3"))
    assert np.array_equal(h, np.broadcast_to(h[0:1], h.shape))


@pytest.mark.parametrize("kind,epi", [(k, e) for k, f, e in ACT_CASES if f], ids=[i for i, (k, f, e) in zip(ACT_IDS, ACT_CASES) if f])
def test_fp16_saturation_epilogues(cuda, kind, epi):
    """pack2_sat / split2<FMT, true> of the 16-bit epilogues: 7e4 (a bias, or 76 800 through the product where the bias travels as fp16 pieces) is
    stored as 65504 with a zero lo plane; 65520, which RNE alone would turn into inf, too."""
    route = kind.split("-")[0]
    v, hot = sat_probe()
    M = 77
    if route in ("ln_gemm", "ln_gemm_rs"):
        K = D if route == "ln_gemm" else 768
        pat = P.sign_rows(1, 602, width=K)[0]
        W = np.zeros((F, K), dtype=np.float32)
        W[hot] = (SAT_Z / K) * pat[None, :]
        bias = np.where(hot, 0.0, v).astype(np.float32)
        o = unplane(run_epilogue(kind, True, M, dev(bias), epi=epi, X=dev(np.tile(pat, (M, 1))), W=dev(W)), True)
    else:
        x = v.copy()
        x[hot] = np.where(np.arange(int(hot.sum())) % 2 == 0, 7e4, 65520.0)
        o = unplane(run_epilogue(kind, True, M, dev(x), epi=epi), True)
    assert np.isfinite(o).all(), (kind, int((~np.isfinite(o)).sum()))
    assert (o[0][:, hot] == P.FP16_MAX).all() and (o[1:][:, :, hot] == 0).all(), (kind, o[:, 0, hot][:, :4])
    if epi == capi.EPI_GELU:
        check_gelu_values(f"sat-{kind}", o[:, 0].sum(axis=0)[~hot], v[~hot].astype(np.float64), True, planes_of(kind), planes_of(kind) == 2,
                          pre_err(kind, True))


# ------------------------------------------------------------------------------------------------ probe 5, the qkv tails
TAILS = [("tail2", False, 0), ("tail2", True, 0), ("tail3", False, 0), ("tail3", True, 0), ("tail3", True, 1), ("tail4", False, 0), ("tail4", True, 0)]


def run_tail(kind, fp16, v_bf16, X, Wqkv, bq, B, ntok, npad, H, qscale):
    """block_tail_fused / block_tail_fused3 / block_tail_fused4 with a zero ctx, zero Wproj / bproj, zero W1 / b1 / W2 / b2, gamma = 1, beta = 0,
    eps = 0: X passes through, then q, k, v = split(LayerNorm1(X) Wqkv^T + bq).  Returns (X out, q, k, v as int16 [planes, B, H, npad, 64])."""
    lib = capi.lib()
    M = B * ntok
    planes = 2 if kind == "tail3" else 1
    out = X.clone()
    one, z_d, z_f = torch.ones(D, device="cuda"), zeros(D), zeros(F)
    W1, W2, Wpr = zeros(F, D), zeros(D, F), zeros(D, D)
    q = torch.full((planes, B, H, npad, 64), NAN16, dtype=torch.int16, device="cuda")
    k, v = q.clone(), q.clone()
    if kind == "tail2":
        with options(op_fmt=fp16):
            Wp, Wq, Wqp = i16(lib.dinoseg_op_mlp_fused_pack_elems(D, F)), i16(lib.dinoseg_op_proj_pack_elems(D)), i16(lib.dinoseg_op_qkv_pack_elems(D))
            capi.check(lib.dinoseg_op_pack_mlp(W1.data_ptr(), W2.data_ptr(), D, F, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_pack_proj(Wpr.data_ptr(), D, Wq.data_ptr(), S()))
            capi.check(lib.dinoseg_op_pack_qkv(Wqkv.data_ptr(), D, Wqp.data_ptr(), S()))
            c16 = i16(M, D)
            capi.check(lib.dinoseg_op_block_tail_fused(out.data_ptr(), c16.data_ptr(), Wq.data_ptr(), z_d.data_ptr(), one.data_ptr(), z_d.data_ptr(), 0.0,
                                                       Wp.data_ptr(), z_f.data_ptr(), z_d.data_ptr(), Wqp.data_ptr(), bq.data_ptr(), one.data_ptr(),
                                                       z_d.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), B, ntok, npad, H, qscale, D, F, S()))
            torch.cuda.synchronize()
    elif kind == "tail3":
        Wp = i16(lib.dinoseg_op_mlp3_pack_elems(D, F))
        capi.check(lib.dinoseg_op_pack_mlp3(Wpr.data_ptr(), W1.data_ptr(), z_f.data_ptr(), W2.data_ptr(), one.data_ptr(), z_d.data_ptr(), Wqkv.data_ptr(),
                                            bq.data_ptr(), one.data_ptr(), z_d.data_ptr(), D, F, int(fp16), Wp.data_ptr(), S()))
        c16 = i16(2, M, D)
        capi.check(lib.dinoseg_op_block_tail_fused3(out.data_ptr(), c16.data_ptr(), M * D, z_d.data_ptr(), 0.0, Wp.data_ptr(), z_d.data_ptr(), q.data_ptr(),
                                                    k.data_ptr(), v.data_ptr(), B * H * npad * 64, B, ntok, npad, H, qscale, v_bf16, D, F, int(fp16), S()))
        torch.cuda.synchronize()
    else:
        Wp = i16(lib.dinoseg_op_mlp4_pack_elems(D, F))
        capi.check(lib.dinoseg_op_pack_mlp4(Wpr.data_ptr(), W1.data_ptr(), z_f.data_ptr(), W2.data_ptr(), one.data_ptr(), z_d.data_ptr(), Wqkv.data_ptr(),
                                            bq.data_ptr(), one.data_ptr(), z_d.data_ptr(), D, F, int(fp16), Wp.data_ptr(), S()))
        c16 = i16(M, D)
        capi.check(lib.dinoseg_op_block_tail_fused4(out.data_ptr(), c16.data_ptr(), z_d.data_ptr(), 0.0, Wp.data_ptr(), z_d.data_ptr(), q.data_ptr(),
                                                    k.data_ptr(), v.data_ptr(), B, ntok, npad, H, qscale, D, F, int(fp16), S()))
        torch.cuda.synchronize()
    return out, q, k, v


@pytest.mark.parametrize("B,ntok", [(1, 77), (3, 130)])
@pytest.mark.parametrize("kind,fp16,v_bf16", TAILS, ids=[f"{k}-{'fp16' if f else 'bf16'}{'-vbf16' if vb else ''}" for k, f, vb in TAILS])
def test_layernorm_qkv_tails(cuda, kind, fp16, v_bf16, B, ntok):
    """Probe 5 on the qkv tails: the rows of +-1 pass the zeroed projection and MLP unchanged (bit for bit), LayerNorm1 with eps = 0 returns them,
    and q / k / v are fmt(z qscale), fmt(z), fmt(z) of the exact z = X Wqkv^T + bq per element, in the [B, heads, npad, 64] layout; V is bf16
    on one plane and with v_bf16.  Every |Wqkv| >= 1 is more than twice the bound of K and V, and qscale of it more than twice the bound of Q
    (asserted).  Pad rows keep the NaN pattern they had."""
    H, npad, M = 6, (ntok + 63) // 64 * 64, B * ntok
    planes = 2 if kind == "tail3" else 1
    qs = float(np.float32(0.125 * LOG2E))
    X, W, bq, z, zerr = ln_fc1_case(M, 0.0, fp16, planes, rows=3 * D, seed=701)
    got, q, k, v = run_tail(kind, fp16, v_bf16, dev(X), dev(W), dev(bq), B, ntok, npad, H, qs)
    assert torch.equal(got.cpu(), torch.from_numpy(X)), "X did not pass through unchanged"
    lay = lambda a: a.reshape(B, ntok, 3, H, 64).transpose(2, 0, 3, 1, 4)
    z, zerr = lay(z), lay(np.broadcast_to(zerr, z.shape))
    v_fp16 = fp16 and kind == "tail3" and not v_bf16
    for name, t, f16, want, werr in (("q", q, fp16, z[0] * qs, zerr[0] * qs + P.U * np.abs(z[0] * qs)), ("k", k, fp16, z[1], zerr[1]),
                                     ("v", v, v_fp16, z[2], zerr[2])):
        o = unplane(t, f16)
        g = o[:, :, :, :ntok].sum(axis=0)
        bound = P.half_ulp(np.abs(want) + werr, f16, planes) + werr
        assert (2.0 * bound <= (qs if name == "q" else 1.0)).all(), (name, float(bound.max()))
        err = np.abs(g - want)
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        print(f"tail {kind} fp16={fp16} v_bf16={v_bf16} B={B} ntok={ntok} {name}: worst |err| / bound {err[i] / bound[i]:.3f} (|err| {err[i]:.3e})")
        assert (err <= bound).all(), (kind, name, i, g[i], want[i], bound[i])
        assert bool((t[:, :, :, ntok:] == NAN16).all()), f"{name}: pad rows were written"


# ------------------------------------------------------------------------------------------------ probe 6 on Q / K / V
QKV_SAT = [("tail2", 0), ("tail3", 0), ("tail3", 1), ("tail4", 0), ("ln_gemm", 0), ("gemm_rs", 0), ("ln_gemm_rs", 0)]
SAT_Q = 393216.0       # 3 x 2^17 = 384 x 1024 = 768 x 512: times qscale = 0.18 it is 70 911, beyond 65504; every partial sum exact in fp32


def run_qkv_epilogue(route, X, Wqkv, bq, B, ntok, npad, H, qscale):
    """q (x qscale), k, v = split(LayerNorm(X) Wqkv^T + bq) through the QKV epilogue (epi 4) of gemm_ln12.hip (ln_gemm, K = 384) and gemm_rs.hip
    (gemm_rs on the rows as they are, ln_gemm_rs with the LayerNorm inside; K = 768), fp16 operands, gamma = 1, beta = 0, eps = 0.
    Returns q, k, v as int16 [1, B, H, npad, 64], NaN-filled before the launch."""
    lib = capi.lib()
    M, K = X.shape
    N = 3 * K
    q = torch.full((1, B, H, npad, 64), NAN16, dtype=torch.int16, device="cuda")
    k, v = q.clone(), q.clone()
    one, zero = torch.ones(K, device="cuda"), zeros(K)
    with options(op_fmt=1):
        if route == "ln_gemm":
            n = lib.dinoseg_op_ln_gemm_slab_elems(N, K, 1)
            assert n > 0
            Wp = i16(n)
            capi.check(lib.dinoseg_op_pack_slabs(Wqkv.data_ptr(), N, K, 1, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), one.data_ptr(), zero.data_ptr(), 0.0, Wp.data_ptr(), N * K, bq.data_ptr(), M, N, K, 1, 4, None,
                                              0, q.data_ptr(), k.data_ptr(), v.data_ptr(), B * H * npad * 64, ntok, npad, H, qscale, None, None, S()))
        elif route == "gemm_rs":
            A, Wp = one_plane(X, True), i16(N * K)
            capi.check(lib.dinoseg_op_pack_rs(Wqkv.data_ptr(), N, K, 0, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_gemm_rs(A.data_ptr(), K, Wp.data_ptr(), bq.data_ptr(), M, N, K, 4, None, None, 0, q.data_ptr(), k.data_ptr(),
                                              v.data_ptr(), ntok, npad, H, qscale, S()))
        else:
            Wp, bf = i16(N * K), zeros(N)
            capi.check(lib.dinoseg_op_pack_rs_ln(Wqkv.data_ptr(), one.data_ptr(), zero.data_ptr(), bq.data_ptr(), N, K, Wp.data_ptr(), bf.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 0.0, Wp.data_ptr(), bf.data_ptr(), M, N, K, 4, None, 0, q.data_ptr(), k.data_ptr(),
                                                 v.data_ptr(), ntok, npad, H, qscale, S()))
        torch.cuda.synchronize()
    return q, k, v


@pytest.mark.parametrize("kind,v_bf16", QKV_SAT, ids=[f"{k}{'-vbf16' if vb else ''}" for k, vb in QKV_SAT])
def test_fp16_saturation_qkv(cuda, kind, v_bf16):
    """Probe 6 on the Q / K stores of the qkv tails (pack2_sat in mlp_fused2.hip and mlp_fused4.hip, the clamps in mlp_fused3.hip's epi_gap) and of
    the QKV epilogues (pack2_sat in gemm_ln12.hip's store_block and gemm_rs.hip's epilogue_gap), fp16 operands.  The rows are +- one pattern of
    +-1, a seeded sign per row, so their LayerNorm is the row; every seventh column of Wqkv is 1024 (Q) or 200 (K, V) times that pattern
    (512 / 100 at K = 768) with a zero bias, so its z is +-393 216 (Q: +-70 911 after qscale) or +-76 800, exactly, and each such column holds
    both signs.  Q and K must hold +65504 and -65504 there: finite, and a zero lo plane on two planes.  V is bf16 on one plane and with v_bf16 and
    is not clamped: +-76 800, a number of bf16; as two fp16 planes (block_tail_fused3) it is clamped like Q and K.  Every other column is the
    block-sparse Wqkv of probe 5 with bias 64 and is held to probe 5's bound, so a clamp cannot disturb its neighbours; X passes through the
    tails unchanged; pad rows keep their NaN pattern."""
    tail = kind.startswith("tail")
    dm = D if tail or kind == "ln_gemm" else 768
    H, B, ntok = dm // 64, 3, 130
    npad, M = (ntok + 63) // 64 * 64, B * ntok
    planes = 2 if kind == "tail3" else 1
    qs = float(np.float32(0.125 * LOG2E))
    pat = P.sign_rows(1, 801, width=dm)[0]
    sgn = np.where(np.random.default_rng(802).integers(0, 2, M) == 0, 1.0, -1.0).astype(np.float32)
    X = sgn[:, None] * pat[None, :]
    W = block_sparse_w1(3 * dm, 803, width=dm)
    bq = np.full(3 * dm, 64.0, dtype=np.float32)
    hot = np.zeros(3 * dm, dtype=bool)
    hot[::7] = True
    W[hot] = np.where(np.arange(3 * dm)[hot] < dm, SAT_Q / dm, SAT_Z / dm)[:, None].astype(np.float32) * pat[None, :]
    bq[hot] = 0.0
    assert (P.rne(W, True) == W).all()
    z = X.astype(np.float64) @ W.astype(np.float64).T + bq.astype(np.float64)[None, :]
    assert (np.abs(z[:, hot][:, :8] * qs) > P.FP16_MAX).all() and (np.abs(z[:, hot]) >= SAT_Z).all() and (np.abs(z[:, ~hot]) <= 120.0).all()
    sabs = np.abs(W).sum(axis=1).astype(np.float64)
    zerr = P.sum_bound(np.abs(bq).astype(np.float64) + sabs, dm) + ((2.0 ** -22 if planes == 2 else 0.0) + 4.0 * P.U) * sabs      # (ln_fc1_case)
    if tail:
        got, q, k, v = run_tail(kind, True, v_bf16, dev(X), dev(W), dev(bq), B, ntok, npad, H, qs)
        assert torch.equal(got.cpu(), torch.from_numpy(X)), "X did not pass through unchanged"
    else:
        q, k, v = run_qkv_epilogue(kind, dev(X), dev(W), dev(bq), B, ntok, npad, H, qs)
    lay = lambda a: a.reshape(B, ntok, 3, H, 64).transpose(2, 0, 3, 1, 4)
    z, zerr, hot3 = lay(z), lay(np.broadcast_to(zerr[None, :], z.shape)), lay(np.broadcast_to(hot[None, :], z.shape))
    v_fp16 = kind == "tail3" and not v_bf16
    for name, t, f16, want, werr, top in (("q", q, True, z[0] * qs, zerr[0] * qs + P.U * np.abs(z[0] * qs), P.FP16_MAX),
                                          ("k", k, True, z[1], zerr[1], P.FP16_MAX), ("v", v, v_fp16, z[2], zerr[2], P.FP16_MAX if v_fp16 else SAT_Z)):
        o = unplane(t, f16)[:, :, :, :ntok]
        h3 = hot3[{"q": 0, "k": 1, "v": 2}[name]]
        assert np.isfinite(o).all(), (kind, name, int((~np.isfinite(o)).sum()))
        want = np.clip(want, -top, top)
        hi_hot, sign_hot = o[0][h3], np.sign(want[h3])
        assert (sign_hot > 0).any() and (sign_hot < 0).any()
        assert (hi_hot == top * sign_hot).all(), (kind, name, hi_hot[hi_hot != top * sign_hot][:4])
        assert (o[1:][:, h3] == 0).all(), (kind, name, "lo plane")
        g = o.sum(axis=0)
        bound = P.half_ulp(np.abs(want) + werr, f16, planes) + werr
        err = np.where(h3, 0.0, np.abs(g - want))
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
        print(f"sat qkv {kind} v_bf16={v_bf16} {name}: worst |err| / bound beside the clamped columns {err[i] / bound[i]:.3f} (|err| {err[i]:.3e})")
        assert (err <= bound).all(), (kind, name, i, g[i], want[i], bound[i])
        assert bool((t[:, :, :, ntok:] == NAN16).all()), f"{name}: pad rows were written"
