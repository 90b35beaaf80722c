"""Per-element probes of the stand-alone GEMMs behind a LIVE K loop: gemm.hip (128-row and 64-row tiles), gemm_big.hip (256 x 384 and
128 x 384 x 2 persistent tiles), gemm_ln.hip, gemm_ln12.hip, gemm_rs.hip (gemm_bstat plain and with the LayerNorm prologue, gemm_cstat).

tests/test_forward_probes_gpu.py reaches these kernels with W = 0 only (its probes 1, 2 and 6); tests/test_ops_gpu.py and tests/test_fp16_gpu.py
hold their K loops and scatter epilogues on seeded normal data to bars that scale with the tensor's largest element.  Here, with the builders
of tests/probe_util.py:

  G1  accumulation into fp32 outputs (EPI_PLAIN, EPI_RESID in place and with a separate `resid`, EPI_PATCH, gemm_cstat): operands exact in the
      format (six bits on one plane, hi + lo on two), W dense and then banded by the kernel's own k-step -- 64 in gemm.hip (BK), 32 in
      gemm_big.hip (big::BK), 64 in gemm_cstat (a step is a pair of 32-wide k-tiles: nk2 = K / 64) -- so one lost step stands alone in its
      columns.  |got - ref| <= sum_bound(sum |a w|, K) + 4 U (|X| + |bias| + |pos|) per element against fp64 on the device, the lo x lo
      products the two-plane kernels leave out taken out of the reference.
  G2  the GELU / ReLU epilogues of all eight GEMMS kinds: rows of +-1 (LayerNorm kinds: eps 0 and 1e-6), block_sparse_w1 at the kernel's
      width, bias 64: every z in [8, 120] where both GELU forms return z itself, the stored value is fmt(z) within half_ulp(|z| + zerr) + zerr,
      and 2 bound <= min |W| (asserted): one dropped or duplicated product cannot pass.  With the training forward's aux_out the
      pre-activation planes equal split(z) bit for bit.
  G3  the Q / K / V scatter of every stand-alone QKV epilogue, per element in [B, heads, npad, 64]: q = fmt(z qscale), k = fmt(z),
      v = fmt_v(z); pad rows keep the NaN pattern.

Every bound is one probe_util derives; nothing is fitted to an output.  Every probe prints its worst |err| / bound.

What a launcher refuses, with the line that does: fp16 has no EPI_PLAIN (gemm.hip launch_gemm_small "the fp16 operand format covers the
inference epilogues only", gemm_big.hip launch_big_one); one fp16 plane has no EPI_RELU in gemm.hip (the same line; gemm_big.hip has it);
gemm_ln.hip on two planes is bf16 only (dinoseg_op_ln_gemm: fmt = planes == 1 ? op_fmt : FMT_BF16); gemm_big.hip takes neither `resid` nor
`aux_out` nor EPI_PATCH (gemm_big_supported: epi <= EPI_QKV, resid == nullptr, aux_out == nullptr); aux_out is bf16 only (launch_gemm_small's
fp16 table asks aux_out == nullptr); the QKV epilogue needs dmodel % 128 == 0 in gemm.hip, dmodel % 384 == 0 in gemm_big.hip, K = 384 in
gemm_ln*.hip (gemm_ln_supported) and dmodel = 768 in gemm_rs.hip (gemm_rs_supported).
"""
import functools

import numpy as np
import pytest
import torch

from dino_amd import capi, options
from tests import probe_util as P
from tests.gpu_util import Guarded
from tests.probe_util import (FMT_IDS, G2_CASES, G2_MS, G3_CASES, G3_SHAPES, KSTEP, NAN16, QS, WIDTH, accum_reference, add_bound, banded, check_patch,
                              check_qkv, check_stored, exact_operand, g2_eps, g2_widths, ln_fc1_case, planes_of, unplane, v_is_fp16, within)

pytestmark = pytest.mark.gpu

S = capi.stream_ptr


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.float32, device="cuda")


def to_planes(x64, fp16, planes):
    """fp64 device tensor of values the format holds exactly (hi + lo on two planes) -> int16 [planes, rows, cols]"""
    dt = P.tdtype(fp16)
    x = x64.float()
    hi = x.to(dt)
    ps = [hi] if planes == 1 else [hi, (x - hi.float()).to(dt)]
    back = sum(p.double() for p in ps)
    assert torch.equal(back, x64), "operand is not exact in the format"
    return torch.stack(ps).contiguous().view(torch.int16)


def nan16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda")


# ------------------------------------------------------------------------------------------------ probe G1: accumulation into fp32 outputs
MMAX = 673
G1_MS = (1, 77, 673)


def _operands(rows, K, seed, fp16, planes, lo, hi):
    v, v_lo = exact_operand((rows, K), seed, fp16, planes, lo, hi)
    v, v_lo = t64(v), t64(v_lo)
    return v, v_lo, to_planes(v, fp16, planes)


@functools.lru_cache(maxsize=None)
def a_rows(K, fp16, planes):
    """A [673, K] in [0.25, 2): value, lo part (fp64, device) and the planes.  The cases with fewer rows take its first rows."""
    return _operands(MMAX, K, 1101, fp16, planes, 0.25, 2.0)


@functools.lru_cache(maxsize=None)
def w_rows(N, K, fp16, planes):
    """W [N, K] in [2^-5, 2^-3)"""
    return _operands(N, K, 1102, fp16, planes, 2.0 ** -5, 2.0 ** -3)


@functools.lru_cache(maxsize=None)
def _seeded_cached(shape, seed):
    return dev(np.random.default_rng(seed).standard_normal(shape))


def seeded(shape, seed):
    """seeded normal fp32 values on the device; kept for the shapes every case shares, built afresh for the two walk cases"""
    return _seeded_cached(shape, seed) if int(np.prod(shape)) <= MMAX * 1536 else _seeded_cached.__wrapped__(shape, seed)


def masks(N, K, ks):
    """dense, and banded by the k-step (K = one step: dense is banded already)"""
    out = [("dense", None)]
    if K > ks:
        out.append(("banded", t64(banded((N, K), tile=ks, ntiles=K // ks))))
    return out


def gemm_f32(route, fp16, planes, Ap, a_plane, Wp, M, N, K, epi, bias, out, resid=None, route_ab=0):
    lib = capi.lib()
    with options(op_fmt=int(fp16), gemm_big=P.GEMM_BIG_OPTION[route], route_ab=route_ab):
        if resid is None:
            capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), a_plane, K, Wp.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), out.data_ptr(), None,
                                           0, 0, S()))
        else:
            capi.check(lib.dinoseg_op_gemm_train(Ap.data_ptr(), a_plane, K, Wp.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), resid.data_ptr(),
                                                 out.data_ptr(), None, 0, 0, None, 0, S()))
        torch.cuda.synchronize()


def g1_variants(route, fp16):
    """(name, epi, separate resid, route_ab): what the route's launcher accepts (module docstring)"""
    v = [] if fp16 else [("plain", capi.EPI_PLAIN, False, 0)]
    if route == "gemm":
        v += [("resid64", capi.EPI_RESID, False, 0), ("resid128", capi.EPI_RESID, False, 1),
              ("resid64-src", capi.EPI_RESID, True, 0), ("resid128-src", capi.EPI_RESID, True, 1)]
    else:
        v += [("resid", capi.EPI_RESID, False, 0)]
    return v


def g1_run(route, fp16, planes, N, K, Ms, A3, W3):
    """every variant x mask x M of one (route, format, planes, N, K); A3 / W3 = (value, lo part, planes)"""
    A, A_lo, Ap = A3
    Wd, Wd_lo, _ = W3
    rows = A.shape[0]
    bias, X = seeded((N,), 1103), seeded((rows, N), 1104)
    top = 0.0
    for mname, mask in masks(N, K, KSTEP[route]):
        W, W_lo = (Wd, Wd_lo) if mask is None else (Wd * mask, Wd_lo * mask)
        Wp = to_planes(W, fp16, planes)
        s, sb = accum_reference(A, A_lo, W, W_lo, K)
        for M in Ms:
            for vname, epi, src, ab in g1_variants(route, fp16):
                name = f"G1 {route}-{planes} {FMT_IDS[fp16]} N={N} K={K} M={M} {mname} {vname}"
                if epi == capi.EPI_PLAIN:
                    out = torch.full((M, N), float("nan"), device="cuda")
                    gemm_f32(route, fp16, planes, Ap, rows * K, Wp, M, N, K, epi, bias, out)
                    ref, bound = s[:M] + bias.double(), sb[:M] + add_bound(bias.double())
                else:
                    x0 = X[:M].clone()
                    out = torch.full((M, N), float("nan"), device="cuda") if src else x0.clone()
                    gemm_f32(route, fp16, planes, Ap, rows * K, Wp, M, N, K, epi, bias, out, resid=x0 if src else None, route_ab=ab)
                    assert torch.equal(x0, X[:M]), f"{name}: resid was written"
                    ref, bound = X[:M].double() + s[:M] + bias.double(), sb[:M] + add_bound(X[:M].double(), bias.double())
                top = max(top, within(name, (out.double() - ref).abs(), bound))
    return top


G1_SMALL = [(N, K) for N in (128, 384, 640) for K in (64, 192, 1536)]
G1_BIG = [(N, K) for N in (384, 1152) for K in (32, 96, 768)]


@pytest.mark.parametrize("N,K", G1_SMALL, ids=[f"N{n}-K{k}" for n, k in G1_SMALL])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("planes", [1, 2])
def test_accumulation_gemm(cuda, planes, fp16, N, K):
    """G1 on gemm.hip: EPI_PLAIN (bf16), EPI_RESID in place and through `resid` into a NaN-filled output, on the 64-row tiles (the default at these
    sizes: 2 x workgroups <= CUs) and the 128-row tiles (route_ab bit 0); M = 1, 77, 673: one row, ragged tiles of either height, several panels."""
    g1_run("gemm", fp16, planes, N, K, G1_MS, a_rows(K, fp16, planes), w_rows(N, K, fp16, planes))


@pytest.mark.parametrize("N,K", G1_BIG, ids=[f"N{n}-K{k}" for n, k in G1_BIG])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("planes", [1, 2])
def test_accumulation_gemm_big(cuda, planes, fp16, N, K):
    """G1 on gemm_big.hip (gemm_big 2): EPI_PLAIN (bf16) and EPI_RESID in place; K = 32 and 96 are the K % 64 != 0 route that only this kernel
    takes.  M = 1, 77, 673: the ragged last panel (the plain path of the residual epilogue) and full 128 / 256-row wave tiles (its register ring)."""
    g1_run("gemm_big", fp16, planes, N, K, G1_MS, a_rows(K, fp16, planes), w_rows(N, K, fp16, planes))


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("planes", [1, 2])
def test_accumulation_gemm_big_walk(cuda, planes, fp16):
    """G1 on gemm_big.hip's persistent walk.  launch_big_cfg starts min(CUs / 8, pairs per XCD) workgroups per XCD, pairs per XCD =
    ceil(panels / 8) x (N / 384); at N = 1152, M = 20 557 there are 81 panels of 256 rows (161 of 128 on two planes): 33 (63) pairs per XCD, more
    than the 32 workgroups a 256-CU device gives an XCD, so workgroups walk on to a second tile with the ring running.  K = 32, the smallest."""
    M, N, K = 256 * 80 + 77, 1152, 32
    props = torch.cuda.get_device_properties(0)
    assert ((M + 255) // 256 + 7) // 8 * (N // 384) > props.multi_processor_count // 8, "not more pairs than workgroups on this device"
    g1_run("gemm_big", fp16, planes, N, K, (M,), _operands(M, K, 1111, fp16, planes, 0.25, 2.0), w_rows(N, K, fp16, planes))


def cstat_run(fp16, K, Ms, A3):
    N, lib = 768, capi.lib()
    A, A_lo, Ap = A3
    rows = A.shape[0]
    Wd = w_rows(N, K, fp16, 1)[0]
    bias, X = seeded((N,), 1103), seeded((rows, N), 1104)
    for mname, mask in masks(N, K, KSTEP["gemm_cstat"]):
        W = Wd if mask is None else Wd * mask
        to_planes(W, fp16, 1)                                    # (exact in the format: the packed copy holds W itself)
        Wp = torch.zeros(N * K, dtype=torch.int16, device="cuda")
        s, sb = accum_reference(A, A_lo, W, torch.zeros_like(W), K)
        with options(op_fmt=int(fp16)):
            capi.check(lib.dinoseg_op_pack_rs(W.float().contiguous().data_ptr(), N, K, 1, Wp.data_ptr(), S()))
            for M in Ms:
                out = X[:M].clone()
                capi.check(lib.dinoseg_op_gemm_rs(Ap.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), M, N, K, capi.EPI_RESID, out.data_ptr(), None, 0, None,
                                                  None, None, 0, 0, 0, 0.0, S()))
                torch.cuda.synchronize()
                ref, bound = X[:M].double() + s[:M] + bias.double(), sb[:M] + add_bound(X[:M].double(), bias.double())
                within(f"G1 gemm_cstat {FMT_IDS[fp16]} K={K} M={M} {mname}", (out.double() - ref).abs(), bound)


@pytest.mark.parametrize("K", [576, 768, 3072])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
def test_accumulation_gemm_cstat(cuda, fp16, K):
    """G1 on gemm_rs.hip's gemm_cstat (x += A W^T + bias in place, N = 768, one plane).  K = 576 is the smallest K gemm_rs_supported takes
    (K % 192 == 0, K >= 576): nine steps, the head and the tail of the step program with one pass of its loop."""
    cstat_run(fp16, K, G1_MS, a_rows(K, fp16, 1))


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
def test_accumulation_gemm_cstat_walk(cuda, fp16):
    """... and its persistent walk: launch_gemm_rs_fmt starts ceil(n2 / ceil(n2 / CUs)) workgroups (made even) for n2 = 2 ceil(M / 128) items;
    M = 16 531 gives 260 items, more than the 256 CUs: every workgroup takes a second item with the weight ring running.  K = 576."""
    M, K = 128 * 129 + 19, 576
    assert 2 * ((M + 127) // 128) > torch.cuda.get_device_properties(0).multi_processor_count, "not more items than workgroups on this device"
    cstat_run(fp16, K, (M,), _operands(M, K, 1112, fp16, 1, 0.25, 2.0))


PATCH_SHAPES = [(B, n, K, N) for B, n in ((1, 1), (3, 35), (2, 130)) for K in (192, 768) for N in (128, 384, 768)]


@pytest.mark.parametrize("B,n,K,N", PATCH_SHAPES, ids=[f"B{b}-n{n}-K{k}-N{nn}" for b, n, k, nn in PATCH_SHAPES])
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("planes", [1, 2])
def test_accumulation_patch_embedding(cuda, planes, fp16, B, n, K, N):
    """G1 on EPI_PATCH (gemm.hip): X_out[b (n + 1) + 1 + p] = A[b n + p] W^T + bias + pos[1 + p].  (3, 35) and (2, 130): frames straddle the
    128-row tiles, so the row remap changes inside a tile.  X_out is NaN-filled between guard bands: the CLS rows b (n + 1) and the bands must
    still be NaN afterwards."""
    lib = capi.lib()
    M = B * n
    A, A_lo, Ap = a_rows(K, fp16, planes)
    A, A_lo, Ap = A[:M], A_lo[:M], Ap[:, :M].contiguous()
    Wd, Wd_lo, _ = w_rows(N, K, fp16, planes)
    bias, pos = seeded((N,), 1103), seeded((n + 1, N), 1105)
    for mname, mask in masks(N, K, KSTEP["gemm"]):
        W, W_lo = (Wd, Wd_lo) if mask is None else (Wd * mask, Wd_lo * mask)
        Wp = to_planes(W, fp16, planes)
        G = Guarded(1, B * (n + 1), N, torch.float32)
        with options(op_fmt=int(fp16)):
            capi.check(lib.dinoseg_op_patch_gemm(Ap.data_ptr(), Wp.data_ptr(), bias.data_ptr(), pos.data_ptr(), B, n, N, K, planes, G.ptr(), S()))
            torch.cuda.synchronize()
        assert G.guards_untouched(), "a guard band was written"
        out = G.dense()[0].reshape(B, n + 1, N).double()
        s, sb = accum_reference(A, A_lo, W, W_lo, K)
        ref = s.reshape(B, n, N) + bias.double() + pos[1:].double()[None]
        bound = sb.reshape(B, n, N) + add_bound(bias.double(), pos[1:].double())[None]
        check_patch(f"G1 patch-{planes} {FMT_IDS[fp16]} B={B} n={n} K={K} N={N} {mname}", out, ref, bound)


# ------------------------------------------------------------------------------------------------ probe G2: 16-bit epilogues behind a live K loop
def run_act(kind, fp16, X, W, bias, epi, eps=0.0, aux=False):
    """act(rows W^T + bias) through the 16-bit epilogue `kind` names: int16 planes [planes, M, N].  rows = LayerNorm(X) inside the launch for the
    LayerNorm kinds (gamma = 1, beta = 0), X itself as operand planes for the others.  aux: through dinoseg_op_gemm_train, returns
    (activation planes, pre-activation planes)."""
    lib = capi.lib()
    route, planes = kind.split("-")[0], planes_of(kind)
    M, K = X.shape
    N = bias.numel()
    out = nan16(planes, M, N)
    with options(op_fmt=int(fp16), gemm_big=P.GEMM_BIG_OPTION.get(route, 1)):
        if route in ("gemm", "gemm_big"):
            A, Wp = to_planes(X.double(), fp16, planes), to_planes(W.double(), fp16, planes)
            if aux:
                pre = nan16(planes, M, N)
                capi.check(lib.dinoseg_op_gemm_train(A.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), None, None,
                                                     out.data_ptr(), M * N, N, pre.data_ptr(), M * N, S()))
                torch.cuda.synchronize()
                return out, pre
            capi.check(lib.dinoseg_op_gemm(A.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, epi, bias.data_ptr(), None, out.data_ptr(),
                                           M * N, N, S()))
        elif route == "ln_gemm":
            n = lib.dinoseg_op_ln_gemm_slab_elems(N, K, planes)
            assert n > 0
            Wp = torch.zeros(n, dtype=torch.int16, device="cuda")
            capi.check(lib.dinoseg_op_pack_slabs(W.data_ptr(), N, K, planes, Wp.data_ptr(), S()))
            gam, bet = torch.ones(K, device="cuda"), zeros(K)
            capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), eps, Wp.data_ptr(), N * K, bias.data_ptr(), M, N, K, planes,
                                              epi, out.data_ptr(), M * N, None, None, None, 0, 0, 0, 6, 0.0, None, None, S()))
        elif route == "gemm_rs":
            A, Wp = to_planes(X.double(), fp16, 1), torch.zeros(N * K, dtype=torch.int16, device="cuda")
            capi.check(lib.dinoseg_op_pack_rs(W.data_ptr(), N, K, 0, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_gemm_rs(A.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), M, N, K, epi, None, out.data_ptr(), N, None, None, None,
                                              0, 0, 0, 0.0, S()))
        else:
            Wp, bf = torch.zeros(N * K, dtype=torch.int16, device="cuda"), zeros(N)
            gam, bet = torch.ones(K, device="cuda"), zeros(K)
            capi.check(lib.dinoseg_op_pack_rs_ln(W.data_ptr(), gam.data_ptr(), bet.data_ptr(), bias.data_ptr(), N, K, Wp.data_ptr(), bf.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), eps, Wp.data_ptr(), bf.data_ptr(), M, N, K, epi, out.data_ptr(), N, None, None, None,
                                                 0, 0, 0, 0.0, S()))
        torch.cuda.synchronize()
    return out


G2_IDS = [f"{k}-{FMT_IDS[f]}-{'gelu' if e == capi.EPI_GELU else 'relu'}" for k, f, e in G2_CASES]


@functools.lru_cache(maxsize=None)
def g2_case(M, eps, fp16, planes, N, K):
    return ln_fc1_case(M, eps, fp16, planes, rows=N, seed=1201, width=K)


@pytest.mark.parametrize("kind,fp16,epi", G2_CASES, ids=G2_IDS)
def test_epilogue_behind_k_loop(cuda, kind, fp16, epi):
    """G2.  The stored activation is fmt(z) of z = rows W^T + 64 per element and one number of the format (hi + lo on two planes)."""
    route, planes = kind.split("-")[0], planes_of(kind)
    K = WIDTH[route]
    for N in g2_widths(kind):
        for M in G2_MS:
            for eps in g2_eps(kind):
                X, W, b, z, zerr = g2_case(M, eps, fp16, planes, N, K)
                assert z.min() >= 8.0 and z.max() <= 120.0
                o = unplane(run_act(kind, fp16, dev(X), dev(W), dev(b), epi, eps=eps), fp16)
                check_stored(f"G2 {kind} {FMT_IDS[fp16]} epi={epi} N={N} M={M} eps={eps}", o, z, zerr, W, fp16, planes)


@pytest.mark.parametrize("planes", [1, 2])
def test_preactivation_planes(cuda, planes):
    """G2 with the training forward's aux_out (gemm.hip, bf16): z is exact here (multiples of 0.25 below 128 and so is every partial sum, in
    any order), so the pre-activation planes are split(z) bit for bit -- hi alone on one plane -- and the activation planes are those of the
    launch without aux_out."""
    kind, N = f"gemm-{planes}", 1536
    for M in G2_MS:
        X, W, b, z, _ = g2_case(M, 0.0, False, planes, N, WIDTH["gemm"])
        plain = run_act(kind, False, dev(X), dev(W), dev(b), capi.EPI_GELU)
        act, pre = run_act(kind, False, dev(X), dev(W), dev(b), capi.EPI_GELU, aux=True)
        assert torch.equal(act, plain), "aux_out changed the activation"
        hi, lo = P.split(z.astype(np.float32), False)
        assert (z.astype(np.float32).astype(np.float64) == z).all()
        p = unplane(pre, False)
        assert (p[0] == hi).all(), ("hi", int((p[0] != hi).sum()))
        if planes == 2:
            assert (p[1] == lo).all(), ("lo", int((p[1] != lo).sum()))


# ------------------------------------------------------------------------------------------------ probe G3: the Q / K / V scatter per element
G3_IDS = [f"{k}-H{H}-{FMT_IDS[f]}{'-vbf16' if vb else ''}" for k, H, f, vb in G3_CASES]


def run_qkv(kind, fp16, v_bf16, X, W, bq, B, ntok, npad, H):
    """q (x qscale), k, v of rows W^T + bq through the QKV epilogue `kind` names (rows: as in run_act, eps = 0): int16 [planes, B, H, npad, 64],
    NaN-filled before the launch"""
    lib = capi.lib()
    route, planes = kind.split("-")[0], planes_of(kind)
    M, K = X.shape
    N = 3 * K
    q = nan16(planes, B, H, npad, 64)
    k, v = q.clone(), q.clone()
    plane = B * H * npad * 64
    one, zero = torch.ones(K, device="cuda"), zeros(K)
    with options(op_fmt=int(fp16), op_v_bf16=v_bf16, gemm_big=P.GEMM_BIG_OPTION.get(route, 1)):
        if route in ("gemm", "gemm_big"):
            A, Wp = to_planes(X.double(), fp16, planes), to_planes(W.double(), fp16, planes)
            capi.check(lib.dinoseg_op_qkv_gemm(A.data_ptr(), M * K, Wp.data_ptr(), N * K, bq.data_ptr(), B, ntok, npad, H, planes, QS, q.data_ptr(),
                                               k.data_ptr(), v.data_ptr(), plane, S()))
        elif route == "ln_gemm":
            n = lib.dinoseg_op_ln_gemm_slab_elems(N, K, planes)
            assert n > 0
            Wp = torch.zeros(n, dtype=torch.int16, device="cuda")
            capi.check(lib.dinoseg_op_pack_slabs(W.data_ptr(), N, K, planes, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm(X.data_ptr(), one.data_ptr(), zero.data_ptr(), 0.0, Wp.data_ptr(), N * K, bq.data_ptr(), M, N, K, planes, 4,
                                              None, 0, q.data_ptr(), k.data_ptr(), v.data_ptr(), plane, ntok, npad, H, QS, None, None, S()))
        elif route == "gemm_rs":
            A, Wp = to_planes(X.double(), fp16, 1), torch.zeros(N * K, dtype=torch.int16, device="cuda")
            capi.check(lib.dinoseg_op_pack_rs(W.data_ptr(), N, K, 0, Wp.data_ptr(), S()))
            capi.check(lib.dinoseg_op_gemm_rs(A.data_ptr(), K, Wp.data_ptr(), bq.data_ptr(), M, N, K, 4, None, None, 0, q.data_ptr(), k.data_ptr(),
                                              v.data_ptr(), ntok, npad, H, QS, S()))
        else:
            Wp, bf = torch.zeros(N * K, dtype=torch.int16, device="cuda"), zeros(N)
            capi.check(lib.dinoseg_op_pack_rs_ln(W.data_ptr(), one.data_ptr(), zero.data_ptr(), bq.data_ptr(), N, K, Wp.data_ptr(), bf.data_ptr(), S()))
            capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 0.0, Wp.data_ptr(), bf.data_ptr(), M, N, K, 4, None, 0, q.data_ptr(), k.data_ptr(),
                                                 v.data_ptr(), ntok, npad, H, QS, S()))
        torch.cuda.synchronize()
    return q, k, v


@functools.lru_cache(maxsize=None)
def g3_case(M, fp16, planes, dm):
    return ln_fc1_case(M, 0.0, fp16, planes, rows=3 * dm, seed=1301, width=dm)


@pytest.mark.parametrize("kind,H,fp16,v_bf16", G3_CASES, ids=G3_IDS)
def test_qkv_scatter(cuda, kind, H, fp16, v_bf16):
    """G3.  (B, ntok) = (1, 77), (3, 130), (2, 257): frames end inside row tiles of every height, npad = 128, 192, 320 leaves 51, 62 and 63 pad rows."""
    planes, dm = planes_of(kind), 64 * H
    for B, ntok in G3_SHAPES:
        npad, M = (ntok + 63) // 64 * 64, B * ntok
        X, W, bq, z, zerr = g3_case(M, fp16, planes, dm)
        q, k, v = run_qkv(kind, fp16, v_bf16, dev(X), dev(W), dev(bq), B, ntok, npad, H)
        check_qkv(f"G3 {kind} H={H} {FMT_IDS[fp16]} v_bf16={v_bf16} B={B} ntok={ntok}", q, k, v, z, zerr, fp16, planes, v_is_fp16(fp16, planes, v_bf16),
                  B, ntok, H)
