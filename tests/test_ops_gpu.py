"""Per-kernel parity tests (-m gpu): each HIP operator, called through the C-ABI, against the CPU oracle
(oracle/dinoseg_oracle.py) or an fp64 restatement on the same seeded inputs."""
import math

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import capi
from oracle import dinoseg_oracle as O
from tests.gpu_util import pack, pack_slabs, quant_like, seeded, unpack

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
LOG2E = 1.4426950408889634


def test_library_loads_and_torch_shares_runtime(cuda):
    assert capi.lib().dinoseg_version() >= 100
    x = seeded((5, 7), 0)
    p = pack(x, 2)
    torch.cuda.synchronize()
    rec = unpack(p)
    assert torch.allclose(rec, x, rtol=0, atol=2.0 ** -15 * float(x.abs().max()))
    hi = pack(x, 1)
    assert torch.equal(hi.view(torch.bfloat16)[0], x.to(torch.bfloat16))   # round-to-nearest-even, bit exact


def test_pack_padding(cuda):
    x = seeded((3, 10), 1)
    p = pack(x, 2, rows_pad=8, cols_pad=16)
    rec = unpack(p)
    assert torch.all(rec[3:] == 0) and torch.all(rec[:, 10:] == 0)
    assert torch.allclose(rec[:3, :10], x, atol=1e-4)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("M,N,K", [(300, 256, 192), (128, 128, 64), (1, 128, 384), (515, 384, 1536),
                                   (300, 384, 192), (1000, 768, 64), (25613, 1152, 96), (257, 384, 32)])
def test_gemm_plain(cuda, planes, M, N, K):
    # N % 384 == 0 with planes == 1 runs the 256x384 persistent kernel (gemm_big.hip), everything else gemm.hip
    if planes == 2 and K % 64 != 0:
        pytest.skip("the 128x128 kernel needs K % 64 == 0")
    # asymmetric operands: a transposed / permuted fragment map cannot pass
    A = seeded((M, K), 10 + M) + torch.arange(K, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    W = seeded((N, K), 20 + N) * 0.1 + torch.arange(N, device="cuda", dtype=torch.float32)[:, None] * 1e-3
    bias = seeded((N,), 3)
    out = torch.full((M, N), float("nan"), device="cuda")
    Ap, Wp = pack(A, planes), pack(W, planes)
    capi.check(capi.lib().dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_PLAIN,
                                          bias.data_ptr(), out.data_ptr(), None, 0, 0, S()))
    torch.cuda.synchronize()
    ref_q = (quant_like(A, planes).double() @ quant_like(W, planes).double().t() + bias.double()).float()
    scale = float(ref_q.abs().max())
    assert torch.isfinite(out).all()
    # same quantised operands, fp32 accumulation: only summation-order noise (+ dropped lo*lo term) remains
    assert float((out - ref_q).abs().max()) <= (2e-6 if planes == 1 else 3e-5) * scale * math.sqrt(K / 64)
    if planes == 2:   # split precision must track the true fp32 product
        ref = (A.double() @ W.double().t() + bias.double()).float()
        assert float((out - ref).abs().max()) <= 4e-5 * scale


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("N", [256, 384])
def test_gemm_epilogues(cuda, planes, N):
    M, K = 261, 128
    A, W, bias = seeded((M, K), 1), seeded((N, K), 2) * 0.2, seeded((N,), 3)
    Ap, Wp = pack(A, planes), pack(W, planes)
    base = (quant_like(A, planes).double() @ quant_like(W, planes).double().t() + bias.double()).float()
    lib = capi.lib()
    # residual: X += acc + bias
    X0 = seeded((M, N), 4)
    X = X0.clone()
    capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_RESID,
                                   bias.data_ptr(), X.data_ptr(), None, 0, 0, S()))
    assert torch.allclose(X, X0 + base, atol=2e-4, rtol=1e-5)
    # GELU / ReLU -> bf16 planes
    for epi, fn in ((capi.EPI_GELU, O.gelu_erf), (capi.EPI_RELU, torch.relu)):
        outp = torch.zeros((planes, M, N), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, epi,
                                       bias.data_ptr(), None, outp.data_ptr(), M * N, N, S()))
        got = unpack(outp)
        want = fn(base.cpu()).cuda()
        tol = 2.0 ** -8 if planes == 1 else 2.0 ** -15
        assert float((got - want).abs().max()) <= tol * float(want.abs().max()) + 2e-4


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("M,K", [(3601, 1536), (3601, 384), (70, 128), (1, 64)])
def test_residual_gemm_small_batch_tiles(cuda, planes, M, K):
    """The residual GEMMs of a small batch (attn.proj / mlp.fc2 of one frame: 29 x 3 tiles of 128 x 128 on 256 CUs) run on 64 x 128
    tiles (gemm.hip, HALFM); every output element sees the same MFMAs in the same order: bit-identical to the 128-row tiles
    (route_ab bit 0 forces those) and right against the fp64 product of the operands the kernel saw."""
    N = 384
    A, W, bias = seeded((M, K), 61), seeded((N, K), 62) * 0.2, seeded((N,), 63)
    Ap, Wp = pack(A, planes), pack(W, planes)
    X0 = seeded((M, N), 64)
    lib = capi.lib()
    outs = []
    with dino_amd.options():
        for ab in (1, 0):
            capi.check(lib.dinoseg_set_option(b"route_ab", ab))
            X = X0.clone()
            capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_RESID,
                                           bias.data_ptr(), X.data_ptr(), None, 0, 0, S()))
            outs.append(X)
    assert torch.equal(outs[0], outs[1])
    base = (quant_like(A, planes).double() @ quant_like(W, planes).double().t() + bias.double()).float()
    assert torch.allclose(outs[1], X0 + base, atol=3e-4 * math.sqrt(K / 64), rtol=1e-5)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("H,ntok", [(2, 197), (6, 197), (6, 65)])
def test_qkv_gemm_layout(cuda, planes, H, ntok):
    B = 2
    D, npad = H * 64, (ntok + 63) // 64 * 64
    A, W, bias = seeded((B * ntok, D), 5), seeded((3 * D, D), 6) * 0.1, seeded((3 * D,), 7)
    Ap, Wp = pack(A, planes), pack(W, planes)
    plane = B * H * npad * 64
    q = torch.zeros((planes, B, H, npad, 64), dtype=torch.int16, device="cuda")
    k = torch.zeros_like(q)
    vt = torch.zeros_like(q)
    qscale = 0.125 * LOG2E
    capi.check(capi.lib().dinoseg_op_qkv_gemm(Ap.data_ptr(), B * ntok * D, Wp.data_ptr(), 3 * D * D, bias.data_ptr(), B,
                                              ntok, npad, H, planes, qscale, q.data_ptr(), k.data_ptr(), vt.data_ptr(),
                                              plane, S()))
    ref = (quant_like(A, planes).double() @ quant_like(W, planes).double().t() + bias.double()).float()
    ref = ref.reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)     # vision_transformer.py:82
    tol = (2.0 ** -8 if planes == 1 else 2.0 ** -15) * float(ref.abs().max()) + 1e-4
    gq, gk, gv = unpack(q), unpack(k), unpack(vt)
    assert float((gq[:, :, :ntok] - ref[0] * qscale).abs().max()) <= tol
    assert float((gk[:, :, :ntok] - ref[1]).abs().max()) <= tol
    assert float((gv[:, :, :ntok] - ref[2]).abs().max()) <= tol
    assert torch.all(gq[:, :, ntok:] == 0) and torch.all(gk[:, :, ntok:] == 0) and torch.all(gv[:, :, ntok:] == 0)


def _attention_case(B, H, ntok, planes, seed, spike=False, want_lse=True):
    npad = (ntok + 63) // 64 * 64
    g = np.random.default_rng(seed)
    Q = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    K = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    V = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32))
    if spike:   # force the online-softmax rescale late in the sweep: one key dominates one query row
        # (True: log2-domain score ~104, still a finite 2^S; "over": ~208, 2^S overflows fp32 -> the zero-reference kernel's
        #  exact recomputation; "under": every score of row 7 below -126, every 2^S flushes to 0 -> same path)
        #  "bigv": score ~122 with |V| ~ 1000: the row sum stays finite (2^122) while sum(P V) passes 2^128 -> only the safe band
        #  on the row sum [2^-60, 2^60] sends the row to the exact path; "lowmax": row 7's scores around -117 +- 7: the sum stays
        #  > 0 but its entries below -126 are flushed by v_exp -> same band)
        K[:, :, ntok - 3] = Q[:, :, 5] * {"over": 8.0, "bigv": 4.7}.get(spike, 4.0)
        if spike == "bigv":
            V = V * 1000.0
        if spike in ("under", "lowmax"):
            u = torch.zeros(64)
            u[3] = 1.0
            Q[:, :, 7] = (30.0 if spike == "under" else 25.0) * u
            K = K - (30.0 if spike == "under" else 24.5) * u
    qs = Q * (0.125 * LOG2E)

    def planes_of(x, shape_pad):
        full = torch.zeros(shape_pad, dtype=torch.float32)
        full[tuple(slice(0, s) for s in x.shape)] = x
        flat = full.reshape(-1, shape_pad[-1]).cuda()
        return pack(flat, planes)

    qp = planes_of(qs, (B, H, npad, 64))
    kp = planes_of(K, (B, H, npad, 64))
    vp = planes_of(V, (B, H, npad, 64))
    ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
    lse = torch.zeros((B, H, ntok), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_attention(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), B * H * npad * 64,
                                               ctx.data_ptr(), B * ntok * H * 64, lse.data_ptr() if want_lse else None, B, H, ntok,
                                               npad, planes, S()))
    torch.cuda.synchronize()
    # fp64 reference on the operands the kernel saw
    qq = unpack(qp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu() / LOG2E
    kk = unpack(kp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    vv = unpack(vp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    s = qq @ kk.transpose(-1, -2)
    p = torch.softmax(s, dim=-1)
    ref = (p @ vv).transpose(1, 2).reshape(B * ntok, H * 64).float()
    ref_lse = (torch.logsumexp(s, dim=-1) * LOG2E).float()
    got = unpack(ctx).cpu()
    return got, ref, lse.cpu(), ref_lse


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("B,H,ntok", [(1, 1, 64), (2, 2, 197), (1, 3, 65), (1, 1, 901), (1, 2, 3601)])
def test_attention(cuda, planes, B, H, ntok):
    got, ref, lse, ref_lse = _attention_case(B, H, ntok, planes, seed=ntok + planes)
    tol = 1.2e-2 if planes == 1 else 1e-4      # bf16 probabilities vs hi+lo split
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max()) <= tol
    # l is summed on the matrix core from the bf16(/hi+lo) probabilities: ~2^-9 (2^-16) relative on l
    assert float((lse - ref_lse).abs().max()) <= (6e-3 if planes == 1 else 1e-4)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("spike", [True, "over", "under", "bigv", "lowmax"])
def test_attention_rescale_branch(cuda, planes, spike):
    """One key dominating a row late in the sweep (the reference-moving path of the online-softmax kernels), scores whose 2^S
    overflows fp32 and a row whose 2^S all flush to zero (the exact two-pass recomputation of the zero-reference kernel).
    bf16 mode: the zero-reference kernel rounds the dominant probability to bf16 (2^-9 relative on that row's output) where a
    kernel whose reference is the row maximum has it exactly 1."""
    got, ref, lse, ref_lse = _attention_case(1, 1, 300, planes, seed=77, spike=spike)
    assert torch.isfinite(got).all() and torch.isfinite(lse).all()
    # ("under" / "lowmax" multiply operands of magnitude 25-30: the dropped lo*lo term of the hi+lo products is 2^-18 of scores of
    #  ~600-900; "bigv" scales the outputs by 1000)
    tol2 = 5e-3 if spike in ("under", "lowmax") else 1e-4
    vs = 1000.0 if spike == "bigv" else 1.0
    assert float((got - ref).abs().max()) <= (2e-2 if planes == 1 else tol2) * vs
    assert float((lse - ref_lse).abs().max()) <= (6e-3 if planes == 1 else 50 * tol2)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 11, 27])
def test_attention_kernel_variants(cuda, planes, variant):
    """dinoseg_set_option('attn_variant'): bit 0 = overflow check on the row sums instead of a per-tile row maximum, bit 1 =
    idle waves of the last q-tile skip the tile work, (bit 2 = software-pipelined kernel: only in `make EXPERIMENTS=1` builds), bit 3 = zero-reference kernel
    (bf16, the default), bit 4 = zero-reference hi+lo kernel (12 waves; measured, not the default).  Without a rescale after the first tile both bits do the same
    arithmetic in the same order as the base kernel."""
    lib = capi.lib()
    with dino_amd.options(attn_variant=0):
        base, ref, lse0, ref_lse = _attention_case(2, 2, 197, planes, seed=5)
        capi.check(lib.dinoseg_set_option(b"attn_variant", variant))
        got, _, lse, _ = _attention_case(2, 2, 197, planes, seed=5)
        got2, ref2, lse2, ref_lse2 = _attention_case(1, 1, 300, planes, seed=77, spike=True)     # rescale path
        got3, ref3, _, _ = _attention_case(1, 2, 3601, planes, seed=9)      # 17 valid rows in the last q-tile
        small = [_attention_case(1, 1, n, planes, seed=n) for n in (1, 33, 64, 65, 128, 129)]   # 1, 2 and 3 tiles, ragged or not
    tol = 1.2e-2 if planes == 1 else 1e-4
    lse_tol = 6e-3 if planes == 1 else 1e-4
    # (the pipelined / zero-reference kernels (bits 2, 3: bf16 only; bit 4: the hi+lo zero-reference kernel) round differently)
    if not (variant & 12) if planes == 1 else not (variant & 16):
        assert torch.equal(got, base) and torch.equal(lse, lse0)
    assert float((got - ref).abs().max()) <= tol and float((lse - ref_lse).abs().max()) <= lse_tol
    assert float((got2 - ref2).abs().max()) <= (2e-2 if planes == 1 else tol) and float((got3 - ref3).abs().max()) <= tol
    assert float((lse2 - ref_lse2).abs().max()) <= lse_tol
    for g, r, l, rl in small:
        assert float((g - r).abs().max()) <= tol and float((l - rl).abs().max()) <= lse_tol


@pytest.mark.parametrize("mq", [1, 2])
@pytest.mark.parametrize("fp16", [False, True])
def test_attention_za_is_bit_identical_to_the_compiled_kernel(cuda, fp16, mq):
    """attention_za.hip (attn_variant bits 10 + 11: the tile loop as a hand-scheduled assembly pipeline, at every grid size) against
    attn_fwd_z_kernel<1, 4, 8> (bit 9: no key split; bit 12: its 256-query workgroups at every grid size -- the exact recomputation is
    decided per workgroup, so the two kernels must cut the queries alike): ctx and the log-sum-exp equal BIT FOR BIT on one to 57 tiles,
    ragged or not (1, 17, 32, 33, 63 valid keys in the last tile), one and several (batch, head) pairs per XCD, idle waves in the last
    q-tile, and on the exact-recomputation path (a 2^S that overflows, a row whose 2^S all flush, |V| ~ 1000, flushed entries)."""
    lib = capi.lib()
    shapes = [(1, 1, 1), (1, 1, 17), (1, 1, 50), (1, 1, 64), (1, 3, 65), (1, 1, 96), (1, 1, 128), (2, 2, 129), (2, 2, 197), (1, 1, 255),
              (1, 2, 256), (1, 1, 257), (1, 9, 300), (1, 1, 901), (2, 5, 1000), (1, 2, 3601)]
    spikes = ["over", "under", "bigv", "lowmax", True]

    def run(variant):
        capi.check(lib.dinoseg_set_option(b"attn_variant", variant))
        out = []
        for B, H, ntok in shapes:
            got, ref, lse, ref_lse = (_attention_case_fp16(B, H, ntok) if fp16 else _attention_case(B, H, ntok, 1, seed=ntok))
            out.append((got, lse, ref, ref_lse))
        if not fp16:
            for sp in spikes:
                got, ref, lse, ref_lse = _attention_case(1, 1, 300, 1, seed=77, spike=sp)
                out.append((got, lse, ref, ref_lse))
        return out
    with dino_amd.options():
        base = run(11 | 512 | 4096)
        new = run(11 | 512 | 1024 | 2048 | (65536 if mq == 2 else 0))       # (bit 16: 64 queries per wave)
    names = [f"{s}" for s in shapes] + ([f"spike {s}" for s in spikes] if not fp16 else [])
    for name, (g0, l0, ref, _), (g1, l1, _, _) in zip(names, base, new):
        assert torch.isfinite(g1).all(), name
        assert float((g1 - ref).abs().max()) <= (2e-2 * (1000.0 if "bigv" in name else 1.0)), name
        assert torch.equal(g0, g1), f"{name}: {(g0 != g1).float().mean():.4f} of ctx differs, max {float((g0 - g1).abs().max()):.3e}"
        if l0 is not None:
            assert torch.equal(l0, l1), f"{name}: lse differs"


@pytest.mark.parametrize("planes", [1, 2])
def test_attention_za_bit_identical_at_14401_tokens(cuda, planes):
    """BASELINE configs[2]'s sequence (960 x 960: 14 401 tokens = 226 tiles, 57 q-tiles, the last with one query row): the assembly
    kernels against the compiled ones, outputs only (the fp64 reference of this size is test_attention_14401_tokens_sampled_rows')."""
    lib = capi.lib()
    B, H, ntok = 1, 2, 14401
    npad = (ntok + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(14401 + planes)
    mk = lambda sc: (torch.randn((planes, B * H * npad, 64), device="cuda", generator=g) * sc).to(torch.bfloat16).view(torch.int16)
    q, k, v = mk(0.5), mk(0.5), mk(1.0)
    outs = []
    with dino_amd.options():
        for variant in ((11 | 512 | 4096, 11 | 512 | 1024 | 2048, 11 | 512 | 1024 | 2048 | 65536) if planes == 1 else (11 | 16, 11 | 16 | 1024 | 2048)):
            capi.check(lib.dinoseg_set_option(b"attn_variant", variant))
            ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
            lse = torch.zeros((B, H, ntok), dtype=torch.float32, device="cuda")
            capi.check(lib.dinoseg_op_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B * H * npad * 64, ctx.data_ptr(),
                                                B * ntok * H * 64, lse.data_ptr(), B, H, ntok, npad, planes, S()))
            torch.cuda.synchronize()
            outs.append((ctx, lse))
    assert torch.isfinite(outs[0][1]).all() and bool((outs[0][0] != 0).any())
    for ctx, lse in outs[1:]:
        assert torch.equal(ctx, outs[0][0]) and torch.equal(lse, outs[0][1])


@pytest.mark.parametrize("fp16", [False, True])
def test_attention_za_hi_lo_planes_bit_identical(cuda, fp16):
    """attention_za.hip's hi + lo body (three MFMAs per product, probabilities split in registers, 32 KiB ring slots) against the compiled
    zero-reference hi + lo kernel attn_fwd_z_kernel<2, 3, 12, FMT> (attn_variant bit 4, bit 10 clear): ctx planes and log-sum-exp bit for
    bit, bf16 planes and the mixed format of precision 'fp16x3' at large batch (Q / K / ctx fp16 hi + lo, V and P bf16 hi + lo), exact
    path included (one workgroup on both sides: the two kernels cut the queries differently, 384 / 256 per workgroup)."""
    lib = capi.lib()
    shapes = [(1, 1, 1), (1, 1, 50), (1, 3, 65), (1, 1, 128), (2, 2, 197), (1, 2, 256), (1, 9, 300), (2, 5, 1000), (1, 2, 3601)]
    spikes = ["over", "under", "bigv", "lowmax", True]

    def run(variant):
        capi.check(lib.dinoseg_set_option(b"attn_variant", variant))
        out = [_attention_case_x3(B, H, ntok, fp16) for B, H, ntok in shapes]
        out += [_attention_case_x3(1, 1, 200, fp16, spike=sp) for sp in spikes]
        return out
    with dino_amd.options():
        base = run(11 | 16)
        new = run(11 | 16 | 1024 | 2048)
    names = [f"{s}" for s in shapes] + [f"spike {s}" for s in spikes]
    for name, (g0, l0, ref, ref_lse), (g1, l1, _, _) in zip(names, base, new):
        assert torch.isfinite(g1).all(), name
        tol = 1e-4 * (1000.0 if "bigv" in name else 1.0) * (50.0 if ("under" in name or "lowmax" in name) else 1.0)
        assert float((g1 - ref).abs().max()) <= tol, f"{name}: {float((g1 - ref).abs().max()):.3e}"
        assert torch.equal(g0, g1), f"{name}: {(g0 != g1).float().mean():.4f} of ctx differs, max {float((g0 - g1).abs().max()):.3e}"
        if l0 is not None:
            assert torch.equal(l0, l1), f"{name}: lse differs"
            assert float((l1 - ref_lse).abs().max()) <= 5e-3, name


def _attention_case_x3(B, H, ntok, fp16, spike=False):
    """hi + lo planes through dinoseg_op_attention; fp16: Q / K fp16 planes, V bf16 planes (option op_v_bf16), ctx fp16 planes, no LSE;
    returns (ctx as fp32 = hi + lo, lse or None, fp64 reference on the operands the kernel saw, reference lse)"""
    npad = (ntok + 63) // 64 * 64
    g = np.random.default_rng(1000 + ntok)
    Q = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    K = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    V = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32))
    if spike:
        K[:, :, ntok - 3] = Q[:, :, 5] * {"over": 8.0, "bigv": 4.7}.get(spike, 4.0)
        if spike == "bigv":
            V = V * 1000.0
        if spike in ("under", "lowmax"):
            u = torch.zeros(64)
            u[3] = 1.0
            Q[:, :, 7] = (30.0 if spike == "under" else 25.0) * u
            K = K - (30.0 if spike == "under" else 24.5) * u
    qs = Q * (0.125 * LOG2E)

    def padded(x):
        full = torch.zeros((B, H, npad, 64), dtype=torch.float32)
        full[:, :, :ntok] = x
        return full.reshape(-1, 64).cuda()
    lib = capi.lib()
    h16 = lambda t: t.view(torch.float16).float().sum(dim=0)
    with dino_amd.options(op_fmt=int(fp16), op_v_bf16=int(fp16)):
        qp, kp = pack(padded(qs), 2), pack(padded(K), 2)
        with dino_amd.options(op_fmt=0):
            vp = pack(padded(V), 2)
        ctx = torch.zeros((2, B * ntok, H * 64), dtype=torch.int16, device="cuda")
        lse = None if fp16 else torch.zeros((B, H, ntok), dtype=torch.float32, device="cuda")
        capi.check(lib.dinoseg_op_attention(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), B * H * npad * 64, ctx.data_ptr(),
                                            B * ntok * H * 64, capi.ptr(lse), B, H, ntok, npad, 2, S()))
        torch.cuda.synchronize()
    un = h16 if fp16 else unpack
    qq = un(qp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu() / LOG2E
    kk = un(kp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    vv = unpack(vp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    sc = qq @ kk.transpose(-1, -2)
    ref = (torch.softmax(sc, dim=-1) @ vv).transpose(1, 2).reshape(B * ntok, H * 64).float()
    ref_lse = (torch.logsumexp(sc, dim=-1) * LOG2E).float()
    return un(ctx).cpu(), None if lse is None else lse.cpu(), ref, ref_lse


def _attention_case_fp16(B, H, ntok):
    """fp16 Q / K (pre-scaled), bf16 V: the operand formats of precision 'fp16'; returns (ctx, fp64 reference, None, None)"""
    npad = (ntok + 63) // 64 * 64
    g = np.random.default_rng(ntok)
    Q = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5 * (0.125 * LOG2E)
    K = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    V = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32))

    def padded(x):
        full = torch.zeros((B, H, npad, 64), dtype=torch.float32)
        full[:, :, :ntok] = x
        return full.reshape(-1, 64).cuda()
    lib = capi.lib()
    with dino_amd.options(op_fmt=1):
        qp, kp = pack(padded(Q), 1), pack(padded(K), 1)
        with dino_amd.options(op_fmt=0):
            vp = pack(padded(V), 1)
        ctx = torch.zeros((1, B * ntok, H * 64), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_attention(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), B * H * npad * 64, ctx.data_ptr(),
                                            B * ntok * H * 64, None, B, H, ntok, npad, 1, S()))
        torch.cuda.synchronize()
    h = lambda t: t.view(torch.float16).float()
    qq = h(qp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu() / LOG2E
    kk = h(kp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    vv = unpack(vp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    ref = (torch.softmax(qq @ kk.transpose(-1, -2), dim=-1) @ vv).transpose(1, 2).reshape(B * ntok, H * 64).float()
    return h(ctx[0]).cpu(), ref, None, None


@pytest.mark.parametrize("D", [128, 384, 768])
def test_layernorm(cuda, D):
    M, ntok = 2 * 37, 37
    x = seeded((M, D), 8) * 3 + 0.7
    g, b = 1 + 0.2 * seeded((D,), 9), 0.1 * seeded((D,), 10)
    ref = O.layer_norm(x.cpu(), g.cpu(), b.cpu(), 1e-6)
    lib = capi.lib()
    for planes in (1, 2):
        outp = torch.zeros((planes, M, D), dtype=torch.int16, device="cuda")
        of = torch.zeros((M, D), device="cuda")
        capi.check(lib.dinoseg_op_layernorm(x.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-6, M, D, outp.data_ptr(), M * D,
                                            planes, of.data_ptr(), 0, ntok, S()))
        assert float((of.cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-6
        assert float((unpack(outp).cpu() - ref).abs().max()) <= (2.0 ** -8 if planes == 1 else 2.0 ** -15) * float(ref.abs().max())
    # drop-CLS remap used by the final norm (vision_transformer.py:243 + pl_torch_modules.py:243)
    of = torch.zeros((M - 2, D), device="cuda")
    capi.check(lib.dinoseg_op_layernorm(x.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-6, M, D, None, 0, 1, of.data_ptr(), 1,
                                        ntok, S()))
    want = ref.reshape(2, ntok, D)[:, 1:].reshape(-1, D)
    assert float((of.cpu() - want).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-6


@pytest.mark.parametrize("o", [8, 28, 30, 60, 120])
def test_pos_resample(cuda, o):
    g, D = 28, 64
    pe = seeded((1, g * g + 1, D), 11)
    ref = O.resample_pos_embed(pe.cpu(), o)[0]
    out = torch.zeros((o * o + 1, D), device="cuda")
    capi.check(capi.lib().dinoseg_op_pos_resample(pe.data_ptr(), g, D, o, out.data_ptr(), S()))
    assert float((out.cpu() - ref).abs().max()) <= 1e-5


def test_patch_gather(cuda):
    B, r = 2, 64
    frames = np.random.default_rng(3).integers(0, 256, (B, r, r, 3), dtype=np.uint8)
    x = O.preprocess(frames)                                     # fp32 [B,3,r,r]
    o = r // 8
    want = x.reshape(B, 3, o, 8, o, 8).permute(0, 2, 4, 1, 3, 5).reshape(B * o * o, 192)
    lib = capi.lib()
    fr = torch.from_numpy(frames).cuda()
    out = torch.zeros((2, B * o * o, 192), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_patch_gather(fr.data_ptr(), capi.INPUT_U8_HWC, B, r, out.data_ptr(), B * o * o * 192, 2, S()))
    assert float((unpack(out).cpu() - want).abs().max()) <= 2.0 ** -15 * 3
    xc = x.cuda().contiguous()
    out1 = torch.zeros((1, B * o * o, 192), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_patch_gather(xc.data_ptr(), capi.INPUT_F32_CHW, B, r, out1.data_ptr(), B * o * o * 192, 1, S()))
    assert torch.equal(out1.view(torch.bfloat16)[0].cpu(), want.to(torch.bfloat16))


@pytest.mark.parametrize("C,K,ld", [(7, 100, 128), (7, 384, 384), (21, 100, 128)])
def test_head_final(cuda, C, K, ld):
    M = 333
    x = torch.zeros((M, ld))
    x[:, :K] = torch.relu(seeded((M, K), 12).cpu())
    Wc, b = seeded((C, K), 13) * 0.3, seeded((C,), 14)
    xp = pack(x.cuda(), 2)
    logp = torch.zeros((M, C), device="cuda")
    am = torch.zeros((M,), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_head_final(xp.data_ptr(), M * ld, ld, M, K, Wc.data_ptr(), b.data_ptr(), C,
                                                logp.data_ptr(), am.data_ptr(), S()))
    z = unpack(xp).cpu()[:, :K] @ Wc.cpu().t() + b.cpu()
    ref = torch.log_softmax(z, dim=1)
    assert float((logp.cpu() - ref).abs().max()) <= 2e-5
    assert torch.equal(am.cpu().long(), ref.argmax(dim=1))


@pytest.mark.parametrize("B,H,ntok", [(1, 6, 3601), (1, 2, 1024), (2, 3, 901), (1, 1, 257)])
def test_attention_key_split_for_small_grids(cuda, B, H, ntok):
    """Fewer 128-query workgroups than CUs (a single frame) in an inference call (no LSE asked for): attn_fwd_zs_kernel splits the K/V
    tiles of a q-tile over two or three wave groups and adds the partial O / row sums.  Against the unsplit kernel (attn_variant bit 9):
    the same result up to the summation order -- one place of the bf16 output on a few elements per thousand -- and both within the
    usual bound of the fp64 reference; on the exact path (a dominant key late in the sweep) group 0 recomputes in the unsplit kernel's
    order: identical.  With an LSE output (the training forward) the keys are never split: one arithmetic at every batch size."""
    with dino_amd.options(attn_variant=dino_amd.get_option("attn_variant") | 512):
        base, ref, _, _ = _attention_case(B, H, ntok, 1, seed=ntok, want_lse=False)
        ex0 = _attention_case(1, 1, 300, 1, seed=77, spike="over", want_lse=False)
        tr0 = _attention_case(B, H, ntok, 1, seed=ntok)
    got, _, _, _ = _attention_case(B, H, ntok, 1, seed=ntok, want_lse=False)
    ex1 = _attention_case(1, 1, 300, 1, seed=77, spike="over", want_lse=False)
    tr1 = _attention_case(B, H, ntok, 1, seed=ntok)
    assert float((got - ref).abs().max()) <= 1.5e-2 and float((base - ref).abs().max()) <= 1.5e-2
    d = (got - base).abs()
    assert bool((d > 0).any()), "the split kernel was not dispatched"
    assert float((d / (base.abs() + 1e-3)).max()) <= 2.0 ** -7 and float((d > 0).float().mean()) <= 5e-3
    assert torch.equal(ex0[0], ex1[0])
    assert torch.equal(tr0[0], tr1[0]) and torch.equal(tr0[2], tr1[2])


@pytest.mark.parametrize("planes,M", [(1, 3000), (2, 3000), (2, 1409)])
def test_gemm_big_matches_small_kernel(cuda, planes, M):
    """Same operands through both GEMM kernels (dinoseg_set_option('gemm_big', 0/1/2)): identical up to fp32 summation order.
    planes = 2: the 128x384 hi+lo configuration of the persistent kernel (three MFMAs per product)."""
    N, K = 1152, 384                  # M = 3000: 11.7 row panels of 256 / 23.4 of 128 -- the last one is ragged (plain residual path)
    A, W, bias = seeded((M, K), 31), seeded((N, K), 32) * 0.1, seeded((N,), 33)
    Ap, Wp = pack(A, planes), pack(W, planes)
    lib = capi.lib()
    outs = []
    X0 = seeded((M, N), 34)
    for big in (0, 1, 2):          # 0: 128x128 kernel; 1: auto; 2: persistent kernel wherever it applies
        with dino_amd.options(gemm_big=big):
            out = torch.zeros((M, N), device="cuda")
            capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_PLAIN,
                                           bias.data_ptr(), out.data_ptr(), None, 0, 0, S()))
            X = X0.clone()
            capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_RESID,
                                           bias.data_ptr(), X.data_ptr(), None, 0, 0, S()))
            g = torch.zeros((planes, M, N), dtype=torch.int16, device="cuda")
            capi.check(lib.dinoseg_op_gemm(Ap.data_ptr(), M * K, K, Wp.data_ptr(), N * K, M, N, K, planes, capi.EPI_GELU,
                                           bias.data_ptr(), None, g.data_ptr(), M * N, N, S()))
            outs.append((out, X, unpack(g)))
    scale = float(outs[0][0].abs().max())
    ref = (unpack(Ap).double() @ unpack(Wp).double().t() + bias.double())
    for big in (1, 2):
        assert float((outs[0][0] - outs[big][0]).abs().max()) <= 2e-5 * scale, big
        assert float((outs[0][1] - outs[big][1]).abs().max()) <= 2e-5 * scale, big
        gtol = 2.0 ** -7 if planes == 1 else 2.0 ** -14      # planes = 1: one kernel uses the fitted GELU, the other the erf form
        assert float((outs[0][2] - outs[big][2]).abs().max()) <= gtol * float(outs[0][2].abs().max()), big
    # against fp64 on the packed operands (fp32 accumulation; planes = 2 drops only the lo*lo terms), and no worse than the 128x128 kernel
    err_big, err_small = (float((outs[i][0].double() - ref).abs().max()) for i in (2, 0))
    assert err_big <= 2e-5 * scale and err_big <= 2.0 * err_small + 1e-7 * scale, (err_big, err_small, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("sh,sw,dh,dw", [(48, 64, 40, 40), (30, 30, 64, 64), (64, 64, 32, 32), (1, 1, 8, 8), (37, 91, 24, 56),
                                         (480, 640, 480, 480)])
def test_resize_u8(cuda, sh, sw, dh, dw):
    """dinoseg_op_resize_u8 (cv2.INTER_LINEAR fixed-point restatement) is bit-exact against the scalar oracle (small cases)
    and the host mirror (the 640x480 robot-frame case, too slow for the pixel-at-a-time oracle)."""
    from dino_amd.preprocess import resize_linear_u8
    from oracle.resize_oracle import resize_linear_u8 as ref
    img = np.random.default_rng(sh * 1000 + sw).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    src = torch.from_numpy(img).cuda()
    dst = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().dinoseg_op_resize_u8(src.data_ptr(), sh, sw, dst.data_ptr(), dh, dw, S()))
    got = dst.cpu().numpy()
    assert np.array_equal(got, resize_linear_u8(img, dh, dw))
    if sh * sw <= 64 * 64 and dh * dw <= 64 * 64:
        assert np.array_equal(got, ref(img, dh, dw))


@pytest.mark.parametrize("planes", [1, 2])
def test_attention_14401_tokens_sampled_rows(cuda, planes):
    """The @960 sequence length (226 key tiles, 113 query tiles per head) in both precisions against an fp64 reference on
    sampled query rows (the full 14 401^2 reference would take minutes on the host)."""
    B, H, ntok = 1, 2, 14401
    npad = (ntok + 63) // 64 * 64
    g = np.random.default_rng(960 + planes)
    Q = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    K = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32)) * 1.5
    V = torch.from_numpy(g.standard_normal((B, H, ntok, 64)).astype(np.float32))

    def planes_of(x):
        full = torch.zeros((B, H, npad, 64), dtype=torch.float32)
        full[:, :, :ntok] = x
        return pack(full.reshape(-1, 64).cuda(), planes)

    qp, kp, vp = planes_of(Q * (0.125 * LOG2E)), planes_of(K), planes_of(V)
    ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
    lse = torch.zeros((B, H, ntok), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().dinoseg_op_attention(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), B * H * npad * 64, ctx.data_ptr(),
                                               B * ntok * H * 64, lse.data_ptr(), B, H, ntok, npad, planes, S()))
    torch.cuda.synchronize()
    rows = torch.from_numpy(np.sort(np.concatenate([g.choice(ntok, 500, replace=False), [0, 127, 128, 14335, 14336, 14400]])))
    qq = unpack(qp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()[:, :, rows] / LOG2E
    kk = unpack(kp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    vv = unpack(vp).reshape(B, H, npad, 64)[:, :, :ntok].double().cpu()
    s = qq @ kk.transpose(-1, -2)
    ref = (torch.softmax(s, dim=-1) @ vv).float()                     # [B, H, rows, 64]
    ref_lse = (torch.logsumexp(s, dim=-1) * LOG2E).float()
    got = unpack(ctx).cpu().reshape(B, ntok, H, 64).permute(0, 2, 1, 3)[:, :, rows]
    assert torch.isfinite(unpack(ctx)).all()
    assert float((got - ref).abs().max()) <= (1.2e-2 if planes == 1 else 1e-4)
    assert float((lse.cpu()[:, :, rows] - ref_lse).abs().max()) <= (6e-3 if planes == 1 else 1e-4)


def _ln_ref(X, g, b, eps=1e-6):
    return O.layer_norm(X.cpu(), g.cpu(), b.cpu(), eps)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("M_,N", [(394, 768), (115, 768), (128 * 3, 1536), (128 * 300 + 77, 640)])
def test_ln_gemm_gelu(cuda, planes, M_, N):
    """LayerNorm fused into the fc1 GEMM (gemm_ln.hip): out = gelu(LN(X) W^T + b), plus the by-products a training forward
    keeps (normalised planes, pre-activation planes); ragged last panel, single partial panel, whole panels."""
    K = 384             # N = 640: a partial last column tile; M = 38 477: several panels per workgroup (persistent walk)
    X = seeded((M_, K), 11) * 1.7 + 0.4
    gam, bet = 1 + 0.2 * seeded((K,), 12), 0.1 * seeded((K,), 13)
    W, bias = seeded((N, K), 14) * 0.1, seeded((N,), 15)
    Wp = pack_slabs(W, planes)
    out = torch.zeros((planes, M_, N), dtype=torch.int16, device="cuda")
    aout = torch.zeros((planes, M_, K), dtype=torch.int16, device="cuda")
    pre = torch.zeros((planes, M_, N), dtype=torch.int16, device="cuda")
    capi.check(capi.lib().dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), N * K, bias.data_ptr(),
                                             M_, N, K, planes, capi.EPI_GELU, out.data_ptr(), M_ * N, None, None, None, 0, 0, 0, 6, 0.0,
                                             aout.data_ptr(), pre.data_ptr(), S()))
    A = _ln_ref(X, gam, bet)
    tol = 2.0 ** -8 if planes == 1 else 2.0 ** -15
    got_a = unpack(aout).cpu()
    assert float((got_a - A).abs().max()) <= tol * float(A.abs().max()) + 1e-5
    # the product of the operands the kernel saw (its own normalised planes)
    z = (got_a.double() @ quant_like(W, planes).cpu().double().t() + bias.cpu().double()).float()
    got_pre = unpack(pre).cpu()
    assert float((got_pre - z).abs().max()) <= tol * float(z.abs().max()) + 2e-4
    want = O.gelu_erf(z)
    assert float((unpack(out).cpu() - want).abs().max()) <= tol * float(want.abs().max()) + 2e-4
    # without the by-products: same output bits
    out2 = torch.zeros_like(out)
    capi.check(capi.lib().dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), N * K, bias.data_ptr(),
                                             M_, N, K, planes, capi.EPI_GELU, out2.data_ptr(), M_ * N, None, None, None, 0, 0, 0, 6, 0.0,
                                             None, None, S()))
    assert torch.equal(out2, out)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("B,ntok", [(2, 197), (1, 65), (3, 130)])
def test_ln_gemm_qkv_layout(cuda, planes, B, ntok):
    """LayerNorm fused into the qkv GEMM: same [B,H,npad,64] scatter, Q pre-scaled, pad rows untouched (zero)."""
    H, K = 6, 384
    D, npad, M_ = 384, (ntok + 63) // 64 * 64, B * ntok
    X = seeded((M_, K), 21) * 2.0 - 0.3
    gam, bet = 1 + 0.2 * seeded((K,), 22), 0.1 * seeded((K,), 23)
    W, bias = seeded((3 * D, K), 24) * 0.1, seeded((3 * D,), 25)
    Wp = pack_slabs(W, planes)
    plane = B * H * npad * 64
    q = torch.zeros((planes, B, H, npad, 64), dtype=torch.int16, device="cuda")
    k, vt = torch.zeros_like(q), torch.zeros_like(q)
    qscale = 0.125 * LOG2E
    capi.check(capi.lib().dinoseg_op_ln_gemm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), 3 * D * K,
                                             bias.data_ptr(), M_, 3 * D, K, planes, 4, None, 0, q.data_ptr(), k.data_ptr(), vt.data_ptr(),
                                             plane, ntok, npad, H, qscale, None, None, S()))
    A = quant_like(_ln_ref(X, gam, bet).cuda(), planes)
    ref = (A.double() @ quant_like(W, planes).double().t() + bias.double()).float()
    ref = ref.reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    # the kernel's own LayerNorm differs from the oracle's by fp32 rounding, which can move a bf16 rounding point of A
    tol = (2.0 ** -7 if planes == 1 else 2.0 ** -14) * float(ref.abs().max()) + 1e-4
    gq, gk, gv = unpack(q), unpack(k), unpack(vt)
    assert float((gq[:, :, :ntok] - ref[0] * qscale).abs().max()) <= tol
    assert float((gk[:, :, :ntok] - ref[1]).abs().max()) <= tol
    assert float((gv[:, :, :ntok] - ref[2]).abs().max()) <= tol
    assert torch.all(gq[:, :, ntok:] == 0) and torch.all(gk[:, :, ntok:] == 0) and torch.all(gv[:, :, ntok:] == 0)


def pack_mlp(W1: torch.Tensor, W2: torch.Tensor) -> torch.Tensor:
    F_, D_ = W1.shape
    n = capi.lib().dinoseg_op_mlp_fused_pack_elems(D_, F_)
    assert n == 2 * D_ * F_
    out = torch.empty((n,), dtype=torch.int16, device=W1.device)
    capi.check(capi.lib().dinoseg_op_pack_mlp(W1.contiguous().data_ptr(), W2.contiguous().data_ptr(), D_, F_, out.data_ptr(), S()))
    return out


@pytest.mark.parametrize("M_", [128, 77, 128 * 5 + 33, 128 * 300 + 19])
def test_mlp_fused(cuda, M_):
    """LN2 + fc1 + GELU + fc2 + residual in one launch (mlp_fused2.hip), bf16 operands: against fp64 on the operands the kernel
    sees (bf16 LayerNorm output, bf16 weights, bf16 GELU output).  M = 38 419: more items than CUs (persistent walk, the weight
    ring running on across items), ragged last item; M = 77: one partial item."""
    D_, F_ = 384, 1536
    X = seeded((M_, D_), 31) * 1.7 + 0.4 + torch.arange(D_, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    gam, bet = 1 + 0.2 * seeded((D_,), 32), 0.1 * seeded((D_,), 33)
    W1 = seeded((F_, D_), 34) * 0.06 + torch.arange(F_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b1 = seeded((F_,), 35) * 0.5
    W2 = seeded((D_, F_), 36) * 0.04 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b2 = seeded((D_,), 37)
    Wp = pack_mlp(W1, W2)
    got = X.clone()
    capi.check(capi.lib().dinoseg_op_mlp_fused(got.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), b1.data_ptr(),
                                               b2.data_ptr(), M_, D_, F_, S()))
    torch.cuda.synchronize()
    A = quant_like(_ln_ref(X, gam, bet).cuda(), 1).double()
    z = A @ quant_like(W1, 1).double().t() + b1.double()
    Hq = quant_like(O.gelu_erf(z.float().cpu()).cuda(), 1).double()
    delta = (Hq @ quant_like(W2, 1).double().t() + b2.double())
    want = (X.double() + delta).float()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    scale = float(delta.abs().max())
    # what is left: fp32 summation order, the fitted GELU (2.6e-5), and bf16 rounding points of LN / GELU outputs that the
    # kernel's own fp32 arithmetic moves by one ulp (each moves one of 1536 products by 2^-8 of itself)
    assert err <= 2.0 ** -9 * scale + 1e-3, (err, scale)
    # and the update is not a near-miss of something else: it carries the whole MLP term
    assert float((got - X).abs().max()) > 0.5 * scale


@pytest.mark.parametrize("M_", [128, 77, 128 * 5 + 33, 128 * 300 + 19])
def test_proj_mlp_fused(cuda, M_):
    """The attention output projection + the MLP half of a block in ONE launch (mlp_fused2.hip, PROJ):
        x += ctx . Wproj^T + bproj;   x += fc2(gelu(fc1(LayerNorm(x))))      (vision_transformer.py:104-105, :123, :135)
    against fp64 on the operands the kernel sees (bf16 ctx / weights, bf16 LayerNorm and GELU outputs), and against the two-launch
    path it replaces (dinoseg_op_gemm EPI_RESID, then dinoseg_op_mlp_fused).  M = 38 419: more items than CUs (the projection
    k-tiles and ctx tiles of the next item are prefetched across the item boundary); 77 / 673: ragged last item (clamped rows)."""
    D_, F_ = 384, 1536
    X = seeded((M_, D_), 41) * 1.7 + 0.4 + torch.arange(D_, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    ctx = quant_like(seeded((M_, D_), 48) * 0.8, 1)
    Wpr = seeded((D_, D_), 49) * 0.07 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    bpr = seeded((D_,), 50) * 0.3
    gam, bet = 1 + 0.2 * seeded((D_,), 42), 0.1 * seeded((D_,), 43)
    W1 = seeded((F_, D_), 44) * 0.06 + torch.arange(F_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b1 = seeded((F_,), 45) * 0.5
    W2 = seeded((D_, F_), 46) * 0.04 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b2 = seeded((D_,), 47)
    lib = capi.lib()
    Wp = pack_mlp(W1, W2)
    n = lib.dinoseg_op_proj_pack_elems(D_)
    assert n == D_ * D_
    Wprp = torch.empty((n,), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_pack_proj(Wpr.data_ptr(), D_, Wprp.data_ptr(), S()))
    ctx_b = pack(ctx, 1)          # bf16 [1][M][D]
    got = X.clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused(got.data_ptr(), ctx_b.data_ptr(), Wprp.data_ptr(), bpr.data_ptr(), gam.data_ptr(),
                                             bet.data_ptr(), 1e-6, Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(), M_, D_, F_, S()))
    torch.cuda.synchronize()
    # fp64 on the kernel's operands
    xmid = X.double() + ctx.double() @ quant_like(Wpr, 1).double().t() + bpr.double()
    A = quant_like(_ln_ref(xmid.float(), gam, bet).cuda(), 1).double()
    z = A @ quant_like(W1, 1).double().t() + b1.double()
    Hq = quant_like(O.gelu_erf(z.float().cpu()).cuda(), 1).double()
    delta = Hq @ quant_like(W2, 1).double().t() + b2.double()
    want = (xmid + delta).float()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    scale = float(delta.abs().max())
    assert err <= 2.0 ** -9 * scale + 1e-3, (err, scale)
    assert float((got - X).abs().max()) > 0.5 * scale
    # the two launches it replaces
    two = X.clone()
    Wq = pack(Wpr, 1)
    capi.check(lib.dinoseg_op_gemm(ctx_b.data_ptr(), M_ * D_, D_, Wq.data_ptr(), D_ * D_, M_, D_, D_, 1, capi.EPI_RESID, bpr.data_ptr(),
                                   two.data_ptr(), None, 0, D_, S()))
    capi.check(lib.dinoseg_op_mlp_fused(two.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(),
                                        M_, D_, F_, S()))
    torch.cuda.synchronize()
    assert float((got - two).abs().max()) <= 2.0 ** -9 * scale + 1e-3


def _q1(x: torch.Tensor, fp16: bool) -> torch.Tensor:
    """the fp32 value of x rounded to the one-plane operand format"""
    return x.to(torch.float16 if fp16 else torch.bfloat16).float()


def _pack_mlp4(Wpr, W1, b1, W2, gam, bet, fp16: bool, tail=None) -> torch.Tensor:
    """tail: (Wqkv_next, bqkv_next, gamma1_next, beta1_next) or None"""
    F_, D_ = W1.shape
    n = capi.lib().dinoseg_op_mlp4_pack_elems(D_, F_)
    assert n == (54 + 18) * 48 * 512 + 2 * (F_ + 3 * D_)      # (the slots, then the folded biases as fp32)
    out = torch.zeros((n,), dtype=torch.int16, device=W1.device)
    t = [x.contiguous().data_ptr() for x in tail] if tail is not None else [None] * 4
    capi.check(capi.lib().dinoseg_op_pack_mlp4(None if Wpr is None else Wpr.contiguous().data_ptr(), W1.contiguous().data_ptr(), b1.data_ptr(),
                                                W2.contiguous().data_ptr(), gam.data_ptr(), bet.data_ptr(), t[0], t[1], t[2], t[3], D_, F_, int(fp16),
                                                out.data_ptr(), S()))
    return out


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B,ntok", [(1, 65), (3, 130), (2, 901), (11, 3601)])
def test_block_tail_fused_one_wave(cuda, B, ntok, fp16):
    """mlp_fused4.hip with the qkv tail: projection + MLP of block i, then LayerNorm1 + qkv of block i + 1 in the same launch
    (vision_transformer.py:123, :135, then :122 -> :75 / :82), one operand plane.  X must equal the launch without the tail bit for bit; Q / K / V
    against fp64 on the operands the kernel sees ((x - mean) rstd and Wqkv diag(gamma1) rounded to the format, the folded bias), in the
    [B, heads, npad, 64] layout with Q pre-scaled, V as bf16 and the pad rows untouched.  (11, 3601): 39 611 rows = more items than CUs, ragged."""
    D_, F_, H = 384, 1536, 6
    M_ = B * ntok
    npad = (ntok + 63) // 64 * 64
    c = _mlp3_case(M_, fp16, 470, tail=True)
    lib = capi.lib()
    ctx_i, _ = _one_plane(c["ctx"], fp16)
    Wp = _pack_mlp4(c["Wpr"], c["W1"], c["b1"], c["W2"], c["gam"], c["bet"], fp16, tail=(c["Wqkv"], c["bq"], c["gam1"], c["bet1"]))
    ref = c["X"].clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused4(ref.data_ptr(), ctx_i.data_ptr(), c["bpr"].data_ptr(), 1e-6, Wp.data_ptr(), c["b2"].data_ptr(), M_, D_, F_,
                                              int(fp16), S()))
    got = c["X"].clone()
    q = torch.zeros((B, H, npad, 64), dtype=torch.int16, device="cuda")
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    qscale = 0.125 * LOG2E
    capi.check(lib.dinoseg_op_block_tail_fused4(got.data_ptr(), ctx_i.data_ptr(), c["bpr"].data_ptr(), 1e-6, Wp.data_ptr(), c["b2"].data_ptr(),
                                                q.data_ptr(), k.data_ptr(), v.data_ptr(), B, ntok, npad, H, qscale, D_, F_, int(fp16), S()))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    xo = got.double()
    mu = xo.mean(dim=1, keepdim=True)
    xhat = (xo - mu) / torch.sqrt(((xo - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
    A = _q1(xhat.float(), fp16).double()
    z = (A @ _q1(c["Wqkv"] * c["gam1"][None, :], fp16).double().t() + (c["bq"].double() + c["Wqkv"].double() @ c["bet1"].double())).float()
    z = z.reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    dt = torch.float16 if fp16 else torch.bfloat16
    gq, gk, gv = q.view(dt).float(), k.view(dt).float(), v.view(torch.bfloat16).float()
    ulp = 2.0 ** -10 if fp16 else 2.0 ** -7
    tol = lambda r, e: 3 * e * float(r.abs().max()) + 1e-4
    eq, ek, ev = (float((g[:, :, :ntok] - r).abs().max()) for g, r in ((gq, z[0] * qscale), (gk, z[1]), (gv, z[2])))
    print(f"tail4 B={B} ntok={ntok} fp16={fp16}: dq {eq:.2e} dk {ek:.2e} dv {ev:.2e}")
    assert eq <= tol(z[0] * qscale, ulp) and ek <= tol(z[1], ulp) and ev <= tol(z[2], 2.0 ** -7)
    assert float(gk.abs().max()) > 0.5
    for t in (q, k, v):
        assert torch.all(t[:, :, ntok:] == 0)
    # bit-repeatable
    q2, k2, v2 = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    again = c["X"].clone()
    capi.check(lib.dinoseg_op_block_tail_fused4(again.data_ptr(), ctx_i.data_ptr(), c["bpr"].data_ptr(), 1e-6, Wp.data_ptr(), c["b2"].data_ptr(),
                                                q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), B, ntok, npad, H, qscale, D_, F_, int(fp16), S()))
    torch.cuda.synchronize()
    assert torch.equal(again, got) and torch.equal(q2, q) and torch.equal(k2, k) and torch.equal(v2, v)


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("M_", [128, 77, 128 * 5 + 33, 128 * 300 + 19])
def test_proj_mlp_fused_one_wave(cuda, M_, fp16):
    """mlp_fused4.hip: the attention output projection + the MLP half of a block in ONE launch with one wave per SIMD, one operand plane:
        x += ctx . Wproj^T + bproj;   x += fc2(gelu(fc1(LayerNorm(x))))      (vision_transformer.py:104-105, :123, :135 -> :59-65)
    against fp64 on the operands the kernel sees (ctx / weights / LayerNorm and GELU outputs rounded to the operand format), and -- bf16
    operands -- against mlp_fused2.hip's launch, which it replaces.  M = 38 419: more items than CUs (the weight stream runs on across
    the item boundary, the next item's rows are loaded in the last step's gaps); 77 / 673: ragged last item (clamped rows)."""
    D_, F_ = 384, 1536
    X = seeded((M_, D_), 41) * 1.7 + 0.4 + torch.arange(D_, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    ctx_i, ctx = _one_plane(seeded((M_, D_), 48) * 0.8, fp16)
    Wpr = seeded((D_, D_), 49) * 0.07 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    bpr = seeded((D_,), 50) * 0.3
    gam, bet = 1 + 0.2 * seeded((D_,), 42), 0.1 * seeded((D_,), 43)
    W1 = seeded((F_, D_), 44) * 0.06 + torch.arange(F_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b1 = seeded((F_,), 45) * 0.5
    W2 = seeded((D_, F_), 46) * 0.04 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b2 = seeded((D_,), 47)
    lib = capi.lib()
    Wp = _pack_mlp4(Wpr, W1, b1, W2, gam, bet, fp16)
    got = X.clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused4(got.data_ptr(), ctx_i.data_ptr(), bpr.data_ptr(), 1e-6, Wp.data_ptr(), b2.data_ptr(), M_, D_, F_,
                                              int(fp16), S()))
    torch.cuda.synchronize()
    xmid = X.double() + ctx.double() @ _q1(Wpr, fp16).double().t() + bpr.double()
    # (the kernel's operands: (x - mean) rstd and W1 diag(gamma), each rounded to the format; the folded bias b1 + W1 beta in fp32)
    mu = xmid.mean(dim=1, keepdim=True)
    xhat = (xmid - mu) / torch.sqrt(((xmid - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
    A = _q1(xhat.float(), fp16).double()
    z = A @ _q1(W1 * gam[None, :], fp16).double().t() + (b1.double() + W1.double() @ bet.double())
    Hq = _q1(O.gelu_erf(z.float().cpu()).cuda(), fp16).double()
    delta = Hq @ _q1(W2, fp16).double().t() + b2.double()
    want = (xmid + delta).float()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    scale = float(delta.abs().max())
    assert err <= 2.0 ** -9 * scale + 1e-3, (err, scale)
    assert float((got - X).abs().max()) > 0.5 * scale
    # deterministic: a second launch on the same input gives the same bits
    again = X.clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused4(again.data_ptr(), ctx_i.data_ptr(), bpr.data_ptr(), 1e-6, Wp.data_ptr(), b2.data_ptr(), M_, D_, F_,
                                              int(fp16), S()))
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    # the MLP half alone (ctx = null) on the projected rows: the same kernel without its projection steps
    mid = xmid.float().contiguous()
    capi.check(lib.dinoseg_op_proj_mlp_fused4(mid.data_ptr(), None, None, 1e-6, Wp.data_ptr(), b2.data_ptr(), M_, D_, F_, int(fp16), S()))
    torch.cuda.synchronize()
    assert float((mid - want).abs().max()) <= 2.0 ** -9 * scale + 1e-3
    if not fp16:
        # the two-waves-per-SIMD kernel it replaces (op_fmt = bf16)
        two = X.clone()
        n = lib.dinoseg_op_proj_pack_elems(D_)
        Wprp = torch.empty((n,), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_pack_proj(Wpr.data_ptr(), D_, Wprp.data_ptr(), S()))
        capi.check(lib.dinoseg_op_proj_mlp_fused(two.data_ptr(), ctx_i.data_ptr(), Wprp.data_ptr(), bpr.data_ptr(), gam.data_ptr(),
                                                 bet.data_ptr(), 1e-6, pack_mlp(W1, W2).data_ptr(), b1.data_ptr(), b2.data_ptr(), M_, D_, F_, S()))
        torch.cuda.synchronize()
        # (the two kernels round different operands -- LayerNorm(x) and W1 there, (x - mean) rstd and W1 diag(gamma) here: each is within the bound above
        #  of ITS operands' fp64 result, their difference within the format's own rounding)
        assert float((got - two).abs().max()) <= 2.0 ** -8 * scale + 1e-3


def _split_planes(x: torch.Tensor, fp16: bool):
    """fp32 -> (int16 planes [2, ...] as the hi + lo kernels read them, the fp32 value the two planes carry)"""
    dt = torch.float16 if fp16 else torch.bfloat16
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt)
    return torch.stack([hi, lo]).contiguous().view(torch.int16), hi.float() + lo.float()


def _mlp3_case(M_, fp16, seed0, tail=False):
    D_, F_ = 384, 1536
    X = seeded((M_, D_), seed0 + 1) * 1.7 + 0.4 + torch.arange(D_, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    ctx = seeded((M_, D_), seed0 + 8) * 0.8
    Wpr = seeded((D_, D_), seed0 + 9) * 0.07 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    bpr = seeded((D_,), seed0 + 10) * 0.3
    gam, bet = 1 + 0.2 * seeded((D_,), seed0 + 2), 0.1 * seeded((D_,), seed0 + 3)
    W1 = seeded((F_, D_), seed0 + 4) * 0.06 + torch.arange(F_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b1 = seeded((F_,), seed0 + 5) * 0.5
    W2 = seeded((D_, F_), seed0 + 6) * 0.04 + torch.arange(D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    b2 = seeded((D_,), seed0 + 7)
    lib = capi.lib()
    Wqkv = seeded((3 * D_, D_), seed0 + 11) * 0.05 + torch.arange(3 * D_, device="cuda", dtype=torch.float32)[:, None] * 1e-5
    bq = seeded((3 * D_,), seed0 + 12) * 0.4
    gam1, bet1 = 1 + 0.2 * seeded((D_,), seed0 + 13), 0.1 * seeded((D_,), seed0 + 14)
    n = lib.dinoseg_op_mlp3_pack_elems(D_, F_)
    assert n == 2 * (D_ * D_ + 2 * D_ * F_ + 3 * D_ * D_) + 2 * (F_ + 3 * D_)      # (the slots, then the folded biases as fp32)
    Wp = torch.zeros((n,), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_pack_mlp3(Wpr.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                        Wqkv.data_ptr() if tail else None, bq.data_ptr() if tail else None, gam1.data_ptr() if tail else None,
                                        bet1.data_ptr() if tail else None, D_, F_, int(fp16), Wp.data_ptr(), S()))
    return dict(X=X, ctx=ctx, Wpr=Wpr, bpr=bpr, gam=gam, bet=bet, W1=W1, b1=b1, W2=W2, b2=b2, Wp=Wp, Wqkv=Wqkv, bq=bq, gam1=gam1, bet1=bet1)


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("proj", [True, False])
@pytest.mark.parametrize("M_", [128, 77, 128 * 5 + 33, 128 * 300 + 19])
def test_proj_mlp_fused_hi_lo_planes(cuda, M_, proj, fp16):
    """The attention output projection + the MLP half of a block in ONE launch on hi + lo operand planes (mlp_fused3.hip; what the
    parity modes fp16x3 / bf16x3 run at large batch):
        x += ctx . Wproj^T + bproj;   x += fc2(gelu(fc1(LayerNorm(x))))      (vision_transformer.py:104-105, :123, :135 -> :59-65)
    against fp64 on the operands the kernel sees (two-plane ctx / weights / LayerNorm and GELU outputs) and against fp64 on the
    UNSPLIT operands (the split must track the fp32 module).  M = 38 419: more items than CUs (the weight ring runs on across the
    items of the persistent walk); 77 / 673: ragged last item (clamped rows)."""
    c = _mlp3_case(M_, fp16, 140)
    lib = capi.lib()
    D_, F_ = 384, 1536
    q2 = lambda t: _split_planes(t, fp16)[1]
    ctx_pl, ctx_q = _split_planes(c["ctx"], fp16)
    got = c["X"].clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused3(got.data_ptr(), ctx_pl.data_ptr() if proj else None, M_ * D_, c["bpr"].data_ptr(), 1e-6,
                                              c["Wp"].data_ptr(), c["b2"].data_ptr(), M_, D_, F_, int(fp16), S()))
    torch.cuda.synchronize()

    def model(quant):
        xmid = c["X"].double()
        if proj:
            xmid = xmid + (quant(c["ctx"]) if quant else c["ctx"]).double() @ (quant(c["Wpr"]) if quant else c["Wpr"]).double().t() + c["bpr"].double()
        ln = _ln_ref(xmid.float(), c["gam"], c["bet"]).cuda() if quant else \
            torch.nn.functional.layer_norm(xmid, (D_,), c["gam"].double(), c["bet"].double(), 1e-6)
        A = quant(ln).double() if quant else ln
        z = A @ (quant(c["W1"]) if quant else c["W1"]).double().t() + c["b1"].double()
        g = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
        Hq = quant(g.float()).double() if quant else g
        delta = Hq @ (quant(c["W2"]) if quant else c["W2"]).double().t() + c["b2"].double()
        return xmid, delta

    xmid, delta = model(q2)
    want = (xmid + delta).float()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    scale = float(delta.abs().max())
    # left over: fp32 summation order, the dropped lo . lo products (2^-16 / 2^-22 of a product), the erf approximation (1.5e-7), and
    # rounding points of the LayerNorm / GELU planes that the kernel's own fp32 arithmetic moves by one ulp of the lo plane
    assert err <= (2.0e-5 if fp16 else 6.0e-5) * scale + 1e-5, (err, scale)
    assert float((got - c["X"]).abs().max()) > 0.5 * scale
    xm0, d0 = model(None)
    err0 = float((got - (xm0 + d0).float()).abs().max())
    assert err0 <= (3.0e-5 if fp16 else 2.0e-4) * scale + 1e-5, (err0, scale)
    print(f"mlp3 M={M_} proj={proj} fp16={fp16}: err {err:.3e} err_true {err0:.3e} scale {scale:.3f}")


@pytest.mark.parametrize("fp16,v_bf16", [(True, 1), (True, 0), (False, 0)])
@pytest.mark.parametrize("B,ntok", [(1, 65), (3, 130), (2, 901), (11, 3601)])
def test_block_tail_fused_hi_lo_planes(cuda, B, ntok, fp16, v_bf16):
    """mlp_fused3.hip with the qkv tail: projection + MLP of block i, then LayerNorm1 + qkv of block i + 1 in the same launch
    (vision_transformer.py:123, :135, then :122 -> :75 / :82).  X must equal the launch without the tail bit for bit; Q / K / V against fp64
    on the operands the kernel sees (two-plane LayerNorm output and weights), in the [B, heads, npad, 64] layout with Q pre-scaled and the
    pad rows untouched; v_bf16: V as bf16 planes next to fp16 Q / K (what the zero-reference hi + lo attention reads).  (11, 3601): 39 611
    rows = more items than CUs, ragged last item."""
    D_, F_, H = 384, 1536, 6
    M_ = B * ntok
    npad = (ntok + 63) // 64 * 64
    c = _mlp3_case(M_, fp16, 170, tail=True)
    lib = capi.lib()
    q2 = lambda t: _split_planes(t, fp16)[1]
    ctx_pl, _ = _split_planes(c["ctx"], fp16)
    ref = c["X"].clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused3(ref.data_ptr(), ctx_pl.data_ptr(), M_ * D_, c["bpr"].data_ptr(), 1e-6, c["Wp"].data_ptr(),
                                              c["b2"].data_ptr(), M_, D_, F_, int(fp16), S()))
    got = c["X"].clone()
    plane = B * H * npad * 64
    q = torch.zeros((2, B, H, npad, 64), dtype=torch.int16, device="cuda")
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    qscale = 0.125 * LOG2E
    capi.check(lib.dinoseg_op_block_tail_fused3(got.data_ptr(), ctx_pl.data_ptr(), M_ * D_, c["bpr"].data_ptr(), 1e-6, c["Wp"].data_ptr(),
                                                c["b2"].data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), plane, B, ntok, npad, H, qscale,
                                                v_bf16, D_, F_, int(fp16), S()))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    A = q2(_ln_ref(got, c["gam1"], c["bet1"]).cuda()).double()
    z = (A @ q2(c["Wqkv"]).double().t() + c["bq"].double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    dt = torch.float16 if fp16 else torch.bfloat16
    un = lambda t, d: t.view(d).to(torch.float32).sum(dim=0)
    gq, gk, gv = un(q, dt), un(k, dt), un(v, torch.bfloat16 if (v_bf16 or not fp16) else torch.float16)
    # (the kernel's own LayerNorm differs from the oracle's by fp32 rounding, which can move a rounding point of the lo plane)
    tol = (2.0 ** -18 if fp16 else 2.0 ** -14) * float(z.abs().max()) + 2e-5
    eq, ek, ev = (float((g[:, :, :ntok] - r).abs().max()) for g, r in ((gq, z[0] * qscale), (gk, z[1]), (gv, z[2])))
    print(f"tail3 B={B} ntok={ntok} fp16={fp16} v_bf16={v_bf16}: dq {eq:.2e} dk {ek:.2e} dv {ev:.2e} tol {tol:.2e}")
    assert eq <= tol and ek <= tol and ev <= (tol if (fp16 and not v_bf16) else 2.0 ** -14 * float(z.abs().max()) + 2e-5)
    assert torch.all(q[:, :, :, ntok:] == 0) and torch.all(k[:, :, :, ntok:] == 0) and torch.all(v[:, :, :, ntok:] == 0)


@pytest.mark.parametrize("B,ntok", [(1, 65), (3, 130), (2, 901), (11, 3601)])
def test_block_tail_fused(cuda, B, ntok):
    """One launch from `x = x + proj(attn)` of block i to `qkv = qkv(norm1(x))` of block i+1 (mlp_fused2.hip, PROJ + QKV):
        x += ctx . Wproj^T + bproj;  x += fc2(gelu(fc1(LN2(x))));  q, k, v = split(LN1'(x) . Wqkv'^T + bqkv')     (vision_transformer.py
        :104-105, :123, :135, then :122 -> :75 of the next block).
    X against the projection + MLP launch (the same arithmetic: bit-identical), Q / K / V against fp64 on the operands the kernel
    sees (bf16 LayerNorm output of ITS x, bf16 weights) and against the LayerNorm-fused qkv GEMM run on that x; pad rows stay zero.
    (11, 3601): 39 611 rows = 310 items, more than the 256 CUs (the qkv tail's tiles, the next item's projection tiles and row
    loads interleave across the item boundary); (1, 65) / (3, 130): ragged single items, frames that straddle 32-row blocks."""
    D_, F_, H = 384, 1536, 6
    M_, npad = B * ntok, (ntok + 63) // 64 * 64
    X = seeded((M_, D_), 61) * 1.7 + 0.4 + torch.arange(D_, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    ctx = quant_like(seeded((M_, D_), 62) * 0.8, 1)
    Wpr, bpr = seeded((D_, D_), 63) * 0.07, seeded((D_,), 64) * 0.3
    gam2, bet2 = 1 + 0.2 * seeded((D_,), 65), 0.1 * seeded((D_,), 66)
    W1, b1 = seeded((F_, D_), 67) * 0.06, seeded((F_,), 68) * 0.5
    W2, b2 = seeded((D_, F_), 69) * 0.04, seeded((D_,), 70)
    gam1, bet1 = 1 + 0.2 * seeded((D_,), 71), 0.1 * seeded((D_,), 72)
    Wqkv, bqkv = seeded((3 * D_, D_), 73) * 0.1, seeded((3 * D_,), 74)
    lib = capi.lib()
    Wp = pack_mlp(W1, W2)
    Wprp = torch.empty((lib.dinoseg_op_proj_pack_elems(D_),), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_pack_proj(Wpr.data_ptr(), D_, Wprp.data_ptr(), S()))
    nq = lib.dinoseg_op_qkv_pack_elems(D_)
    assert nq == 3 * D_ * D_
    Wqp = torch.empty((nq,), dtype=torch.int16, device="cuda")
    capi.check(lib.dinoseg_op_pack_qkv(Wqkv.data_ptr(), D_, Wqp.data_ptr(), S()))
    ctx_b = pack(ctx, 1)
    qscale = 0.125 * LOG2E
    q = torch.zeros((1, B, H, npad, 64), dtype=torch.int16, device="cuda")
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    got = X.clone()
    capi.check(lib.dinoseg_op_block_tail_fused(got.data_ptr(), ctx_b.data_ptr(), Wprp.data_ptr(), bpr.data_ptr(), gam2.data_ptr(),
                                               bet2.data_ptr(), 1e-6, Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(), Wqp.data_ptr(),
                                               bqkv.data_ptr(), gam1.data_ptr(), bet1.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                               B, ntok, npad, H, qscale, D_, F_, S()))
    torch.cuda.synchronize()
    # the block output: same kernel arithmetic as the launch without the tail
    two = X.clone()
    capi.check(lib.dinoseg_op_proj_mlp_fused(two.data_ptr(), ctx_b.data_ptr(), Wprp.data_ptr(), bpr.data_ptr(), gam2.data_ptr(),
                                             bet2.data_ptr(), 1e-6, Wp.data_ptr(), b1.data_ptr(), b2.data_ptr(), M_, D_, F_, S()))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, two)
    # q / k / v from that output: fp64 on the kernel's operands
    A = quant_like(_ln_ref(got, gam1, bet1).cuda(), 1)
    ref = (A.double() @ quant_like(Wqkv, 1).double().t() + bqkv.double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    tol = 2.0 ** -7 * float(ref.abs().max()) + 1e-4
    gq, gk, gv = unpack(q), unpack(k), unpack(v)
    assert float((gq[:, :, :ntok] - ref[0] * qscale).abs().max()) <= tol
    assert float((gk[:, :, :ntok] - ref[1]).abs().max()) <= tol
    assert float((gv[:, :, :ntok] - ref[2]).abs().max()) <= tol
    assert torch.all(gq[:, :, ntok:] == 0) and torch.all(gk[:, :, ntok:] == 0) and torch.all(gv[:, :, ntok:] == 0)
    # ... and the launch it replaces for the next block
    Ws = pack_slabs(Wqkv, 1)
    q2, k2, v2 = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    capi.check(lib.dinoseg_op_ln_gemm(got.data_ptr(), gam1.data_ptr(), bet1.data_ptr(), 1e-6, Ws.data_ptr(), 3 * D_ * D_, bqkv.data_ptr(),
                                      M_, 3 * D_, D_, 1, 4, None, 0, q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), B * H * npad * 64, ntok,
                                      npad, H, qscale, None, None, S()))
    torch.cuda.synchronize()
    for a, b_ in ((gq, unpack(q2)), (gk, unpack(k2)), (gv, unpack(v2))):
        assert float((a - b_).abs().max()) <= tol


def _one_plane(x: torch.Tensor, fp16: bool):
    """fp32 -> (int16 [rows, cols] as the one-plane kernels read it, the fp32 value it carries)"""
    dt = torch.float16 if fp16 else torch.bfloat16
    q = x.to(dt)
    return q.contiguous().view(torch.int16), q.float()


def _pack_rs(W: torch.Tensor, kind: int) -> torch.Tensor:
    N, K = W.shape
    out = torch.empty((N * K,), dtype=torch.int16, device="cuda")
    capi.check(capi.lib().dinoseg_op_pack_rs(W.contiguous().data_ptr(), N, K, kind, out.data_ptr(), S()))
    return out


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("M_,K", [(128, 768), (77, 768), (128 * 5 + 33, 3072), (128 * 300 + 19, 768), (128 * 260 + 1, 3072)])
def test_gemm_rs_residual(cuda, M_, K, fp16):
    """gemm_rs.hip, accumulator-stationary kernel: x += A W^T + bias at N = 768 (ViT-B's attn.proj and mlp.fc2 with the residual add:
    vision_transformer.py:105 + :123, :63 + :135), against fp64 on the one-plane operands.  38 419 / 33 281 rows: more items than CUs (the
    weight ring runs on across the items of the persistent walk), ragged last item (clamped rows)."""
    N = 768
    lib = capi.lib()
    with dino_amd.options(op_fmt=int(fp16)):
        A = seeded((M_, K), 201) + torch.arange(K, device="cuda", dtype=torch.float32)[None, :] * 1e-4
        W = seeded((N, K), 202) * 0.05 + torch.arange(N, device="cuda", dtype=torch.float32)[:, None] * 1e-5
        bias = seeded((N,), 203)
        X = seeded((M_, N), 204) * 2.0
        Ap, Aq = _one_plane(A, fp16)
        Wq = _one_plane(W, fp16)[1]
        got = X.clone()
        Wp = _pack_rs(W, 1)
        capi.check(lib.dinoseg_op_gemm_rs(Ap.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), M_, N, K, capi.EPI_RESID,
                                          got.data_ptr(), None, 0, None, None, None, 0, 0, 0, 0.0, S()))
        torch.cuda.synchronize()
    delta = Aq.double() @ Wq.double().t() + bias.double()
    want = (X.double() + delta).float()
    scale = float(delta.abs().max())
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 2e-6 * scale * math.sqrt(K / 64) + 1e-5
    assert float((got - X).abs().max()) > 0.5 * scale


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("M_", [128, 77, 128 * 5 + 33, 128 * 270 + 19])
def test_gemm_rs_gelu(cuda, M_, fp16):
    """gemm_rs.hip, operand-stationary kernel with the GELU epilogue: H = gelu(A W^T + b), K = 768, N = 3072 (ViT-B's mlp.fc1 + act:
    vision_transformer.py:60-61), one 16-bit plane out, against fp64 + the exact GELU on the one-plane operands (the fitted logistic form
    of the one-plane modes: |error| <= 2.6e-5, below the rounding of the stored activation)."""
    N, K = 3072, 768
    lib = capi.lib()
    with dino_amd.options(op_fmt=int(fp16)):
        A = seeded((M_, K), 211) + torch.arange(K, device="cuda", dtype=torch.float32)[None, :] * 1e-4
        W = seeded((N, K), 212) * 0.04 + torch.arange(N, device="cuda", dtype=torch.float32)[:, None] * 1e-6
        bias = seeded((N,), 213) * 0.5
        Ap, Aq = _one_plane(A, fp16)
        Wq = _one_plane(W, fp16)[1]
        out = torch.zeros((M_, N), dtype=torch.int16, device="cuda")
        Wp = _pack_rs(W, 0)
        capi.check(lib.dinoseg_op_gemm_rs(Ap.data_ptr(), K, Wp.data_ptr(), bias.data_ptr(), M_, N, K, capi.EPI_GELU, None,
                                          out.data_ptr(), N, None, None, None, 0, 0, 0, 0.0, S()))
        torch.cuda.synchronize()
    z = Aq.double() @ Wq.double().t() + bias.double()
    want = (0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))).float()
    got = out.view(torch.float16 if fp16 else torch.bfloat16).float()
    assert torch.isfinite(got).all()
    rel = 2.0 ** -11 if fp16 else 2.0 ** -8
    assert float(((got - want).abs() - rel * want.abs()).max()) <= 1e-4
    assert float(got.abs().max()) > 1.0


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B,ntok", [(1, 65), (3, 130), (10, 3601)])
def test_gemm_rs_qkv_layout(cuda, B, ntok, fp16):
    """gemm_rs.hip, operand-stationary kernel with the Q / K / V scatter at embed_dim 768 (12 heads): the [B, H, npad, 64] layout of
    vision_transformer.py:82, Q pre-scaled, V as bf16 in either format (the one-plane attention's P.V product), pad rows untouched."""
    H, D = 12, 768
    M_, npad = B * ntok, (ntok + 63) // 64 * 64
    lib = capi.lib()
    with dino_amd.options(op_fmt=int(fp16)):
        A, W, bias = seeded((M_, D), 221), seeded((3 * D, D), 222) * 0.05, seeded((3 * D,), 223)
        Ap, Aq = _one_plane(A, fp16)
        Wq = _one_plane(W, fp16)[1]
        q = torch.zeros((B, H, npad, 64), dtype=torch.int16, device="cuda")
        k, v = torch.zeros_like(q), torch.zeros_like(q)
        qscale = 0.125 * LOG2E
        Wp = _pack_rs(W, 0)
        capi.check(lib.dinoseg_op_gemm_rs(Ap.data_ptr(), D, Wp.data_ptr(), bias.data_ptr(), M_, 3 * D, D, 4, None, None,
                                          0, q.data_ptr(), k.data_ptr(), v.data_ptr(), ntok, npad, H, qscale, S()))
        torch.cuda.synchronize()
    ref = (Aq.double() @ Wq.double().t() + bias.double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    dt = torch.float16 if fp16 else torch.bfloat16
    gq, gk, gv = q.view(dt).float(), k.view(dt).float(), v.view(torch.bfloat16).float()
    tol = lambda r, d: (2.0 ** -11 if d == torch.float16 else 2.0 ** -8) * float(r.abs().max()) + 1e-4
    assert float((gq[:, :, :ntok] - ref[0] * qscale).abs().max()) <= tol(ref[0] * qscale, dt)
    assert float((gk[:, :, :ntok] - ref[1]).abs().max()) <= tol(ref[1], dt)
    assert float((gv[:, :, :ntok] - ref[2]).abs().max()) <= tol(ref[2], torch.bfloat16)
    assert torch.all(q[:, :, ntok:] == 0) and torch.all(k[:, :, ntok:] == 0) and torch.all(v[:, :, ntok:] == 0)


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B,ntok", [(1, 65), (3, 130), (10, 3601)])
def test_ln_gemm_rs(cuda, B, ntok, fp16):
    """gemm_rs.hip with the LayerNorm inside the launch (`self.qkv(self.norm1(x))` / `self.fc1(self.norm2(x))`, vision_transformer.py:122 -> :75,
    :134 -> :60-61, embed_dim 768): the prologue computes (x - mean) rstd, the LayerNorm's weight and bias ride in the packed copy
    (W diag(gamma), b + W beta: dinoseg_op_pack_rs_ln).  Against fp64 on the operands the kernel sees (the normalised rows and the scaled weight
    rounded to the operand format), against the fp64 module on unrounded operands within the format's error, and against the two launches it
    replaces; Q / K / V layout and pad rows as without the LayerNorm.  (10, 3601): 36 010 rows = more items than CUs, ragged last item."""
    H, D, F_ = 12, 768, 3072
    M_, npad = B * ntok, (ntok + 63) // 64 * 64
    lib = capi.lib()
    X = seeded((M_, D), 231) * 1.6 + 0.3 + torch.arange(D, device="cuda", dtype=torch.float32)[None, :] * 1e-3
    X[:, 7] += 25.0          # (an outlier channel, as the residual stream has them: the statistics are two-pass)
    gam, bet = 1 + 0.2 * seeded((D,), 232), 0.1 * seeded((D,), 233)
    Wq_, bq = seeded((3 * D, D), 234) * 0.05, seeded((3 * D,), 235)
    W1, b1 = seeded((F_, D), 236) * 0.04, seeded((F_,), 237) * 0.5
    qscale = 0.125 * LOG2E
    dt = torch.float16 if fp16 else torch.bfloat16
    with dino_amd.options(op_fmt=int(fp16)):
        A16 = torch.zeros((1, M_, D), dtype=torch.int16, device="cuda")
        capi.check(lib.dinoseg_op_layernorm(X.data_ptr(), gam.data_ptr(), bet.data_ptr(), 1e-6, M_, D, A16.data_ptr(), M_ * D, 1, None, 0, ntok, S()))
        Wpq, Wp1 = _pack_rs(Wq_, 0), _pack_rs(W1, 0)
        fold = {}
        for name, W_, b_ in (("q", Wq_, bq), ("1", W1, b1)):
            wf = torch.empty((W_.numel(),), dtype=torch.int16, device="cuda")
            bf = torch.empty((W_.shape[0],), device="cuda")
            capi.check(lib.dinoseg_op_pack_rs_ln(W_.data_ptr(), gam.data_ptr(), bet.data_ptr(), b_.data_ptr(), W_.shape[0], D, wf.data_ptr(),
                                                 bf.data_ptr(), S()))
            fold[name] = (wf, bf)
        outs = {}
        for ln in (False, True):
            q = torch.zeros((B, H, npad, 64), dtype=torch.int16, device="cuda")
            k, v = torch.zeros_like(q), torch.zeros_like(q)
            hb = torch.zeros((M_, F_), dtype=torch.int16, device="cuda")
            if ln:
                capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 1e-6, fold["q"][0].data_ptr(), fold["q"][1].data_ptr(), M_, 3 * D, D, 4, None, 0,
                                                     q.data_ptr(), k.data_ptr(), v.data_ptr(), ntok, npad, H, qscale, S()))
                capi.check(lib.dinoseg_op_ln_gemm_rs(X.data_ptr(), 1e-6, fold["1"][0].data_ptr(), fold["1"][1].data_ptr(), M_, F_, D, capi.EPI_GELU,
                                                     hb.data_ptr(), F_, None, None, None, 0, 0, 0, 0.0, S()))
            else:
                capi.check(lib.dinoseg_op_gemm_rs(A16.data_ptr(), D, Wpq.data_ptr(), bq.data_ptr(), M_, 3 * D, D, 4, None, None, 0, q.data_ptr(),
                                                  k.data_ptr(), v.data_ptr(), ntok, npad, H, qscale, S()))
                capi.check(lib.dinoseg_op_gemm_rs(A16.data_ptr(), D, Wp1.data_ptr(), b1.data_ptr(), M_, F_, D, capi.EPI_GELU, None, hb.data_ptr(), F_,
                                                  None, None, None, 0, 0, 0, 0.0, S()))
            torch.cuda.synchronize()
            outs[ln] = (q.view(dt).float(), k.view(dt).float(), v.view(torch.bfloat16).float(), hb.view(dt).float(), q, k, v)
    ulp = 2.0 ** -10 if fp16 else 2.0 ** -7
    for t in outs[True][:4]:
        assert torch.isfinite(t).all()
    # the folded bias: b + W beta
    assert float((fold["q"][1].double() - (bq.double() + Wq_.double() @ bet.double())).abs().max()) <= 1e-5
    # fp64 on the operands the kernel sees: xhat = (x - mean) rstd rounded to the format, W diag(gamma) rounded to the format, the folded bias
    mu = X.double().mean(dim=1, keepdim=True)
    xhat = (X.double() - mu) / torch.sqrt(((X.double() - mu) ** 2).mean(dim=1, keepdim=True) + 1e-6)
    Aq = _q1(xhat.float(), fp16).double()
    refq = (Aq @ _q1(Wq_ * gam[None, :], fp16).double().t() + fold["q"][1].double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    tol = lambda r, e: 3 * e * float(r.abs().max()) + 1e-4
    assert float((outs[True][0][:, :, :ntok] - refq[0] * qscale).abs().max()) <= tol(refq[0] * qscale, ulp)
    assert float((outs[True][1][:, :, :ntok] - refq[1]).abs().max()) <= tol(refq[1], ulp)
    assert float((outs[True][2][:, :, :ntok] - refq[2]).abs().max()) <= tol(refq[2], 2.0 ** -7)
    z1 = Aq @ _q1(W1 * gam[None, :], fp16).double().t() + fold["1"][1].double()
    want1 = (0.5 * z1 * (1.0 + torch.erf(z1 / math.sqrt(2.0)))).float()
    # (the kernel's fp32 statistics can round an operand the other way than the fp64 ones: with the outlier channel one such flip moves an output by
    #  ~ |w| ulp(15): the worst element gets the bound of the qkv checks, the mean stays at the format's rounding)
    d1 = (outs[True][3] - want1).abs()
    assert float(d1.max()) <= tol(want1, ulp)
    assert float(d1.mean()) <= 0.25 * ulp * float(want1.abs().mean()) + 1e-5
    # the module itself in fp64 (nothing rounded), and the two launches this one replaces: operand rounding only
    ln64 = xhat * gam.double() + bet.double()
    true_q = (ln64 @ Wq_.double().t() + bq.double()).float().reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)
    e_new = float((outs[True][1][:, :, :ntok] - true_q[1]).abs().max())
    e_old = float((outs[False][1][:, :, :ntok] - true_q[1]).abs().max())
    print(f"ln_gemm_rs B={B} ntok={ntok} fp16={fp16}: |K - fp64 module| {e_new:.3e} with the LayerNorm inside, {e_old:.3e} as two launches")
    assert e_new <= 2.0 * e_old + 1e-3
    for t in outs[True][4:]:
        assert torch.all(t[:, :, ntok:] == 0)
