"""What the probes of tests/test_gemm_probes_gpu.py claim about themselves, checked without a GPU: the operands and partial sums are exact where
the probes say so, every `2 bound <= min |W|` condition holds for every parametrised case (K = 768 included), an fp32 numpy emulation of a
correct GEMM -- k-steps in a seeded order, the sums inside a step in the order numpy's matrix product takes -- passes every check of
tests/probe_util.py that the GPU file runs, and each of nine mutants of that emulation fails at least one of them.

What a probe cannot see, so that nobody reads more into it: a truncating 16-bit store is caught by the Q check of G3 (z qscale lies off the
format's grid) and not by G2 or the K / V checks on one plane, where every z is a multiple of 0.25 that the format holds or an exact tie whose
two neighbours are both half an ulp away, and not on fp16 hi + lo planes, whose 22 bits lose less than the fp32 accumulation may (the store-rounding
probe of tests/test_forward_probes_gpu.py holds these epilogues bit for bit on ties, plane by plane).  Q scaled
after the rounding differs from Q scaled before it only where fmt(z) != z: on one bf16 plane (z in [64, 120] off the 0.5 grid)."""
import numpy as np
import pytest
import torch

from tests import probe_util as P

KS = 64                     # the k-step of the emulated kernel (gemm.hip's)
TM = 64                     # ... and its row tile: M = 77 leaves a ragged last tile of 13 rows
M, N, K = 77, 128, 192
FORMATS = [(1, False), (1, True), (2, False), (2, True)]
FORMAT_IDS = [f"{P.FMT_IDS[f]}-{p}" for p, f in FORMATS]


# ------------------------------------------------------------------------------------------------ the emulation
def emu_product(Ap, Wp, ks=KS, seed=0, drop=None, dup=None):
    """fp32 accumulation of A W^T from operand planes (lists of fp32 [M, K] / [N, K]: hi, or hi and lo): the k-steps in a seeded order, per step
    lo x hi, hi x lo, hi x hi as the two-plane kernels do.  drop = (step, rows, cols): that step's products are lost in that tile;
    dup = (m, n, k): that product is added twice."""
    acc = np.zeros((Ap[0].shape[0], Wp[0].shape[0]), dtype=np.float32)
    for j in np.random.default_rng(seed).permutation(Ap[0].shape[1] // ks):
        sl = slice(j * ks, (j + 1) * ks)
        part = np.zeros_like(acc)
        if len(Ap) == 2:
            part += Ap[1][:, sl] @ Wp[0][:, sl].T
            part += Ap[0][:, sl] @ Wp[1][:, sl].T
        part += Ap[0][:, sl] @ Wp[0][:, sl].T
        if drop is not None and drop[0] == j:
            part[drop[1], drop[2]] = 0.0
        acc += part
    if dup is not None:
        m, n, k = dup
        acc[m, n] += Ap[0][m, k] * Wp[0][n, k]
    return acc


def planes32(v, v_lo):
    """value and lo part (fp64) -> the fp32 operand planes"""
    hi = (v - v_lo).astype(np.float32)
    return [hi] if not v_lo.any() else [hi, v_lo.astype(np.float32)]


def trunc16(v32, fp16):
    """fp32 -> the 16-bit format, rounded toward zero (the mutant's store), as fp32"""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    if not fp16:
        return (v32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = v32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v32)
    return np.where(over, np.nextafter(h, np.float16(0.0)), h).astype(np.float32)


def store(v32, fp16, planes, trunc=False):
    """fp32 values -> int16 planes [planes, ...] (torch, host) as the epilogues write them: RNE(v), and RNE(v - hi) on two planes"""
    dt = P.tdtype(fp16)
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    cvt = (lambda x: trunc16(x, fp16)) if trunc else (lambda x: P.rne(x, fp16).astype(np.float32))
    hi = cvt(v32)
    ps = [hi] if planes == 1 else [hi, cvt(v32 - hi)]
    return torch.stack([torch.from_numpy(p).to(dt) for p in ps]).contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ G1
_g1 = {}


def g1_case(planes, fp16):
    if (planes, fp16) not in _g1:
        A, A_lo = P.exact_operand((M, K), 1101, fp16, planes, 0.25, 2.0)
        W, W_lo = P.exact_operand((N, K), 1102, fp16, planes, 2.0 ** -5, 2.0 ** -3)
        g = np.random.default_rng(1103)
        _g1[(planes, fp16)] = A, A_lo, W, W_lo, g.standard_normal(N).astype(np.float32), g.standard_normal((M, N)).astype(np.float32)
    return _g1[(planes, fp16)]


def g1_check(name, planes, fp16, mask, mutant=None):
    """the EPI_RESID check of tests/test_gemm_probes_gpu.py::g1_run on the emulation; mutant: drop / dup / swap / no_resid"""
    A, A_lo, W, W_lo, bias, X = g1_case(planes, fp16)
    W, W_lo = W * mask, W_lo * mask
    band_cols = np.flatnonzero(np.arange(N) % (K // KS) == 1)          # the columns that multiply k-step 1 only, when banded
    acc = emu_product(planes32(A, A_lo), planes32(W, W_lo), seed=5,
                      drop=(1, slice(TM, M), band_cols[:8]) if mutant == "drop" else None,
                      dup=(3, 5, 134) if mutant == "dup" else None)
    out = acc + bias[None, :] if mutant == "no_resid" else (acc + bias[None, :]) + X
    if mutant == "swap":
        out[[M - 2, M - 1]] = out[[M - 1, M - 2]]
    s, sb = P.accum_reference(A, A_lo, W, W_lo, K)
    ref = X.astype(np.float64) + s + bias.astype(np.float64)
    return P.within(name, np.abs(out.astype(np.float64) - ref), sb + P.add_bound(X.astype(np.float64), bias.astype(np.float64)))


@pytest.mark.parametrize("planes,fp16", FORMATS, ids=FORMAT_IDS)
def test_accumulation_probe(planes, fp16):
    """Operands exact in the format with exact products; the emulation passes dense and banded; the banded mask gives every k-step columns of its
    own; the four accumulation mutants fail."""
    A, A_lo, W, W_lo, _, _ = g1_case(planes, fp16)
    for v, v_lo in ((A, A_lo), (W, W_lo)):
        hi, lo = P.split(v.astype(np.float32), fp16)
        assert (v.astype(np.float32).astype(np.float64) == v).all() and (hi + lo == v).all() and (lo == v_lo).all()
        assert (planes == 2) == bool(v_lo.any())
    prod = (A - A_lo)[:, None, :8] * (W - W_lo)[None, :, :8]
    assert (prod.astype(np.float32).astype(np.float64) == prod).all(), "hi x hi products are not exact in fp32"
    dense, band = np.ones((N, K), dtype=bool), P.banded((N, K), tile=KS, ntiles=K // KS)
    assert (band.reshape(N, K // KS, KS).all(axis=2).sum(axis=1) == 1).all() and (band.sum(axis=1) == KS).all()      # one whole k-step per column
    assert (band.reshape(N, K // KS, KS)[:, :, 0].sum(axis=0) >= N // (K // KS)).all()                                # every step has columns
    for nm, mask in (("dense", dense), ("banded", band)):
        assert g1_check(f"emulation {nm}", planes, fp16, mask) <= 1.0
    for mutant, mask in (("drop", band), ("dup", dense), ("dup", band), ("swap", dense), ("no_resid", dense)):
        with pytest.raises(AssertionError):
            g1_check(f"mutant {mutant}", planes, fp16, mask, mutant=mutant)


@pytest.mark.parametrize("planes,fp16", FORMATS, ids=FORMAT_IDS)
def test_patch_probe(planes, fp16):
    """EPI_PATCH: the emulation with the row remap b (n + 1) + 1 + p passes check_patch; a CLS row overwritten and a position row off by one fail."""
    B, n = 2, 35                                                      # 70 rows: frame 1 straddles the 64-row tile
    A, A_lo, W, W_lo, bias, _ = g1_case(planes, fp16)
    A, A_lo = A[:B * n], A_lo[:B * n]
    pos = np.random.default_rng(1105).standard_normal((n + 1, N)).astype(np.float32)
    acc = emu_product(planes32(A, A_lo), planes32(W, W_lo), seed=6)
    s, sb = P.accum_reference(A, A_lo, W, W_lo, K)
    ref = s.reshape(B, n, N) + bias.astype(np.float64) + pos[1:].astype(np.float64)[None]
    bound = sb.reshape(B, n, N) + P.add_bound(bias.astype(np.float64), pos[1:].astype(np.float64))[None]

    def run(mutant=None):
        out = np.full((B, n + 1, N), np.nan)
        rows = pos[:-1] if mutant == "pos" else pos[1:]
        out[:, 1:] = ((acc + bias[None, :]).reshape(B, n, N) + rows[None]).astype(np.float64)
        if mutant == "cls":
            out[1, 0] = out[0, n]                                     # frame 0's last patch row lands one row late
        return P.check_patch(f"patch {mutant}", out, ref, bound)

    assert run() <= 1.0
    for mutant in ("cls", "pos"):
        with pytest.raises(AssertionError):
            run(mutant)


# ------------------------------------------------------------------------------------------------ G2
_z = {}


def z_case(Mr, eps, fp16, planes, rows, width, seed):
    key = (Mr, eps, fp16, planes, rows, width, seed)
    if key not in _z:
        _z[key] = P.ln_fc1_case(Mr, eps, fp16, planes, rows=rows, seed=seed, width=width)
    return _z[key]


def emu_z(X, W, b, eps, fp16, planes, ln, drop=None, dup=None):
    """fp32 pre-activation of the emulated launch: rows = X, or LayerNorm(X) = X rstd rounded to the operand planes (ln)"""
    rows = [X.astype(np.float32)]
    if ln:
        xn = X.astype(np.float32) * np.float32(1.0 / np.sqrt(np.float32(1.0) + np.float32(eps)))
        hi, lo = P.split(xn, fp16)
        rows = [hi.astype(np.float32)] if planes == 1 else [hi.astype(np.float32), lo.astype(np.float32)]
    Wp = [W] if len(rows) == 1 else [W, np.zeros_like(W)]
    return emu_product(rows, Wp, ks=P.KSL, seed=7, drop=drop, dup=dup) + b[None, :]


def test_every_bound_condition_and_the_emulation():
    """Every G2 and G3 case of the GPU file: z in [8, 120], every partial sum exact (multiples of 0.25 below 2^7), 2 bound <= min |W| (inside
    check_stored / check_qkv), and the emulation's stored planes pass."""
    seen = set()
    for kind, fp16, epi in P.G2_CASES:
        route, planes = kind.split("-")[0], P.planes_of(kind)
        for Nw in P.g2_widths(kind):
            for eps in P.g2_eps(kind):
                key = (route in P.LN_ROUTES, planes, fp16, Nw, P.WIDTH[route], eps)
                if key in seen:
                    continue
                seen.add(key)
                for Mr in P.G2_MS:
                    X, W, b, z, zerr = z_case(Mr, eps, fp16, planes, Nw, P.WIDTH[route], 1201)
                    assert z.min() >= 8.0 and z.max() <= 120.0
                    csum = np.abs(W).reshape(Nw, -1, P.KSL).sum(axis=2)
                    assert ((csum != 0).sum(axis=1) == 1).all() and csum.max() <= 56.0 and (W * 4 == np.round(W * 4)).all()
                    z32 = emu_z(X, W, b, eps, fp16, planes, route in P.LN_ROUTES)
                    if eps == 0.0:
                        assert (z32.astype(np.float64) == z).all(), "z is not exact"
                    o = P.unplane(store(z32, fp16, planes), fp16)
                    assert P.check_stored(f"emulation {kind} {P.FMT_IDS[fp16]} N={Nw} M={Mr} eps={eps}", o, z, zerr, W, fp16, planes) <= 1.0
    for kind, H, fp16, v_bf16 in P.G3_CASES:
        planes, dm = P.planes_of(kind), 64 * H
        vf = P.v_is_fp16(fp16, planes, v_bf16)
        for B, ntok in P.G3_SHAPES:
            q, k, v, z, zerr = qkv_emulation(B, ntok, H, fp16, planes, vf)
            assert P.check_qkv(f"emulation {kind} H={H}", q, k, v, z, zerr, fp16, planes, vf, B, ntok, H) <= 1.0


@pytest.mark.parametrize("planes,fp16", FORMATS, ids=FORMAT_IDS)
def test_epilogue_mutants(planes, fp16):
    """G2: one k-slice dropped in the ragged last tile and one duplicated product move z by at least min |W| = 1: they fail."""
    X, W, b, z, zerr = z_case(77, 0.0, fp16, planes, 128, 384, 1201)
    j = int(np.flatnonzero(W[5])[0]) // P.KSL
    for kw in ({"drop": (j, slice(TM, 77), slice(0, 128))}, {"dup": (70, 5, int(np.flatnonzero(W[5])[3]))}):
        o = P.unplane(store(emu_z(X, W, b, 0.0, fp16, planes, False, **kw), fp16, planes), fp16)
        with pytest.raises(AssertionError):
            P.check_stored(f"mutant {list(kw)[0]}", o, z, zerr, W, fp16, planes)


# ------------------------------------------------------------------------------------------------ G3
def scatter(t, B, ntok, npad, H):
    """int16 planes [planes, M, dm] -> [planes, B, H, npad, 64], NAN16 in the pad rows"""
    planes = t.shape[0]
    out = torch.full((planes, B, H, npad, 64), P.NAN16, dtype=torch.int16)
    out[:, :, :, :ntok] = t.reshape(planes, B, ntok, H, 64).permute(0, 1, 3, 2, 4)
    return out


def qkv_emulation(B, ntok, H, fp16, planes, v_fp16, mutant=None):
    dm, Mr, npad = 64 * H, B * ntok, (ntok + 63) // 64 * 64
    X, W, bq, z, zerr = z_case(Mr, 0.0, fp16, planes, 3 * dm, dm, 1301)
    z32 = emu_z(X, W, bq, 0.0, fp16, planes, False)
    zq, zk, zv = z32[:, :dm], z32[:, dm:2 * dm], z32[:, 2 * dm:]
    trunc = mutant == "trunc"
    if mutant == "q_after":                      # round, then scale, then the 16-bit store of the product
        q32 = P.stored(zq, fp16, planes, sat=False).astype(np.float32) * np.float32(P.QS)
    else:
        q32 = zq * np.float32(P.QS)
    q, k = store(q32, fp16, planes, trunc), store(zk, fp16, planes, trunc)
    v = store(zv, v_fp16 != (mutant == "v_fmt"), planes, trunc)
    return tuple(scatter(t, B, ntok, npad, H) for t in (q, k, v)) + (z, zerr)


G3_MUTANTS = [(1, False, False), (1, True, False), (2, False, False), (2, True, False), (2, True, True)]      # (planes, fp16, V is fp16)


@pytest.mark.parametrize("planes,fp16,v_fp16", G3_MUTANTS, ids=[f"{P.FMT_IDS[f]}-{p}{'-vfp16' if vf else ''}" for p, f, vf in G3_MUTANTS])
def test_qkv_mutants(planes, fp16, v_fp16):
    """G3: V in the other format fails in every format, a truncating store in every format but fp16 hi + lo; Q scaled after the rounding fails where fmt(z) != z (one bf16 plane:
    module docstring) and is the same numbers elsewhere."""
    B, ntok, H = 3, 130, 6
    run = lambda m: P.check_qkv(f"mutant {m}", *qkv_emulation(B, ntok, H, fp16, planes, v_fp16, mutant=m), fp16, planes, v_fp16, B, ntok, H)
    assert run(None) <= 1.0
    with pytest.raises(AssertionError):
        run("v_fmt")
    if planes == 2 and fp16:
        assert run("trunc") <= 1.0              # (22 bits of 24: what a truncated lo plane loses lies below the accumulation's own bound)
    else:
        with pytest.raises(AssertionError):
            run("trunc")
    if planes == 1 and not fp16:
        with pytest.raises(AssertionError):
            run("q_after")
    else:
        got, want = qkv_emulation(B, ntok, H, fp16, planes, v_fp16, mutant="q_after")[0], qkv_emulation(B, ntok, H, fp16, planes, v_fp16)[0]
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ the test entries
def test_gemm_test_entries_refuse_on_the_host():
    """dinoseg_op_patch_gemm and dinoseg_op_gemm_train refuse what the 128 x 128 kernel's launcher refuses before any launch, each with a message
    that starts with its own name."""
    from dino_amd import capi, options
    lib = capi.lib()
    fake = 256      # never dereferenced: every call below is refused on the host

    def refused(rc, text):
        assert rc == -1 and capi.last_error().startswith(text), capi.last_error()

    patch = lambda A=fake, pos=fake, B=2, n=35, N=384, K=192, planes=1: lib.dinoseg_op_patch_gemm(A, fake, fake, pos, B, n, N, K, planes, fake, None)
    refused(patch(A=None), "dinoseg_op_patch_gemm: null pointer")
    refused(patch(pos=None), "dinoseg_op_patch_gemm: null pointer")
    for kw in ({"B": 0}, {"n": 0}, {"N": 192}, {"K": 96}, {"planes": 3}, {"B": 70000, "n": 70000}):
        refused(patch(**kw), "dinoseg_op_patch_gemm: unsupported shape")

    def train(epi=1, resid=fake, out=512, out16=None, aux=None, M=77, N=384, K=192, lda=192, ldo=0, planes=1):
        return lib.dinoseg_op_gemm_train(fake, M * lda, lda, fake, N * K, M, N, K, planes, epi, fake, resid, out, out16, M * N, ldo, aux, M * N, None)
    for epi in (0, 3, 4, 5):
        refused(train(epi=epi), "dinoseg_op_gemm_train: epi must be 1 (residual) or 2 (GELU)")
    refused(train(resid=None), "dinoseg_op_gemm_train: epi 1 needs resid and out_f32")
    refused(train(resid=512), "dinoseg_op_gemm_train: epi 1 needs resid and out_f32")        # in place: that is dinoseg_op_gemm
    refused(train(epi=2, out16=fake), "dinoseg_op_gemm_train: epi 1 needs resid and out_f32 (two buffers), epi 2 needs out_bf16 and aux_out")
    for kw in ({"N": 192}, {"K": 96}, {"lda": 100}, {"planes": 0}, {"M": 0}):
        refused(train(**kw), "dinoseg_op_gemm_train: unsupported shape")
    refused(train(epi=2, out16=fake, aux=fake, ldo=380), "dinoseg_op_gemm_train: unsupported shape")
    with options(op_fmt=1):
        refused(train(epi=2, out16=fake, aux=fake, ldo=384), "dinoseg_op_gemm_train: the pre-activation planes (aux_out) are bf16 only")
