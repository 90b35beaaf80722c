"""Per-kernel parity tests of the fine-tune step's backward (-m gpu): every kernel the step runs, called alone through its
stand-alone C-ABI entry with the launcher and arguments the step uses, against an fp64 restatement on the very values the
kernel read.  Bounds are per element and scale with that element's own magnitude (the fp64 sum of the absolute terms), never
with the tensor's max or norm: one wrong ragged tile, border tap or tail row fails the test however small its share of the norm.

Notation: U = 2^-24 (fp32 unit roundoff).  A sum of n products accumulated in fp32 (MFMA chains, split-K slices, atomics) is
held to c * U * sum|terms| with c = 4 sqrt(n) + (a few per reduction stage).  On two planes the GEMMs multiply hi*hi + hi*lo +
lo*hi by design; the dropped lo*lo products are added to the bound exactly (|lo|^T |lo|).  bf16 outputs add their own rounding:
bf16 keeps 8 significant bits, so round-to-nearest is 2^-8 relative for one plane and 2^-16 for hi + lo (lo = bf16(x - hi))."""
import math

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import capi
from tests.gpu_util import pack, seeded, unpack

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
U = 2.0 ** -24
LOG2E = 1.4426950408889634
SENT = 12345.0                      # fp32 sentinel of outputs a kernel must not touch
SENT16 = 0x7F7F                     # bf16 sentinel (a large finite value)
EPI_PLAIN, EPI_BF16, EPI_DGELU, EPI_DRELU = 0, 6, 8, 9


def planes64(p: torch.Tensor) -> torch.Tensor:
    """int16 bf16 planes [planes, ...] -> fp64 [planes, ...] (each plane on its own)."""
    return p.view(torch.bfloat16).double()


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).view(torch.int16)


def check(got, ref, bound, what):
    """Every element within its bound; a NaN or inf anywhere in `got` fails (err <= bound is False for NaN)."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} element(s) out of bound; first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])}, ref {float(ref.reshape(-1)[i])}, bound {float(bound.reshape(-1)[i])}")
    return float((err / bound.clamp_min(1e-300)).max())


def products_bound(Aq, Bq, c, Alo=None, Blo=None):
    """c * U * |A| |B| (+ |A_lo| |B_lo|, the products the two-plane kernels leave out)."""
    b = c * U * (Aq.abs() @ Bq.abs())
    if Alo is not None:
        b = b + Alo.abs() @ Blo.abs()
    return b


# --------------------------------------------------------------------------------------------------- gemm_tn + split-K reduce
# (N, Kc, ldy, k_cols, M, planes, ksplit, ldw - k_cols): the classifier's 64-wide d logits (C = 7), an N that is not a multiple of
# 128 (150 classes), the MLP head's k_pad route (100 of 128 columns), fc2 / fc1 / qkv of the blocks; ragged last 32-row chunks
# (1, 31, 33, 3601, 28 808), the 2-D grid (ksplit 1, 3), the XCD-aware 1-D grid (8, 16, 40), slices that own no rows (33 rows =
# 2 chunks over 8 slices; 3601 rows = 113 chunks over 40 slices: 38 used), the scalar reduce (ldw not a multiple of 4).
# Keep the small-M cases: at M = 28 808 the bound 4 sqrt(M) U sum|y x| is about one row's product per element, so the deep cases
# cannot see a single wrong, dropped or duplicated batch row (the ragged-chunk zeroing); M = 1, 31, 33 and 3601 can.
TN_CASES = [
    (7, 384, 64, 384, 28800, 2, 8, 4),
    (7, 384, 64, 384, 1, 1, 1, 4),
    (150, 384, 192, 384, 3601, 2, 3, 1),
    (150, 384, 192, 384, 33, 1, 1, 4),
    (256, 384, 256, 384, 31, 1, 1, 4),
    (256, 384, 256, 384, 3600, 2, 16, 4),
    (100, 128, 128, 100, 28800, 2, 40, 4),
    (100, 128, 128, 100, 33, 1, 3, 1),
    (384, 1536, 384, 1536, 28808, 1, 8, 4),
    (384, 1536, 384, 1536, 3601, 2, 40, 4),
    (384, 1536, 384, 1536, 33, 1, 8, 4),
    (1536, 384, 1536, 384, 28808, 2, 16, 4),
    (1536, 384, 1536, 384, 33, 2, 3, 4),
    (1152, 384, 1152, 384, 28808, 1, 3, 4),
    (1152, 384, 1152, 384, 3601, 1, 16, 4),
]


@pytest.mark.parametrize("N,Kc,ldy,k_cols,M,planes,ksplit,extra", TN_CASES)
def test_gemm_tn_weight_gradient(cuda, N, Kc, ldy, k_cols, M, planes, ksplit, extra):
    yp = pack(seeded((M, ldy), 11 + M + N), planes)        # (columns >= N of dY are live data: they must not leak into dW)
    xp = pack(seeded((M, Kc), 12 + M + Kc), planes)
    row_tiles = (N + 127) // 128
    part = torch.full((ksplit * row_tiles * 128 * Kc,), math.nan, device="cuda")     # (a slice the reduce sums but nobody wrote: NaN)
    ldw = k_cols + extra
    dW = torch.full((N + 2, ldw), SENT, device="cuda")
    dW[:N, :k_cols] = 0
    colsum = torch.full((N + 1,), SENT, device="cuda")
    colsum[:N] = 0
    capi.check(capi.lib().dinoseg_op_gemm_tn(yp.data_ptr(), M * ldy, ldy, xp.data_ptr(), M * Kc, Kc, M, N, Kc, planes, ksplit,
                                             part.data_ptr(), dW.data_ptr(), ldw, k_cols, colsum.data_ptr(), S()))
    torch.cuda.synchronize()
    Y, X = planes64(yp)[:, :, :N], planes64(xp)[:, :, :k_cols]
    Yq, Xq = Y.sum(0), X.sum(0)
    ref = Yq.T @ Xq
    c = 4 * math.sqrt(M) + 2 * ksplit + 4
    lo = (Y[1].T, X[1]) if planes == 2 else (None, None)
    q = check(dW[:N, :k_cols], ref, products_bound(Yq.T, Xq, c, *lo), "dW")
    qc = check(colsum[:N], Yq.sum(0), c * U * Yq.abs().sum(0), "colsum")
    assert bool((dW[N:] == SENT).all()), "dW rows >= N written"
    assert bool((dW[:, k_cols:] == SENT).all()), "dW columns >= k_cols written"
    assert float(colsum[N]) == SENT, "colsum beyond N written"
    print(f"gemm_tn N={N} Kc={Kc} M={M} planes={planes} ksplit={ksplit}: worst |err|/bound dW {q:.3g} colsum {qc:.3g}")


# --------------------------------------------------------------------------------------------------- dgrad: backward epilogues
def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


GELU_SPECIAL = torch.tensor([0.0, 1e-3, -1e-3, 3.0, -3.0, 10.0, -10.0])


@pytest.mark.parametrize("epi,M,N,K,planes", [
    (EPI_DGELU, 33, 1536, 384, 1), (EPI_DGELU, 33, 1536, 384, 2), (EPI_DGELU, 3601, 1536, 384, 2),
    (EPI_DRELU, 33, 128, 64, 2), (EPI_DRELU, 3601, 256, 128, 1), (EPI_DRELU, 3601, 128, 64, 2),
    (EPI_BF16, 3601, 384, 384, 1), (EPI_BF16, 33, 384, 384, 2),
    (EPI_PLAIN, 33, 384, 1152, 2), (EPI_PLAIN, 3601, 384, 256, 1),
])
def test_gemm_backward_epilogues(cuda, epi, M, N, K, planes):
    ap = pack(seeded((M, K), 21 + M + K), planes)
    wp = pack(seeded((N, K), 22 + N, scale=0.05), planes)
    aux = None
    if epi == EPI_DGELU:        # saved fc1 pre-activations, with 0, +-1e-3, +-3, +-10 sprinkled in
        a = seeded((M, N), 23, scale=2.0)
        flat = a.view(-1)
        sel = flat[::5]
        flat[::5] = GELU_SPECIAL.to("cuda").repeat(sel.numel() // 7 + 1)[: sel.numel()]
        aux = pack(a, planes)
    elif epi == EPI_DRELU:      # saved post-ReLU activations: exact zeros on about half the entries
        aux = pack(torch.relu(seeded((M, N), 24)), planes)
    lib = capi.lib()
    out16 = torch.full((2, M + 1, N), SENT16, dtype=torch.int16, device="cuda")
    out32 = torch.full((M + 1, N), SENT, device="cuda")
    bf16_out = epi != EPI_PLAIN
    capi.check(lib.dinoseg_op_gemm_bwd(ap.data_ptr(), M * K, K, wp.data_ptr(), N * K, M, N, K, planes, epi,
                                       None if bf16_out else out32.data_ptr(), N, out16.data_ptr() if bf16_out else None,
                                       (M + 1) * N, N, aux.data_ptr() if aux is not None else None, M * N, S()))
    torch.cuda.synchronize()
    A, W = planes64(ap), planes64(wp)
    Aq, Wq = A.sum(0), W.sum(0)
    acc = Aq @ Wq.T
    lo = (A[1], W[1].T) if planes == 2 else (None, None)
    err = products_bound(Aq, Wq.T, 4 * math.sqrt(K) + 8, *lo)
    if epi == EPI_DGELU:
        d = gelu_grad64(planes64(aux).sum(0))
        val = acc * d
        err = err * d.abs() + acc.abs() * 2.0 ** -19      # gelu' in fp32: A&S 7.1.26 erf (|error| <= 1.5e-7) + exp2 / rcp
    elif epi == EPI_DRELU:
        d = (planes64(aux)[0] > 0).double()                 # (the kernel tests the hi plane: > 0 exactly when the value is)
        val = acc * d
        err = err * d
    else:
        val = acc
    if not bf16_out:
        q = check(out32[:M], val, err + U * val.abs(), "dX fp32")
        assert bool((out32[M] == SENT).all()), "row M written"
    else:
        o = planes64(out16)
        hi = o[0, :M]
        q = check(hi, val, err + 2.0 ** -8 * (val.abs() + err) + 1e-300, "hi plane")
        if planes == 2:
            q = max(q, check(o[0, :M] + o[1, :M], val, err * (1 + 2.0 ** -7) + 2.0 ** -16 * val.abs() + 1e-300, "hi + lo planes"))
            assert bool((o[1, :M].abs() <= 2.0 ** -8 * o[0, :M].abs()).all()), "hi plane is not the nearest bf16 of hi + lo"
        else:
            assert bool((out16[1] == SENT16).all()), "one-plane output wrote a second plane"
        assert bool((out16[:, M] == SENT16).all()), "row M written"
    print(f"gemm_bwd epi={epi} M={M} N={N} K={K} planes={planes}: worst |err|/bound {q:.3g}")


# --------------------------------------------------------------------------------------------------- narrow-layer weight gradient
@pytest.mark.parametrize("kind,planes,ksplit,drop_cls", [
    ("patch", 1, 85, 1), ("patch", 2, 85, 1), ("patch", 2, 1, 1), ("patch", 1, 7, 0),
    ("head", 2, 1, 0), ("head", 1, 5, 0), ("head", 2, 56, 0),
])
def test_wgrad_narrow_layer(cuda, kind, planes, ksplit, drop_cls):
    """The transposed-operand route: dY (+ bias column sums, drop_cls) and X transposed, the NT kernel over the batch rows,
    fp32 atomics (ksplit 1) or split-K partial tiles + the reduce.  patch: the patch embedding at 8 frames @480 (dY = the fp32
    residual-stream gradient with its CLS rows, X = the 192-wide patch planes); head: a 7-class linear head on 384 features."""
    lib = capi.lib()
    if kind == "patch":
        B, ntok, N, K = 8, 3601, 384, 192
        M = B * (ntok - 1) if drop_cls else B * ntok - 5
        dy32 = seeded((B * ntok, N), 31, scale=0.01)
        ldy = N
    else:
        ntok, N, K, M = 0, 7, 384, 3600
        ldy = 64
        dyp = pack(seeded((M, ldy), 32), planes)
    xp = pack(seeded((M, K), 33), planes)
    m_pad = (M + 63) // 64 * 64
    n_pad, k_pad = (N + 127) // 128 * 128, (K + 127) // 128 * 128
    t_plane = max(n_pad, k_pad) * m_pad
    T1 = torch.zeros(planes * t_plane, dtype=torch.int16, device="cuda")
    T2 = torch.zeros(planes * t_plane, dtype=torch.int16, device="cuda")
    part = torch.full((max(ksplit, 1) * n_pad * k_pad,), math.nan, device="cuda")
    dW = torch.full((N + 1, K), SENT, device="cuda")
    dW[:N] = 0
    colsum = torch.full((N + 1,), SENT, device="cuda")
    colsum[:N] = 0
    if kind == "patch":
        args = (dy32.data_ptr(), None, 0, ldy)
    else:
        args = (None, dyp.data_ptr(), M * ldy, ldy)
    capi.check(lib.dinoseg_op_wgrad_nt(*args, xp.data_ptr(), M * K, K, M, N, K, planes, drop_cls, ntok, ksplit, T1.data_ptr(),
                                       T2.data_ptr(), t_plane, m_pad, part.data_ptr(), dW.data_ptr(), colsum.data_ptr(), S()))
    torch.cuda.synchronize()
    if kind == "patch":
        rows = dy32.double()
        if drop_cls:
            rows = rows.reshape(B, ntok, N)[:, 1:].reshape(-1, N)
        rows = rows[:M]
        hi = rows.float().to(torch.bfloat16).double()
        Y = torch.stack([hi, (rows.float() - hi.float()).to(torch.bfloat16).double()])[:planes]
        cs_src = rows                                      # (the transpose kernel sums the fp32 values themselves)
    else:
        Y = planes64(dyp)[:, :, :N]
        cs_src = Y.sum(0)
    X = planes64(xp)
    Yq, Xq = Y.sum(0), X.sum(0)
    c = 4 * math.sqrt(m_pad) + 2 * ksplit + 4
    lo = (Y[1].T, X[1]) if planes == 2 else (None, None)
    q = check(dW[:N], Yq.T @ Xq, products_bound(Yq.T, Xq, c, *lo), "dW")
    qc = check(colsum[:N], cs_src.sum(0), c * U * cs_src.abs().sum(0), "colsum")
    assert bool((dW[N] == SENT).all()) and float(colsum[N]) == SENT, "written beyond N rows"
    print(f"wgrad_nt {kind} planes={planes} ksplit={ksplit} drop_cls={drop_cls}: worst |err|/bound dW {q:.3g} colsum {qc:.3g}")


# --------------------------------------------------------------------------------------------------- nll_loss + log-softmax backward
def _nll_inputs(M, C, seed, mode):
    g = np.random.default_rng(seed)
    logits = torch.from_numpy(g.standard_normal((M, C)).astype(np.float32) * 3)
    logp = torch.log_softmax(logits.double(), dim=1).float()
    if mode == "ignored":
        labels = np.full(M, -100, dtype=np.int64)
    else:           # valid, ignored (-100) and out-of-range (C, -1, 10**6) labels
        labels = g.integers(0, C, size=M).astype(np.int64)
        r = g.random(M)
        labels[r < 0.15] = -100
        if mode == "bad":
            labels[(r >= 0.15) & (r < 0.2)] = C
            labels[(r >= 0.2) & (r < 0.22)] = -1
            labels[0] = 10 ** 6
    return logp.cuda(), torch.from_numpy(labels).cuda()


def _run_nll(logp, labels, dlogp, M, C):
    ldz = (C + 63) // 64 * 64
    dz = torch.full((2, M, ldz), SENT16, dtype=torch.int16, device="cuda")
    acc = torch.zeros(2, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    loss = torch.full((1,), SENT, device="cuda")
    capi.check(capi.lib().dinoseg_op_nll_loss_grad(logp.data_ptr(), labels.data_ptr() if labels is not None else None,
                                                   dlogp.data_ptr() if dlogp is not None else None, M, C, acc.data_ptr(),
                                                   flags.data_ptr(), loss.data_ptr(), dz.data_ptr(), M * ldz, ldz, S()))
    torch.cuda.synchronize()
    return dz, float(loss), int(flags[0])


@pytest.mark.parametrize("C", [1, 7, 32, 33, 150, 256])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 28800])
def test_nll_loss_grad(cuda, C, M):
    mode = "bad" if M % 2 == 1 else "mixed"
    logp, labels = _nll_inputs(M, C, 100 * C + M, mode)
    dz, loss, flag = _run_nll(logp, labels, None, M, C)
    lp, lab = logp.double(), labels
    valid = (lab >= 0) & (lab < C)
    n = int(valid.sum())
    assert flag == int(bool(((lab != -100) & ~valid).any())), "bad-label flag"
    onehot = torch.zeros_like(lp)
    onehot[valid.nonzero()[:, 0], lab[valid]] = 1.0
    if n == 0:
        assert math.isnan(loss), "mean over zero rows must be nan (torch)"
        ref = torch.zeros_like(lp)
        bound = torch.full_like(lp, 1e-300)
    else:
        ref_loss = float(-(lp * onehot).sum() / n)
        assert abs(loss - ref_loss) <= (4 * math.sqrt(M) + 4) * U * abs(ref_loss), (loss, ref_loss)
        dl = -onehot / n
        rowsum = dl.sum(1, keepdim=True)
        e = lp.exp()
        ref = dl - e * rowsum
        # -1/n, expf, the product and the difference: a few roundings of each term
        bound = 8 * U * (dl.abs() + e * rowsum.abs()) + 1e-300
    D = planes64(dz)
    q = check(D[0, :, :C] + D[1, :, :C], ref, bound * (1 + 2.0 ** -7) + 2.0 ** -16 * ref.abs(), "dz hi + lo")
    assert bool((D[1, :, :C].abs() <= 2.0 ** -8 * D[0, :, :C].abs()).all()), "hi plane is not the nearest bf16 of hi + lo"
    assert bool((dz[:, :, C:] == 0).all()), "padding columns of the d logits must be zero in both planes"
    # the autograd path: d loss / d logp = nll_loss's own gradient gives the same planes bit for bit (torch's nll_loss backward:
    # +0 everywhere but -1/n at the label; a -0 would turn the ignored rows' +0 into -0)
    if n > 0:
        dlogp = torch.zeros((M, C), device="cuda")
        dlogp[valid.nonzero()[:, 0], lab[valid]] = -float(np.float32(1.0) / np.float32(n))
        dz2, _, _ = _run_nll(logp, None, dlogp, M, C)
        assert torch.equal(dz2, dz), "dlogp path differs from the labels path"
    print(f"nll_loss_grad C={C} M={M}: worst |err|/bound {q:.3g}")


def test_nll_loss_grad_all_rows_ignored(cuda):
    for C in (7, 150):
        logp, labels = _nll_inputs(300, C, 7, "ignored")
        dz, loss, flag = _run_nll(logp, labels, None, 300, C)
        assert math.isnan(loss) and flag == 0
        assert bool((dz == 0).all()), C


@pytest.mark.parametrize("C,M", [(7, 257), (150, 28800), (256, 255)])
def test_log_softmax_backward_of_a_dense_dlogp(cuda, C, M):
    """The autograd path with an arbitrary upstream gradient: dz = dl - exp(logp) * sum_c dl."""
    logp, _ = _nll_inputs(M, C, 5 + C, "mixed")
    dlogp = seeded((M, C), 9 + C)
    dz, _, _ = _run_nll(logp, None, dlogp, M, C)
    lp, dl = logp.double(), dlogp.double()
    e = lp.exp()
    rowsum = dl.sum(1, keepdim=True)
    ref = dl - e * rowsum
    bound = (C + 8) * U * (dl.abs() + e * dl.abs().sum(1, keepdim=True))
    D = planes64(dz)
    q = check(D[0, :, :C] + D[1, :, :C], ref, bound * (1 + 2.0 ** -7) + 2.0 ** -16 * ref.abs() + 1e-300, "dz hi + lo")
    assert bool((dz[:, :, C:] == 0).all())
    print(f"log_softmax_bwd dense C={C} M={M}: worst |err|/bound {q:.3g}")


# --------------------------------------------------------------------------------------------------- pos-embed resample backward
@pytest.mark.parametrize("oh,ow", [(28, 28), (8, 8), (1, 60), (60, 1), (16, 49), (28, 29), (60, 80), (120, 120)])
def test_pos_resample_backward(cuda, oh, ow):
    from tests.test_rect_cpu import resample_pos_embed_hw
    g, D = 28, 384
    dpos = seeded((oh * ow + 1, D), 41 + oh * 1000 + ow)
    dpe0 = seeded((g * g + 1, D), 42)
    scratch = torch.full((g * max(ow, g) * D,), math.nan, device="cuda")
    out = []
    for start in (torch.zeros_like(dpe0), dpe0.clone()):
        capi.check(capi.lib().dinoseg_op_pos_resample_bwd_hw(dpos.data_ptr(), g, D, oh, ow, start.data_ptr(), scratch.data_ptr(), S()))
        out.append(start)
    torch.cuda.synchronize()
    grad, acc = out
    # dpe is accumulated: the same gradient added to what was there, one fp32 add per element
    assert torch.equal(acc, dpe0 + grad), "dpe is not dpe + the gradient"
    pe = torch.zeros((1, g * g + 1, D), dtype=torch.float64, requires_grad=True)
    resample_pos_embed_hw(pe, oh, ow).backward(dpos.double().cpu()[None])
    ref = pe.grad[0]
    # The bound, term by term (the identity grid copies dpos exactly):
    # - the kernel's two fma chains (n_y outputs per stored row, then n_x per stored column) and the add into dpe:
    #   (n_y + n_x + 1) U sum |w_y w_x d|;
    # - the weights: the kernel and the reference both evaluate them in fp32, each within e of the exact Keys weight:
    #   e = (1.35 * 3 (g + 1) + 74) U = |K'| <= 1.35 on [0, 2] times the source coordinate (y + 0.5) * scale - 0.5 after three fp32
    #   roundings of values below g + 1, plus the nested cubic (at most 6 roundings of intermediates below 12: 72 U; 2 U for
    #   x = t + 1 / 2 - t).  A stored index collects every tap that clamps onto it, so with C = the count of such taps the
    #   difference E = 2 e enters as sum (|W_y| + E C_y)(|W_x| + E C_x)|d| - sum |W_y||W_x||d|.  C counts the taps floor - 2 ..
    #   floor + 3 of each output: one beyond the four on each side, since the two fp32 coordinates may floor differently.
    d = dpos.double().cpu()
    bound = torch.full_like(ref, 1e-300)
    if not (oh == g and ow == g):
        def axis_weights(o, along_y):       # [o, g]: the reference's own weights (one-hot channels; the other axis sums to 1)
            onehot = torch.zeros((1, g * g + 1, g), dtype=torch.float64)
            yy, xx = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
            idx = (yy if along_y else xx).reshape(-1)
            onehot[0, 1 + torch.arange(g * g), idx] = 1.0
            r = resample_pos_embed_hw(onehot, oh, ow)[0, 1:].reshape(oh, ow, g)
            return (r[:, 0, :] if along_y else r[0, :, :]).abs()

        def tap_counts(o):                  # [o, g]
            sy = (torch.arange(o, dtype=torch.float64) + 0.5) * (g / (o + 0.1)) - 0.5
            f = torch.floor(sy).long()
            cnt = torch.zeros((o, g), dtype=torch.float64)
            for a in range(-2, 4):
                cnt[torch.arange(o), (f + a).clamp(0, g - 1)] += 1
            return cnt

        Wy, Wx = axis_weights(oh, True), axis_weights(ow, False)
        Cy, Cx = tap_counts(oh), tap_counts(ow)
        E = 2 * (1.35 * 3 * (g + 1) + 74) * U
        n_y, n_x = int((Cy > 0).sum(0).max()), int((Cx > 0).sum(0).max())
        dg = d[1:].reshape(oh, ow, D).abs()
        s11 = torch.einsum("yi,yxd,xj->ijd", Wy, dg, Wx).reshape(g * g, D)
        full = torch.einsum("yi,yxd,xj->ijd", Wy + E * Cy, dg, Wx + E * Cx).reshape(g * g, D)
        bound[1:] += (n_y + n_x + 1) * U * s11 + (full - s11)
    got = grad.double().cpu()
    q = check(got, ref, bound, "dpe")
    print(f"pos_resample_bwd {oh}x{ow}: worst |err|/bound {q:.3g}")


# --------------------------------------------------------------------------------------------------- LayerNorm backward
LN_CASES = [    # (D, M, ntok, drop_cls, accumulate, planes, route_ab)
    (384, 28808, 3601, 1, 0, 2, 0),         # the final norm of the fine-tune step (8 frames @480)
    (384, 28808, 3601, 0, 1, 2, 0),         # norm1 / norm2 of a block
    (384, 16385, 3601, 0, 1, 1, 0),         # one row past the sixteen-lane kernel's 1024 x 16-row grid
    (128, 16385, 3601, 0, 0, 1, 0),
    (128, 87, 29, 1, 1, 2, 0),
    (768, 28808, 3601, 1, 1, 2, 0),         # one wave per row
    (768, 87, 29, 0, 0, 1, 0),
    (384, 87, 29, 1, 0, 1, 0),
    (384, 28808, 3601, 1, 1, 2, 2),         # route_ab bit 1: the one-wave-per-row kernel at D = 384
    (384, 16385, 3601, 0, 0, 1, 2),
]


@pytest.mark.parametrize("D,M,ntok,drop_cls,accumulate,planes,route", LN_CASES)
def test_layernorm_backward(cuda, D, M, ntok, drop_cls, accumulate, planes, route):
    lib = capi.lib()
    eps = 1e-6
    x = seeded((M, D), 51 + D) * 2 + 0.3
    gamma = 1 + 0.2 * seeded((D,), 52)
    nrows_dy = M - M // ntok if drop_cls else M
    dy = seeded((nrows_dy, D), 53 + M)
    dx0 = seeded((M, D), 54)
    dx = dx0.clone()
    dg = torch.zeros(D + 1, device="cuda")
    db = torch.zeros(D + 1, device="cuda")
    cs = torch.zeros(D + 1, device="cuda")
    dg[D] = db[D] = cs[D] = SENT
    dxp = torch.full((2, M, D), SENT16, dtype=torch.int16, device="cuda")
    with dino_amd.options(**({"route_ab": route} if route else {})):
        capi.check(lib.dinoseg_op_layernorm_bwd2(dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), eps, M, D, dx.data_ptr(), accumulate,
                                                 dg.data_ptr(), db.data_ptr(), drop_cls, ntok, dxp.data_ptr(), M * D, planes,
                                                 cs.data_ptr(), S()))
        torch.cuda.synchronize()
    # fp64 restatement (native_layer_norm_backward)
    xd, gd = x.double(), gamma.double()
    dyd = torch.zeros((M, D), dtype=torch.float64, device="cuda")
    if drop_cls:
        keep = (torch.arange(M, device="cuda") % ntok) != 0
        dyd[keep] = dy.double()
    else:
        dyd = dy.double()
    mu = xd.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (xd - mu) * rstd
    gg = dyd * gd
    sg, sgx = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    ref_dx = rstd * (gg - sg - xh * sgx) + (dx0.double() if accumulate else 0)
    # per-element magnitude of dx's terms; xhat carries the error of the mean, which scales with mean|x|, not with |x - mean|
    cD = 4 * math.sqrt(D) + 16
    xh_mag = xh.abs() + rstd * xd.abs().mean(1, keepdim=True)
    mag = rstd * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh_mag * (gg * xh).abs().mean(1, keepdim=True))
    b_dx = cD * U * mag + U * ref_dx.abs() + 1e-300
    q = {"dx": check(dx, ref_dx, b_dx, "dx")}
    cM = 4 * math.sqrt(M) + 16
    q["dgamma"] = check(dg[:D], (dyd * xh).sum(0), cM * U * (dyd.abs() * xh_mag).sum(0) + cD * U * (dyd.abs() * xh_mag).sum(0), "dgamma")
    q["dbeta"] = check(db[:D], dyd.sum(0), cM * U * dyd.abs().sum(0) + 1e-300, "dbeta")
    q["colsum"] = check(cs[:D], ref_dx.sum(0), cM * U * ref_dx.abs().sum(0) + b_dx.sum(0), "colsum")
    assert float(dg[D]) == SENT and float(db[D]) == SENT and float(cs[D]) == SENT
    # dxp: exactly the split of the kernel's own fp32 dx rows
    hi = bf16_bits(dx)
    assert torch.equal(dxp[0], hi), "dxp hi plane is not bf16(dx)"
    if planes == 2:
        lo = bf16_bits(dx - hi.view(torch.bfloat16).float())
        assert torch.equal(dxp[1], lo), "dxp lo plane is not bf16(dx - hi)"
    else:
        assert bool((dxp[1] == SENT16).all()), "one-plane dxp wrote a second plane"
    print(f"layernorm_bwd D={D} M={M} drop_cls={drop_cls} acc={accumulate} planes={planes} route={route}: worst |err|/bound "
          + ", ".join(f"{k} {v:.3g}" for k, v in q.items()))


# --------------------------------------------------------------------------------------------------- attention backward
def _attn_bwd_run(B, H, ntok, planes, seed, variant=None):
    """Forward (for O and the LSE) and backward on seeded operands; returns the planes and the backward's dqkv planes."""
    npad = (ntok + 63) // 64 * 64
    lib = capi.lib()

    def padded(shape_seed, scale=1.0):
        full = torch.zeros((B, H, npad, 64), device="cuda")
        full[:, :, :ntok] = seeded((B, H, ntok, 64), shape_seed) * scale
        return pack(full.reshape(-1, 64), planes)

    qp = padded(seed, 0.125 * LOG2E)
    kp, vp = padded(seed + 1), padded(seed + 2)
    dop = pack(seeded((B * ntok, H * 64), seed + 3, scale=0.1), planes)
    plane = B * H * npad * 64
    ctx = torch.zeros((planes, B * ntok, H * 64), dtype=torch.int16, device="cuda")
    lse = torch.zeros((B, H, ntok), device="cuda")
    capi.check(lib.dinoseg_op_attention(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), plane, ctx.data_ptr(), B * ntok * H * 64,
                                        lse.data_ptr(), B, H, ntok, npad, planes, S()))
    scratch = torch.zeros(2 * B * H * npad, device="cuda")
    dqkv = torch.full((planes, B * ntok, 3 * H * 64), SENT16, dtype=torch.int16, device="cuda")
    with dino_amd.options(**({} if variant is None else {"attn_variant": variant})):
        capi.check(lib.dinoseg_op_attention_bwd(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), plane, dop.data_ptr(), ctx.data_ptr(),
                                                B * ntok * H * 64, lse.data_ptr(), scratch.data_ptr(), dqkv.data_ptr(),
                                                B * ntok * 3 * H * 64, B, H, ntok, npad, planes, S()))
        torch.cuda.synchronize()
    return qp, kp, vp, dop, dqkv, npad


def _attn_pair_ref(qp, kp, vp, dop, B, H, ntok, npad, b, h):
    """fp64 gradients of softmax(q k^T / 8) v for one (frame, head) pair, on the operands the kernels read."""
    def rows(p):
        return unpack(p).reshape(B, H, npad, 64)[b, h, :ntok].double()
    q = rows(qp) / (0.125 * LOG2E)
    k, v = rows(kp), rows(vp)
    dO = unpack(dop).reshape(B, ntok, H, 64)[b, :, h].double()
    P = torch.softmax((q @ k.T) * 0.125, dim=-1)
    dV = P.T @ dO
    dP = dO @ v.T
    dS = P * (dP - (dP * P).sum(1, keepdim=True))
    return dS @ k * 0.125, dS.T @ q * 0.125, dV


def _pair_grads(dqkv, B, H, ntok, b, h):
    g = unpack(dqkv).reshape(B, ntok, 3, H, 64)[b, :, :, h].double()
    return g[:, 0], g[:, 1], g[:, 2]


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("B,H,ntok", [(1, 6, 61), (8, 6, 3601), (2, 6, 4801)])
def test_attention_backward_per_block(cuda, planes, B, H, ntok):
    """Relative Frobenius error of dQ, dK, dV per 64-token block of the first, a middle and the last (frame, head) pair: a wrong
    or zeroed tail block cannot hide behind the rest.  Bounds as test_train_gpu.test_attention_bwd (P and dS are rounded to the
    operand planes inside the kernels)."""
    tol = 2e-2 if planes == 1 else 2e-4
    qp, kp, vp, dop, dqkv, npad = _attn_bwd_run(B, H, ntok, planes, seed=ntok + planes)
    # every (plane, token row, q / k / v, head) slice of 64 was written, in the pairs the fp64 check below does not sample too
    written = (dqkv.reshape(planes, B * ntok, 3 * H, 64) != SENT16).any(dim=-1)
    if not bool(written.all()):
        pl, row, j = (int(v) for v in (~written).nonzero()[0])
        raise AssertionError(f"dqkv slice not written: plane {pl}, token row {row}, {'qkv'[j // H]} of head {j % H}")
    worst = 0.0
    npairs = B * H
    for pair in sorted({0, npairs // 2, npairs - 1}):
        b, h = divmod(pair, H)
        ref = _attn_pair_ref(qp, kp, vp, dop, B, H, ntok, npad, b, h)
        got = _pair_grads(dqkv, B, H, ntok, b, h)
        for name, r, g in zip("qkv", ref, got):
            for t0 in range(0, ntok, 64):
                rb, gb = r[t0:t0 + 64], g[t0:t0 + 64]
                e = float((gb - rb).norm() / rb.norm())
                worst = max(worst, e / tol)
                assert e <= tol, (name, b, h, t0, e)
    print(f"attention_bwd B={B} H={H} ntok={ntok} planes={planes}: worst block error / bound {worst:.3g}")


def test_attention_backward_dq_8_wave_route_is_bit_identical_to_4_wave(cuda):
    """8 frames @480 (48 pairs x 3601 tokens) selects the 256-query dQ workgroups; attn_variant bit 64 forces the 128-query ones.
    Same arithmetic per row (launch_attention_bwd): the planes must agree bit for bit."""
    B, H, ntok = 8, 6, 3601
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ((B * H + 7) // 8 * 8) * ((ntok + 127) // 128) >= 2 * ncu, "shape no longer selects the 8-wave dQ kernel"
    *_, d8, _ = _attn_bwd_run(B, H, ntok, 1, seed=77)
    *_, d4, _ = _attn_bwd_run(B, H, ntok, 1, seed=77, variant=dino_amd.get_option("attn_variant") | 64)
    assert torch.equal(d8, d4), f"{int((d8 != d4).sum())} elements differ between the 8-wave and the 4-wave dQ route"
