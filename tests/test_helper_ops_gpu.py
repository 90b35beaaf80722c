"""The helper kernels of elementwise.hip and the optimiser / refresh tail of train.hip, each called alone through its
dinoseg_op_* entry and compared with an fp64 restatement of the reference's operation at ragged and production shapes (-m gpu).

Bars.  No bar here is copied from another test or tuned to the kernel.  For every comparison that is not exact the test evaluates,
on the same inputs, the same formula in plain float32 on the CPU: its distance from the fp64 result is what fp32 arithmetic alone
costs.  The kernel may be 4 x that (another summation order, fused multiply-adds, the 1-ulp hardware exp2) plus one ulp of the
output format at the output's scale: 2^-23 for fp32, 2^-8 / 2^-15 for one / two bf16 planes, 2^-11 / 2^-22 for fp16 planes.
Errors are max |err| / max |ref| (Adam: relative to the summed magnitudes of each expression's terms).  Every case prints one
`helper_ops` line: the kernel's error, the restatement's, their ratio and the bar (profiles/helper_ops_parity_lines.txt holds a run).
For 16-bit outputs the kernel's error contains the rounding of the output format, so the ratio can pass 4 there while the bar holds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames
from oracle import dinoseg_oracle as O
from tests.gpu_util import NAN16, nan16, pack, untouched

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
LOG2E = 1.4426950408889634
TOL = 1e-3                              # the parity modes' bar on an embedding (tests/test_model_gpu.py)
ULP32 = 2.0 ** -23
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
FMT = {"bf16": 0, "fp16": 1}
ULP16 = {("bf16", 1): 2.0 ** -8, ("bf16", 2): 2.0 ** -15, ("fp16", 1): 2.0 ** -11, ("fp16", 2): 2.0 ** -22}


def op_fmt(fmt):
    return dino_amd.options(op_fmt=FMT[fmt])


def unpack64(p, fmt):
    """int16 planes [planes, ...] -> fp64 sum of the planes"""
    return p.view(DT[fmt]).double().sum(dim=0)


def rng_normal(g, shape, scale=1.0):
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32)) * scale


def ramp(n, step):
    return torch.arange(n, dtype=torch.float32) * step


def relerr(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def report(kernel, case, what, err, e32, ulp):
    bar = 4.0 * e32 + ulp
    ratio = err / e32 if e32 > 0 else float("nan")
    print(f"helper_ops {kernel} [{case}] {what}: kernel {err:.3e} fp32 {e32:.3e} ratio {ratio:.2f} bar {bar:.3e}")
    return bar


# ------------------------------------------------------------------------------------------------ layernorm
def _ln(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(dim=-1, keepdim=True)
    return xc * torch.rsqrt(var + eps) * g + b


# (D, M, ntok, planes, fmt, drop_cls, family, outputs): every D / 128, the row counts around the 4-rows-per-block and the 4096-block
# grid cap (16 384 rows) and the headline's 115 232, both plane counts and formats, drop_cls with either output
LN_CASES = [
    (128, 1, 1, 1, "bf16", 0, "plain", "both"),
    (256, 3, 3, 2, "bf16", 0, "offset", "f32"),
    (384, 4, 2, 1, "fp16", 1, "plain", "p16"),
    (512, 5, 5, 2, "fp16", 0, "plain", "both"),
    (640, 16384, 64, 1, "bf16", 1, "offset", "f32"),
    (768, 16385, 3277, 2, "fp16", 1, "plain", "p16"),
    (896, 5, 5, 1, "fp16", 0, "offset", "both"),
    (1024, 16385, 3277, 2, "bf16", 0, "plain", "both"),
    (384, 115232, 3601, 1, "fp16", 1, "plain", "p16"),
    (384, 115232, 3601, 2, "fp16", 1, "offset", "both"),
    (768, 16384, 64, 2, "fp16", 0, "offset", "both"),
    (128, 16385, 3277, 1, "bf16", 1, "plain", "both"),
    (1024, 4, 4, 1, "bf16", 0, "offset", "p16"),
    (256, 16384, 64, 2, "bf16", 1, "plain", "p16"),
    (640, 3, 3, 1, "fp16", 0, "plain", "f32"),
    (896, 16385, 3277, 1, "bf16", 0, "offset", "both"),
    (512, 4, 2, 2, "bf16", 1, "offset", "f32"),
    (768, 1, 1, 2, "fp16", 0, "plain", "both"),
]


@pytest.mark.parametrize("D,M,ntok,planes,fmt,drop_cls,family,outs", LN_CASES)
def test_layernorm_shapes_formats_and_drop_cls(cuda, D, M, ntok, planes, fmt, drop_cls, family, outs):
    g_ = np.random.default_rng(1000 + D + M + planes)
    mean, std = (0.7, 3.0) if family == "plain" else (10.0, 0.1)
    x = rng_normal(g_, (M, D), std) + mean + std * 0.05 * (ramp(D, 1.0 / D)[None, :] + ramp(M, 1.0)[:, None] % 7 / 7)
    zero_row = M - 1 if M >= 3 else None          # an all-zero row: mean 0, variance 0, the result is beta exactly
    if zero_row is not None:
        x[zero_row] = 0.0
    gam = 1 + 0.2 * rng_normal(g_, (D,)) + ramp(D, 0.5 / D)
    bet = 0.1 * rng_normal(g_, (D,)) - ramp(D, 0.2 / D)
    eps = float(np.float32(1e-6))
    B = M // ntok
    assert B * ntok == M
    rows_out = B * (ntok - 1) if drop_cls else M
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    of = torch.full((rows_out + 4, D), float("nan"), device="cuda") if outs != "p16" else None
    op = nan16((planes, rows_out + 4, D)) if outs != "f32" else None
    with op_fmt(fmt):
        capi.check(capi.lib().dinoseg_op_layernorm(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), eps, M, D, capi.ptr(op), (rows_out + 4) * D,
                                                   planes, capi.ptr(of), drop_cls, ntok, S()))
        torch.cuda.synchronize()
    # fp64 on the device (all rows), the float32 restatement on the CPU
    keep = (torch.arange(M) % ntok != 0) if drop_cls else torch.ones(M, dtype=torch.bool)
    ref = _ln(xd.double(), gd.double(), bd.double(), eps)[keep.cuda()]
    r32 = _ln(x, gam, bet, torch.tensor(eps, dtype=torch.float32))[keep]
    assert r32.dtype == torch.float32 and tuple(ref.shape) == (rows_out, D)
    e32 = relerr(r32.cuda(), ref)
    case = f"D={D} M={M} planes={planes} {fmt} drop_cls={drop_cls} {family} {outs}"
    zr = None if zero_row is None else int(keep[:zero_row].sum())      # its output row
    if of is not None:
        assert torch.isfinite(of[:rows_out]).all() and untouched(of[rows_out:]), "exactly the B x (ntok - 1) / M rows are written"
        err = relerr(of[:rows_out], ref)
        assert err <= report("layernorm", case, "fp32 rows", err, e32, ULP32)
        if zr is not None:
            assert torch.equal(of[zr], bd)
    if op is not None:
        assert untouched(op[:, rows_out:]) and not bool(torch.isnan(op[:, :rows_out].view(DT[fmt]).float()).any())
        err = relerr(unpack64(op[:, :rows_out], fmt), ref)
        assert err <= report("layernorm", case, "16-bit planes", err, e32, ULP16[fmt, planes])
        if zr is not None:
            hi = bd.to(DT[fmt])
            assert torch.equal(op[0, zr].view(DT[fmt]), hi)
            if planes == 2:
                assert torch.equal(op[1, zr].view(DT[fmt]), (bd - hi.float()).to(DT[fmt]))


# ------------------------------------------------------------------------------------------------ head_final
# (C, K, ld, M, fmt, tie): C around the CMAX = 8 template switch and the second store slot (16 / 17), C * ld = 16384 = the LDS limit,
# M around the 16 rows of a workgroup and 115 200 (the grid-stride loop), ties between two identical classifier rows
HEAD_CASES = [
    (1, 100, 128, 1, "bf16", None),
    (7, 384, 384, 15, "fp16", None),
    (8, 500, 512, 16, "bf16", None),
    (9, 600, 640, 17, "fp16", None),
    (16, 100, 128, 333, "bf16", None),
    (17, 384, 384, 333, "fp16", None),
    (21, 600, 640, 333, "bf16", None),
    (32, 500, 512, 333, "fp16", None),
    (32, 384, 384, 115200, "fp16", None),
    (7, 100, 128, 115200, "bf16", None),
    (21, 500, 512, 17, "bf16", None),
    (9, 384, 384, 333, "bf16", (2, 5)),
    (32, 384, 384, 333, "fp16", (3, 20)),
    (8, 100, 128, 16, "fp16", (0, 7)),
]


@pytest.mark.parametrize("C_,K,ld,M,fmt,tie", HEAD_CASES)
def test_head_final_classes_rows_and_ties(cuda, C_, K, ld, M, fmt, tie):
    g_ = np.random.default_rng(2000 + C_ + K + M)
    x = torch.ones((M, ld))                                     # columns K .. ld are finite junk: the kernel's staged W is zero there
    x[:, :K] = torch.relu(rng_normal(g_, (M, K)) + ramp(K, 0.3 / K)[None, :])
    Wc = 0.3 * rng_normal(g_, (C_, K)) + ramp(C_, 0.02 / C_)[:, None]
    b = rng_normal(g_, (C_,))
    if tie:
        Wc[tie[1]] = Wc[tie[0]]
        z0 = x[:, :K] @ Wc.t() + b                              # (from the inputs alone) the bias that lets the pair win on the median row
        rest = z0.clone()
        rest[:, list(tie)] = -float("inf")
        b[tie[0]] = b[tie[1]] = b[tie[0]] + float((rest.max(dim=1).values - z0[:, tie[0]]).median())
    lib = capi.lib()
    logp = torch.full((M + 16, C_), float("nan"), device="cuda")
    am = torch.full((M + 16,), -7, dtype=torch.int32, device="cuda")
    Wd, bd = Wc.cuda(), b.cuda()
    with op_fmt(fmt):
        xp = pack(x.cuda(), 2)
        capi.check(lib.dinoseg_op_head_final(xp.data_ptr(), M * ld, ld, M, K, Wd.data_ptr(), bd.data_ptr(), C_, logp.data_ptr(), am.data_ptr(),
                                             S()))
        torch.cuda.synchronize()
    xs = unpack64(xp, fmt)[:, :K]                               # the operands the kernel saw, fp64 on the device
    z = xs @ Wd.double().t() + bd.double()
    ref = torch.log_softmax(z, dim=1)
    xs32 = xs.float().cpu()
    assert torch.equal(xs32.double(), xs.cpu())                 # (hi + lo is an fp32 number)
    r32 = torch.log_softmax(xs32 @ Wc.t() + b, dim=1)
    scale = max(float(ref.abs().max()), 1e-300)
    e32 = relerr(r32.cuda(), ref) if C_ > 1 else 0.0
    assert untouched(logp[M:]) and bool((am[M:] == -7).all()), "rows beyond M stay untouched"
    err = float((logp[:M].double() - ref).abs().max()) / (scale if C_ > 1 else 1.0)
    bar = report("head_final", f"C={C_} K={K} ld={ld} M={M} {fmt} tie={tie}", "logp", err, e32, ULP32)
    assert err <= bar
    got = am[:M].long()
    if C_ == 1:
        assert bool((got == 0).all()) and bool((logp[:M] == 0).all())
        return
    margin_bar = 2.0 * bar * scale                              # argmax compared where the fp64 top-2 margin exceeds twice the logp bar
    if tie:
        zt = z.clone()
        zt[:, tie[1]] = -float("inf")                            # the pair counts as one class: the lower index
        top2 = zt.topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > margin_bar
        want = zt.argmax(dim=1)
        assert int((want[safe] == tie[0]).sum()) >= max(1, M // 16), "the tied pair must win somewhere"
        assert torch.equal(got[safe], want[safe]), "a tie goes to the lower class, as torch.argmax gives it"
    else:
        top2 = z.topk(2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > margin_bar
        assert int((~safe).sum()) <= 1e-3 * M, "at most 0.1 % of the rows may be left out of the argmax comparison"
        assert torch.equal(got[safe], z.argmax(dim=1)[safe])


@pytest.mark.parametrize("C_", [26, 32])
def test_head_final_refuses_a_classifier_beyond_the_lds(cuda, C_):
    lib = capi.lib()
    M, K, ld = 16, 600, 640
    xp = torch.zeros((2, M, ld), dtype=torch.int16, device="cuda")
    Wd, bd = torch.zeros((C_, K), device="cuda"), torch.zeros((C_,), device="cuda")
    logp = torch.full((M, C_), float("nan"), device="cuda")
    am = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    assert lib.dinoseg_op_head_final(xp.data_ptr(), M * ld, ld, M, K, Wd.data_ptr(), bd.data_ptr(), C_, logp.data_ptr(), am.data_ptr(), S()) == -1
    assert f"C * ld <= 16384 (C={C_} K=600 ld=640)" in capi.last_error()
    torch.cuda.synchronize()
    assert untouched(logp) and bool((am == -7).all())


# ------------------------------------------------------------------------------------------------ patch_gather (patch 8)
# 32 x 480 x 640 = 1 228 800 work items crosses the 4096 x 256 grid cap: the grid-stride loop runs
GATHER_CASES = [(B, H, W, kind, planes, fmt) for (B, H, W) in [(1, 8, 8), (3, 64, 128)] for kind in (0, 1) for planes in (1, 2)
                for fmt in ("bf16", "fp16")]
GATHER_CASES += [(32, 480, 640, 0, 2, "fp16"), (32, 480, 640, 1, 1, "bf16"), (32, 480, 640, 0, 1, "fp16"), (32, 480, 640, 1, 2, "bf16")]


@pytest.mark.parametrize("B,H,W,kind,planes,fmt", GATHER_CASES)
def test_patch_gather_patch8(cuda, B, H, W, kind, planes, fmt):
    frames = np.random.default_rng(B + H + W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[..., 0] //= 2                                         # the three channels differ in distribution as well as in constants
    fr = torch.from_numpy(frames).cuda()
    x32 = O.preprocess(frames).cuda()                            # the float32 evaluation [B, 3, H, W]
    hp, wp = H // 8, W // 8
    n = B * hp * wp

    def rows(t):
        return t.reshape(B, 3, hp, 8, wp, 8).permute(0, 2, 4, 1, 3, 5).reshape(n, 192)
    if kind == 0:
        mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64, device="cuda")
        sd = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64, device="cuda")
        ref = rows(((fr.double() - 255.0 * mean) / (255.0 * sd)).permute(0, 3, 1, 2))
        src = fr
    else:
        ref = rows(x32.double())
        src = x32.contiguous()
    want32 = rows(x32)
    out = nan16((planes, n + 2, 192))
    with op_fmt(fmt):
        capi.check(capi.lib().dinoseg_op_patch_gather_p(src.data_ptr(), kind, B, H, W, 8, out.data_ptr(), (n + 2) * 192, planes, S()))
        torch.cuda.synchronize()
    assert untouched(out[:, n:])
    e32 = relerr(want32, ref)
    err = relerr(unpack64(out[:, :n], fmt), ref)
    assert err <= report("patch_gather", f"B={B} {H}x{W} kind={kind} planes={planes} {fmt}", "planes", err, e32, ULP16[fmt, planes])
    if planes == 1:                                              # one plane: the rounding of the float32 value, bit for bit
        assert torch.equal(out[0, :n].view(DT[fmt]), want32.to(DT[fmt]))


# ------------------------------------------------------------------------------------------------ attn_probs
# (B, heads, ntok, planes, fmt, spike): one token, one 16-query group, one row into the second, 197 (B > 1), and the working
# resolutions 3601 / 4801 (15 / 19 passes of every thread's key loop; the last query group holds one valid row)
PROBS_CASES = [
    (1, 1, 1, 1, "bf16", False),
    (1, 2, 16, 2, "fp16", False),
    (2, 2, 17, 1, "fp16", False),
    (2, 3, 197, 2, "bf16", False),
    (2, 3, 197, 1, "bf16", True),
    (1, 2, 257, 2, "fp16", True),
    (1, 6, 3601, 2, "fp16", False),
    (1, 2, 3601, 1, "bf16", False),
    (1, 2, 4801, 1, "fp16", False),
    (1, 2, 4801, 2, "bf16", False),
]


def _qkv_planes(x, npad, planes, fmt):
    """[G, ntok, 64] fp32 -> planes [planes, G * npad, 64] with NaN in the padded rows, and the fp64 values the kernel sees"""
    G, ntok, _ = x.shape
    full = torch.full((G, npad, 64), float("nan"))
    full[:, :ntok] = x
    with op_fmt(fmt):
        p = pack(full.reshape(-1, 64).cuda(), planes)
    return p, unpack64(p, fmt).reshape(G, npad, 64)[:, :ntok]


def _softmax2(s):
    """softmax of log2-domain scores, the kernel's form: 2^(s - max) / sum"""
    e = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)


@pytest.mark.parametrize("B,H,ntok,planes,fmt,spike", PROBS_CASES)
def test_attn_probs(cuda, B, H, ntok, planes, fmt, spike):
    g_ = np.random.default_rng(3000 + ntok + planes + H)
    npad = (ntok + 63) // 64 * 64
    G = B * H
    Q = 1.5 * rng_normal(g_, (G, ntok, 64)) + ramp(64, 0.004)[None, None, :] + (ramp(ntok, 1.0) % 13 / 40)[None, :, None]
    K = 1.5 * rng_normal(g_, (G, ntok, 64)) - ramp(64, 0.003)[None, None, :] + ramp(G, 0.05)[:, None, None]
    if spike:                                                    # one key late in the row dominates query 5
        K[:, ntok - 3] = Q[:, 5] * 4.0
    qp, q64 = _qkv_planes(Q * (0.125 * LOG2E), npad, planes, fmt)
    kp, k64 = _qkv_planes(K, npad, planes, fmt)
    out = torch.full((G * ntok * ntok + 64,), float("nan"), device="cuda")
    with op_fmt(fmt):
        capi.check(capi.lib().dinoseg_op_attn_probs(qp.data_ptr(), kp.data_ptr(), G * npad * 64, planes, B, H, ntok, npad, out.data_ptr(), S()))
        torch.cuda.synchronize()
    assert untouched(out[G * ntok * ntok:])
    a = out[:G * ntok * ntok].reshape(G, ntok, ntok)
    assert torch.isfinite(a).all()
    if ntok > 1000:                                              # row 0, the last row and 62 seeded rows; every key of those rows
        rows_ = np.unique(np.concatenate([[0, ntok - 1], np.random.default_rng(ntok).choice(np.arange(1, ntok - 1), 62, replace=False)]))
    else:
        rows_ = np.arange(ntok)
    rows_t = torch.from_numpy(rows_).cuda()
    ref = _softmax2(q64[:, rows_t] @ k64.transpose(-1, -2))                                  # fp64, on the device
    r32 = _softmax2(q64[:, rows_t].float().cpu() @ k64.float().cpu().transpose(-1, -2))      # float32, on the CPU
    assert r32.dtype == torch.float32
    e32 = relerr(r32.cuda(), ref)
    err = relerr(a[:, rows_t], ref)
    case = f"B={B} H={H} ntok={ntok} planes={planes} {fmt} spike={spike}"
    assert err <= report("attn_probs", case, "probabilities", err, e32, ULP32)
    # row sums: every row of the kernel's output on the device, every row of the float32 restatement on the CPU
    full32 = r32 if ntok <= 1000 else _softmax2(q64.float().cpu() @ k64.float().cpu().transpose(-1, -2))
    s32 = float((full32.double().sum(-1) - 1).abs().max())
    serr = float((a.double().sum(-1) - 1).abs().max())
    assert serr <= report("attn_probs", case, "row sums", serr, s32, ULP32)
    if spike:
        assert float(a[:, 5, ntok - 3].min()) > 0.99


# ------------------------------------------------------------------------------------------------ cls_mask_attn
# (ntok, heads, n_masks, mask family, planes, fmt, probs): 256 / 257 = one pass / one key into the second pass of the 256-thread
# loops, 3601 the working resolution, 14 401 = 57.6 KB of the 60 KB score buffer
MASK_CASES = [
    (2, 2, 1, "ones", 1, "bf16", True),
    (65, 6, 3, "rand01", 2, "fp16", True),
    (256, 2, 64, "real", 1, "fp16", False),
    (257, 6, 3, "zeros", 2, "bf16", True),
    (257, 2, 3, "real", 1, "fp16", True),
    (3601, 6, 3, "real", 2, "fp16", True),
    (3601, 2, 64, "rand01", 1, "bf16", True),
    (3601, 2, 1, "ones", 1, "fp16", False),
    (14401, 2, 1, "ones", 1, "fp16", True),
    (14401, 6, 3, "real", 2, "bf16", True),
    (65, 2, 1, "zeros", 1, "bf16", False),
]


def _masks(family, n_masks, n, g_):
    if family == "ones":
        return torch.ones((n_masks, n))
    if family == "zeros":
        return torch.zeros((n_masks, n))
    if family == "rand01":
        return torch.from_numpy((g_.random((n_masks, n)) < 0.5).astype(np.float32))
    return rng_normal(g_, (n_masks, n))                          # real-valued: negative factors flip logits


def _cls_mask_ref(q, k, v, mask):
    """q, k, v [H, ntok, 64] (q in the log2 domain), mask [Nm, ntok - 1] -> probabilities [H, Nm, ntok], context [Nm, H * 64]"""
    s = (k @ q[:, 0, :, None])[:, :, 0]                          # [H, ntok]: the CLS query against every key
    f = torch.cat([torch.zeros((mask.shape[0], 1), dtype=q.dtype, device=q.device), mask.to(q.dtype)], dim=1)
    p = _softmax2(s[:, None, :] * f[None, :, :])
    ctx = (p @ v).permute(1, 0, 2).reshape(mask.shape[0], -1)
    return p, ctx


@pytest.mark.parametrize("ntok,H,n_masks,family,planes,fmt,want_probs", MASK_CASES)
def test_cls_mask_attn(cuda, ntok, H, n_masks, family, planes, fmt, want_probs):
    g_ = np.random.default_rng(4000 + ntok + H + n_masks)
    npad = (ntok + 63) // 64 * 64
    Q = 1.5 * rng_normal(g_, (H, ntok, 64)) + ramp(64, 0.004)[None, None, :]
    K = 1.5 * rng_normal(g_, (H, ntok, 64)) + ramp(H, 0.05)[:, None, None] + (ramp(ntok, 1.0) % 11 / 30)[None, :, None]
    V = rng_normal(g_, (H, ntok, 64)) + ramp(64, 0.01)[None, None, :] + (ramp(ntok, 1.0) % 17 / 20)[None, :, None]
    vfmt = fmt if planes == 2 else "bf16"                        # one fp16 plane: V stays bf16, as the fused attention has it
    qp, q64 = _qkv_planes(Q * (0.125 * LOG2E), npad, planes, fmt)
    kp, k64 = _qkv_planes(K, npad, planes, fmt)
    vp, v64 = _qkv_planes(V, npad, planes, vfmt)
    mask = _masks(family, n_masks, ntok - 1, g_)
    md = mask.cuda()
    W = H * 64
    cplane = n_masks * W + 64                                    # 64 guard elements behind every plane
    ctx = nan16((planes * cplane,))
    probs = torch.full((H * n_masks * ntok + 64,), float("nan"), device="cuda") if want_probs else None
    with op_fmt(fmt):
        capi.check(capi.lib().dinoseg_op_cls_mask_attn(qp.data_ptr(), kp.data_ptr(), vp.data_ptr(), H * npad * 64, planes, H, ntok, npad,
                                                       md.data_ptr(), n_masks, ctx.data_ptr(), cplane, capi.ptr(probs), S()))
        torch.cuda.synchronize()
    pref, cref = _cls_mask_ref(q64, k64, v64, md)
    p32, c32 = _cls_mask_ref(q64.float().cpu(), k64.float().cpu(), v64.float().cpu(), mask)
    assert p32.dtype == torch.float32 and c32.dtype == torch.float32
    case = f"ntok={ntok} H={H} masks={n_masks} {family} planes={planes} {fmt} probs={want_probs}"
    cp = ctx.reshape(planes, cplane)
    assert untouched(cp[:, n_masks * W:])
    got = unpack64(cp[:, :n_masks * W], fmt).reshape(n_masks, W)
    assert torch.isfinite(got).all()
    err = relerr(got, cref)
    assert err <= report("cls_mask_attn", case, "context", err, relerr(c32.cuda(), cref), ULP16[fmt, planes])
    if want_probs:
        assert untouched(probs[H * n_masks * ntok:])
        pg = probs[:H * n_masks * ntok].reshape(H, n_masks, ntok)
        assert torch.isfinite(pg).all()
        err = relerr(pg, pref)
        assert err <= report("cls_mask_attn", case, "probabilities", err, relerr(p32.cuda(), pref), ULP32)
        serr = float((pg.double().sum(-1) - 1).abs().max())
        assert serr <= report("cls_mask_attn", case, "row sums", serr, float((p32.double().sum(-1) - 1).abs().max()), ULP32)


def test_cls_mask_attn_refuses_more_tokens_than_the_score_buffer(cuda):
    ntok, npad = 15361, 15424
    small = torch.zeros((64,), dtype=torch.int16, device="cuda")             # never read: the launcher refuses on the host
    mask = torch.zeros((64,), device="cuda")
    ctx = nan16((2 * 64,))
    probs = torch.full((64,), float("nan"), device="cuda")
    rc = capi.lib().dinoseg_op_cls_mask_attn(small.data_ptr(), small.data_ptr(), small.data_ptr(), npad * 64, 1, 1, ntok, npad, mask.data_ptr(), 1,
                                             ctx.data_ptr(), 64, probs.data_ptr(), S())
    assert rc == -1 and "cls_mask_attn: 15361 tokens exceed the LDS score buffer" in capi.last_error()
    torch.cuda.synchronize()
    assert untouched(ctx) and untouched(probs)


# ------------------------------------------------------------------------------------------------ cls_rows / broadcast_row0 / batch_sum_rows
# (32 x 3601 x 384 and 2 x 3601 x 768 cross the 4096 x 256 grid of batch_sum_rows)
ROW_CASES = [(1, 2, 128), (2, 3601, 768), (32, 3601, 384), (32, 2, 384), (2, 2, 768), (1, 3601, 128)]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("B,ntok,D", ROW_CASES)
def test_cls_rows(cuda, B, ntok, D):
    g_ = np.random.default_rng(5000 + B + ntok + D)
    cls = (rng_normal(g_, (D,)) + ramp(D, 0.01)).cuda()
    pos = (rng_normal(g_, (2, D)) - ramp(D, 0.02)[None, :]).cuda()          # row 1 is not row 0
    X = torch.full((B * ntok + 1, D), float("nan"), device="cuda")
    X[1] = 3.0
    before = X.clone()
    capi.check(capi.lib().dinoseg_op_cls_rows(X.data_ptr(), cls.data_ptr(), pos.data_ptr(), B, ntok, D, S()))
    torch.cuda.synchronize()
    want = before.clone()
    want[0:B * ntok:ntok] = cls + pos[0]                                     # a single fp32 add
    assert torch.equal(_bits(X), _bits(want))


@pytest.mark.parametrize("D,n", [(128, 1), (384, 3), (768, 64), (384, 0), (128, 64)])
def test_broadcast_row0(cuda, D, n):
    X = torch.full((n + 2, D), float("nan"), device="cuda")
    X[0] = (rng_normal(np.random.default_rng(D + n), (D,)) + ramp(D, 0.01)).cuda()
    before = X.clone()
    capi.check(capi.lib().dinoseg_op_broadcast_row0(X.data_ptr(), D, n, S()))
    torch.cuda.synchronize()
    want = before.clone()
    want[1:n + 1] = before[0]
    assert torch.equal(_bits(X), _bits(want))                                # the row behind the last one is still NaN


@pytest.mark.parametrize("B,ntok,D", ROW_CASES)
def test_batch_sum_rows(cuda, B, ntok, D):
    g_ = np.random.default_rng(6000 + B + ntok + D)
    X = (rng_normal(g_, (B, ntok, D)) + ramp(B, 0.3)[:, None, None] + ramp(D, 0.002)[None, None, :] + (ramp(ntok, 1.0) % 19 / 19)[None, :, None])
    Xd = X.cuda()
    out = torch.full((ntok * D + 64,), float("nan"), device="cuda")
    capi.check(capi.lib().dinoseg_op_batch_sum_rows(Xd.data_ptr(), B, ntok, D, out.data_ptr(), S()))
    torch.cuda.synchronize()
    assert untouched(out[ntok * D:])
    got = out[:ntok * D].reshape(ntok, D)
    if B == 1:
        assert torch.equal(got, Xd[0])
        return
    ref = Xd.double().sum(dim=0)
    r32 = torch.zeros((ntok, D))
    for b in range(B):                                                        # the float32 restatement: one add per frame
        r32 += X[b]
    e32 = relerr(r32.cuda(), ref)
    err = relerr(got, ref)
    assert err <= report("batch_sum_rows", f"B={B} ntok={ntok} D={D}", "sums", err, e32, ULP32)


# ------------------------------------------------------------------------------------------------ confusion
# n = 300 007 exceeds the 1024 x 256 grid; C <= 32 runs confusion_kernel, C > 32 the slab kernel
@pytest.mark.parametrize("C_,n", [(1, 1), (7, 255), (32, 100003), (7, 300007), (32, 300007), (1, 100003), (32, 1), (40, 100003), (150, 300007)])
def test_confusion_counts_labels_and_accumulates(cuda, C_, n):
    rng = np.random.default_rng(C_ + n)
    gt = rng.integers(0, C_, n).astype(np.int64)
    pred = rng.integers(0, C_, n).astype(np.int32)
    gt[::97] = -100                         # ignore_index
    gt[5::211] = C_ + 1                     # out of range labels
    gt[11::53] = 2 ** 32 + 3 % C_           # int64 labels whose low 32 bits name a class: ignored, not narrowed
    gt[13::59] = -2 ** 32 + 1 % C_
    pred[::89] = -1                         # out of range predictions
    pred[3::101] = C_
    pred[7::53] = pred[7::53] // 7          # a few heavy cells
    if n == 1:
        gt[0] = 2 ** 32 + 3 % C_
        pred[0] = 0
    start = rng.integers(0, 1000, (C_, C_)).astype(np.int64)                 # the matrix already holds counts
    cm = torch.from_numpy(start.copy()).cuda()
    pred_d, gt_d = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    capi.check(capi.lib().dinoseg_op_confusion(pred_d.data_ptr(), gt_d.data_ptr(), n, C_, cm.data_ptr(), S()))
    torch.cuda.synchronize()
    keep = (gt >= 0) & (gt < C_) & (pred >= 0) & (pred < C_)
    want = start + np.bincount(gt[keep] * C_ + pred[keep], minlength=C_ * C_).reshape(C_, C_)
    assert np.array_equal(cm.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ multi_pack
def _pack_jobs():
    """45 jobs (two launches: 40 + 5): the mix of a ViT-S refresh, odd shapes and an empty job in the middle"""
    blk = [(1152, 384, 1152, 384), (384, 384, 384, 384), (1536, 384, 1536, 384), (384, 1536, 384, 1536)]
    jobs = blk * 4 + [(384, 192, 384, 192), (100, 384, 128, 384), (7, 100, 32, 128), (1, 1, 1, 1), (63, 65, 64, 128), (0, 0, 0, 0), (65, 63, 65, 63),
                      (130, 70, 192, 128)] + blk * 5 + [(7, 100, 128, 128)]
    assert len(jobs) == 45
    return jobs


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("planes", [1, 2])
def test_multi_pack_is_bit_exact(cuda, planes, fmt, flip):
    jobs = _pack_jobs()
    g_ = np.random.default_rng(7000 + planes + flip)
    # magnitudes over 2^-6 .. 2^7, inside fp16's normal range; each job reads its own window of the pool
    pool = torch.from_numpy((np.exp2(g_.uniform(-6, 6, 1 << 21)) * (1 + g_.random(1 << 21)) * g_.choice([-1.0, 1.0], 1 << 21)).astype(np.float32))
    pool_d = pool.cuda()
    dt = DT[fmt]
    offs, srcs, pos = [], [], 64
    for i, (r, c, rp, cp) in enumerate(jobs):
        s0 = (i * 40009) % ((1 << 21) - r * c)
        srcs.append(s0)
        offs.append(pos)
        pos += planes * (rp * cp + 64)
    total = pos
    dst = nan16((total,))
    want = torch.full((total,), NAN16, dtype=torch.int16)
    count = len(jobs)
    transposed = [(i + flip) % 2 for i in range(count)]
    for i, (r, c, rp, cp) in enumerate(jobs):
        x = pool[srcs[i]:srcs[i] + r * c].reshape(r, c)
        hi = x.to(dt)
        pl = [hi, (x - hi.float()).to(dt)][:planes]              # RNE of x, RNE of x - hi (the subtraction is exact in fp32)
        for k, p in enumerate(pl):
            full = torch.zeros((rp, cp), dtype=dt)
            full[:r, :c] = p
            if transposed[i]:
                full = full.t().contiguous()
            o = offs[i] + k * (rp * cp + 64)
            want[o:o + rp * cp] = full.reshape(-1).view(torch.int16)
    i32 = lambda xs: (C.c_int32 * count)(*xs)
    src_a = (C.c_void_p * count)(*[pool_d.data_ptr() + 4 * s for s in srcs])
    dst_a = (C.c_void_p * count)(*[dst.data_ptr() + 2 * o for o in offs])
    plane_a = (C.c_int64 * count)(*[rp * cp + 64 for (_, _, rp, cp) in jobs])
    capi.check(capi.lib().dinoseg_op_multi_pack(count, src_a, dst_a, plane_a, i32([j[0] for j in jobs]), i32([j[1] for j in jobs]),
                                                i32([j[2] for j in jobs]), i32([j[3] for j in jobs]), i32([planes] * count), i32(transposed),
                                                i32([FMT[fmt]] * count), S()))
    torch.cuda.synchronize()
    got = dst.cpu()
    for i, (r, c, rp, cp) in enumerate(jobs):                    # per job first, for a readable failure
        o, e = offs[i], planes * (rp * cp + 64)
        assert torch.equal(got[o:o + e], want[o:o + e]), f"job {i} {jobs[i]} transposed={transposed[i]}"
    assert torch.equal(got, want), "guards and padding"
    # dinoseg_op_pack on the same inputs gives the same bits
    with op_fmt(fmt):
        for i, (r, c, rp, cp) in enumerate(jobs):
            if transposed[i] or rp * cp == 0 or not (i < 2 or 16 <= i < 24):
                continue
            one = nan16((planes, rp * cp + 64))
            capi.check(capi.lib().dinoseg_op_pack(pool_d.data_ptr() + 4 * srcs[i], r, c, one.data_ptr(), rp * cp + 64, rp, cp, planes, S()))
            torch.cuda.synchronize()
            assert torch.equal(one.reshape(-1).cpu(), want[offs[i]:offs[i] + planes * (rp * cp + 64)]), f"dinoseg_op_pack, job {i}"


# ------------------------------------------------------------------------------------------------ adam / adam_multi / multi_zero
ADAM_SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 589824]
GUARD = 16


def _adam_layout():
    """70 tensors (two launches: 64 + 6), empty at positions 0, 33 and 69, 16 guard elements behind each"""
    sizes = []
    for i in range(70):
        if i in (0, 33, 69):
            sizes.append(0)
        elif i in (7, 66):
            sizes.append(589824)
        else:
            sizes.append(ADAM_SIZES[i % 7])
    offs = np.cumsum([0] + [s + GUARD for s in sizes])[:-1]
    return sizes, [int(o) for o in offs], int(sum(sizes) + GUARD * len(sizes))


def _adam_ref(p, g, m, v, lr, b1, b2, eps, wd, decoupled, step, gs, f):
    """torch.optim.Adam / AdamW in the arithmetic of dtype f (train.hip's header comment); returns p, m, v and the magnitudes of
    the terms each of them is summed from"""
    lr, b1, b2, eps, wd, gs = (f(np.float32(t)) for t in (lr, b1, b2, eps, wd, gs))
    one = f(1.0)
    p, g, m, v = (t.astype(f) for t in (p, g, m, v))
    bc1 = one - f(np.power(b1, f(step)))
    bc2s = np.sqrt(one - f(np.power(b2, f(step))))
    gi = g * gs
    gmag = np.abs(gi)
    pi = p
    if decoupled:
        pi = p * (one - lr * wd)
    elif wd != 0:
        gi = gi + wd * p
        gmag = gmag + wd * np.abs(p)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    upd = (lr / bc1) * (mi / (np.sqrt(vi) / bc2s + eps))
    mags = (np.abs(pi) + np.abs(upd), b1 * np.abs(m) + (one - b1) * gmag, b2 * np.abs(v) + (one - b2) * gmag * gmag)
    return (pi - upd, mi, vi), mags


ADAM_CASES = [(1e-3, 0.0, 0, 1, 1.0), (1e-3, 1e-2, 0, 2, 0.5), (1e-6, 1e-2, 1, 1000, 1.0), (1e-3, 1e-2, 0, 100000, 1.0), (1e-6, 1e-2, 1, 1, 0.5),
              (1e-3, 0.0, 0, 1000, 0.5), (1e-6, 1e-2, 1, 2, 1.0), (1e-3, 1e-2, 0, 1, 1.0), (1e-6, 1e-2, 1, 100000, 0.5)]


@pytest.mark.parametrize("lr,wd,decoupled,step,gs", ADAM_CASES)
def test_adam_single_and_multi_tensor(cuda, lr, wd, decoupled, step, gs):
    sizes, offs, total = _adam_layout()
    g_ = np.random.default_rng(8000 + step + decoupled)
    b1, b2, eps = 0.9, 0.999, 1e-8
    p0 = (0.5 * g_.standard_normal(total)).astype(np.float32)
    g0 = (np.power(10.0, g_.uniform(-8, 0, total)) * g_.choice([-1.0, 1.0], total)).astype(np.float32)      # 1e-8 .. 1
    m0 = (0.01 * g_.standard_normal(total)).astype(np.float32)
    v0 = (1e-4 * g_.random(total) + 1e-12).astype(np.float32)
    live = np.zeros(total, dtype=bool)
    for s, o in zip(sizes, offs):
        live[o:o + s] = True
    for a in (p0, g0, m0, v0):
        a[~live] = np.nan                                        # guards
    lib = capi.lib()
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    gd = dev(g0)
    # the multi-tensor entry on one copy of the state ...
    pm, mm, vm = dev(p0), dev(m0), dev(v0)
    k = len(sizes)
    arr = lambda t: (C.c_void_p * k)(*[t.data_ptr() + 4 * o for o in offs])
    capi.check(lib.dinoseg_adam_step_multi(k, arr(pm), arr(gd), arr(mm), arr(vm), (C.c_int64 * k)(*sizes), lr, b1, b2, eps, wd, decoupled, step, gs,
                                           S()))
    # ... the single-tensor entry, tensor by tensor, on another
    ps, ms, vs = dev(p0), dev(m0), dev(v0)
    for s, o in zip(sizes, offs):
        capi.check(lib.dinoseg_adam_step(ps.data_ptr() + 4 * o, gd.data_ptr() + 4 * o, ms.data_ptr() + 4 * o, vs.data_ptr() + 4 * o, s, lr, b1, b2,
                                         eps, wd, decoupled, step, gs, S()))
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):                              # (the guards are NaN)
        (rp, rm, rv), mags = _adam_ref(p0, g0, m0, v0, lr, b1, b2, eps, wd, decoupled, step, gs, np.float64)
        (fp_, fm, fv), _ = _adam_ref(p0, g0, m0, v0, lr, b1, b2, eps, wd, decoupled, step, gs, np.float32)
    assert fp_.dtype == np.float32
    case = f"lr={lr} wd={wd} decoupled={decoupled} step={step} grad_scale={gs}"
    for name, got_m, got_s, ref, r32, mag, orig in (("p", pm, ps, rp, fp_, mags[0], p0), ("m", mm, ms, rm, fm, mags[1], m0),
                                                    ("v", vm, vs, rv, fv, mags[2], v0)):
        gm, gs_ = got_m.cpu().numpy(), got_s.cpu().numpy()
        assert np.array_equal(gm[~live].view(np.int32), orig[~live].view(np.int32)), f"{name}: guards untouched"
        e32 = float(np.max(np.abs(r32[live].astype(np.float64) - ref[live]) / mag[live]))
        for entry, got in (("adam_multi", gm), ("adam", gs_)):
            assert np.isfinite(got[live]).all()
            err = float(np.max(np.abs(got[live].astype(np.float64) - ref[live]) / mag[live]))
            assert err <= report(entry, case, name, err, e32, ULP32)
        assert np.array_equal(gm.view(np.int32), gs_.view(np.int32)), f"{name}: the two entries agree bit for bit"
    assert np.array_equal(gd.cpu().numpy().view(np.int32), g0.view(np.int32)), "gradients are read only"
    if step <= 2:                                                # pin the restatement to torch.optim itself (fp64, CPU)
        n = 4097
        sel = np.flatnonzero(live)[:n]
        w = torch.from_numpy(p0[sel].astype(np.float64)).requires_grad_(True)
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([w], lr=float(np.float32(lr)), betas=(float(np.float32(b1)), float(np.float32(b2))),
                                                                     eps=float(np.float32(eps)), weight_decay=float(np.float32(wd)))
        opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m0[sel].astype(np.float64)),
                        "exp_avg_sq": torch.from_numpy(v0[sel].astype(np.float64))}
        w.grad = torch.from_numpy(g0[sel].astype(np.float64) * float(np.float32(gs)))
        opt.step()
        st = opt.state[w]
        for got, ref, mag in ((w.detach().numpy(), rp, mags[0]), (st["exp_avg"].numpy(), rm, mags[1]), (st["exp_avg_sq"].numpy(), rv, mags[2])):
            assert float(np.max(np.abs(got - ref[sel]) / mag[sel])) <= 1e-13         # fp64 against fp64: a few hundred ulps of the terms


def test_multi_zero(cuda):
    sizes, offs, total = _adam_layout()
    buf = torch.full((total,), float("nan"), device="cuda")
    k = len(sizes)
    capi.check(capi.lib().dinoseg_op_multi_zero(k, (C.c_void_p * k)(*[buf.data_ptr() + 4 * o for o in offs]), (C.c_int64 * k)(*sizes), S()))
    torch.cuda.synchronize()
    want = torch.full((total,), float("nan"))
    for s, o in zip(sizes, offs):
        want[o:o + s] = 0.0
    assert torch.equal(_bits(buf.cpu()), _bits(want))            # exact +0, guards untouched


# ------------------------------------------------------------------------------------------------ the two side paths at 480 x 480
_ORACLE_480 = {}


def _oracle_480():
    if not _ORACLE_480:
        cfg = ViTConfig(n_blocks=2)
        sd = procedural_state_dict(cfg)
        x = O.preprocess(synthetic_frames(1, 480, seed=480))
        rng = np.random.default_rng(481)
        masks = torch.stack([torch.ones((60, 60)), torch.zeros((60, 60)), torch.from_numpy((rng.random((60, 60)) < 0.5).astype(np.float32))])
        W = O.to_torch(sd)
        with torch.no_grad():
            _ORACLE_480.update(cfg=cfg, sd=sd, x=x, masks=masks, attn=O.last_selfattention(x, W, cfg.num_heads),
                               emb=O.forward_mask(x, W, cfg.num_heads, masks),
                               mattn=O.forward_mask(x, W, cfg.num_heads, masks, return_attention=True))
    return _ORACLE_480


@pytest.mark.parametrize("precision", ["bf16x3", "fp16x3"])
def test_side_paths_at_480(cuda, precision):
    """get_last_selfattention and forward_mask of ViT-S/8 (2 blocks) at 480 x 480 = 3601 tokens against the CPU oracle: 15 passes of
    the key loops of attn_probs_kernel and cls_mask_attn_kernel inside the model.  Bars: those of the golden tests of the same outputs."""
    o = _oracle_480()
    cfg = o["cfg"]
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in o["sd"].items()}, strict=True)
    m.to("cuda:0")
    x = o["x"].cuda()
    a = m.dino.get_last_selfattention(x)
    assert tuple(a.shape) == (1, cfg.num_heads, 3601, 3601)
    rows_ = np.unique(np.concatenate([[0, 3600], np.random.default_rng(3601).choice(np.arange(1, 3600), 62, replace=False)]))
    rows_t = torch.from_numpy(rows_)
    e_attn = float((a[0][:, rows_t.cuda()].cpu() - o["attn"][0][:, rows_t]).abs().max())
    e_sum = float((a.double().sum(-1) - 1).abs().max())
    emb = m.dino.forward_mask(x, o["masks"]).cpu()
    att = m.dino.get_last_selfattention(x, cls_mask=o["masks"]).cpu()
    assert emb.shape == o["emb"].shape and att.shape == o["mattn"].shape
    e_emb, e_matt = float((emb - o["emb"]).abs().max()), float((att - o["mattn"]).abs().max())
    print(f"helper_ops side_paths_480 [{precision}] attention {e_attn:.3e} row sums {e_sum:.3e} mask embedding {e_emb:.3e} masked attention {e_matt:.3e}")
    assert e_attn <= 2e-4 and e_sum <= 1e-5
    assert e_emb <= TOL and e_matt <= 1e-4
