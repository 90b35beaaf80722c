"""Yardsticks of the image-guided iterative refinement (include/dinoseg.h, dinoseg_op_refine_iterate).

``weights_ref`` / ``pass_ref`` / ``refine_ref`` restate the rule in exact integers (taps, sums, Nv, |differences|) and fp64
(everything else) with the fp32-rounded constant the library uses, vectorised over the pixels.  ``pass_f32_constant`` restates the
constant-guide pass in NumPy float32, bit for bit.  ``pass_bars`` bounds one pass's fp32 error per pixel from the operation counts.
"""
import math

import numpy as np

LOG2E = 1.44269504088896340736
DEFAULT_DILATIONS = (1, 2, 4, 8, 12, 24)
U = 2.0 ** -24                  # the unit roundoff of fp32 under round-to-nearest


def refine_constant(sigma, n_dil):
    """k = log2(e) sqrt(S (S - 1)) / (3 sigma), S = 9 M: computed in fp64, rounded once to fp32 (returned as that fp32's fp64 value)."""
    S = 9.0 * n_dil
    return float(np.float32(LOG2E * math.sqrt(S * (S - 1.0)) / (3.0 * float(sigma))))


def taps(dilations):
    """the 8 M offsets (dy, dx): dilation ascending, then dy ascending, then dx ascending, without (0, 0)"""
    return [(dy, dx) for d in dilations for dy in (-d, 0, d) for dx in (-d, 0, d) if (dy, dx) != (0, 0)]


def shifted(a, dy, dx):
    """a [..., OH, OW] read at (y + dy, x + dx) clamped to the frame (replicate border)"""
    OH, OW = a.shape[-2], a.shape[-1]
    yy = np.clip(np.arange(OH) + dy, 0, OH - 1)
    xx = np.clip(np.arange(OW) + dx, 0, OW - 1)
    return a[..., yy[:, None], xx[None, :]]


def weights_ref(guide, dilations=DEFAULT_DILATIONS, sigma=0.1):
    """guide uint8 [B, OH, OW, 3] -> (w fp64 [T, B, OH, OW] = exp2(e_t - e_max), W fp64 [B, OH, OW] = their sum in tap order,
    E fp64 [B, OH, OW] = max_t |e_t|)."""
    M = len(dilations)
    S = 9 * M
    k = refine_constant(sigma, M)
    g = np.ascontiguousarray(np.moveaxis(guide.astype(np.int64), -1, 1))        # [B, 3, OH, OW]
    s1 = M * g
    s2 = M * g * g
    tp = taps(dilations)
    for dy, dx in tp:
        q = shifted(g, dy, dx)
        s1 = s1 + q
        s2 = s2 + q * q
    Nv = S * s2 - s1 * s1
    assert int(Nv.min()) >= 0 and int(Nv.max()) < 2 ** 31
    r = np.where(Nv == 0, 0.0, k / np.sqrt(np.maximum(Nv, 1).astype(np.float64)))
    e = np.empty((len(tp),) + (g.shape[0],) + g.shape[2:], dtype=np.float64)
    for t, (dy, dx) in enumerate(tp):
        a = np.abs(g - shifted(g, dy, dx)).astype(np.float64)
        e[t] = -(a[:, 0] * r[:, 0] + a[:, 1] * r[:, 1] + a[:, 2] * r[:, 2])
    emax = e.max(0)
    E = np.abs(e).max(0)
    w = np.exp2(e - emax[None])
    W = np.zeros_like(emax)
    for t in range(len(tp)):
        W += w[t]
    return w, W, E


def pass_ref(P, w, W, dilations=DEFAULT_DILATIONS):
    """One pass in fp64: P [B, C, OH, OW] -> sum_t w_t P(q_t) / W."""
    P = np.asarray(P, dtype=np.float64)
    acc = np.zeros_like(P)
    for t, (dy, dx) in enumerate(taps(dilations)):
        acc += w[t][:, None] * shifted(P, dy, dx)
    return acc / W[:, None]


def refine_ref(P0, guide, dilations=DEFAULT_DILATIONS, sigma=0.1, iters=10):
    """`iters` passes in fp64 from the state P0 [B, C, OH, OW]."""
    w, W, _ = weights_ref(guide, dilations, sigma)
    P = np.asarray(P0, dtype=np.float64)
    for _ in range(iters):
        P = pass_ref(P, w, W, dilations)
    return P


def labels_of(P):
    """the FIRST maximum over classes, -1 where it is not > 0; and the top-2 margin (inf with one class)"""
    lab = P.argmax(1)
    top = P.max(1)
    lab = np.where(top > 0, lab, -1)
    if P.shape[1] == 1:
        return lab, np.full(lab.shape, np.inf)
    part = np.partition(P, P.shape[1] - 2, axis=1)
    return lab, part[:, -1] - part[:, -2]


def seed_labels_ref(labels, C):
    """int labels [B, OH, OW] -> one-hot fp32 [B, C, OH, OW]; a label outside [0, C) gives an all-zero pixel"""
    k = np.arange(C).reshape(1, C, 1, 1)
    return (np.asarray(labels)[:, None] == k).astype(np.float32)


def bilinear_coords(i, o):
    """the exact coordinate rule of dinoseg_op_upsample_argmax along one axis: (i0, i1, lambda as an exact fp64 quotient)"""
    d = np.arange(o, dtype=np.int64)
    num = np.maximum((2 * d + 1) * i - o, 0)
    den = 2 * o
    q = num // den
    rem = num - q * den
    sat = q >= i - 1
    q = np.where(sat, i - 1, q)
    rem = np.where(sat, 0, rem)
    return q, np.minimum(q + 1, i - 1), rem.astype(np.float64) / float(den)


def bilinear_ref(scores, hp, wp, OH, OW):
    """scores [B, hp*wp, C] -> fp64 [B, C, OH, OW]: a + (b - a) lambda along x, then along y"""
    B, C = scores.shape[0], scores.shape[-1]
    L = np.asarray(scores, dtype=np.float64).reshape(B, hp, wp, C).transpose(0, 3, 1, 2)
    x0, x1, lx = bilinear_coords(wp, OW)
    y0, y1, ly = bilinear_coords(hp, OH)
    h = L[..., x0] + (L[..., x1] - L[..., x0]) * lx
    return h[:, :, y0] + (h[:, :, y1] - h[:, :, y0]) * ly[:, None]


def softmax_ref(v, gain):
    g = float(np.float32(gain)) * np.asarray(v, dtype=np.float64)
    x = np.exp(g - g.max(1, keepdims=True))
    return x / x.sum(1, keepdims=True)


def seed_scores_ref(scores, hp, wp, OH, OW, gain=1.0):
    """softmax over classes of gain x the exact bilinear enlargement, fp64 [B, C, OH, OW]"""
    return softmax_ref(bilinear_ref(scores, hp, wp, OH, OW), gain)


def seed_bar(C, vmax, gain=1.0, teacher_forced=False):
    """A bound on |device seed - fp64 seed| per element, with u = 2^-24, vmax = max |score| and every probability <= 1.
      the enlargement: a lerp a + (b - a) lambda rounds b - a (u 2 vmax) and the fmaf (u vmax); the two row values carry 3 u vmax
        each into the third lerp, which adds its own 3 u vmax and the rounded difference of the carried errors -> <= 8 u vmax
        (absent when the fp64 side starts from the device's own enlargement)
      g_k = gain v_k rounded: u gain vmax; so g_k and m = max g each carry (8 + 1) gain vmax u, the rounded difference g_k - m
        adds u 2 gain vmax, and up_exp's rounded product with log2(e) moves the argument by u |g_k - m| <= u 2 gain vmax
        -> da = (2 (8 + 1) + 4) gain vmax u = 22 gain vmax u, or (2 + 4) gain vmax u teacher-forced
      a perturbation da of every argument moves a softmax value p by at most (e^(2 da) - 1) p <= 2 da (1 + 2 da)
      v_exp_f32: one ulp (2 u relative) on x_k and on the sum; the sum of C terms in class order: (C - 1) u relative; the
        reciprocal and the final product u each -> (C + 5) u."""
    da = (6.0 if teacher_forced else 22.0) * float(gain) * float(vmax) * U
    return 2.0 * da * (1.0 + 2.0 * da) + (C + 5) * U + 2.0 ** -120


def pass_f32_constant(P, dilations=DEFAULT_DILATIONS, iters=1):
    """The pass under a constant guide in NumPy float32: every weight is exactly 1, so acc = fmaf(1, P(q_t), acc) is one rounded
    addition per tap in tap order from 0, W = T exactly, and P' = acc * fl(1 / T)."""
    P = np.asarray(P, dtype=np.float32)
    tp = taps(dilations)
    inv = np.float32(1.0) / np.float32(len(tp))
    for _ in range(iters):
        acc = np.zeros_like(P)
        for dy, dx in tp:
            acc = acc + shifted(P, dy, dx)
        P = acc * inv
    return P


def pass_bars(P, E, dilations=DEFAULT_DILATIONS):
    """A bound on one pass's fp32 error, fp64 [B, 1, OH, OW], relative to the largest |tap value| of the pixel (over classes and taps).

    With u = 2^-24 and per pixel E = max_t |e_t|, Pmax = max |P_k(q_t)|:
      r = k / sqrt(float(Nv)): conversion u, square root u / 2 + u, quotient u             -> relative error <= 3 u (rounded up)
      e_t: three same-sign terms, a product and two fmaf, each rounded once                 -> |de_t| <= (3 + 3) u |e_t| <= 6 u E
      e_max likewise (a maximum is 1-Lipschitz); the difference e_t - e_max is rounded once -> |dd_t| <= (6 + 6 + 1) u E = 13 u E
      w_t = exp2(d_t): relative error ln(2) |dd_t| plus one ulp of the instruction (2 u)    -> eps_w <= (13 ln 2 E + 2) u
      numerator: eps_w sum w |P| from the weights, T fmaf roundings of partial sums each <= sum w |P| <= W Pmax
                                                                                            -> (eps_w + T u) W Pmax
      W: the same with P = 1                                                                -> relative (eps_w + T u)
      the reciprocal and the final product: u each
    so |dP'| <= (2 T + 2 (13 ln 2 E + 2) + 2) u Pmax, stated as (2 T + 8 + 19 E) u Pmax (13 ln 2 x 2 = 18.03 rounded up, and two
    units of slack for second-order terms).  A flushed denormal weight moves the result by less than 2^-126 T Pmax."""
    P = np.abs(np.asarray(P, dtype=np.float64))
    T = 8 * len(dilations)
    pm = P.max(1, keepdims=True)                                                # max over classes first: then over the taps
    pmax = np.zeros_like(pm)
    for dy, dx in taps(dilations):
        pmax = np.maximum(pmax, shifted(pm, dy, dx))
    return (2 * T + 8 + 19.0 * E[:, None]) * U * pmax + 2.0 ** -120 * pmax


def torch_plain(P, guide, dilations=DEFAULT_DILATIONS, sigma=0.1, iters=1):
    """A plain torch statement written from the rule: F.pad(mode="replicate"), shifted slices, torch.std(unbiased=True); fp64.
    P [B, C, OH, OW], guide uint8 [B, OH, OW, 3] (NumPy in, NumPy out)."""
    import torch
    import torch.nn.functional as F
    P = torch.as_tensor(np.asarray(P, dtype=np.float64))
    g = torch.as_tensor(np.asarray(guide)).permute(0, 3, 1, 2).to(torch.float64)
    D = max(dilations)
    OH, OW = g.shape[-2:]

    def stack(a, with_centre):
        ap = F.pad(a, (D, D, D, D), mode="replicate")
        out = []
        for d in dilations:
            for dy in (-d, 0, d):
                for dx in (-d, 0, d):
                    if (dy, dx) == (0, 0) and not with_centre:
                        continue
                    out.append(ap[:, :, D + dy:D + dy + OH, D + dx:D + dx + OW])
        return torch.stack(out, 2)                                              # [B, ch, taps, OH, OW]

    std = torch.std(stack(g, True), dim=2, unbiased=True)                       # [B, 3, OH, OW]
    k = refine_constant(sigma, len(dilations)) / math.sqrt(9 * len(dilations) * (9 * len(dilations) - 1.0))    # log2(e) / (3 sigma)
    a = (stack(g, False) - g[:, :, None]).abs()
    scaled = torch.where(std[:, :, None] > 0, a * k / std[:, :, None].clamp_min(1e-300), torch.zeros_like(a))
    w = torch.softmax(-scaled.sum(1) * math.log(2.0), dim=1)                    # exp2(e - e_max) / W
    for _ in range(iters):
        P = (stack(P, False) * w[:, None]).sum(2)
    return P.numpy()


def make_guides(rng, B, OH, OW):
    """Two guides: uniform random bytes, and 8 x 8-pixel blocks of one colour each with uniform noise of +-4."""
    noise = rng.integers(0, 256, size=(B, OH, OW, 3), dtype=np.uint8)
    by, bx = (OH + 7) // 8, (OW + 7) // 8
    blocks = rng.integers(4, 252, size=(B, by, bx, 3)).astype(np.int64)
    blocks = np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)[:, :OH, :OW]
    blocks = blocks + rng.integers(-4, 5, size=blocks.shape)
    return noise, np.ascontiguousarray(blocks.astype(np.uint8))


def make_state(rng, B, C, OH, OW):
    """softmax over classes of 2 randn, fp32 [B, C, OH, OW]"""
    z = 2.0 * rng.standard_normal((B, C, OH, OW))
    x = np.exp(z - z.max(1, keepdims=True))
    return (x / x.sum(1, keepdims=True)).astype(np.float32)


def edge_case(e, noise=0, seed=0):
    """The edge-following construction: a 48 x 64 two-colour guide, left (200, 40, 40), right (40, 40, 200), its edge at column e
    (uniform noise of +-`noise` on every byte), a one-hot two-class label seed whose boundary lies at the nearest multiple of 8.
    Returns (seed labels int32 [1, 48, 64], guide uint8 [1, 48, 64, 3], the expected labels [1, 48, 64])."""
    OH, OW = 48, 64
    xx = np.broadcast_to(np.arange(OW), (OH, OW))
    right = xx >= e
    guide = np.where(right[..., None], np.array([40, 40, 200]), np.array([200, 40, 40])).astype(np.int64)
    if noise:
        guide = guide + np.random.default_rng(seed).integers(-noise, noise + 1, size=guide.shape)
    seed_edge = 8 * ((e + 4) // 8)
    return (xx >= seed_edge).astype(np.int32)[None], np.ascontiguousarray(guide.astype(np.uint8))[None], right.astype(np.int64)[None]
