"""Library options across weight refreshes (-m gpu).

dinoseg_refresh_weights lays out the packed copies of every linear, and four options decide there which extra copies exist
(kernels.h Options): fp16_patch_planes and gemm_rs_ln act from the next refresh on and only then; mlp_fused4 and each bit of
gemm_rs run a route only while they were on at the last refresh AND are still on at the forward.  A refresh happens on every
load_state_dict, in-place weight update and fine-tune step, so a handle meets every order of "set an option" and "refresh".

The contract checked here: every forward is bit-identical (log-probabilities and argmax) to the same forward of a FRESH model with
the same weights whose first refresh ran under
    fp16_patch_planes, gemm_rs_ln     = their values at the last refresh,
    mlp_fused4, gemm_rs               = (value at the last refresh) AND (current value), bit by bit,
    every other option                = its current value.
Each fresh model is checked once against the CPU oracle (oracle/dinoseg_oracle.py) with the bars the suite already applies
(FP16_BOUND of test_fp16_gpu.py, test_g7_vitb8_fp16, test_model_gpu.py's bf16 bars), so the copies compared with are right, not
merely equal.  Batches of 2 frames: the two-stream split stays off.

In the sequences, "R" is a refresh (load_state_dict of the same values, copied in place; "R+" an in-place add_ of a parameter to
itself and its inverse) followed by a forward, and "then X" sets X with no refresh before the forward.
"""
import numpy as np
import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames
from oracle import dinoseg_oracle as O

pytestmark = pytest.mark.gpu

# every option this file sets: a test keeps their values in a dict that starts from what the library reads (_current)
TRACKED = ("mlp_fused", "proj_fused", "qkv_fused", "mlp_fused4", "gemm_rs", "gemm_rs_ln", "gemm_rs_min_rows", "fp16_patch_planes",
           "streams", "split_min")

VITS = ViTConfig(n_blocks=3)
VITB = ViTConfig(embed_dim=768, num_heads=12, n_blocks=2)
VITB_R6 = ViTConfig(embed_dim=768, num_heads=12, mlp_ratio=6, n_blocks=2)      # fc1 is 4608 wide: more than gemm_rs takes

# (max |dlogp|, largest fraction of argmax flips or None) against the oracle: ViT-S fp16 FP16_BOUND (test_fp16_gpu.py), bf16
# test_model_gpu.py's 0.2 / 1 %; ViT-B bf16 test_g7_vitb8_batch16's 0.1 / 1 %.  Those were measured at 480 px, mostly at 12 blocks.
# Two do NOT hold at the shapes here (2 frames of 240 px, 2 blocks), on every route, gemm_rs off included -- the mode, not a route:
#  * ViT-B fp16, test_g7_vitb8_fp16's 1.2e-2 (256 sampled rows of one 480 px frame, 12 blocks): 1.35e-2 .. 1.60e-2 here; the CPU
#    emulation of the mode's operand rounding alone (oracle/precision_ablation.py) gives 1.21e-2 here against 7.5e-3 at the G7
#    shape.  Held instead to the relation test_fp16_is_closer_to_the_reference_than_bf16_at_batch_32 applies: under 0.4 x the error
#    of the bf16 model with the same options (measured 0.23 .. 0.30 x).
#  * ViT-B bf16, 1 % flips: 18 of 1800 with gemm_rs 0 or gemm_rs_ln 0, 20 (1.11 %) with gemm_rs 7 and gemm_rs_ln 0 (the separate
#    LayerNorm's bf16 round trip: 8.1e-2 against 5.4e-2 with the LayerNorm inside gemm_rs).  The 0.1 bar on max |dlogp| still holds,
#    so every flip is a near-tie (oracle top-2 margin <= 0.2); the count is not asserted at this shape.
BARS = {(384, "fp16"): (4e-2, None), (384, "bf16"): (0.2, 0.01), (768, "fp16"): (None, None), (768, "bf16"): (0.1, None)}


def _set(opts):
    for k, v in opts.items():
        dino_amd.set_option(k, v)


def _current():
    return {k: dino_amd.get_option(k) for k in TRACKED}


def _tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _model(cfg, precision, sd):
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=precision, arch=cfg)
    m.load_state_dict(_tensors(sd), strict=True)
    return m.to("cuda:0")


def _forward(m, frames):
    lp, am = m.forward_frames(frames)
    torch.cuda.synchronize()
    return lp.cpu(), am.cpu().long()


def _generation(m):
    return capi.lib().dinoseg_state_generation(m._handle)


def _refresh(m, sd, how):
    """Weights change in place through a public path: the next call re-binds and refreshes."""
    if how == "R":
        m.load_state_dict(_tensors(sd))
    else:
        p = m.dino.blocks[0].mlp.fc1.weight
        before = p.detach().clone()
        with torch.no_grad():
            p.add_(before)          # 2w and back: both steps are exact
            p.sub_(before)
        assert torch.equal(p.detach(), before)


def contract(snap, cur):
    """The options of the fresh model a forward must equal (module docstring)."""
    want = dict(cur)
    want["fp16_patch_planes"] = snap["fp16_patch_planes"]
    want["gemm_rs_ln"] = snap["gemm_rs_ln"]
    want["mlp_fused4"] = snap["mlp_fused4"] & cur["mlp_fused4"]
    want["gemm_rs"] = snap["gemm_rs"] & cur["gemm_rs"]
    return want


_SD, _ORACLE, _FRESH = {}, {}, {}


def _weights(cfg):
    if cfg not in _SD:
        _SD[cfg] = procedural_state_dict(cfg)
    return _SD[cfg]


def _frames(B, r, seed):
    return synthetic_frames(B, r, seed=seed)


def _oracle(cfg, frames_np, key):
    if (cfg, key) not in _ORACLE:
        with torch.no_grad():
            _ORACLE[(cfg, key)] = O.dinoseg_forward(O.preprocess(frames_np), O.to_torch(_weights(cfg)), cfg.num_heads)
    return _ORACLE[(cfg, key)]


def fresh(cfg, precision, frames_np, key, opts):
    """Output of a fresh model whose first refresh and forward run under `opts` (in a scope of their own); the first time an
    option set is seen, the output is also checked against the oracle."""
    k = (cfg, precision, key, tuple(sorted(opts.items())))
    if k not in _FRESH:
        with dino_amd.options(**opts):
            m = _model(cfg, precision, _weights(cfg))
            lp, am = _forward(m, torch.from_numpy(frames_np).cuda())
            m._release()
        ref = _oracle(cfg, frames_np, key)
        err = float((lp - ref).abs().max())
        flips = float((am != ref.argmax(1)).float().mean())
        tol, max_flips = BARS[(cfg.embed_dim, precision)]
        print(f"oracle D={cfg.embed_dim} F={cfg.hidden} L={cfg.n_blocks} {precision} {dict(opts)}: max|dlogp| {err:.3e}, "
              f"flips {flips:.4f}")
        assert torch.isfinite(lp).all()
        if tol is None:
            tol = 0.4 * float((fresh(cfg, "bf16", frames_np, key, opts)[0] - ref).abs().max())
        assert err <= tol, (opts, err, tol)
        assert max_flips is None or flips <= max_flips, (opts, flips)
        _FRESH[k] = (lp, am)
    return _FRESH[k]


def run_sequence(cfg, precision, base, steps, B=2, r=240, seed=31):
    """Runs `steps` [(kind, options)] on one new model: kind "R" / "R+" refreshes (_refresh) before the forward, "then" does not.
    Every forward must equal the fresh model of contract(options at the last refresh, current options).  Returns the distinct
    contract option sets met, in order, with their outputs."""
    sd = _weights(cfg)
    frames_np = _frames(B, r, seed)
    key = (B, r, seed)
    frames = torch.from_numpy(frames_np).cuda()
    cur = dict(_current(), **base)
    snap = None
    met = {}
    with dino_amd.options(**cur):
        m = _model(cfg, precision, sd)
        for i, (kind, opts) in enumerate(steps):
            _set(opts)
            cur.update(opts)
            if kind in ("R", "R+"):
                if snap is not None:        # (the first forward is the model's first refresh)
                    _refresh(m, sd, kind)
                snap = dict(cur)
            else:
                assert kind == "then" and snap is not None
            lp, am = _forward(m, frames)
            want = contract(snap, cur)
            ref_lp, ref_am = fresh(cfg, precision, frames_np, key, want)
            assert torch.equal(lp, ref_lp) and torch.equal(am, ref_am), \
                (f"step {i} ({kind} {opts}): max |dlogp| {float((lp - ref_lp).abs().max()):.3e} against a fresh model with {want}")
            met.setdefault(tuple(sorted(want.items())), lp)
        m._release()
    return met


def _assert_distinct(met):
    """The option sets of a sequence change the arithmetic: without this the comparisons above could not tell them apart."""
    outs = list(met.values())
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not torch.equal(outs[i], outs[j])


def _seq(spec, option):
    """'1 R 0 R then 1' -> [("R", {option: 1}), ("R", {option: 0}), ("then", {option: 1})]; 'R+' is the add_ refresh."""
    tok = spec.split()
    return [("then", {option: int(v)}) if k == "then" else (v, {option: int(k)}) for k, v in zip(tok[::2], tok[1::2])]


def _id(spec):
    return spec.replace(" ", "")


# ---------------------------------------------------------------------------------------------------------------- a: mlp_fused4
@pytest.mark.parametrize("spec", ["1 R 0 R", "0 R 1 R+", "1 R then 0", "0 R then 1"], ids=_id)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_mlp_fused4_across_refreshes(cuda, precision, spec):
    """ViT-S/8, 3 blocks, every block's projection + MLP half fused (mlp_fused = 2, no qkv tail): the one-wave launch
    (mlp_fused4.hip) against the two-wave one (mlp_fused2.hip).  "1 R 0 R" is the stale one-wave copies' case: the second refresh
    must not re-pack them over the two-wave copies that now live at their offsets.  Against the oracle: fp16 3.25e-2 / 1 flip of
    1800 (two waves), 3.36e-2 / 0 (one wave); bf16 0.139 / 0.72 %, 0.135 / 0.67 %."""
    met = run_sequence(VITS, precision, {"mlp_fused": 2, "qkv_fused": 0}, _seq(spec, "mlp_fused4"))
    _assert_distinct(met)


# -------------------------------------------------------------------------------------------------- b: gemm_rs and gemm_rs_ln
@pytest.mark.parametrize("option,spec", [("gemm_rs", "3 R 0 R then 3"), ("gemm_rs", "3 R then 0"), ("gemm_rs", "0 R 7 R"),
                                         ("gemm_rs_ln", "1 R 0 R"), ("gemm_rs_ln", "0 R 1 R"), ("gemm_rs_ln", "1 R 0 R then 1")],
                         ids=lambda v: _id(v) if " " in v else v)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_gemm_rs_across_refreshes(cuda, precision, option, spec):
    """ViT-B/8, 2 blocks, the row-stationary GEMMs (gemm_rs.hip) from the first row on.  A copy packed with the LayerNorm folded in
    (gemm_rs_ln) and its folded bias must leave together with the option at a refresh, and a route switched off at a refresh
    must stay off when the option comes back before the next one.  Against the oracle over gemm_rs 0 / 3 / 7 x gemm_rs_ln 0 / 1:
    fp16 1.40e-2 .. 1.60e-2 (0.11-0.28 % flips), bf16 5.4e-2 .. 8.2e-2 (0.61-1.11 % flips): BARS."""
    met = run_sequence(VITB, precision, {"gemm_rs_min_rows": 1}, _seq(spec, option))
    _assert_distinct(met)


# ------------------------------------------------------------------------------------------------------- c: fp16_patch_planes
@pytest.mark.parametrize("spec", ["1 R 2 R", "2 R 1 R", "1 R then 2"], ids=_id)
def test_fp16_patch_planes_across_refreshes(cuda, spec):
    """ViT-S/8, 3 blocks, fp16: the patch embedding on one fp16 plane or on bf16 hi + lo planes.  The option is read at refresh
    only ("then 2" changes nothing), and a copy that changes size moves every copy after it.  Against the oracle: 3.16e-2 / 1 flip
    of 1800 on one plane, 3.07e-2 / 2 on hi + lo planes."""
    met = run_sequence(VITS, "fp16", {}, _seq(spec, "fp16_patch_planes"))
    _assert_distinct(met)


# ----------------------------------------------------------------------------------------- d: a refresh that re-allocates
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_gemm_rs_ln_off_then_buffer_grows(cuda, precision):
    """gemm_rs_ln 1 R 0 R, then gemm_rs 7 R: the projection and fc2 copies join, the buffer is re-allocated (a new state
    generation), then gemm_rs_ln 1 with no refresh -- nothing may still point into the freed buffer."""
    cfg = VITB
    sd = _weights(cfg)
    frames_np = _frames(2, 240, 31)
    frames = torch.from_numpy(frames_np).cuda()
    cur = dict(_current(), gemm_rs_min_rows=1)
    with dino_amd.options(**cur):
        m = _model(cfg, precision, sd)
        _forward(m, frames)
        _set({"gemm_rs_ln": 0})
        cur["gemm_rs_ln"] = 0
        _refresh(m, sd, "R")
        _forward(m, frames)
        gen = _generation(m)
        _set({"gemm_rs": 7})
        cur["gemm_rs"] = 7
        _refresh(m, sd, "R")
        lp, am = _forward(m, frames)
        assert _generation(m) > gen
        want = dict(cur)
        ref_lp, ref_am = fresh(cfg, precision, frames_np, (2, 240, 31), want)
        assert torch.equal(lp, ref_lp) and torch.equal(am, ref_am)
        _set({"gemm_rs_ln": 1})
        cur["gemm_rs_ln"] = 1
        lp, am = _forward(m, frames)
        ref_lp, ref_am = fresh(cfg, precision, frames_np, (2, 240, 31), want)
        assert torch.equal(lp, ref_lp) and torch.equal(am, ref_am)
        m._release()


# -------------------------------------------------------------------------------------------------------------- e: hi + lo modes
@pytest.mark.parametrize("precision", ["fp16x3", "bf16x3"])
def test_hi_lo_modes_ignore_the_one_plane_options_across_refreshes(cuda, precision):
    """The four options concern one-plane copies only: in the hi + lo modes changing them across two refreshes changes no bit of
    the output and no copy, so the state generation stays put (a captured forward stays valid)."""
    cfg = VITS
    sd = _weights(cfg)
    frames = torch.from_numpy(_frames(2, 240, 31)).cuda()
    with dino_amd.options():
        m = _model(cfg, precision, sd)
        lp0, am0 = _forward(m, frames)
        gen0 = _generation(m)
        for opts in ({"mlp_fused4": 1, "gemm_rs": 7, "gemm_rs_ln": 0, "fp16_patch_planes": 2},
                     {"mlp_fused4": 0, "gemm_rs": 0, "gemm_rs_ln": 1, "fp16_patch_planes": 1}):
            _set(opts)
            _refresh(m, sd, "R")
            lp, am = _forward(m, frames)
            assert torch.equal(lp, lp0) and torch.equal(am, am0), opts
            assert _generation(m) == gen0, opts
        m._release()


# ------------------------------------------------------------------------------------------------ f: a captured predict() graph
@pytest.mark.parametrize("before,after", [({"fp16_patch_planes": 2}, {"fp16_patch_planes": 1}),
                                          ({"mlp_fused": 2, "mlp_fused4": 1}, {"mlp_fused": 2, "mlp_fused4": 0})],
                         ids=["fp16_patch_planes", "mlp_fused4"])
def test_predict_graph_follows_a_refresh_that_moves_the_copies(cuda, before, after):
    """predict() replays its captured graph while dinoseg_state_generation is unchanged.  A refresh under changed options that
    changes the packed copies (fewer patch-embedding planes, no one-wave copies) must change the generation: the map is then the
    eager map of a fresh model and the graph a new one.  A refresh that keeps the copies keeps the graph."""
    cfg = VITS
    sd = _weights(cfg)
    frame = _frames(1, 480, 37)[0]

    def eager(opts):
        with dino_amd.options(**opts):
            ref = _model(cfg, "fp16", sd)
            ref.predict_graph = False
            out = ref.predict(frame)
            ref._release()
        return out

    cur = dict(_current(), **before)
    with dino_amd.options(**cur):
        want0 = eager(cur)
        m = _model(cfg, "fp16", sd)
        a = m.predict(frame)
        graph0 = m._pred_graphs[480]["graph"]
        assert np.array_equal(a, want0)
        assert np.array_equal(m.predict(frame), want0) and m._pred_graphs[480]["graph"] is graph0
        _set(after)
        cur.update(after)
        want1 = eager(cur)
        m.load_state_dict(_tensors(sd))                       # in place: the next call refreshes under the new options
        b = m.predict(frame)
        graph1 = m._pred_graphs[480]["graph"]
        assert graph1 is not graph0
        assert np.array_equal(b, want1)
        m.load_state_dict(_tensors(sd))                       # the same options: the same copies, the same graph
        assert np.array_equal(m.predict(frame), want1) and m._pred_graphs[480]["graph"] is graph1
        m._release()


# ------------------------------------------------------------------------------------------- g: a linear gemm_rs cannot take
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_fc1_wider_than_gemm_rs_runs_layernorm_and_the_regular_gemm(cuda, precision):
    """embed_dim 768 with mlp_ratio 6: fc1 is 4608 wide, beyond gemm_rs.hip's bias table (N * 4 <= 16 KiB).  With the default
    gemm_rs = 3 the forward succeeds, and fc1 runs LayerNorm + the regular GEMM -- bit-identical to gemm_rs = 2, which never
    asks for fc1 -- while qkv stays on gemm_rs.  Against the oracle: fp16 1.35e-2 (gemm_rs 3 and 2), 1.38e-2 (0); bf16 5.88e-2 /
    0.44 % flips (3 and 2), 7.96e-2 / 0.50 % (0)."""
    cfg = VITB_R6
    frames_np = _frames(2, 240, 31)
    cur = dict(_current(), gemm_rs_min_rows=1)
    with dino_amd.options(**cur):
        both = fresh(cfg, precision, frames_np, (2, 240, 31), dict(cur))
        only_qkv = fresh(cfg, precision, frames_np, (2, 240, 31), dict(cur, gemm_rs=2))
        no_rs = fresh(cfg, precision, frames_np, (2, 240, 31), dict(cur, gemm_rs=0))
    assert torch.equal(both[0], only_qkv[0]) and torch.equal(both[1], only_qkv[1])
    assert not torch.equal(both[0], no_rs[0])          # (qkv did run on gemm_rs)
