"""The class DEFAULT (`precision="auto"`: inference runs fp16x3 -- what `DINOSeg.load_from_checkpoint(path).predict / forward_frames` give a
user, pl_torch_modules.py:276-300) at the BASELINE.json batch shapes, against the fixtures captured from the reference (-m gpu).

`bench.py --full` prints the same comparison as `parity_mode.parity`; here it is asserted: |dlogp| <= 3e-4 (the north-star bar is 1e-3), argmax
identical to the reference (a tie of the reference itself excepted at 14 400 patches, as tests/test_fp16_gpu.py), and every copy of the
frame in the batch bit-identical -- the batch goes through the large-batch dispatch (fused projection + MLP launch on hi + lo planes,
persistent GEMMs, assembly attention, two streams) that a single frame never sees."""
import numpy as np
import pytest
import torch

from dino_amd import ViTConfig
from dino_amd.weights import VIT_B8, synthetic_frames
from tests.test_model_gpu import build, load

pytestmark = pytest.mark.gpu


def _batch_of_copies(m, g, n, res, patches):
    one = synthetic_frames(1, res, seed=int(g["frame_seed"]))
    if res != 480:
        m.set_resolution(res)
    lp, am = m.forward_frames(torch.from_numpy(np.repeat(one, n, axis=0)).cuda())
    lp = lp.cpu().reshape(n, patches, -1)
    am = am.cpu().long().reshape(n, patches)
    assert torch.isfinite(lp).all()
    assert float((lp - lp[0:1]).abs().max()) == 0.0 and bool((am == am[0:1]).all())      # frames are independent: every copy alike
    return lp[0], am[0]


def test_default_mode_32_frames_480(cuda, golden_dir):
    """BASELINE configs[1]'s shape: 32 copies of the G3 L=12 frame."""
    g = load(golden_dir, "g3_vits8_L12_r480")
    m, _, _ = build(12, "auto")
    assert m.precision == "auto"
    lp, am = _batch_of_copies(m, g, 32, 480, 3600)
    err = float((lp - torch.from_numpy(g["logp"])).abs().max())
    print(f"auto, 32 x 480: max|dlogp| {err:.3e}")
    assert err <= 3e-4
    assert torch.equal(am, torch.from_numpy(g["argmax"].astype(np.int64)))


def test_default_mode_vitb_16_frames(cuda, golden_dir):
    """BASELINE configs[4]'s per-GPU shape: 16 copies of the G7 ViT-B/8 frame (fixture: 256 sampled rows)."""
    g = load(golden_dir, "g7_vitb8_L12_r480")
    m, _, _ = build(ViTConfig(embed_dim=VIT_B8.embed_dim, num_heads=VIT_B8.num_heads, n_blocks=12), "auto")
    lp, am = _batch_of_copies(m, g, 16, 480, 3600)
    rows = torch.from_numpy(g["rows"])
    err = float((lp[rows] - torch.from_numpy(g["logp_rows"])).abs().max())
    print(f"auto, ViT-B/8 16 x 480: max|dlogp| {err:.3e}")
    assert err <= 3e-4
    assert torch.equal(am[rows], torch.from_numpy(g["logp_rows"]).argmax(1))


def test_default_mode_8_frames_960(cuda, golden_dir):
    """BASELINE configs[2]'s shape: 8 copies of the G4 L=12 frame at 960 x 960 (14 401 tokens)."""
    g = load(golden_dir, "g4_vits8_L12_r960")
    m, _, _ = build(12, "auto")
    lp, am = _batch_of_copies(m, g, 8, 960, 14400)
    rows = torch.from_numpy(g["rows"])
    err = float((lp[rows] - torch.from_numpy(g["logp_rows"])).abs().max())
    differ = am.numpy() != g["argmax"].astype(np.int64)
    print(f"auto, 8 x 960: max|dlogp| {err:.3e}, flips {int(differ.sum())} / 14400, reference margins there {g['margin'][differ]}")
    # a patch whose two best classes differ by less than the reference's own fp32 rounding noise has no defined winner (test_fp16_gpu.py)
    assert err <= 3e-4 and np.all(g["margin"][differ] <= 6e-5) and int(differ.sum()) <= 2
