"""The split normalized-cut entries without a device: the symbols, the host-only queries and their refusals, and the plan layer's
``split`` argument (tests/test_ncut_cpu.py covers everything that does not change)."""
import numpy as np
import pytest
import torch

from dino_amd import DINOSeg, capi
from dino_amd.dense_plan import NCUT_MAX_CELLS, NCUT_SPLIT_MAX_CELLS, NcutPlan, ncut_plan
from tests import ncut_util as NC

NAMES = ("dinoseg_ncut_split_max_cells", "dinoseg_ncut_split_graph_bytes", "dinoseg_ncut_split_scratch_bytes",
         "dinoseg_op_ncut_graph_split", "dinoseg_op_ncut_iterate_split")
BAD_SHAPES = ((0, 80), (1, 0), (1, -1), (-1, 80), (1 << 30, 4800))


def frame(hp, wp, B=1):
    return torch.zeros((B, 8 * hp, 8 * wp, 3), dtype=torch.uint8)


def test_symbols_are_declared_bound_and_exported():
    lib, declared = capi.lib(), capi.header_symbols()
    for name in NAMES:
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name), name
    assert len(capi.SIGNATURES["dinoseg_op_ncut_iterate_split"][1]) == 16     # the existing entry's 14, rows_per_group and the scratch
    assert capi.SIGNATURES["dinoseg_op_ncut_graph_split"] == capi.SIGNATURES["dinoseg_op_ncut_graph"]


def test_host_queries():
    lib = capi.lib()
    cells, old = lib.dinoseg_ncut_split_max_cells(), lib.dinoseg_ncut_max_cells()
    assert cells == NCUT_SPLIT_MAX_CELLS and old == NCUT_MAX_CELLS == 10160   # the old limit stays
    assert cells >= 14400 > old                                         # 960 x 960 at patch 8 fits the split entries only
    assert cells == (160 * 1024 - 1024 - 256) // 4                      # one fp32 vector beside the slots and the pad (the header)
    g, s = lib.dinoseg_ncut_split_graph_bytes, lib.dinoseg_ncut_split_scratch_bytes
    for B, n in ((1, 1), (2, 64), (1, 65), (1, 3600), (32, 4800), (1, 10201), (1, 14400), (3, cells)):
        assert g(B, n) == 8 * B * n * NC.words_of(n), (B, n)
        assert s(B, n) == 24 * B * n, (B, n)                            # six fp32 vectors per frame: O(B n), nothing with n^2
        if n <= old:
            assert g(B, n) == lib.dinoseg_ncut_graph_bytes(B, n)
    for bad in BAD_SHAPES + ((1, cells + 1),):
        assert g(*bad) == -1 and s(*bad) == -1, bad
    assert lib.dinoseg_ncut_graph_bytes(1, old + 1) == -1               # the old query still refuses what it refused


def test_plan_accepts_split_and_refuses_what_it_must():
    assert NcutPlan._fields[-1] == "split"
    small = frame(5, 7, B=3)
    assert ncut_plan(8, small).split == 0 and ncut_plan(8, small, split=False).split == 0
    assert ncut_plan(8, small, split=True).split == -1 and ncut_plan(8, small, split=np.bool_(True)).split == -1
    assert ncut_plan(8, small, split=16).split == 16 and ncut_plan(8, small, split=np.int64(1)).split == 1
    assert ncut_plan(8, small, split=1 << 40).split >= 35               # more rows than the frame has: one row workgroup
    assert ncut_plan(8, small)[:-1] == ncut_plan(8, small, split=7)[:-1]
    for hp, wp in ((101, 101), (120, 120)):
        p = ncut_plan(8, frame(hp, wp), split=True)
        assert (p.hp, p.wp, p.split) == (hp, wp, -1)
        assert ncut_plan(8, frame(hp, wp), split=32).split == 32
        with pytest.raises(ValueError, match=str(NCUT_MAX_CELLS)):      # without split these grids still raise, with the old message
            ncut_plan(8, frame(hp, wp))
        with pytest.raises(ValueError):
            ncut_plan(8, frame(hp, wp), split=False)
    assert 160 * 254 == NCUT_SPLIT_MAX_CELLS
    assert ncut_plan(8, frame(160, 254), split=True).wp == 254          # the largest grid
    with pytest.raises(ValueError, match=f"{NCUT_SPLIT_MAX_CELLS}.*NCUT_SPLIT_MAX_CELLS"):
        ncut_plan(8, frame(202, 202), split=True)                       # 40 804 cells
    for bad in (-1, 0, 1.5, "yes", None, 2.0, [16], -7):
        with pytest.raises(ValueError, match="split"):
            ncut_plan(8, small, split=bad)
        with pytest.raises(ValueError, match="split"):
            ncut_plan(8, frame(101, 101), split=bad)


def test_a_cpu_model_reaches_no_cpu_path_only_after_every_value_error():
    m = DINOSeg(head="linear", n_blocks=1)
    x = frame(5, 7, B=3)
    for kw in (dict(split=-1), dict(split=1.5), dict(split="yes"), dict(split=True, tau=1.0), dict(split=True, iters=-1),
               dict(split=True, n_blocks=2), dict(split=4, size=(4, 56)), dict(split=True, x=frame(202, 202)), dict(x=frame(101, 101))):
        args = dict(x=x)
        args.update(kw)
        with pytest.raises(ValueError):
            m.ncut(**args)
    for kw in (dict(split=True), dict(split=16), dict(split=True, x=frame(101, 101))):
        args = dict(x=x)
        args.update(kw)
        with pytest.raises(capi.DinosegError, match="no CPU path"):
            m.ncut(**args)
