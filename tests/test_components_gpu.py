"""Connected components on the device: dinoseg_op_components through the C-ABI against the host restatement of the rule
(tests/components_util.py), exactly, with status == 0 everywhere and every output and the scratch between guard bands
(tests/gpu_util.py: Guarded); refusals; DINOSeg.components against the operator called by hand; DINOSeg.discover from planted maps
and end to end against ncut(split=True), the operator and the composition applied by hand."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import ComponentsResult, DiscoverResult, NcutResult, capi
from tests import components_util as CU
from tests import gpu_util as GU
from tests import test_ncut_gpu as T

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
BAND = 4096                             # int16 elements in front of and behind every payload
FILL = 0x5A5A5A5A

# the smallest shapes that exercise every boundary of a 64 x 32 tile: one pixel, one row, one column, a ragged tile, exactly one tile,
# one pixel more along both axes (four tiles), ragged tiles in a 2 x 3 and a 4 x 3 arrangement
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 9), (32, 64), (33, 65), (40, 150), (97, 130)]


class Band:
    """an int32 array of `shape` inside a gpu_util.Guarded buffer of 16-bit guard words (an int32 -1 written into a band does not
    look like a guard word; it would look like a NaN)"""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.g = GU.Guarded(1, 1, 2 * n, torch.int16, band=BAND, exact=True)
        self.t = self.g.out.view(torch.int32).view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return self.g.guards_untouched()


def scratch_bytes(B, H, W):
    n = capi.lib().dinoseg_components_scratch_bytes(B, H, W)
    assert n == (4 * B * H * W + 12 * B * H * ((W + 63) // 64) + 15) // 16 * 16
    return n


def outputs(B, H, W, M, fill=None):
    out = dict(ids=Band((B, H, W), fill), count=Band((B,), fill), first=Band((B, M), fill), label=Band((B, M), fill),
               area=Band((B, M), fill), box=Band((B, M, 4), fill), status=Band((B,), fill))
    out["scratch"] = Band((scratch_bytes(B, H, W) // 4,), fill)
    return out


def call(labels, connectivity, ignore, M, out):
    B, H, W = labels.shape
    return capi.lib().dinoseg_op_components(labels.data_ptr(), B, H, W, connectivity, ignore, M, out["ids"].ptr(), out["count"].ptr(),
                                            out["first"].ptr(), out["label"].ptr(), out["area"].ptr(), out["box"].ptr(),
                                            out["status"].ptr(), out["scratch"].ptr(), S())


def run(labels_np, connectivity, ignore=-1, M=256):
    """the operator between guard bands -> dict of host arrays (status included); the bands are checked here"""
    labels = torch.from_numpy(np.array(labels_np, dtype=np.int32, order="C")).cuda()
    B, H, W = labels.shape
    out = outputs(B, H, W, M)
    capi.check(call(labels, connectivity, ignore, M, out))
    torch.cuda.synchronize()
    for k, v in out.items():
        assert v.intact(), f"{k}: a guard band was written"
    return {k: v.t.cpu().numpy() for k, v in out.items() if k != "scratch"}


def assert_equal(got, want, what):
    assert not got["status"].any(), f"status {what}"
    for k in CU.FIELDS:
        assert np.array_equal(got[k], want[k]), f"{k} {what}"


@functools.lru_cache(maxsize=None)
def maps_of(H, W):
    """(name, map, ignore) of every kind of map of the suite at one shape"""
    seed = 1000 * H + W
    three = CU.random_map(seed + 4, H, W, classes=3, void=0.1)
    maps = [(f"p{p}", CU.random_map(seed + i, H, W, p=p), -1) for i, p in enumerate((0.3, 0.59, 0.7))]
    maps += [("three-ignore1", three, 1), ("three-negatives", three, -1),
             ("one-label", np.full((H, W), 3, dtype=np.int32), -1), ("all-void", np.full((H, W), -2, dtype=np.int32), -1),
             ("all-ignored", np.full((H, W), 4, dtype=np.int32), 4), ("checkerboard", CU.checkerboard(H, W), -1),
             ("rows", CU.stripes(H, W, False), -1), ("columns", CU.stripes(H, W, True), -1), ("serpentine", CU.serpentine(H, W), -1),
             ("serpentine-T", np.ascontiguousarray(CU.serpentine(W, H).T), -1), ("comb", CU.comb(H, W), -1),
             ("corner-main", CU.corner_pair(H, W, True), -1), ("corner-anti", CU.corner_pair(H, W, False), -1)]
    for _, m, _ in maps:
        m.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def host(H, W, i, connectivity, M=256):
    """the restatement of one map (and of its mirror image), computed once"""
    _, m, ignore = maps_of(H, W)[i]
    return CU.components_host(np.stack([m, m[:, ::-1]]), connectivity, ignore, M)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_operator_is_the_restatement(cuda, H, W, connectivity):
    """Every kind of map at one shape and connectivity, as one frame and as the first of three (the second another map, the third its
    own mirror image): ids, count and the table are the restatement's, status is 0, nothing outside the outputs is written."""
    maps = maps_of(H, W)
    for i, (name, m, ignore) in enumerate(maps):
        want = host(H, W, i, connectivity)
        one = run(m[None], connectivity, ignore)
        assert_equal(one, {k: v[:1] for k, v in want.items()}, f"{name} B=1")
        j = (i + 1) % len(maps)
        if maps[j][2] != ignore:                                        # (the neighbour in the list under this map's ignore value)
            other = CU.components_host(maps[j][1][None], connectivity, ignore, 256)
        else:
            other = {k: v[:1] for k, v in host(H, W, j, connectivity).items()}
        three = run(np.stack([m, maps[j][1], m[:, ::-1]]), connectivity, ignore)
        assert_equal(three, {k: np.concatenate([want[k][:1], other[k], want[k][1:]]) for k in CU.FIELDS}, f"{name} B=3")
    # what the maps are for
    names = [n for n, _, _ in maps]
    board, one_label = host(H, W, names.index("checkerboard"), 4), host(H, W, names.index("one-label"), connectivity)
    assert board["count"][0] == H * W and host(H, W, names.index("checkerboard"), 8)["count"][0] == (2 if min(H, W) > 1 else H * W)
    assert one_label["count"][0] == 1 and one_label["area"][0, 0] == H * W and tuple(one_label["box"][0, 0]) == (0, 0, W, H)
    assert host(H, W, names.index("all-void"), connectivity)["count"][0] == 0
    assert host(H, W, names.index("serpentine"), 4)["count"][0] == 1
    if H > 32 and W > 64:
        for n in ("corner-main", "corner-anti"):
            assert host(H, W, names.index(n), 4)["count"][0] == 2 and host(H, W, names.index(n), 8)["count"][0] == 1


@pytest.mark.parametrize("H,W,name", [(33, 65, "p0.59"), (40, 150, "three-negatives"), (97, 130, "checkerboard"), (5, 9, "p0.3")])
def test_ids_and_count_do_not_depend_on_max_objects(cuda, H, W, name):
    maps = maps_of(H, W)
    i = [n for n, _, _ in maps].index(name)
    _, m, ignore = maps[i]
    for connectivity in (4, 8):
        full = host(H, W, i, connectivity)
        count = int(full["count"][0])
        for M in sorted({1, count, max(count - 1, 1), 256}):
            want = CU.components_host(m[None], connectivity, ignore, M)
            assert np.array_equal(want["ids"], full["ids"][:1]) and want["count"][0] == count
            assert_equal(run(m[None], connectivity, ignore, M), want, f"{name} M={M}")


def test_two_runs_are_bit_identical(cuda):
    H, W = 97, 130
    maps = maps_of(H, W)
    stack = np.stack([maps[1][1], maps[4][1], maps[11][1]])
    for connectivity in (4, 8):
        a, b = run(stack, connectivity, -1, 512), run(stack, connectivity, -1, 512)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def camera_case():
    m = CU.random_map(59, 480, 640, p=0.59)
    return m, CU.components_host(m[None], 4, -1, 256)


def test_camera_sized_frame_near_the_percolation_threshold(cuda):
    m, want = camera_case()
    assert_equal(run(m[None], 4, -1, 256), want, "480 x 640 at p = 0.59")


def test_refusals_return_minus_one_without_launching(cuda):
    B, H, W, M = 2, 33, 65, 16
    lib = capi.lib()
    labels = torch.from_numpy(np.stack([CU.random_map(1, H, W, p=0.5), CU.random_map(2, H, W, p=0.5)])).cuda()
    out = outputs(B, H, W, M, fill=FILL)
    good = dict(labels=labels.data_ptr(), B=B, H=H, W=W, connectivity=4, ignore=-1, M=M, **{k: v.ptr() for k, v in out.items()})

    def op(**kw):
        g = dict(good)
        g.update(kw)
        return lib.dinoseg_op_components(g["labels"], g["B"], g["H"], g["W"], g["connectivity"], g["ignore"], g["M"], g["ids"], g["count"],
                                         g["first"], g["label"], g["area"], g["box"], g["status"], g["scratch"], S())

    shapes = [dict(B=0), dict(B=-1), dict(H=0), dict(H=-5), dict(W=0), dict(W=-1), dict(H=8193), dict(W=8193), dict(B=32, H=8192, W=8192),
              dict(B=1 << 30, H=2, W=1)]
    others = [dict(M=0), dict(M=-1), dict(M=(1 << 20) + 1), dict(connectivity=0), dict(connectivity=6), dict(connectivity=-4),
              dict(connectivity=12)]
    nulls = [{k: None} for k in ("labels", "ids", "count", "first", "label", "area", "box", "status", "scratch")]
    skew = [dict(labels=labels.data_ptr() + 2), dict(ids=out["ids"].ptr() + 1), dict(box=out["box"].ptr() + 2),
            dict(scratch=out["scratch"].ptr() + 4), dict(scratch=out["scratch"].ptr() + 8)]
    for kw in shapes + others + nulls + skew:
        assert op(**kw) == -1, kw
        assert "dinoseg_op_components" in capi.last_error(), kw
    for kw in shapes:
        g = dict(good)
        g.update(kw)
        assert lib.dinoseg_components_scratch_bytes(g["B"], g["H"], g["W"]) == -1, kw
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v.t == FILL).all()) and v.intact(), k
    assert op() == 0                                                    # ... and the good call runs
    torch.cuda.synchronize()
    want = CU.components_host(labels.cpu().numpy(), 4, -1, M)
    assert_equal({k: v.t.cpu().numpy() for k, v in out.items()}, want, "after the refusals")
    assert all(v.intact() for v in out.values())
    assert lib.dinoseg_components_scratch_bytes(31, 8192, 8192) == 4 * 31 * (1 << 26) + 12 * 31 * 8192 * 128


# ------------------------------------------------------------------------------------------------ model level
def by_hand(labels_i32, connectivity, ignore, M):
    B, H, W = labels_i32.shape
    out = outputs(B, H, W, M)
    capi.check(call(labels_i32, connectivity, ignore, M, out))
    assert not bool(out["status"].t.any())
    return ComponentsResult(*(out[k].t.clone() for k in CU.FIELDS))


def same(a, b):
    return all(torch.equal(T.bits_of(x), T.bits_of(y)) for x, y in zip(a, b))


def test_components_is_the_operator_by_hand(cuda):
    m = T.model("tiny")
    lab = torch.from_numpy(np.stack([CU.random_map(7, 40, 56, classes=3, void=0.1), CU.random_map(8, 40, 56, classes=3)])).cuda()
    want = by_hand(lab, 8, 2, 64)
    res = m.components(lab, connectivity=8, ignore=2, max_objects=64)
    assert isinstance(res, ComponentsResult) and res.ids.shape == (2, 40, 56) and res.box.shape == (2, 64, 4)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in res)
    assert same(res, want)
    assert same(m.components(lab.to(torch.int64), 8, 2, 64), want)
    assert same(m.components(lab.cpu(), 8, 2, 64), want)                # a host tensor
    pos = lab.clamp(min=0)
    want_u8 = by_hand(pos, 4, -1, 256)
    assert same(m.components(pos.to(torch.uint8)), want_u8)
    assert same(m.components(pos[0].to(torch.uint8)), by_hand(pos[:1].contiguous(), 4, -1, 256))       # [H, W] is one frame
    assert same(m.components(pos == 1, ignore=0), by_hand((pos == 1).to(torch.int32), 4, 0, 256))
    with pytest.raises(ValueError):
        m.components(lab.float())
    with pytest.raises(ValueError):
        m.components(lab, connectivity=6)


def test_components_of_segment_have_one_label_each(cuda):
    m = T.model("tiny")
    x = T.frames_of("tiny", 2, seed=31)
    labels, _ = m.segment(x)
    n = labels.shape[1] * labels.shape[2]
    res = m.components(labels, max_objects=n)
    lab, ids, count = labels.cpu().numpy(), res.ids.cpu().numpy(), res.count.cpu().numpy()
    area, label = res.area.cpu().numpy(), res.label.cpu().numpy()
    for b in range(2):
        assert count[b] >= 1 and (ids[b] >= 0).all()
        for k in range(count[b]):
            assert np.all(lab[b][ids[b] == k] == label[b, k])
        assert area[b].sum() == n and area[b, :count[b]].min() >= 1
    want = CU.components_host(lab, 4, -1, n)
    for k, v in zip(CU.FIELDS, res):
        assert np.array_equal(v.cpu().numpy(), want[k]), k
    # void pixels leave the areas: the areas sum to the non-void pixel count
    res0 = m.components(labels, ignore=int(lab[0, 0, 0]), max_objects=n)
    assert int(res0.area[0].sum()) == int((lab[0] != lab[0, 0, 0]).sum()) and int(res0.ids[0, 0, 0]) == -1


def planted(B=2, hp=9, wp=12):
    """fg with two blobs and a margin of random size with fg's sign"""
    fg = np.zeros((B, hp, wp), dtype=np.uint8)
    fg[:, 1:5, 1:6] = 1
    fg[:, 6:8, 9:11] = 1
    g = np.random.default_rng(17)
    margin = np.where(fg.reshape(B, -1) > 0, 1.0, -1.0).astype(np.float32) * (0.1 + g.random((B, hp * wp)).astype(np.float32))
    return fg.reshape(B, -1), margin


def device_discover(m, margin, fg, seeds, hp, wp, size, connectivity=4):
    out = m._discover_from(torch.from_numpy(margin).cuda(), torch.from_numpy(fg).cuda(), torch.tensor(seeds, dtype=torch.int32).cuda(),
                           hp, wp, size[0], size[1], connectivity)
    return dict(zip(("labels", "box", "found", "cells", "area"), (t.cpu().numpy() for t in out)))


def test_discover_from_planted_maps(cuda):
    m = T.model("tiny")
    hp, wp, p = 9, 12, m.cfg.patch
    fg, margin = planted(2, hp, wp)
    seeds = [6 * wp + 9, 0]                                             # frame 0: inside the smaller blob; frame 1: a background cell
    got = device_discover(m, margin, fg, seeds, hp, wp, (hp, wp))
    want = CU.discover_host(margin, fg, seeds, hp, wp, p)
    for k in ("cells", "box", "found", "area"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["labels"].reshape(2, -1), want["grid_labels"])
    small = np.zeros((hp, wp), dtype=np.uint8)
    small[6:8, 9:11] = 1
    assert np.array_equal(got["cells"][0].reshape(hp, wp), small) and np.array_equal(got["labels"][0], small.astype(np.int32))
    assert tuple(got["box"][0]) == (9 * p, 6 * p, 11 * p, 8 * p) and got["area"][0] == 4 and got["found"][0] == 1
    assert got["found"][1] == 0 and not got["cells"][1].any() and not got["box"][1].any() and got["area"][1] == 0
    assert not got["labels"][1].any()
    # the box is in frame coordinates whatever the output size is
    sized = device_discover(m, margin, fg, seeds, hp, wp, (hp * p + 3, wp * p - 5))
    assert sized["labels"].shape == (2, hp * p + 3, wp * p - 5) and np.array_equal(sized["box"], got["box"])
    # a blob joined only diagonally splits at connectivity 4 and holds at 8
    diag = np.zeros((1, hp, wp), dtype=np.uint8)
    diag[0, 1:3, 1:3] = 1
    diag[0, 3:5, 3:6] = 1
    m2 = np.where(diag.reshape(1, -1) > 0, 0.5, -0.5).astype(np.float32)
    for connectivity, area, box in ((4, 4, (p, p, 3 * p, 3 * p)), (8, 10, (p, p, 6 * p, 5 * p))):
        d = device_discover(m, m2, diag.reshape(1, -1), [wp + 1], hp, wp, (hp, wp), connectivity)
        w = CU.discover_host(m2, diag.reshape(1, -1), [wp + 1], hp, wp, p, connectivity)
        assert d["area"][0] == area and tuple(d["box"][0]) == box
        assert np.array_equal(d["cells"], w["cells"]) and np.array_equal(d["labels"].reshape(1, -1), w["grid_labels"])


@pytest.mark.parametrize("tag", ["tiny", "vits8"])
def test_discover_is_ncut_then_the_seed_component(cuda, tag):
    m = T.model(tag)
    from oracle import dinoseg_oracle as O
    x8 = T.frames_of(tag, 3, seed=905)
    for x in (x8, O.preprocess(x8.cpu().numpy()).cuda()):
        B, H, W = x8.shape[:3]
        p = m.cfg.patch
        hp, wp = H // p, W // p
        n = hp * wp
        cut = m.ncut(x, iters=12, split=True)
        res = m.discover(x, iters=12)
        assert isinstance(res, DiscoverResult) and isinstance(res.ncut, NcutResult) and len(res.ncut) == 7
        assert T.same(res.ncut, cut) and res.ncut.graph is None
        assert res.labels.shape == (B, H, W) and res.labels.dtype == torch.int32 and res.box.shape == (B, 4) and res.cells.shape == (B, n)
        assert res.found.dtype == torch.uint8 and res.cells.dtype == torch.uint8 and res.area.dtype == torch.int32
        # the operator by hand on fg, then the composition on the host
        comp = by_hand(cut.fg.view(B, hp, wp).to(torch.int32), 4, 0, n)
        ids, seeds = comp.ids.view(B, n).cpu().numpy(), cut.seed_cell.cpu().numpy()
        fg = cut.fg.cpu().numpy()
        for b in range(B):
            k = ids[b, seeds[b]]
            assert int(res.found[b]) == fg[b, seeds[b]] == (k >= 0)
            cells = (ids[b] == k) & (k >= 0)
            assert np.array_equal(res.cells[b].cpu().numpy().astype(bool), cells)
            assert int(res.area[b]) == cells.sum()
            if k >= 0:
                assert np.array_equal(res.box[b].cpu().numpy(), comp.box[b, k].cpu().numpy() * p)
                ys, xs = np.nonzero(cells.reshape(hp, wp))
                assert tuple(res.box[b].cpu().numpy()) == (xs.min() * p, ys.min() * p, (xs.max() + 1) * p, (ys.max() + 1) * p)
            else:
                assert not bool(res.box[b].any())
        # the labels at the grid's own size are the cells; at the frame's size they are the enlargement of the pushed margin
        grid = m.discover(x, iters=12, size=(hp, wp))
        assert torch.equal(grid.labels.view(B, n), res.cells.to(torch.int32)) and torch.equal(grid.box, res.box)
        _, margin, _ = m._ncut(x, 0.2, 1e-5, 12, 0, None, 0, 32, False, True)
        pushed = torch.where(res.cells.bool(), margin, -margin.abs())
        assert torch.equal(res.labels, m._margin_labels(pushed, hp, wp, H, W))
        # ncut itself returns what it returned before: the comparison of tests/test_ncut_gpu.py
        assert T.same(m.ncut(x, iters=12, seed=9, eps=1e-4, want_graph=True), T.by_hand(m, x, 0.2, 1e-4, 12, 9, 32, (H, W)))
        assert T.same(m.discover(x, iters=12, split=16, connectivity=8).ncut, cut)
    with pytest.raises(ValueError):
        m.discover(x8, connectivity=6)
