"""Multi-object discovery on the device: dinoseg_op_ncut_mask and dinoseg_op_maskcut_select against the integer restatement
(tests/maskcut_util.py), dinoseg_op_maskcut against the operators applied by hand (teacher forcing on the device's own state: the cut
itself is held to fp64 by tests/test_ncut_gpu.py), DINOSeg.discover_all against discover and against the entry by hand, the planted
grids whose expectation tests/test_maskcut_cpu.py establishes, guard bands and refusals.  Everything is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from dino_amd import MaskCutResult, capi, ncut_start
from tests import maskcut_util as MC
from tests import ncut_util as NC
from tests import test_ncut_gpu as T
from tests import test_ncut_split_gpu as SP

pytestmark = pytest.mark.gpu
S = capi.stream_ptr
EPS = 1e-5
GRIDS = [(1, 1), (1, 3), (5, 7), (8, 8), (5, 13), (9, 11), (20, 24), (60, 80)]
SHAPES = [(B, hp, wp) for hp, wp in GRIDS for B in (1, 3) if not (B == 3 and hp == 60)]
ROUND_KEYS = ("cells", "found", "area", "box", "fg", "margin", "eigvec", "seed_cell", "rho")
ALL_KEYS = ROUND_KEYS + ("score", "count")


def sid(s):
    return "x".join(str(v) for v in s)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def graph_of(B, hp, wp, kind):
    """(graph int64 [B, n, W], degree int32 [B, n]) of seeded tokens through dinoseg_op_ncut_graph_split; never written: callers clone"""
    n, D, seed = hp * wp, 64, 1300 + 7 * hp + wp + (kind == "planted")
    tok = NC.normal_tokens(seed, B, n, D) if kind == "normal" else NC.planted_tokens(seed, B, n, D)[0]
    return SP.split_graph(T.normalize(dev(tok)), 0.2)


def alive_dev(alive):
    """bool [B, n] -> the words int64 [B, W] on the device"""
    return dev(np.stack([MC.pack_alive(a) for a in alive]).view(np.int64))


def alive_host(words, n):
    return np.stack([MC.unpack_alive(w, n)[0] for w in words.cpu().numpy().view(np.uint64)])


def op_mask(graph, degree, alive):
    B, n = degree.shape
    capi.check(capi.lib().dinoseg_op_ncut_mask(graph.data_ptr(), degree.data_ptr(), alive.data_ptr(), B, n, S()))


def op_ids(cand, connectivity=4):
    """cand int32 [B, hp, wp] -> ids int32 [B, hp, wp] of dinoseg_op_components with ignore = 0 and a one-row table"""
    B, hp, wp = cand.shape
    lib = capi.lib()
    scratch = torch.empty((lib.dinoseg_components_scratch_bytes(B, hp, wp),), dtype=torch.uint8, device="cuda")
    ids = torch.empty((B, hp, wp), dtype=torch.int32, device="cuda")
    small = [torch.empty((B, k), dtype=torch.int32, device="cuda") for k in (1, 1, 1, 1, 1, 4)]
    capi.check(lib.dinoseg_op_components(cand.data_ptr(), B, hp, wp, connectivity, 0, 1, ids.data_ptr(), small[0].data_ptr(),
                                         small[1].data_ptr(), small[2].data_ptr(), small[3].data_ptr(), small[5].data_ptr(),
                                         small[4].data_ptr(), scratch.data_ptr(), S()))
    return ids


def round_outputs(B, n, K, iters, fill=None):
    spec = dict(cells=((B, K, n), torch.uint8), found=((B, K), torch.uint8), area=((B, K), torch.int32), box=((B, K, 4), torch.int32),
                score=((B, n, K + 1), torch.float32), count=((B,), torch.int32), fg=((B, K, n), torch.uint8),
                margin=((B, K, n), torch.float32), eigvec=((B, K, n), torch.float32), seed_cell=((B, K), torch.int32),
                rho=((B, K, iters), torch.float32))
    if fill is None:
        return {k: torch.empty(s, dtype=dt, device="cuda") for k, (s, dt) in spec.items()}
    return {k: torch.full(s, fill, dtype=dt, device="cuda") for k, (s, dt) in spec.items()}


def op_select(ids, fg, margin, seed, alive, hp, wp, K, t, out):
    B = fg.shape[0]
    return capi.lib().dinoseg_op_maskcut_select(ids.data_ptr(), fg.data_ptr(), margin.data_ptr(), seed.data_ptr(), alive.data_ptr(), B, hp,
                                                wp, K, t, out["cells"].data_ptr(), out["found"].data_ptr(), out["area"].data_ptr(),
                                                out["box"].data_ptr(), out["score"].data_ptr(), S())


def scratch_for(B, hp, wp, K):
    nbytes = capi.lib().dinoseg_maskcut_scratch_bytes(B, hp, wp, K)
    assert nbytes > 0
    return torch.empty((nbytes,), dtype=torch.uint8, device="cuda")


def op_maskcut(graph, degree, hp, wp, z, iters, K, rows=0, connectivity=4, eps=EPS, out=None, scratch=None):
    """the entry on the caller's graph and degree (destroyed) -> the outputs"""
    B, n = degree.shape
    out = out or round_outputs(B, n, K, iters)
    scratch = scratch_for(B, hp, wp, K) if scratch is None else scratch
    capi.check(capi.lib().dinoseg_op_maskcut(
        graph.data_ptr(), degree.data_ptr(), B, hp, wp, float(eps), z.data_ptr(), iters, rows, connectivity, K, out["cells"].data_ptr(),
        out["found"].data_ptr(), out["area"].data_ptr(), out["box"].data_ptr(), out["score"].data_ptr(), out["count"].data_ptr(),
        out["fg"].data_ptr(), out["margin"].data_ptr(), out["eigvec"].data_ptr(), out["seed_cell"].data_ptr(),
        out["rho"].data_ptr() if iters else None, scratch.data_ptr(), S()))
    return out


def by_hand(graph, degree, hp, wp, z, iters, K, connectivity=4, eps=EPS):
    """The rule through the operators, one at a time: mask, dinoseg_op_ncut_iterate_split, the candidates (torch), dinoseg_op_components,
    select -> the entry's outputs (graph and degree are destroyed as the entry destroys them)"""
    B, n = degree.shape
    out = round_outputs(B, n, K, iters)
    out["score"][:, :, 0] = 0.0
    alive = alive_dev(np.ones((B, n), dtype=bool))
    z_before = z.clone()
    for t in range(K):
        op_mask(graph, degree, alive)
        cut = SP.split_iterate(graph, degree, z, iters, eps=eps)
        on = dev(alive_host(alive, n))
        cand = ((cut["fg"] != 0) & on).to(torch.int32).view(B, hp, wp).contiguous()
        ids = op_ids(cand, connectivity)
        capi.check(op_select(ids, cut["fg"], cut["margin"], cut["seed_cell"], alive, hp, wp, K, t, out))
        for k in ("fg", "margin", "eigvec", "seed_cell", "rho"):
            out[k][:, t] = cut[k]
    out["count"] = out["found"].to(torch.int32).sum(1).to(torch.int32)
    assert torch.equal(z, z_before)
    return out


def assert_same(got, want, what="", keys=ALL_KEYS):
    for k in keys:
        assert torch.equal(T.bits_of(got[k]), T.bits_of(want[k])), f"{k} {what}"


# ------------------------------------------------------------------------------------------------ 1. the mask alone
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_mask_is_the_restatement(cuda, shape):
    """Graphs of normal and planted rows under five alive patterns: graph, degree and pad bits equal the restatement's, symmetry is
    kept, masking twice is masking once, and masking with a subset after a superset is masking the original with the subset."""
    B, hp, wp = shape
    n = hp * wp
    g = np.random.default_rng(1400 + n)
    half = g.random((B, n)) < 0.5
    patterns = dict(all=np.ones((B, n), bool), none=np.zeros((B, n), bool), half=half, last=np.tile(np.arange(n) == n - 1, (B, 1)),
                    but_one=np.tile(np.arange(n) != n // 2, (B, 1)))
    for kind in ("normal", "planted"):
        graph0, degree0 = graph_of(B, hp, wp, kind)
        words0 = graph0.cpu().numpy().view(np.uint64)
        for name, alive in patterns.items():
            graph, degree, al = graph0.clone(), degree0.clone(), alive_dev(alive)
            op_mask(graph, degree, al)
            got = graph.cpu().numpy().view(np.uint64)
            for b in range(B):
                want_w, want_d = MC.mask_host(words0[b], MC.pack_alive(alive[b]))
                assert np.array_equal(got[b], want_w) and np.array_equal(degree[b].cpu().numpy(), want_d), (kind, name, b)
                bits, pad = NC.unpack_words(got[b], n)
                assert not pad.any() and np.array_equal(bits, bits.T), (kind, name, b)
            once_g, once_d = graph.clone(), degree.clone()
            op_mask(graph, degree, al)
            assert torch.equal(graph, once_g) and torch.equal(degree, once_d), (kind, name)
            assert torch.equal(al, alive_dev(alive))
        sub = half & (g.random((B, n)) < 0.5)
        g1, d1, g2, d2 = graph0.clone(), degree0.clone(), graph0.clone(), degree0.clone()
        op_mask(g1, d1, alive_dev(half))
        op_mask(g1, d1, alive_dev(sub))
        op_mask(g2, d2, alive_dev(sub))
        assert torch.equal(g1, g2) and torch.equal(d1, d2), kind


# ------------------------------------------------------------------------------------------------ 2. the select alone
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_select_is_the_restatement(cuda, shape):
    """ids of dinoseg_op_components on random candidate maps, random margins (with +0, -0 and an infinity among them), seeds on a
    candidate cell, on a background cell and on a dead cell; K in {1, 3, 16}, t = 0 and K - 1, both connectivities: cells, found, area,
    box, the new alive and the round's score channel bit for bit; every other round's slot and every other channel keeps its fill."""
    B, hp, wp = shape
    n = hp * wp
    g = np.random.default_rng(1500 + n)
    fg = (g.random((B, n)) < 0.6).astype(np.uint8)
    alive = g.random((B, n)) < 0.8
    margin = g.standard_normal((B, n)).astype(np.float32)
    margin[:, ::5] = 0.0
    margin[:, 1::7] = -0.0
    margin[:, n // 2] = np.inf
    cand = np.stack([MC.candidates_host(fg[b], alive[b]) for b in range(B)])
    kinds = dict(candidate=cand == 1, background=(fg == 0) & alive, dead=~alive)

    def seed_of(b, kind):
        at = np.nonzero(kinds[kind][b])[0]
        return int(at[len(at) // 2]) if len(at) else b % n              # (no cell of that kind in the frame: any cell)

    FILL = 0x5B
    for connectivity in (4, 8):
        ids = op_ids(dev(cand.reshape(B, hp, wp)), connectivity)
        ids_h = ids.cpu().numpy().reshape(B, n)
        for shift, (K, t) in enumerate([(1, 0), (3, 0), (3, 2), (16, 0), (16, 15)]):
            order = list(kinds)
            seeds = np.array([seed_of(b, order[(b + shift) % 3]) for b in range(B)], dtype=np.int32)
            out = round_outputs(B, n, K, 1, fill=FILL)
            before = {k: v.clone() for k, v in out.items()}
            al = alive_dev(alive)
            capi.check(op_select(ids, dev(fg), dev(margin), dev(seeds), al, hp, wp, K, t, out))
            new_alive = alive_host(al, n)
            assert not MC.unpack_alive(al[0].cpu().numpy().view(np.uint64), n)[1].any()
            for b in range(B):
                w = MC.select_host(ids_h[b], fg[b], margin[b], seeds[b], alive[b], hp, wp)
                what = (connectivity, K, t, b)
                assert int(out["found"][b, t]) == w["found"] and int(out["area"][b, t]) == w["area"], what
                assert np.array_equal(out["cells"][b, t].cpu().numpy().astype(bool), w["cells"]), what
                assert np.array_equal(out["box"][b, t].cpu().numpy(), w["box"]), what
                assert np.array_equal(new_alive[b], w["alive"]), what
                assert np.array_equal(out["score"][b, :, t + 1].cpu().numpy().view(np.uint32), w["score"]), what
            for k in ("cells", "found", "area", "box"):
                keep = [s for s in range(K) if s != t]
                assert torch.equal(out[k][:, keep], before[k][:, keep]), k
            keep = [c for c in range(K + 1) if c != t + 1]
            assert torch.equal(T.bits_of(out["score"][:, :, keep].contiguous()), T.bits_of(before["score"][:, :, keep].contiguous()))


# ------------------------------------------------------------------------------------------------ 3. the entry
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_entry_is_the_operators_by_hand(cuda, shape):
    """K = 3 rounds: every per-round output, the score, the count and the graph and degree the rounds leave behind equal the operators
    applied by hand, bit for bit; two runs are bit-identical; rows_per_group in {0, 7, n} gives the same bits."""
    B, hp, wp = shape
    n, K, iters = hp * wp, 3, 5
    z = T.start_for(B, n)
    for kind in ("normal", "planted"):
        graph0, degree0 = graph_of(B, hp, wp, kind)
        gh, dh = graph0.clone(), degree0.clone()
        want = by_hand(gh, dh, hp, wp, z, iters, K)
        for rows in (0, 0, 7, n):
            g, d = graph0.clone(), degree0.clone()
            got = op_maskcut(g, d, hp, wp, z, iters, K, rows)
            assert_same(got, want, f"{kind} rows {rows}")
            assert torch.equal(g, gh) and torch.equal(d, dh), (kind, rows)
        assert torch.equal(z, T.start_for(B, n))
    g, d = graph_of(B, hp, wp, "planted")
    g8, d8 = g.clone(), d.clone()
    assert_same(op_maskcut(g8, d8, hp, wp, z, 0, 2, 0, 8), by_hand(g.clone(), d.clone(), hp, wp, z, 0, 2, 8), "connectivity 8, no passes")


def test_a_round_that_finds_nothing_repeats_bit_for_bit(cuda):
    """One cell: nothing is left after the deflation, the seed is background in every round.  A planted two-rectangle grid with K = 5:
    from the first not-found round on every output of a round equals the previous round's."""
    z = T.start_for(1, 1)
    g, d = graph_of(1, 1, 1, "normal")
    out = op_maskcut(g.clone(), d.clone(), 1, 1, z, 4, 3)
    assert not bool(out["found"].any()) and int(out["count"][0]) == 0 and not bool(out["cells"].any()) and not bool(out["box"].any())
    hp, wp, D, rects = MC.PLANTED[0]
    n, K = hp * wp, 5
    graph, degree = SP.split_graph(T.normalize(dev(MC.planted_rect_tokens(1201, hp, wp, D, rects)[None])), 0.2)
    out = op_maskcut(graph, degree, hp, wp, ncut_start(n, 0).cuda().view(1, n).contiguous(), 64, K)
    found = out["found"][0].cpu().numpy()
    first = int(np.argmin(found))
    assert found[first] == 0 and first < K - 1 and not found[first:].any() and int(out["count"][0]) == found.sum()
    for t in range(first + 1, K):
        for k in ROUND_KEYS:
            assert torch.equal(T.bits_of(out[k][:, t].contiguous()), T.bits_of(out[k][:, first].contiguous())), (k, t)
        assert torch.equal(T.bits_of(out["score"][:, :, t + 1].contiguous()), T.bits_of(out["score"][:, :, first + 1].contiguous()))


# ------------------------------------------------------------------------------------------------ 4. planted grids
@pytest.mark.parametrize("case", MC.PLANTED, ids=lambda c: f"{c[0]}x{c[1]}")
def test_planted_rectangles_are_found_as_sets(cuda, case):
    """The expectation of tests/test_maskcut_cpu.py on the device, through the operators from planted tokens (64 passes, start seeds 0
    and 1, two token seeds): the found objects are the rectangles as sets, pairwise disjoint, count == G, and the labels at the grid's
    own size equal the object map at every cell (up to the order of the rounds)."""
    hp, wp, D, rects = case
    n, G = hp * wp, len(rects)
    K = G + 1
    sets, _ = MC.rect_cells(hp, wp, rects)
    for ts in (1201, 1202):
        planes = T.normalize(dev(MC.planted_rect_tokens(ts, hp, wp, D, rects)[None]))
        for ss in (0, 1):
            graph, degree = SP.split_graph(planes, 0.2)
            out = op_maskcut(graph, degree, hp, wp, ncut_start(n, ss).cuda().view(1, n).contiguous(), 64, K)
            cells, found = out["cells"][0].cpu().numpy().astype(bool), out["found"][0].cpu().numpy()
            assert int(out["count"][0]) == G and list(found) == [1] * G + [0], (ts, ss)
            assert MC.found_sets(cells, found) == MC.rect_sets(hp, wp, rects), (ts, ss)
            assert cells.sum(0).max() == 1 and np.array_equal(out["area"][0].cpu().numpy(), cells.sum(1))
            labels = torch.empty((1, hp, wp), dtype=torch.int32, device="cuda")
            capi.check(capi.lib().dinoseg_op_upsample_argmax(out["score"].data_ptr(), 1, hp, wp, K + 1, hp, wp, labels.data_ptr(), None, S()))
            grid = labels.cpu().numpy().reshape(n)
            for t in range(G):
                assert np.array_equal(grid == t + 1, cells[t]), (ts, ss, t)
                ys, xs = np.nonzero(cells[t].reshape(hp, wp))
                assert tuple(out["box"][0, t].cpu().numpy()) == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
            assert np.array_equal(grid == 0, ~sets.any(0))


# ------------------------------------------------------------------------------------------------ 5. guard bands
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 5, 13), (1, 60, 80)], ids=sid)
def test_outputs_graph_and_scratch_stay_between_their_guard_bands(cuda, shape):
    B, hp, wp = shape
    n, W, K, iters = hp * wp, NC.words_of(hp * wp), 3, 3
    graph0, degree0 = graph_of(B, hp, wp, "normal")
    graph = T.Guarded(B * n * W * 8, torch.int64, (B, n, W))
    degree = T.Guarded(B * n * 4, torch.int32, (B, n))
    graph.view.copy_(graph0)
    degree.view.copy_(degree0)
    plain = round_outputs(B, n, K, iters)
    g = {k: T.Guarded(v.numel() * v.element_size(), v.dtype, tuple(v.shape)) for k, v in plain.items()}
    nbytes = capi.lib().dinoseg_maskcut_scratch_bytes(B, hp, wp, K)
    scratch = T.Guarded(nbytes, torch.uint8, (nbytes,))
    z = T.start_for(B, n)
    op_maskcut(graph.view, degree.view, hp, wp, z, iters, K, 5, out={k: v.view for k, v in g.items()}, scratch=scratch.view)
    torch.cuda.synchronize()
    for k, v in list(g.items()) + [("graph", graph), ("degree", degree), ("scratch", scratch)]:
        assert v.bands_intact(), k
    assert_same({k: v.view for k, v in g.items()}, op_maskcut(graph0.clone(), degree0.clone(), hp, wp, z, iters, K, 5))
    # the two operators on their own
    al = T.Guarded(B * W * 8, torch.int64, (B, W))
    al.view.copy_(alive_dev(np.random.default_rng(3).random((B, n)) < 0.5))
    graph.view.copy_(graph0)
    op_mask(graph.view, degree.view, al.view)
    ids = op_ids((g["fg"].view[:, 0] != 0).to(torch.int32).view(B, hp, wp).contiguous())
    capi.check(op_select(ids, g["fg"].view[:, 0].contiguous(), g["margin"].view[:, 0].contiguous(), g["seed_cell"].view[:, 0].contiguous(),
                         al.view, hp, wp, K, 1, {k: v.view for k, v in g.items()}))
    torch.cuda.synchronize()
    for k, v in list(g.items()) + [("graph", graph), ("degree", degree), ("alive", al)]:
        assert v.bands_intact(), k


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_return_minus_one_without_launching(cuda):
    B, hp, wp, K, iters = 2, 5, 7, 3, 2
    n, W = hp * wp, 1
    lib = capi.lib()
    cells = lib.dinoseg_ncut_split_max_cells()
    graph = torch.full((B, n, W + 1), -7, dtype=torch.int64, device="cuda")
    degree = torch.full((B, n), -7, dtype=torch.int32, device="cuda")
    alive = torch.full((B * W + 2,), -1, dtype=torch.int64, device="cuda")
    z = T.start_for(B, n)
    out = round_outputs(B, n, K, iters, fill=9)
    nbytes = lib.dinoseg_maskcut_scratch_bytes(B, hp, wp, K)
    scratch = torch.full((nbytes + 16,), 9, dtype=torch.uint8, device="cuda")
    ids = torch.zeros((B, n), dtype=torch.int32, device="cuda")
    fg = torch.ones((B, n), dtype=torch.uint8, device="cuda")
    margin = torch.ones((B, n), dtype=torch.float32, device="cuda")
    seed = torch.zeros((B,), dtype=torch.int32, device="cuda")
    P = {k: v.data_ptr() for k, v in out.items()}
    good = dict(graph=graph.data_ptr(), degree=degree.data_ptr(), alive=alive.data_ptr(), B=B, hp=hp, wp=wp, n=n, eps=EPS, z=z.data_ptr(),
                iters=iters, rows=0, conn=4, K=K, t=0, scratch=scratch.data_ptr(), ids=ids.data_ptr(), fg_in=fg.data_ptr(),
                margin_in=margin.data_ptr(), seed_in=seed.data_ptr(), **P)

    def mask(**kw):
        a = dict(good)
        a.update(kw)
        return lib.dinoseg_op_ncut_mask(a["graph"], a["degree"], a["alive"], a["B"], a["n"], S())

    def select(**kw):
        a = dict(good)
        a.update(kw)
        return lib.dinoseg_op_maskcut_select(a["ids"], a["fg_in"], a["margin_in"], a["seed_in"], a["alive"], a["B"], a["hp"], a["wp"], a["K"],
                                             a["t"], a["cells"], a["found"], a["area"], a["box"], a["score"], S())

    def entry(**kw):
        a = dict(good)
        a.update(kw)
        return lib.dinoseg_op_maskcut(a["graph"], a["degree"], a["B"], a["hp"], a["wp"], a["eps"], a["z"], a["iters"], a["rows"], a["conn"],
                                      a["K"], a["cells"], a["found"], a["area"], a["box"], a["score"], a["count"], a["fg"], a["margin"],
                                      a["eigvec"], a["seed_cell"], a["rho"], a["scratch"], S())

    def untouched():
        torch.cuda.synchronize()
        return (all(bool((v == 9).all()) for v in out.values()) and bool((scratch == 9).all()) and bool((graph == -7).all())
                and bool((degree == -7).all()) and bool((alive == -1).all()))

    for kw in [dict(graph=None), dict(degree=None), dict(alive=None), dict(graph=graph.data_ptr() + 4), dict(alive=alive.data_ptr() + 4),
               dict(degree=degree.data_ptr() + 2), dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(n=cells + 1), dict(B=1 << 30, n=4800)]:
        assert mask(**kw) == -1, kw
        assert "dinoseg_op_ncut_mask" in capi.last_error(), kw
    assert untouched()
    grids = [dict(B=0), dict(B=-1), dict(hp=0), dict(wp=0), dict(hp=-2), dict(hp=8193, wp=1), dict(hp=1, wp=8193), dict(B=1 << 30, hp=60, wp=80)]
    for kw in [dict(ids=None), dict(fg_in=None), dict(margin_in=None), dict(seed_in=None), dict(alive=None), dict(cells=None), dict(found=None),
               dict(area=None), dict(box=None), dict(score=None), dict(ids=ids.data_ptr() + 2), dict(margin_in=margin.data_ptr() + 2),
               dict(seed_in=seed.data_ptr() + 1), dict(alive=alive.data_ptr() + 4), dict(area=P["area"] + 2), dict(box=P["box"] + 1),
               dict(score=P["score"] + 2), dict(K=0), dict(K=17), dict(K=-1), dict(t=-1), dict(t=K), dict(K=1, t=1)] + grids:
        assert select(**kw) == -1, kw
        assert "dinoseg_op_maskcut_select" in capi.last_error(), kw
    assert untouched()
    for kw in [dict(graph=None), dict(degree=None), dict(z=None), dict(cells=None), dict(found=None), dict(area=None), dict(box=None),
               dict(score=None), dict(count=None), dict(fg=None), dict(margin=None), dict(eigvec=None), dict(seed_cell=None), dict(rho=None),
               dict(scratch=None), dict(graph=graph.data_ptr() + 4), dict(degree=degree.data_ptr() + 2), dict(z=z.data_ptr() + 2),
               dict(area=P["area"] + 2), dict(box=P["box"] + 1), dict(score=P["score"] + 2), dict(count=P["count"] + 2),
               dict(margin=P["margin"] + 2), dict(eigvec=P["eigvec"] + 1), dict(seed_cell=P["seed_cell"] + 2), dict(rho=P["rho"] + 1),
               dict(scratch=scratch.data_ptr() + 4), dict(scratch=scratch.data_ptr() + 8), dict(eps=-1e-9), dict(eps=1.0),
               dict(eps=float("nan")), dict(iters=-1), dict(iters=4097), dict(rows=-1), dict(conn=0), dict(conn=6), dict(conn=-4),
               dict(K=0), dict(K=17), dict(K=-1), dict(hp=202, wp=202), dict(B=1 << 26, hp=8, wp=8, rows=1)] + grids:
        assert entry(**kw) == -1, kw
        assert "dinoseg_op_maskcut" in capi.last_error() and "dinoseg_op_maskcut_select" not in capi.last_error(), kw
    assert untouched()
    q = lib.dinoseg_maskcut_scratch_bytes
    for bad in ((0, 5, 7, 3), (-1, 5, 7, 3), (1, 0, 7, 3), (1, 5, 0, 3), (1, 8193, 1, 3), (1, 202, 202, 3), (1 << 30, 60, 80, 3), (1, 5, 7, 0),
                (1, 5, 7, 17)):
        assert q(*bad) == -1, bad
    # ... and the good calls run inside their rows
    planes = T.normalize(torch.randn((B, n + 1, 64), device="cuda"))
    capi.check(lib.dinoseg_op_ncut_graph_split(planes.data_ptr(), B, n, 64, 0.2, graph.data_ptr(), degree.data_ptr(), S()))
    assert entry() == 0 and entry(rows=1 << 30) == 0
    torch.cuda.synchronize()
    assert not any(bool((v == 9).all()) for v in out.values())
    assert bool((scratch[nbytes:] == 9).all()) and bool((graph.view(-1)[B * n * W:] == -7).all())
    assert mask() == 0 and select() == 0 and entry(iters=0, rho=None) == 0
    torch.cuda.synchronize()
    assert bool((alive[B * W:] == -1).all()) and not bool((alive[:B * W] == -1).any())


# ------------------------------------------------------------------------------------------------ 7. model level
def frames_both(tag, B, seed):
    from oracle import dinoseg_oracle as O
    x8 = T.frames_of(tag, B, seed=seed)
    return x8, O.preprocess(x8.cpu().numpy()).cuda()


def model_by_hand(m, x, K, tau, eps, iters, seed, chunk, size, connectivity=4):
    """discover_all through features(), the graph launch, the entry and the enlargement by hand -> (MaskCutResult, the entry's outputs)"""
    p = m.cfg.patch
    B = x.shape[0]
    H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])
    hp, wp = H // p, W // p
    n = hp * wp
    planes = T.normalize(torch.cat([m.features(x[c:c + chunk]) for c in range(0, B, chunk)]))
    graph, degree = SP.split_graph(planes, float(np.float32(tau)))
    original = graph.clone()
    out = op_maskcut(graph, degree, hp, wp, ncut_start(n, seed).cuda().expand(B, n).contiguous(), iters, K, 0, connectivity, eps)
    OH, OW = size
    labels = torch.empty((B, OH, OW), dtype=torch.int32, device="cuda")
    capi.check(capi.lib().dinoseg_op_upsample_argmax(out["score"].data_ptr(), B, hp, wp, K + 1, OH, OW, labels.data_ptr(), None, S()))
    return MaskCutResult(labels, out["count"], out["found"], out["box"] * p, out["area"], out["cells"], out["seed_cell"], out["rho"],
                         original.view(torch.uint64)), out


@pytest.mark.parametrize("tag", ["tiny", "vits8"])
def test_round_zero_is_discover(cuda, tag):
    m = T.model(tag)
    for x in frames_both(tag, 2, 931):
        one = m.discover(x, iters=12, split=True)
        res = m.discover_all(x, max_objects=1, iters=12)
        assert isinstance(res, MaskCutResult) and res.graph is None
        assert torch.equal(res.labels, one.labels) and torch.equal(res.box[:, 0], one.box) and torch.equal(res.found[:, 0], one.found)
        assert torch.equal(res.cells[:, 0], one.cells) and torch.equal(res.area[:, 0], one.area)
        assert torch.equal(res.seed_cell[:, 0], one.ncut.seed_cell) and torch.equal(T.bits_of(res.rho[:, 0].contiguous()), T.bits_of(one.ncut.rho))
        assert torch.equal(res.count, one.found.to(torch.int32))


@pytest.mark.parametrize("tag", ["tiny", "vits8"])
def test_discover_all_is_the_entry_by_hand(cuda, tag):
    """K = 3 on uint8 and fp32 frames; the default size and another; a two-frame batch equals the two single-frame calls; chunk = 1
    equals chunk = 32; want_graph returns the ORIGINAL graph, the one ncut returns."""
    m = T.model(tag)
    for x in frames_both(tag, 2, 941):
        H, W = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])
        n = (H // m.cfg.patch) * (W // m.cfg.patch)
        res = m.discover_all(x, max_objects=3, iters=10, seed=2, want_graph=True)
        want, _ = model_by_hand(m, x, 3, 0.2, 1e-5, 10, 2, 32, (H, W))
        assert res.labels.shape == (2, H, W) and res.labels.dtype == torch.int32 and res.cells.shape == (2, 3, n)
        assert res.box.shape == (2, 3, 4) and res.rho.shape == (2, 3, 10) and res.graph.dtype == torch.uint64
        assert int(res.labels.min()) >= 0 and int(res.labels.max()) <= 3
        assert T.same(res, want)
        assert torch.equal(T.bits_of(res.graph), T.bits_of(m.ncut(x, iters=0, split=True, want_graph=True).graph))
        assert T.same(m.discover_all(x, max_objects=3, iters=10, seed=2, chunk=1, want_graph=True), res)
        for b in range(2):
            single = m.discover_all(x[b:b + 1], max_objects=3, iters=10, seed=2, want_graph=True)
            assert all(torch.equal(T.bits_of(s), T.bits_of(r[b:b + 1])) for s, r in zip(single, res))
        other = m.discover_all(x, max_objects=2, tau=0.1, eps=1e-4, iters=4, size=(H // 2, W + 8), connectivity=8, split=16)
        want2, _ = model_by_hand(m, x, 2, 0.1, 1e-4, 4, 0, 32, (H // 2, W + 8), 8)
        assert other.graph is None and T.same(other, want2)
        with pytest.raises(ValueError, match="split"):
            m.discover_all(x, split=False)
