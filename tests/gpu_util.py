"""Helpers for the -m gpu parity tests: everything goes through the C-ABI (dino_amd.capi)."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import dino_amd
from dino_amd import capi

# the options dinoseg_refresh_weights reads (which packed copies it lays out): the comment above struct Options in dino_amd/csrc/kernels.h
REFRESH_OPTIONS = ("fp16_patch_planes", "mlp_fused4", "gemm_rs", "gemm_rs_ln")


@contextlib.contextmanager
def route_options(*models, **kw):
    """dino_amd.options(**kw) for models that are alive: where kw holds an option that is read at the refresh, every model refreshes
    its weights after the set and again after the restore."""
    def invalidate():
        if any(k in REFRESH_OPTIONS for k in kw):
            for m in models:
                m.invalidate_weights()
    try:
        with dino_amd.options(**kw):
            invalidate()
            yield
    finally:
        invalidate()


def pack(x: torch.Tensor, planes: int, rows_pad: int = None, cols_pad: int = None) -> torch.Tensor:
    """fp32 [rows, cols] device tensor -> int16 view of bf16 planes [planes, rows_pad, cols_pad]."""
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 2
    x = x.contiguous()
    rows, cols = x.shape
    rows_pad = rows_pad or rows
    cols_pad = cols_pad or cols
    out = torch.empty((planes, rows_pad, cols_pad), dtype=torch.int16, device=x.device)
    capi.check(capi.lib().dinoseg_op_pack(x.data_ptr(), rows, cols, out.data_ptr(), rows_pad * cols_pad, rows_pad,
                                          cols_pad, planes, capi.stream_ptr()))
    return out


def unpack(p: torch.Tensor) -> torch.Tensor:
    """int16 bf16 planes [planes, ...] -> fp32 sum of the planes."""
    return p.view(torch.bfloat16).to(torch.float32).sum(dim=0)


def quant_like(x: torch.Tensor, planes: int) -> torch.Tensor:
    """What the kernels see of an fp32 operand: bf16(x) or bf16(x) + bf16(x - bf16(x))."""
    hi = x.to(torch.bfloat16).to(torch.float32)
    if planes == 1:
        return hi
    return hi + (x - hi).to(torch.bfloat16).to(torch.float32)


def seeded(shape, seed, scale=1.0, device="cuda"):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(device)


def pack_slabs(W: torch.Tensor, planes: int) -> torch.Tensor:
    """fp32 [N, K] device weight -> int16 view of the slab-major bf16 copy gemm_ln.hip streams."""
    N, K = W.shape
    n = capi.lib().dinoseg_op_ln_gemm_slab_elems(N, K, planes)
    assert n > 0
    out = torch.empty((n,), dtype=torch.int16, device=W.device)
    capi.check(capi.lib().dinoseg_op_pack_slabs(W.contiguous().data_ptr(), N, K, planes, out.data_ptr(), capi.stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------ guard patterns
NAN16 = 0x7FC1                          # a NaN in both 16-bit formats: guard pattern of the int16 buffers
# a guard band is one full tile of rows of the tallest tile a forward kernel has: 256 rows in the GEMMs (gemm_big.hip) and the 256-query
# attention workgroups, 384 queries in the 12-wave hi + lo zero-reference attention kernel (attn_fwd_z_kernel<2, 3, 12>)
GUARD_ROWS = 384


def nan16(shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda")


def untouched(t):
    """every element still carries the guard pattern (NaN for floats, NAN16 for int16 planes)"""
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == NAN16).all())


class Guarded:
    """One flat device buffer around a [planes][rows][cols] output (fp32 or 16-bit planes as int16):

        | band | plane 0: rows x ld | band | plane 1: rows x ld | band |         band = GUARD_ROWS x ld elements

    Every element that is not output[p][r][c < cols] carries the guard pattern (NaN / NAN16): the bands in front, between the planes and
    behind, and the ld - cols columns behind every row.  plane = rows * ld + band is the plane stride handed to the entry; ld % 64 == 0 keeps
    every 16-byte alignment the exact layout has.  An overrun of up to one tile of rows in any direction stays inside the allocation.
    exact = True: the minimal strides of an exactly-sized buffer (ld = cols, plane = rows * cols) between a band in front and one behind --
    the layout the value tests use, with the same room for an overrun."""

    def __init__(self, planes, rows, cols, dtype, ld=None, band=None, exact=False):
        ld = ld or cols
        assert dtype in (torch.float32, torch.int16) and ld >= cols and not (exact and ld != cols)
        self.planes, self.rows, self.cols, self.ld = planes, rows, cols, ld
        self.band = band if band is not None else GUARD_ROWS * ld
        assert self.band % 64 == 0 and (band is not None or ld % 64 == 0)
        self.plane = rows * ld + (0 if exact else self.band)
        total = 2 * self.band + planes * self.plane - (0 if exact else self.band)
        self.flat = torch.full((total,), float("nan"), device="cuda") if dtype == torch.float32 else nan16((total,))
        self.out = self.flat.as_strided((planes, rows, cols), (self.plane, ld, 1), self.band)
        mask = torch.ones((total,), dtype=torch.bool, device="cuda")
        mask.as_strided((planes, rows, cols), (self.plane, ld, 1), self.band).fill_(False)
        self._guard = mask

    def ptr(self):
        return self.out.data_ptr()

    def fill(self, x):
        """payload <- x (planes * rows * cols elements in [planes][rows][cols] order); returns self"""
        self.out.copy_(x.reshape(self.planes, self.rows, self.cols))
        return self

    def guards_untouched(self):
        return untouched(self.flat[self._guard])

    def dense(self):
        """the payload as a contiguous [planes, rows, cols] tensor"""
        return self.out.contiguous()


def strided_planes(x, ld=None, gap_rows=3):
    """int16 planes x [planes, rows, cols] (contiguous) re-laid with a row stride ld >= cols and a plane stride of gap_rows extra rows; the
    gaps hold finite garbage (0x3C00 .. 0x43FF: 1 .. 4 as fp16, 0.008 .. 520 as bf16).  Returns (tensor to keep alive, data_ptr, plane, ld)."""
    planes, rows, cols = x.shape
    ld = ld or cols
    plane = (rows + gap_rows) * ld
    assert ld % 64 == 0 and x.dtype == torch.int16
    g = torch.Generator(device="cuda").manual_seed(1234)
    flat = torch.randint(0x3C00, 0x4400, (planes * plane,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    flat.as_strided((planes, rows, cols), (plane, ld, 1)).copy_(x)
    return flat, flat.data_ptr(), plane, ld
