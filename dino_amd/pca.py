"""The host half of the PCA of patch features: the eigen-solve of the device moments and the fitted projection.

``pca_solve`` is a plain host function (numpy, fp64): no GPU and no synchronisation inside it.  The device half -- the streaming
moments, the projection and the colour map -- is csrc/pca.hip behind ``dinoseg_op_token_moments``, ``dinoseg_op_pca_project`` and
``dinoseg_op_pca_colour`` (the rules: include/dinoseg.h)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch


def _np64(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64)


class FeaturePCA:
    """A fitted PCA of patch features: ``mean`` fp32 [D], ``basis`` fp32 [q, D] (unit rows, by descending eigenvalue),
    ``eigenvalues`` fp32 [q], ``total_variance`` (the trace of the covariance), ``rows`` (the rows fitted) and ``n_blocks`` (the
    blocks the features were taken after).  All tensors live on the host; the device copies the projection needs are made once
    per device.  ``state_dict`` / ``load_state_dict`` carry it bit for bit."""

    def __init__(self, mean: torch.Tensor, basis: torch.Tensor, eigenvalues: torch.Tensor, total_variance: float, rows: int,
                 n_blocks: int = 0):
        self._set(mean, basis, eigenvalues, total_variance, rows, n_blocks)

    def _set(self, mean, basis, eigenvalues, total_variance, rows, n_blocks) -> None:
        mean, basis, eigenvalues = (torch.as_tensor(t).detach().to("cpu").contiguous() for t in (mean, basis, eigenvalues))
        if mean.dtype != torch.float32 or basis.dtype != torch.float32 or eigenvalues.dtype != torch.float32:
            raise ValueError("mean, basis and eigenvalues must be fp32")
        if mean.dim() != 1 or basis.dim() != 2 or basis.shape[1] != mean.shape[0] or tuple(eigenvalues.shape) != (basis.shape[0],) \
                or basis.shape[0] < 1:
            raise ValueError(f"expected mean [D], basis [q, D] and eigenvalues [q], got {tuple(mean.shape)}, {tuple(basis.shape)}, "
                             f"{tuple(eigenvalues.shape)}")
        self.mean, self.basis, self.eigenvalues = mean.clone(), basis.clone(), eigenvalues.clone()
        self.total_variance, self.rows, self.n_blocks = float(total_variance), int(rows), int(n_blocks)
        self._device: Dict[str, tuple] = {}

    @property
    def q(self) -> int:
        return int(self.basis.shape[0])

    @property
    def dim(self) -> int:
        return int(self.basis.shape[1])

    def whitening(self) -> torch.Tensor:
        """fp32 [q]: 1 / sqrt(eigenvalue), formed in fp64 and rounded once; 0 for a component whose eigenvalue is not positive."""
        ev = self.eigenvalues.numpy().astype(np.float64)
        safe = np.where(ev > 0.0, ev, 1.0)
        return torch.from_numpy(np.where(ev > 0.0, 1.0 / np.sqrt(safe), 0.0).astype(np.float32))

    def on(self, device) -> tuple:
        """(mean, basis, whitening) on ``device``, copied once."""
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(t.to(device).contiguous() for t in (self.mean, self.basis, self.whitening()))
        return self._device[key]

    def state_dict(self) -> dict:
        return {"mean": self.mean.clone(), "basis": self.basis.clone(), "eigenvalues": self.eigenvalues.clone(),
                "total_variance": self.total_variance, "rows": self.rows, "n_blocks": self.n_blocks}

    def load_state_dict(self, state: dict) -> None:
        self._set(state["mean"], state["basis"], state["eigenvalues"], state["total_variance"], state["rows"], state["n_blocks"])

    @classmethod
    def from_state_dict(cls, state: dict) -> "FeaturePCA":
        return cls(state["mean"], state["basis"], state["eigenvalues"], state["total_variance"], state["rows"], state["n_blocks"])


def pca_solve(sum, outer, count, shift, q: int, n_blocks: int = 0) -> FeaturePCA:
    """The PCA of the moments ``dinoseg_op_token_moments`` accumulates: ``sum`` fp64 [D] and ``outer`` fp64 [D, D] of the shifted
    rows ``x - shift``, ``count`` rows, ``shift`` fp32 [D] (``None``: zeros).  ``numpy.linalg.eigh`` in fp64 of the covariance
    ``(outer - sum sum^T / count) / (count - 1)``; the ``q`` components of largest eigenvalue in descending order; the sign of
    each fixed so that its entry of largest magnitude (the first on a tie) is positive; ``mean = fp32(shift + sum / count)``.
    Refuses ``count < 2`` and ``q`` outside 1 .. D.  Host only: tensors on a device are read back by the caller's ``.cpu()``."""
    s, o = _np64(sum), _np64(outer)
    if s.ndim != 1 or o.shape != (s.shape[0], s.shape[0]):
        raise ValueError(f"expected sum [D] and outer [D, D], got {s.shape} and {o.shape}")
    D = s.shape[0]
    count = int(count.item() if hasattr(count, "item") else count)
    if count < 2:
        raise ValueError(f"a PCA needs at least 2 rows, got count = {count}")
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= int(q) <= D:
        raise ValueError(f"q must be an integer in 1..{D} (the features' width), got {q!r}")
    q = int(q)
    sh = np.zeros(D, np.float64) if shift is None else _np64(shift)
    if sh.shape != (D,):
        raise ValueError(f"expected shift [D = {D}], got {sh.shape}")
    cov = (o - np.outer(s, s) / count) / (count - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")[:q]
    vecs = v[:, order].T.copy()                                        # [q, D]
    for j in range(q):
        if vecs[j, int(np.argmax(np.abs(vecs[j])))] < 0.0:             # (argmax: the first on a tie)
            vecs[j] = -vecs[j]
    mean = (sh + s / count).astype(np.float32)
    return FeaturePCA(torch.from_numpy(mean), torch.from_numpy(vecs.astype(np.float32)),
                      torch.from_numpy(w[order].astype(np.float32)), float(np.trace(cov)), count, n_blocks)
