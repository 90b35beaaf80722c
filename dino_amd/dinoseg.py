"""Host-side mirror of the reference ``DINOSeg`` (dt_segmentation/src/pl_torch_modules.py:141-440).

Same public surface -- ``load_from_checkpoint()``, ``.to()``, ``set_resolution()``, ``predict()``,
``forward()``/``__call__``, ``state_dict()`` keys, ``freeze_bb()/unfreeze_bb()`` -- with every
tensor op replaced by the hand-written gfx950 kernels behind the C-ABI in ``include/dinoseg.h``.
PyTorch only owns the parameters, the I/O tensors and the stream.  There is no CPU path: calling
the model without a ROCm device raises.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import capi
from .dense_plan import (_pair, bank_add_plan, components_plan, context_frames, dense_mode, frame_layout, guide_plan, guided_params, kmeans_plan, knn_plan, label_size,
                         maskcut_plan, multiscale_plan, ncut_plan, ncut_start, out_size, pca_plan, pca_projection, propagate_plan, refine_params, refine_plan,
                         resolution_message, sample_indices, view_sizes, window_origins, window_plan)  # noqa: F401  (view_sizes, window_origins: re-exported)
from .pca import FeaturePCA, pca_solve
from .preprocess import resize_linear_u8
from .weights import VIT_B8, VIT_B16, VIT_S8, VIT_S16, ViTConfig

_IMAGENET_MEAN = (0.485, 0.456, 0.406)
_IMAGENET_STD = (0.229, 0.224, 0.225)
_PRECISIONS = {"bf16": capi.BF16, "bf16x3": capi.BF16X3, "fp16": capi.FP16, "fp16x3": capi.FP16X3}
# precision "auto" (the default): the native handle of a call is chosen by what the call needs -- inference (predict,
# forward_frames, forward under no_grad or with nothing trainable, the visualisation paths) runs fp16 hi+lo planes, the parity mode
# that holds the flat 1e-3 bar with margin; a call that produces gradients runs bf16 hi+lo planes, the parity mode that trains
_AUTO_INFER, _AUTO_TRAIN = "fp16x3", "bf16x3"
# per-handle state of the model object: one set per native handle (precision "auto" keeps up to two)
_SLOT_KEYS = ("_handle", "_bound_sig", "_grad_sig", "_ptr_key", "_fast_index", "_fast_sig", "_pred_graphs")


# --------------------------------------------------------------------------- preprocessing mirror
class _Transforms:
    """Call-compatible stand-in for the albumentations pipeline of ``get_transforms``
    (pl_torch_modules.py:33-41): ``t(image=ndarray)['image']`` -> fp32 CHW tensor.

    Resize(res, res) is the identity for frames already at res x res (the benchmark / golden case);
    other sizes go through cv2.INTER_LINEAR's fixed-point arithmetic restated in dino_amd/preprocess.py
    (parity unpinned: albumentations / OpenCV are not available here -- see DESIGN.md).  ``predict`` does the same
    arithmetic on the GPU (``dinoseg_op_resize_u8``) and never calls this host path.
    """

    def __init__(self, resolution: int):
        self.resolution = int(resolution)

    def resize(self, img: np.ndarray) -> np.ndarray:
        r = self.resolution
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {img.shape}")
        if img.shape[0] == r and img.shape[1] == r:
            return np.ascontiguousarray(img, dtype=np.uint8)
        return resize_linear_u8(img, r, r)

    def __call__(self, image: np.ndarray) -> Dict[str, torch.Tensor]:
        u8 = self.resize(np.asarray(image))
        mean = np.array(_IMAGENET_MEAN, dtype=np.float32) * np.float32(255.0)
        inv = np.reciprocal(np.array(_IMAGENET_STD, dtype=np.float32) * np.float32(255.0))
        x = (u8.astype(np.float32) - mean) * inv
        return {"image": torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))}


def get_transforms(resolution: int = 480) -> _Transforms:
    return _Transforms(resolution)


def metrics_from_confusion(cm: np.ndarray, prefix: str = "val") -> Dict[str, float]:
    """cm[gt][pred] counts -> {prefix_acc (balanced accuracy), prefix_iou (macro Jaccard), prefix_F1 (macro F1)}."""
    tp = np.diag(cm)
    support = cm.sum(axis=1)          # per true class
    predicted = cm.sum(axis=0)        # per predicted class
    present = support > 0
    acc = float(np.mean(tp[present] / support[present])) if present.any() else 0.0
    labels = (support + predicted) > 0                       # sklearn: union of the labels seen in y_true and y_pred
    denom_f1 = 2 * tp + (predicted - tp) + (support - tp)
    denom_iou = tp + (predicted - tp) + (support - tp)
    f1 = float(np.mean(np.where(denom_f1[labels] > 0, 2 * tp[labels] / np.maximum(denom_f1[labels], 1), 0.0))) if labels.any() else 0.0
    iou = float(np.mean(np.where(denom_iou[labels] > 0, tp[labels] / np.maximum(denom_iou[labels], 1), 0.0))) if labels.any() else 0.0
    return {prefix + "_acc": acc, prefix + "_iou": iou, prefix + "_F1": f1}


# --------------------------------------------------------------------------- parameter containers
class _Attn(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.qkv = nn.Linear(D, 3 * D, bias=True)
        self.proj = nn.Linear(D, D)


class _Mlp(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.fc1 = nn.Linear(D, F)
        self.fc2 = nn.Linear(F, D)


class _Block(nn.Module):
    def __init__(self, D, F, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(D, eps=eps)
        self.attn = _Attn(D)
        self.norm2 = nn.LayerNorm(D, eps=eps)
        self.mlp = _Mlp(D, F)


class _PatchEmbed(nn.Module):
    def __init__(self, D, p):
        super().__init__()
        self.proj = nn.Conv2d(3, D, kernel_size=p, stride=p)


class _ViTParams(nn.Module):
    """The backbone as the reference exposes it (``model.dino``): the parameter names of the reference ViT's state_dict
    (vision_transformer.py:161-196) and its call surface -- ``dino(x)``, ``dino.get_last_selfattention(x)``,
    ``dino.forward_mask(x, cls_mask)`` -- with the arithmetic in libdinoseg_hip.so.  It holds a weak reference to the
    owning DINOSeg (which owns the native handle); a detached copy raises instead of computing on stale state."""

    def __init__(self, cfg: ViTConfig):
        super().__init__()
        D = cfg.embed_dim
        self.patch_embed = _PatchEmbed(D, cfg.patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, cfg.pos_grid * cfg.pos_grid + 1, D))
        self.blocks = nn.ModuleList([_Block(D, cfg.hidden, cfg.ln_eps) for _ in range(cfg.n_blocks)])
        self.norm = nn.LayerNorm(D, eps=cfg.ln_eps)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.apply(self._init_weights)
        object.__setattr__(self, "_owner_ref", None)

    def _init_weights(self, m):
        """vision_transformer.py:189-196 (what ``random_init=True`` re-applies, pl_torch_modules.py:181-183)."""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _set_owner(self, owner) -> None:
        object.__setattr__(self, "_owner_ref", weakref.ref(owner))

    def _owner(self):
        ref = self.__dict__.get("_owner_ref")
        owner = ref() if ref is not None else None
        if owner is None:
            raise capi.DinosegError("this backbone is not attached to a DINOSeg (the native handle lives there)")
        return owner

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_owner_ref"] = None          # weak references do not pickle / deep-copy; DINOSeg re-links its copy
        return state

    def forward(self, x: torch.Tensor, all: bool = True, intermediate=False) -> torch.Tensor:
        """VisionTransformer.forward (vision_transformer.py:237-248): fp32 [B,3,H,W] -> final-norm tokens [B, N, D]
        (``all=False``: the CLS row [B, D]); ``intermediate=k`` returns ``norm(x)`` of ALL tokens after block k, whatever ``all``
        says (:241-242) -- unless k is past the last block, where the loop never exits early and ``all`` applies (:243-248)."""
        owner = self._owner()
        k = int(intermediate) if intermediate else 0
        early = 0 < k <= owner.n_blocks
        t = owner.features(x, n_blocks=k if early else 0)
        return t if (all or early) else t[:, 0]

    def get_last_selfattention(self, x, cls_mask=None):
        """vision_transformer.py:273-280; reference call site visualize_attention.py:46."""
        return self._owner().get_last_selfattention(x, cls_mask)

    def cls_attention(self, x, size=None, threshold=None):
        """The CLS row of ``get_last_selfattention(x)`` over the patches at pixel resolution: ``DINOSeg.cls_attention``."""
        return self._owner().cls_attention(x, size, threshold)

    def get_intermediate_layers(self, x: torch.Tensor, n: int = 1) -> list:
        """vision_transformer.py:282-290: ``norm(x)`` of all tokens after each of the last ``n`` blocks, oldest first (a list of
        [B, N, D] tensors; every block when n exceeds the depth).  One ``dinoseg_features`` call per tap: the library keeps one
        residual stream, so the forward is re-run up to the tapped block (n is 1 in every published use of this method)."""
        owner = self._owner()
        L = owner.cfg.n_blocks
        return [owner.features(x, n_blocks=i + 1) for i in range(L) if L - i <= n]

    def forward_mask(self, x, cls_mask):
        """vision_transformer.py:250-271."""
        return self._owner().forward_mask(x, cls_mask)


class _MLPHead(nn.Module):
    def __init__(self, n_classes, input_dim):
        super().__init__()
        self.layer_1 = nn.Linear(input_dim, 200)
        self.layer_2 = nn.Linear(200, 100)
        self.layer_3 = nn.Linear(100, n_classes)


class _LinearHead(nn.Module):
    def __init__(self, n_classes, input_dim):
        super().__init__()
        self.layer_1 = nn.Linear(input_dim, n_classes)


class _DinoSegFunction(torch.autograd.Function):
    """DINOSeg.forward under autograd: forward = dinoseg_train_forward (activations kept in the library's workspace),
    backward = dinoseg_backward(d loss / d logp).  The parameters are inputs only so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, model, x, kind, B, H, W, *params):
        logp = model._autograd_forward(x, kind, B, H, W)
        ctx.model = model
        ctx.epoch = model._fwd_epoch
        ctx.params = params
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        grads = ctx.model._autograd_backward(dlogp, ctx.epoch, ctx.params)
        return (None, None, None, None, None, None) + grads


class _DenseNLLFunction(torch.autograd.Function):
    """Cross-entropy of the bilinearly upsampled log-probs against pixel labels (csrc/upsample_loss.hip).  The forward runs
    ``dinoseg_op_upsample_nll`` and keeps d loss / d logp; the backward scales it by the incoming gradient."""

    @staticmethod
    def forward(ctx, logp, y, hp, wp, ignore_index, flags):
        if not logp.is_cuda:
            raise capi.DinosegError("dense_nll_loss runs only on a ROCm device; there is no CPU path")
        if y.dim() != 3:
            raise ValueError(f"expected pixel labels [B, OH, OW], got {tuple(y.shape)}")
        B, OH, OW = (int(v) for v in y.shape)
        C_ = int(logp.shape[-1])
        if logp.numel() != B * hp * wp * C_:
            raise ValueError(f"logp {tuple(logp.shape)} does not hold B*hp*wp = {B * hp * wp} rows of {C_} classes")
        lp = logp.detach().to(torch.float32).contiguous()
        y = y.to(device=lp.device, dtype=torch.int64).contiguous()
        lib = capi.lib()
        with torch.cuda.device(lp.device):
            nbytes = lib.dinoseg_op_upsample_nll_scratch_bytes(B, hp, wp, C_, OH, OW)
            if nbytes < 0:
                raise capi.DinosegError(f"dinoseg error -1: {capi.last_error()}")
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=lp.device)
            loss = torch.zeros((), dtype=torch.float32, device=lp.device)
            dlogp = torch.empty_like(lp)
            capi.check(lib.dinoseg_op_upsample_nll(lp.data_ptr(), B, hp, wp, C_, OH, OW, y.data_ptr(), int(ignore_index), loss.data_ptr(),
                                                   dlogp.data_ptr(), None, capi.ptr(flags), scratch.data_ptr(),
                                                   capi.stream_ptr(lp.device)))
        ctx.save_for_backward(dlogp)
        ctx.shape = logp.shape
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dlogp,) = ctx.saved_tensors
        return (grad_out * dlogp).view(ctx.shape), None, None, None, None, None


def dense_nll_loss(logp: torch.Tensor, y: torch.Tensor, grid, ignore_index: int = 255, flags: Optional[torch.Tensor] = None):
    """``F.cross_entropy(F.interpolate(logp.view(B, hp, wp, C).permute(0, 3, 1, 2), size=y.shape[1:], mode="bilinear",
    align_corners=False), y, ignore_index=ignore_index)`` in two launches without the [B, C, OH, OW] tensor, differentiable with
    respect to ``logp`` (fp32 [B*hp*wp, C] or [B, hp*wp, C] on the GPU; ``grid = (hp, wp)``; y any integer dtype, [B, OH, OW] with
    OH >= hp, OW >= wp).  Labels equal to ``ignore_index`` or -100 are skipped; any other label outside [0, C) is skipped as well and
    sets ``flags[0]`` (an int32 device tensor, optional).  The gradient is summed in a fixed order: bit-identical run to run."""
    hp, wp = (int(v) for v in grid)
    return _DenseNLLFunction.apply(logp, y, hp, wp, ignore_index, flags)


# --------------------------------------------------------------------------- the model
class DINOSeg(nn.Module):
    """DINO ViT + per-patch segmentation head on MI355X.

    Constructor keywords follow the reference (pl_torch_modules.py:144-147); three extra
    keyword-only arguments select what the reference hard-codes or cannot express:
    ``arch`` ('vit_small' | 'vit_base' | a ViTConfig giving embed_dim/num_heads/mlp_ratio/patch/pos_grid), ``patch_size`` (8 or 16,
    the reference's ``get_dino(patch_size=8)``; None: the ViTConfig's own, 8 for a named arch; at 16 the stored position grid is
    14 x 14 and every frame side is a multiple of 16) and ``precision``: 'auto' (default: 'fp16x3'
    for inference calls, 'bf16x3' when a gradient is requested), 'fp16x3' / 'bf16x3' (parity modes: hi + lo operand planes),
    'fp16' / 'bf16' (benchmark modes: one plane).
    """

    def __init__(self, data_path=None, write_path=None, class_names=None, head="linear", n_blocks=1,
                 batch_size=1, lr=1e-6, optimizer=torch.optim.AdamW, freeze_backbone=True, max_epochs=200,
                 patience=10, grayscale=False, n_classes=7, pretrain_on_sim=False, comet_logger=None,
                 augmented=True, random_init=False, backbone="vit", *, arch="vit_small", patch_size=None, precision="auto"):
        super().__init__()
        if backbone != "vit":
            raise NotImplementedError("only backbone='vit' is on the MI355X hot path (SURVEY.md §2 row 7)")
        if head not in ("linear", "mlp"):
            raise ValueError(f"unknown head {head!r}")
        if precision != "auto" and precision not in _PRECISIONS:
            raise ValueError(f"precision must be 'auto' or one of {sorted(_PRECISIONS)}")
        if patch_size is not None and patch_size not in (8, 16):
            raise ValueError(f"patch_size must be 8 or 16 (the published DINO sizes), got {patch_size!r}")
        if isinstance(arch, ViTConfig):
            base = arch
            if patch_size is not None and int(patch_size) != base.patch:
                raise ValueError(f"patch_size={patch_size} contradicts arch.patch={base.patch}")
        else:
            base = {("vit_small", 8): VIT_S8, ("vit_base", 8): VIT_B8, ("vit_small", 16): VIT_S16,
                    ("vit_base", 16): VIT_B16}[(arch, 8 if patch_size is None else int(patch_size))]
        if base.patch not in (8, 16):
            raise ValueError(f"arch.patch must be 8 or 16 (the published DINO sizes), got {base.patch}")
        self.cfg = ViTConfig(embed_dim=base.embed_dim, num_heads=base.num_heads, mlp_ratio=base.mlp_ratio, n_blocks=int(n_blocks),
                             n_classes=int(n_classes), head=head, patch=base.patch, pos_grid=base.pos_grid)
        self.patch_size = self.cfg.patch
        self.arch = arch
        self.precision = precision
        self.n_blocks = n_blocks
        self.head = head
        self.batch_size = batch_size
        self.lr = lr
        self.optimizer = optimizer
        self.freeze_backbone = freeze_backbone
        self.max_epochs = max_epochs
        self.patience = patience
        self.grayscale = grayscale
        self.n_classes = n_classes
        self.comet_logger = comet_logger
        self.class_names = class_names
        self.pretrain_on_sim = pretrain_on_sim
        self.augmented = augmented
        self.random_init = random_init
        self.backbone = backbone
        self.mlp_input_dim = self.cfg.embed_dim
        self.data_path, self.write_path = data_path, write_path
        self.best_ck = None

        self.resolution = 480
        self.transforms = get_transforms(self.resolution)

        # No network: the pretrained DINO fetch of the reference (dt_utils.py:19-29) is replaced by
        # a random init; real weights arrive through load_state_dict / load_from_checkpoint.
        self.dino = _ViTParams(self.cfg)
        self.clf = (_MLPHead(self.cfg.n_classes, self.cfg.embed_dim) if head == "mlp"
                    else _LinearHead(self.cfg.n_classes, self.cfg.embed_dim))

        self.dino._set_owner(self)
        if random_init:         # pl_torch_modules.py:181-183
            self.dino.apply(self.dino._init_weights)

        self._handle: Optional[C.c_void_p] = None
        self._bound_sig = None
        self._grad_sig = None
        self._weights_epoch = 0

    # ---- plumbing -------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.dino.cls_token.device

    def _require_gpu(self) -> None:
        if self.device.type != "cuda":
            raise capi.DinosegError("DINOSeg runs only on a ROCm device (call .to('cuda:0')); there is no CPU path")

    def _param_signature(self):
        return (self._weights_epoch,) + tuple((k, v.data_ptr(), v._version) for k, v in self.state_dict(keep_vars=True).items())

    # The full signature walks state_dict() (~0.2 ms for 156 tensors): a 20-40 % tax on a single-frame predict().  The fast check
    # below sees the same events without building it: every tensor's version counter and address (in-place updates, optimizer
    # steps, load_state_dict, .to()), the identity of every entry of every module's parameter / buffer / child table (a replaced
    # Parameter or sub-module), and the tables' sizes (an added one).  Only when it differs is the full signature rebuilt.
    def _build_fast_index(self):
        tens, tables = [], []
        for mod in self.modules():
            for d in (mod._parameters, mod._buffers, mod._modules):
                tables.append((d, len(d)))
                tens.extend((d, k, t) for k, t in d.items() if t is not None)
        return tens, tables

    def _fast_signature(self):
        idx = self.__dict__.get("_fast_index")
        if idx is None:
            return None
        tens, tables = idx
        for d, n in tables:
            if len(d) != n:
                return None
        vers = []
        for d, k, t in tens:
            if d.get(k) is not t:
                return None
            if isinstance(t, torch.Tensor):
                vers.append(t._version)
                vers.append(t.data_ptr())
        vers.append(self._weights_epoch)
        return vers

    def invalidate_weights(self) -> None:
        """Force a re-pack of the bf16 weight planes on the next call.  In-place edits through ``p.data`` (or any write that
        does not bump the tensor version counter) are invisible to the automatic check; call this after them."""
        self._weights_epoch += 1

    def _stream(self) -> int:
        """hipStream_t of torch's current stream ON THE MODEL'S DEVICE (not the caller's current device)."""
        return capi.stream_ptr(self.device)

    # the native handle, its bound-pointer signatures and the weak owner link are process state, not model state
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_handle"] = None
        state["_bound_sig"] = None
        state["_grad_sig"] = None
        state.pop("_fast_index", None)
        state.pop("_fast_sig", None)
        state.pop("_pred_graphs", None)
        state.pop("_ptr_key", None)
        state.pop("_adam_state", None)
        state.pop("_grad_bucket_cache", None)
        state.pop("_slots", None)
        state.pop("_active_precision", None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._handle = None
        self._bound_sig = None
        self._grad_sig = None
        self.dino._set_owner(self)

    def _use(self, train: bool) -> None:
        """precision 'auto': make the native handle of the wanted kind the active one (created on first use by _sync_weights).
        Each handle keeps its own bound-pointer signatures, packed weights, workspaces and captured predict() graphs, so an
        evaluation between two training steps costs no re-creation; both read the SAME parameter tensors and re-pack on their
        own next use after an update."""
        if self.precision != "auto":
            return
        want = _AUTO_TRAIN if train else _AUTO_INFER
        cur = self.__dict__.get("_active_precision")
        if cur == want:
            return
        slots = self.__dict__.setdefault("_slots", {})
        if cur is not None:
            slots[cur] = {k: self.__dict__.pop(k, None) for k in _SLOT_KEYS}
        st = slots.pop(want, None) or {}
        for k in _SLOT_KEYS:
            v = st.get(k)
            if v is None and k not in ("_handle", "_bound_sig", "_grad_sig"):
                self.__dict__.pop(k, None)
            else:
                self.__dict__[k] = v
        self._active_precision = want

    def effective_precision(self, train: bool = False) -> str:
        """The operand precision a call of the given kind runs in ('auto' resolved)."""
        if self.precision != "auto":
            return self.precision
        return _AUTO_TRAIN if train else _AUTO_INFER

    def _sync_weights(self, train: bool = False) -> None:
        """Create the native handle if needed and (re)bind + repack when any parameter moved or changed."""
        lib = capi.lib()
        self._require_gpu()
        self._use(train)
        if self._handle is None:
            cfg = capi.Config(self.cfg.embed_dim, self.cfg.num_heads, self.cfg.n_blocks, self.cfg.patch,
                              self.cfg.mlp_ratio, self.cfg.n_classes,
                              capi.HEAD_MLP if self.head == "mlp" else capi.HEAD_LINEAR, self.cfg.pos_grid,
                              self.cfg.ln_eps, _PRECISIONS[self.effective_precision(train)])
            h = C.c_void_p()
            capi.check(lib.dinoseg_create(C.byref(cfg), C.byref(h)))
            self._handle = h
            self._bound_sig = None
        if self._bound_sig is not None:
            fast = self._fast_signature()
            if fast is not None and fast == self.__dict__.get("_fast_sig"):
                return
        sig = self._param_signature()
        if sig == self._bound_sig:
            self._fast_index = self._build_fast_index()
            self._fast_sig = self._fast_signature()
            return
        for name, t in self.state_dict(keep_vars=True).items():
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise capi.DinosegError(f"parameter {name} must be contiguous fp32")
            shape = (C.c_int64 * t.dim())(*t.shape)
            capi.check(lib.dinoseg_bind_weight(self._handle, name.encode(), t.data_ptr(), shape, t.dim()))
        capi.check(lib.dinoseg_refresh_weights(self._handle, self._stream()))
        self._bound_sig = sig
        self._ptr_key = (id(self._handle),) + tuple(e[1] for e in sig[1:])      # parameter storage the library's kernels read directly
        self._fast_index = self._build_fast_index()
        self._fast_sig = self._fast_signature()

    def set_precision(self, precision: str) -> None:
        if precision != "auto" and precision not in _PRECISIONS:
            raise ValueError(f"precision must be 'auto' or one of {sorted(_PRECISIONS)}")
        if precision != self.precision:
            self._release()
            self.precision = precision

    def _release(self) -> None:
        self.__dict__.pop("_pred_graphs", None)          # captured graphs hold the handle's workspace and packed-weight addresses
        for st in self.__dict__.pop("_slots", {}).values():      # precision 'auto': the handle that is not the active one
            if st.get("_handle") is not None:
                capi.lib().dinoseg_destroy(st["_handle"])
        self.__dict__.pop("_active_precision", None)
        if self._handle is not None:
            capi.lib().dinoseg_destroy(self._handle)
            self._handle = None
            self._bound_sig = None
            self._grad_sig = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---- reference API ----------------------------------------------------------------------
    def set_resolution(self, resolution=480):
        if resolution % self.cfg.patch != 0:
            raise ValueError(resolution_message(self.cfg.patch))
        self.transforms = get_transforms(resolution)
        self.resolution = resolution

    def _run(self, x: torch.Tensor, kind: int, B: int, H: int, W: int, want_logp: bool = True, want_argmax: bool = False,
             tap_block: int = -1):
        self._sync_weights()
        n = (H // self.cfg.patch) * (W // self.cfg.patch)
        dev = x.device
        logp = torch.empty((B * n, self.cfg.n_classes), dtype=torch.float32, device=dev) if want_logp else None
        amax = torch.empty((B * n,), dtype=torch.int32, device=dev) if want_argmax else None
        tap = (torch.empty((B * (n + 1), self.cfg.embed_dim), dtype=torch.float32, device=dev)
               if tap_block >= 0 else None)
        capi.check(capi.lib().dinoseg_forward_hw(self._handle, x.data_ptr(), kind, B, H, W, capi.ptr(logp), capi.ptr(amax),
                                                 tap_block, capi.ptr(tap), self._stream()))
        return logp, amax, tap

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [B,3,H,W] (normalised; H, W multiples of 8) -> fp32 [B*(H/8)*(W/8), n_classes] log-probabilities, patches row-major
        (pl_torch_modules.py:239-256; the ViT takes H x W frames, vision_transformer.py:202-235).
        With grad enabled and at least one trainable parameter the result carries an autograd graph: its backward calls
        ``dinoseg_backward`` and hands d loss / d parameter to torch (x itself gets no gradient: the reference never asks)."""
        self._require_gpu()
        x, kind, B, H, W = self._prep_batch(x)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _DinoSegFunction.apply(self, x, kind, B, H, W, *self.parameters())
        logp, _, _ = self._run(x, kind, B, H, W)
        return logp

    def features(self, x: torch.Tensor, n_blocks: int = 0) -> torch.Tensor:
        """``model.dino(x)``: final-norm tokens fp32 [B, N, D] after `n_blocks` blocks (0 = all), CLS token first
        (VisionTransformer.forward, vision_transformer.py:237-248).  Inference only (no autograd graph)."""
        self._require_gpu()
        x, kind, B, H, W = self._prep_batch(x)
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._sync_weights()
        out = torch.empty((B, (H // self.cfg.patch) * (W // self.cfg.patch) + 1, self.cfg.embed_dim), dtype=torch.float32, device=self.device)
        capi.check(capi.lib().dinoseg_features_hw(self._handle, x.data_ptr(), kind, B, H, W, n_blocks, out.data_ptr(),
                                                  self._stream()))
        return out

    @torch.no_grad()
    def forward_frames(self, frames_u8: torch.Tensor, want_logp: bool = True):
        """uint8 [B,H,W,3] device frames -> (log-probs or None, int32 argmax [B*(H/8)*(W/8)]).
        The batched form of predict(): normalisation is fused into the patch gather on device."""
        self._require_gpu()
        kind, B, H, W = frame_layout(frames_u8, self.cfg.patch, multiple=True, u8_only=True)
        logp, amax, _ = self._run(self._to_device(frames_u8, kind), kind, B, H, W, want_logp=want_logp, want_argmax=True)
        return logp, amax

    # ---- pixel-resolution output (bilinear upsample + argmax of the log-probs, fused: csrc/upsample.hip) ----
    def _alloc_out(self, B: int, OH: int, OW: int, want_dense: bool):
        """(labels int32 [B,OH,OW], dense fp32 [B,C,OH,OW] or None) on the model's device."""
        labels = torch.empty((B, OH, OW), dtype=torch.int32, device=self.device)
        dense = torch.empty((B, self.cfg.n_classes, OH, OW), dtype=torch.float32, device=self.device) if want_dense else None
        return labels, dense

    def _bilinear(self, x: torch.Tensor, size, want_dense: bool = False, want_logp: bool = False):
        """The forward and the upsample of its log-probs to ``size`` in one library call: (labels int32 [B,OH,OW], dense fp32
        [B,C,OH,OW] or None, low-res log-probs [B*n, C] or None).  Without ``want_logp`` the low-res log-probs stay in the
        library's workspace; the [B,C,OH,OW] tensor exists only when asked for."""
        kind, B, H, W = frame_layout(x, self.cfg.patch, multiple=True)
        OH, OW = out_size(size, (H, W))
        self._require_gpu()
        x = self._to_device(x, kind)
        self._sync_weights()
        n = (H // self.cfg.patch) * (W // self.cfg.patch)
        labels, dense = self._alloc_out(B, OH, OW, want_dense)
        logp = torch.empty((B * n, self.cfg.n_classes), dtype=torch.float32, device=x.device) if want_logp else None
        capi.check(capi.lib().dinoseg_forward_dense_hw(self._handle, x.data_ptr(), kind, B, H, W, OH, OW, capi.ptr(logp), None,
                                                       labels.data_ptr(), capi.ptr(dense), self._stream()))
        return labels, dense, logp

    @torch.no_grad()
    def segment(self, x: torch.Tensor, size=None, want_logp: bool = False):
        """Pixel-resolution labels: uint8 [B,H,W,3] or fp32 [B,3,H,W] frames -> (labels int32 [B,OH,OW], dense or None).
        The log-probabilities of the patch grid are interpolated bilinearly to ``size = (OH, OW)`` (default: the frames' own
        (H, W); any OH >= H/patch, OW >= W/patch) and the argmax is taken per pixel -- ``F.interpolate(logp.view(B, hp, wp,
        C).permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False).argmax(1)`` with exact coordinates and the first
        maximum -- in one launch behind the head, without the [B,C,OH,OW] transient.  ``want_logp=True`` also returns those
        interpolated log-probabilities (``dense``, fp32 [B,C,OH,OW]: CRFs, multi-scale averaging).  For label boundaries that
        follow the image's edges without that tensor: ``segment_guided``.  Inference only."""
        return self._bilinear(x, size, want_dense=want_logp)[:2]

    # ---- image-guided pixel-resolution output (joint bilateral upsample of the log-probs: csrc/upsample_guided.hip) ----
    def _guided(self, x: torch.Tensor, guide, size, params, want_dense: bool = False):
        """The forward and the guided upsample of its log-probs in one library call: (labels int32 [B,OH,OW], dense fp32
        [B,C,OH,OW] or None, low-res log-probs [B*n, C]).  Without a ``guide`` the frames guide themselves, resized when
        ``size`` is not their own."""
        kind, B, H, W, OH, OW = guide_plan(self.cfg.patch, x, guide, size)
        self._require_gpu()
        x = self._to_device(x, kind)
        if guide is not None:
            guide = guide.to(self.device).contiguous()
        elif (OH, OW) == (H, W):
            guide = x
        else:
            guide = self._resize_view(x, kind, OH, OW)
        self._sync_weights()
        hp, wp = H // self.cfg.patch, W // self.cfg.patch
        logp = torch.empty((B * hp * wp, self.cfg.n_classes), dtype=torch.float32, device=x.device)
        cells = torch.empty((B, hp, wp), dtype=torch.int32, device=x.device)
        labels, dense = self._alloc_out(B, OH, OW, want_dense)
        capi.check(capi.lib().dinoseg_forward_guided_hw(self._handle, x.data_ptr(), kind, B, H, W, guide.data_ptr(), OH, OW, params[0],
                                                        params[1], params[2], logp.data_ptr(), cells.data_ptr(), labels.data_ptr(),
                                                        capi.ptr(dense), self._stream()))
        return labels, dense, logp

    @torch.no_grad()
    def segment_guided(self, x: torch.Tensor, guide: Optional[torch.Tensor] = None, size=None, radius: int = 2,
                       sigma_spatial: float = 1.0, sigma_range: float = 0.1, want_logp: bool = False):
        """``segment`` with label boundaries that follow the image: uint8 [B,H,W,3] or fp32 [B,3,H,W] frames -> (labels int32
        [B,OH,OW], dense or None).  The log-probabilities of the patch grid are enlarged by joint bilateral upsampling (Kopf et al.
        2007): every output pixel averages the (2 radius + 1)^2 cells around its own with a spatial Gaussian (``sigma_spatial``, in
        cells) times a Gaussian of the colour distance (``sigma_range``, of the 0..255 range) between the guide at that pixel and
        the cell's mean colour; the argmax is taken per pixel in the same launch, without the [B,C,OH,OW] transient (the rule:
        include/dinoseg.h, dinoseg_op_upsample_guided).  ``guide`` is a uint8 image [B,OH,OW,3] at the output's size (``size``
        defaults to it; a different ``size`` or batch raises).  Without one the frames guide themselves: uint8 frames only (fp32
        frames raise ``ValueError``), resized by ``dinoseg_op_resize_u8`` when ``size`` is not their own.  ``radius=0`` is the
        nearest-neighbour enlargement.  ``want_logp=True`` also returns the averaged log-probabilities (fp32 [B,C,OH,OW]).  The
        defaults are a starting point: their effect on mIoU has not been measured on any dataset.  Inference only."""
        return self._guided(x, guide, size, guided_params(True, radius, sigma_spatial, sigma_range), want_logp)[:2]

    # ---- image-guided iterative label refinement (PAMR passes at pixel resolution: csrc/refine.hip) ----
    def _refine_buffers(self, B: int, nc: int, OH: int, OW: int, want_probs: bool):
        """(scratch fp32 [2, B, C, OH, OW], labels int32 [B,OH,OW], probs fp32 [B,C,OH,OW] or None) on the model's device."""
        nbytes = capi.lib().dinoseg_refine_scratch_bytes(B, nc, OH, OW)
        if nbytes < 0:
            raise capi.DinosegError(capi.last_error())
        scratch = torch.empty((nbytes // 4,), dtype=torch.float32, device=self.device)
        labels = torch.empty((B, OH, OW), dtype=torch.int32, device=self.device)
        probs = torch.empty((B, nc, OH, OW), dtype=torch.float32, device=self.device) if want_probs else None
        return scratch, labels, probs

    @torch.no_grad()
    def refine(self, seed: torch.Tensor, guide: torch.Tensor, n_classes: Optional[int] = None, grid=None, gain: float = 1.0,
               iters: int = 10, dilations=(1, 2, 4, 8, 12, 24), sigma: float = 0.1, want_probs: bool = False):
        """Image-guided iterative refinement (PAMR, Araslanov & Roth 2020) of a coarse result -> (labels int32 [B,OH,OW], probs
        fp32 [B,C,OH,OW] or None).  ``seed`` is an integer label map [B,OH,OW] at the guide's size with ``n_classes`` (the labels
        of ``segment*``, ``cluster``, ``ncut``, ``discover_all``, ``propagate``, or hand labels; a label outside [0, n_classes)
        is void and takes what its neighbours give), or fp32 scores [B,n,C] on a patch grid ``grid=(hp, wp)`` (log-probs,
        ``cluster``'s scores), enlarged bilinearly and turned into ``softmax(gain * v)``.  ``guide`` is a uint8 image [B,OH,OW,3].
        Every pass averages the state over 8 taps per dilation with weights ``exp(-|colour difference| / (3 sigma std))``, std the
        guide's local deviation per channel, so label boundaries move onto the image's edges (the rule: include/dinoseg.h,
        dinoseg_op_refine_iterate).  A pixel no mass reached is labelled -1.  Uses no model weight.  The defaults are PAMR's; their
        effect on mIoU has not been measured on any dataset."""
        kind, B, nc, OH, OW, hp, wp, gain, iters, dil, sigma = refine_plan(seed, guide, n_classes, grid, gain, iters, dilations, sigma)
        self._require_gpu()
        guide = guide.to(self.device).contiguous()
        seed = seed.to(self.device)
        seed = (seed.to(torch.int32) if kind == 0 else seed).contiguous()
        scratch, labels, probs = self._refine_buffers(B, nc, OH, OW, want_probs)
        lib, s = capi.lib(), self._stream()
        capi.check(lib.dinoseg_op_refine_seed(seed.data_ptr(), kind, B, nc, OH, OW, hp, wp, gain, scratch.data_ptr(), s))
        capi.check(lib.dinoseg_op_refine_iterate(guide.data_ptr(), scratch.data_ptr(), B, nc, OH, OW, (C.c_int32 * len(dil))(*dil),
                                                 len(dil), sigma, iters, labels.data_ptr(), capi.ptr(probs), s))
        return labels, probs

    @torch.no_grad()
    def segment_refined(self, x: torch.Tensor, guide: Optional[torch.Tensor] = None, size=None, gain: float = 1.0, iters: int = 10,
                        dilations=(1, 2, 4, 8, 12, 24), sigma: float = 0.1, want_probs: bool = False):
        """``segment`` followed by ``refine`` in one library call: the forward, then the refinement seeded from its own
        log-probs (``softmax(gain * bilinear enlargement)``) -> (labels int32 [B,OH,OW], probs fp32 [B,C,OH,OW] or None).  The guide
        rules are ``segment_guided``'s: a uint8 ``guide`` [B,OH,OW,3] at the output's size, or none for uint8 frames, which then
        guide themselves (resized when ``size`` is not their own); fp32 frames without a guide raise ``ValueError``.  Inference
        only; the effect on mIoU has not been measured on any dataset."""
        gain, iters, dil, sigma = refine_params(gain, iters, dilations, sigma)
        kind, B, H, W, OH, OW = guide_plan(self.cfg.patch, x, guide, size)
        if OH > (1 << 14) or OW > (1 << 14):
            raise ValueError(f"size {(OH, OW)} exceeds the refinement's 16384 per side")
        self._require_gpu()
        x = self._to_device(x, kind)
        if guide is not None:
            guide = guide.to(self.device).contiguous()
        elif (OH, OW) == (H, W):
            guide = x
        else:
            guide = self._resize_view(x, kind, OH, OW)
        self._sync_weights()
        hp, wp = H // self.cfg.patch, W // self.cfg.patch
        logp = torch.empty((B * hp * wp, self.cfg.n_classes), dtype=torch.float32, device=x.device)
        scratch, labels, probs = self._refine_buffers(B, self.cfg.n_classes, OH, OW, want_probs)
        capi.check(capi.lib().dinoseg_forward_refined_hw(self._handle, x.data_ptr(), kind, B, H, W, guide.data_ptr(), OH, OW, gain,
                                                         (C.c_int32 * len(dil))(*dil), len(dil), sigma, iters, logp.data_ptr(),
                                                         scratch.data_ptr(), labels.data_ptr(), capi.ptr(probs), self._stream()))
        return labels, probs

    # ---- multi-scale + flip ensemble at pixel resolution (csrc/upsample_ensemble.hip) ----
    def _resize_view(self, x: torch.Tensor, kind: int, Hk: int, Wk: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The batch resized to Hk x Wk: F.interpolate for fp32 [B,3,H,W], dinoseg_op_resize_u8 frame by frame for uint8 [B,H,W,3]
        (into ``out`` where the caller owns the destination: the static input of ``predict``'s graph)."""
        if kind != capi.INPUT_U8_HWC:
            return F.interpolate(x, size=(Hk, Wk), mode="bilinear", align_corners=False).contiguous()
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
        if out is None:
            out = torch.empty((B, Hk, Wk, 3), dtype=torch.uint8, device=x.device)
        for i in range(B):
            capi.check(capi.lib().dinoseg_op_resize_u8(x.data_ptr() + i * H * W * 3, H, W, out.data_ptr() + i * Hk * Wk * 3, Hk, Wk,
                                                      self._stream()))
        return out

    def _multiscale(self, x: torch.Tensor, scales, flip: bool, size, want_conf: bool, want_probs: bool):
        """segment_multiscale, also returning the low-res log-probs of the unflipped scale-1.0 view (the first view's without
        one): what a validation step reports as "probs"."""
        p = self.cfg.patch
        kind, B, H, W = frame_layout(x, p, multiple=True)
        views, K, (OH, OW) = multiscale_plan(p, H, W, scales, flip, size)
        self._require_gpu()
        x = self._to_device(x, kind)
        w_axis = 2 if kind == capi.INPUT_U8_HWC else 3
        logps, xv, cur = [], None, None
        for Hk, Wk, f in views:                         # scale-major, the unflipped view first: one resize per scale
            if cur != (Hk, Wk):
                xv, cur = (x if (Hk, Wk) == (H, W) else self._resize_view(x, kind, Hk, Wk)), (Hk, Wk)
            xin = torch.flip(xv, dims=[w_axis]).contiguous() if f else xv
            logps.append(self._run(xin, kind, B, Hk, Wk, want_logp=True)[0])
        del xv, xin
        dev = x.device
        labels = torch.empty((B, OH, OW), dtype=torch.int32, device=dev)
        conf = torch.empty((B, OH, OW), dtype=torch.float32, device=dev) if want_conf else None
        probs = torch.empty((B, self.cfg.n_classes, OH, OW), dtype=torch.float32, device=dev) if want_probs else None
        lib = capi.lib()
        need = int(lib.dinoseg_op_upsample_ensemble_scratch_bytes(K, B, OH, OW))
        if need < 0:
            raise ValueError(f"bad ensemble shape: K={K} B={B} output {OH}x{OW}")
        scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
        i32 = lambda xs: (C.c_int32 * K)(*xs)
        capi.check(lib.dinoseg_op_upsample_ensemble((C.c_void_p * K)(*[t.data_ptr() for t in logps]), i32([v[0] // p for v in views]),
                                                    i32([v[1] // p for v in views]), i32([v[2] for v in views]), K, B,
                                                    self.cfg.n_classes, OH, OW, labels.data_ptr(), capi.ptr(conf), capi.ptr(probs),
                                                    scratch.data_ptr(), self._stream()))
        own = next((i * (2 if flip else 1) for i, s in enumerate(scales) if float(s) == 1.0), 0)
        return labels, conf, probs, logps[own]

    @torch.no_grad()
    def segment_multiscale(self, x: torch.Tensor, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip: bool = True, size=None,
                           want_conf: bool = False, want_probs: bool = False):
        """The multi-scale + horizontal-flip ensemble (the evaluation protocol of ADE20K / COCO-Stuff / Pascal-Context segmenters):
        uint8 [B,H,W,3] or fp32 [B,3,H,W] frames -> (labels int32 [B,OH,OW], conf fp32 [B,OH,OW] or None, probs fp32 [B,C,OH,OW] or
        None).  The model runs on the frame at every scale (``view_sizes``: sizes rounded to the patch; a view at the frame's own
        size is the frame itself, fp32 frames are resized by ``F.interpolate(..., mode="bilinear", align_corners=False)``, uint8
        frames by ``dinoseg_op_resize_u8``) and, with ``flip``, on its mirror image (``torch.flip`` on the width axis); views are
        ordered scale-major, the unflipped one first; at most 12.  One fused launch then interpolates every view's log-probs to
        ``size`` (default (H, W)) -- a mirrored view's grid is flipped back first --, softmaxes each view, adds the probabilities
        in view order and takes the first maximum per pixel: ``labels``, ``conf`` = the mean probability of that label, ``probs``
        = the mean probabilities.  No [B,C,OH,OW] tensor exists unless ``want_probs``; the transient is one fp32 per view and pixel
        plus the views' low-res log-probs.  A view whose grid exceeds ``size`` raises ``ValueError`` before any forward runs.
        Inference only.

        The library keeps one resampled position embedding and one workspace size, so every change of resolution between views
        re-derives them: the views run in a fixed order with each size visited once (the flipped view right after the
        unflipped one).  Measured (``tools/ensemble_cost.py``, ViT-S/8 x12 @480, batch 8, fp16): the K forwards in this order
        against the same forwards each repeated at its own resolution differ by -1.0 .. +0.4 ms of 17 (3 views) to 90 ms (12
        views) -- below what the medians resolve; the fused launch itself is 1.1 / 4.8 ms at 150 classes."""
        return self._multiscale(x, scales, flip, size, want_conf, want_probs)[:3]

    # ---- sliding-window inference at pixel resolution (csrc/windows.hip) ----
    def _windows(self, x: torch.Tensor, window, stride, want_dense: bool, max_windows: int):
        """segment_windows, also returning the windows' low-res log-probs [B*G, n, C]."""
        dev, p, C_ = self.device, self.cfg.patch, self.cfg.n_classes
        kind, B, H, W = frame_layout(x, p, non_empty=True)
        (wh, ww), (sh, sw), (gh, gw) = window_plan(p, H, W, window, stride)
        max_windows = int(max_windows)
        if max_windows < 1:
            raise ValueError(f"max_windows must be positive, got {max_windows}")
        self._require_gpu()
        x = self._to_device(x, kind)
        self._sync_weights()
        lib, total, n = capi.lib(), B * gh * gw, (wh // p) * (ww // p)
        logp = torch.empty((total, n, C_), dtype=torch.float32, device=dev)
        for first in range(0, total, max_windows):      # the flattened window list in chunks, each chunk one crop + one forward
            count = min(max_windows, total - first)
            if kind == capi.INPUT_U8_HWC:
                crop = torch.empty((count, wh, ww, 3), dtype=torch.uint8, device=dev)
            else:
                crop = torch.empty((count, 3, wh, ww), dtype=torch.float32, device=dev)
            capi.check(lib.dinoseg_op_crop_windows(x.data_ptr(), kind, B, H, W, wh, ww, sh, sw, first, count, crop.data_ptr(),
                                                   self._stream()))
            capi.check(lib.dinoseg_forward_hw(self._handle, crop.data_ptr(), kind, count, wh, ww,
                                              logp.data_ptr() + 4 * first * n * C_, None, -1, None, self._stream()))
        del crop
        labels, dense = self._alloc_out(B, H, W, want_dense)
        capi.check(lib.dinoseg_op_window_merge(logp.data_ptr(), B, H, W, p, wh, ww, sh, sw, C_, labels.data_ptr(), capi.ptr(dense),
                                               self._stream()))
        return labels, dense, logp

    @torch.no_grad()
    def segment_windows(self, x: torch.Tensor, window=(480, 480), stride=None, want_logp: bool = False, max_windows: int = 32):
        """Sliding-window inference (mmsegmentation's ``mode='slide'``): uint8 [B,H,W,3] or fp32 [B,3,H,W] frames of ANY
        ``H, W >= patch`` -> (labels int32 [B,H,W], dense fp32 [B,C,H,W] or None).  The frame is cut into windows of ``window``
        pixels (an integer or (rows, cols), multiples of the patch; clamped per axis to the largest patch multiple inside the
        frame) at ``stride`` (default ``(2 * window) // 3`` per axis: 480 -> 320) by the rule of ``window_origins`` -- the last
        row and column of windows are shifted back to end at the frame's edge, so the frame itself is never resized.  The
        flattened window list (frame-major, then row-major) is cropped and run through the forward in chunks of at most
        ``max_windows`` windows; one fused launch then interpolates every window's log-probs to pixel resolution, averages them
        where windows overlap (fp32 adds in window order, divided by the count) and takes the first maximum per pixel.
        ``want_logp=True`` also returns those mean log-probabilities.  No [B,C,H,W] tensor exists otherwise: the transient is the
        windows' low-res log-probs and one chunk of cropped windows.  A window or stride that is not positive, a window that is
        not a patch multiple, and more than 4 windows over one pixel row or column (any stride >= window / 3 is fine) raise
        ``ValueError`` before any forward runs.  Inference only."""
        return self._windows(x, window, stride, want_logp, max_windows)[:2]

    # ---- video label propagation from patch features (csrc/propagate.hip) ----
    @torch.no_grad()
    def propagate(self, frames: torch.Tensor, first: torch.Tensor, n_classes: Optional[int] = None, n_context: int = 7,
                  radius: Optional[int] = 12, topk: int = 5, temperature: float = 0.1, size=None, n_blocks: int = 0,
                  chunk: int = 32, want_seg: bool = False):
        """Label propagation through a clip (the semi-supervised video segmentation protocol of the DINO paper): ``frames`` uint8
        [T,H,W,3] or fp32 [T,3,H,W], ``first`` the labels of frame 0 -> (labels int32 [T,OH,OW], seg fp32 [T,n,C] or None).
        ``first`` is either integer pixel labels [OH0, OW0] (any size at least the patch grid; ``n_classes`` required; a label
        outside [0, n_classes) such as 255 counts for no class) or a soft fp32 [n, C] map over the patch grid, for instance
        ``exp(forward(x0))``; C is independent of the model's head, and no head weight is used.  Every cell of frame t >= 1 takes
        the ``topk`` most similar cells (cosine of the final-norm patch tokens after ``n_blocks`` blocks, 0 = all) within
        ``radius`` cells of itself (``None``: the whole frame) over frame 0 and the ``n_context`` frames before t, and averages
        their soft label rows with weights ``exp((s - s_max) / temperature)``; that soft map is frame t's context entry, and its
        bilinear enlargement to ``size`` (default the frames' own) with the first maximum gives the frame's labels (the rule:
        include/dinoseg.h, dinoseg_op_propagate).  The [n_context, n, n] affinity is never formed.  The backbone runs in batches
        of ``chunk`` frames; only the small propagate launches are sequential.  ``LabelPropagator`` is the streaming form.
        Inference only."""
        plan = propagate_plan(self.cfg.patch, frames, first, n_classes, n_context, radius, topk, temperature, size, chunk)
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._require_gpu()
        x = self._to_device(frames, plan.kind)
        runner = _PropagateRunner(self, plan)
        labels = torch.empty((plan.T, plan.OH, plan.OW), dtype=torch.int32, device=self.device)
        seg = torch.empty((plan.T, plan.hp * plan.wp, plan.C), dtype=torch.float32, device=self.device) if want_seg else None
        for c0 in range(0, plan.T, plan.chunk):
            tokens = self.features(x[c0:c0 + plan.chunk], n_blocks)
            for i in range(tokens.shape[0]):
                t = c0 + i
                seg_t = runner.seed(tokens[i:i + 1], first, labels[t]) if t == 0 else runner.step(tokens[i:i + 1], labels[t])
                if want_seg:
                    seg[t].copy_(seg_t)
        return labels, seg

    # ---- few-shot segmentation: k-NN label retrieval from a memory bank (csrc/knn.hip) ----
    @torch.no_grad()
    def segment_knn(self, x: torch.Tensor, bank: "MemoryBank", topk: int = 10, temperature: float = 0.1, size=None, chunk: int = 32,
                    want_seg: bool = False, want_idx: bool = False, n_blocks: Optional[int] = None) -> "KnnResult":
        """Few-shot segmentation by nearest neighbours in a ``MemoryBank`` of labelled patch features (the k-NN evaluation of the
        DINO paper made dense; the in-context protocol of Hummingbird): ``x`` uint8 [B,H,W,3] or fp32 [B,3,H,W], H and W multiples
        of the patch size -> ``KnnResult(labels int32 [B,OH,OW], seg fp32 [B,n,C] or None, idx int32 [B,n,k] or None)``.  Every
        cell takes the ``topk`` most similar live rows of the bank (cosine of the final-norm patch tokens after the bank's
        ``n_blocks`` blocks; the lower row on an exact tie) and averages their labels with weights ``exp((s - s_max) /
        temperature)`` (the rule: include/dinoseg.h, dinoseg_op_knn_labels); the bilinear enlargement of that soft map to ``size``
        (default the frames' own) with the first maximum gives ``labels``.  The [B n, M] score matrix is never formed.  The
        backbone runs in batches of ``chunk`` frames, each followed by one operator call and one enlargement; ``B = 1`` is the
        camera's streaming form.  ``n_blocks``, when given, must be the bank's.  A bank built with ``project`` has its
        ``FeaturePCA`` applied to the tokens (``dinoseg_op_pca_project``) before they are normalised, and the search runs at the
        projection's width.  No training and no head weight: a row added to the bank takes effect in the next call.  Inference
        only."""
        if not isinstance(bank, MemoryBank):
            raise ValueError(f"bank must be a MemoryBank, got {type(bank).__name__}")
        plan = knn_plan(self.cfg.patch, self.cfg.embed_dim, x, bank.size, bank.dim, bank.n_classes, bank.n_blocks, n_blocks, topk,
                        temperature, size, chunk, bank.project)
        self._require_gpu()
        x = self._to_device(x, plan.kind)
        lib, n, D, k = capi.lib(), plan.hp * plan.wp, bank.dim, plan.topk
        labels = torch.empty((plan.B, plan.OH, plan.OW), dtype=torch.int32, device=self.device)
        seg = torch.empty((plan.B if want_seg else min(plan.chunk, plan.B), n, plan.C), dtype=torch.float32, device=self.device)
        idx = torch.empty((plan.B, n, k), dtype=torch.int32, device=self.device) if want_idx else None
        planes = torch.empty((min(plan.chunk, plan.B), 2, n, D), dtype=torch.float16, device=self.device)
        scratch = None
        for c0 in range(0, plan.B, plan.chunk):
            tokens = bank._rows(self.features(x[c0:c0 + plan.chunk], plan.n_blocks), n)
            Bc = tokens.shape[0]
            nbytes = lib.dinoseg_knn_scratch_bytes(Bc * n, plan.M, k, 0)
            if nbytes < 0:
                raise capi.DinosegError(f"dinoseg_knn_scratch_bytes refused N = {Bc * n}, M = {plan.M}, k = {k}")
            if scratch is None or scratch.numel() < nbytes:
                scratch = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            seg_c = seg[c0:c0 + Bc] if want_seg else seg[:Bc]
            capi.check(lib.dinoseg_op_normalize_tokens(tokens.data_ptr(), Bc, n, D, planes.data_ptr(), self._stream()))
            capi.check(lib.dinoseg_op_knn_labels(planes.data_ptr(), Bc, n, bank.planes.data_ptr(), plan.M, bank.capacity,
                                                 bank.labels.data_ptr(), 1 if bank.hard else 0, D, plan.C, k, plan.temperature, 0,
                                                 seg_c.data_ptr(), capi.ptr(idx[c0:] if want_idx else None), None, scratch.data_ptr(),
                                                 self._stream()))
            capi.check(lib.dinoseg_op_upsample_argmax(seg_c.data_ptr(), Bc, plan.hp, plan.wp, plan.C, plan.OH, plan.OW,
                                                      labels[c0:].data_ptr(), None, self._stream()))
        return KnnResult(labels, seg if want_seg else None, idx)

    # ---- PCA of patch features: moments, projection, colour map (csrc/pca.hip; the solve: pca.py) ----
    @torch.no_grad()
    def pca_fit(self, x: torch.Tensor, q: int = 3, keep: Optional[torch.Tensor] = None, n_blocks: int = 0, chunk: int = 32) -> FeaturePCA:
        """The PCA of the patch features of ``x`` (uint8 [B,H,W,3] or fp32 [B,3,H,W], H and W multiples of the patch size): the
        ``q`` leading components of the final-norm patch tokens after ``n_blocks`` blocks (0 = all), over the cells ``keep`` (bool /
        uint8 [B, n]) keeps -> ``FeaturePCA``.  Exactly one ``PCAFitter`` fed ``x`` in batches of ``chunk`` frames: the moments
        are accumulated on the device (``dinoseg_op_token_moments``), the [D, D] eigen-problem is solved on the host
        (``pca_solve``).  Nothing of the size of the features leaves the device.  Inference only."""
        pca_plan(self.cfg.patch, self.cfg.embed_dim, self.cfg.n_blocks, x, q, keep, n_blocks, chunk)
        fitter = PCAFitter(self, n_blocks)
        fitter.update(x, keep, chunk)
        return fitter.solve(q)

    def _pca_components(self, x: torch.Tensor, plan, pca: FeaturePCA, whiten: bool) -> torch.Tensor:
        """The projection of every frame in the token layout fp32 [B, 1 + n, q] (the CLS rows zero): the backbone in batches of 32
        frames, each projected into its slice of one buffer."""
        n = plan.hp * plan.wp
        mean, basis, scale = pca.on(self.device)
        out = torch.empty((plan.B, n + 1, pca.q), dtype=torch.float32, device=self.device)
        for c0 in range(0, plan.B, 32):
            tokens = self.features(x[c0:c0 + 32], plan.n_blocks)
            capi.check(capi.lib().dinoseg_op_pca_project(tokens.data_ptr(), tokens.shape[0], n, pca.dim, mean.data_ptr(), basis.data_ptr(),
                                                         scale.data_ptr() if whiten else None, pca.q, out[c0:].data_ptr(),
                                                         self._stream()))
        return out

    @torch.no_grad()
    def pca_project(self, x: torch.Tensor, pca: FeaturePCA, whiten: bool = False, n_blocks: Optional[int] = None) -> torch.Tensor:
        """The patch features of ``x`` projected onto a fitted ``FeaturePCA``: fp32 [B, n, q], ``(f - mean) @ basis.T`` in fp32
        (the rule: include/dinoseg.h, dinoseg_op_pca_project), divided by the components' standard deviations with ``whiten``.  The
        result is a view past the zero CLS rows of the token layout [B, 1 + n, q].  ``n_blocks``, when given, must be the
        projection's.  Inference only."""
        plan = pca_plan(self.cfg.patch, self.cfg.embed_dim, self.cfg.n_blocks, x, n_blocks=n_blocks, pca=pca)
        self._require_gpu()
        return self._pca_components(self._to_device(x, plan.kind), plan, pca, bool(whiten))[:, 1:]

    @torch.no_grad()
    def pca_map(self, x: torch.Tensor, pca: FeaturePCA, size=None, keep: Optional[torch.Tensor] = None, lo=None, hi=None) -> torch.Tensor:
        """The three-colour map of the first three components (the DINO / DINOv2 figure): uint8 [B, OH, OW, 3], ``size`` default
        the frames' own.  Per component ``t = (v - lo) / (hi - lo)`` is enlarged bilinearly, clamped to [0, 1] and rounded to a
        byte in one launch (the rule: include/dinoseg.h, dinoseg_op_pca_colour); a pixel whose nearest cell ``keep`` (bool / uint8
        [B, n]) drops is black.  ``lo`` / ``hi`` ``None`` take the call's minimum / maximum of each component over the kept cells
        (the demo's behaviour: one reduction over [B, n, 3]); a camera passes fixed numbers (one, or three) for colours that stay
        stable over time.  The scale is ``1 / (hi - lo)`` in fp32, and 0 -- a channel of zeros -- where ``hi <= lo``.
        Inference only."""
        plan = pca_plan(self.cfg.patch, self.cfg.embed_dim, self.cfg.n_blocks, x, keep=keep, n_blocks=None, pca=pca, size=size, lo=lo, hi=hi, colour=True)
        self._require_gpu()
        comps = self._pca_components(self._to_device(x, plan.kind), plan, pca, False)
        keep_u8 = None if keep is None else keep.to(device=self.device, dtype=torch.uint8).contiguous()
        lo_t, inv_t = self._pca_range(comps, keep_u8, plan.lo, plan.hi)
        rgb = torch.empty((plan.B, plan.OH, plan.OW, 3), dtype=torch.uint8, device=self.device)
        capi.check(capi.lib().dinoseg_op_pca_colour(comps.data_ptr(), plan.B, plan.hp, plan.wp, pca.q, lo_t.data_ptr(), inv_t.data_ptr(),
                                                    capi.ptr(keep_u8), plan.OH, plan.OW, rgb.data_ptr(), self._stream()))
        return rgb

    def _pca_range(self, comps: torch.Tensor, keep_u8: Optional[torch.Tensor], lo, hi):
        """(lo, inv) fp32 [3] on the device for ``dinoseg_op_pca_colour``: the given numbers, or the minimum / maximum of components
        0 .. 2 over the kept cells; ``inv = 1 / (hi - lo)`` in fp32, 0 where ``hi <= lo`` or nothing is kept."""
        if lo is None or hi is None:
            v = comps[:, 1:, :3]
            if keep_u8 is not None:
                kept = keep_u8.bool().unsqueeze(-1)
                v_lo, v_hi = torch.where(kept, v, float("inf")), torch.where(kept, v, float("-inf"))
            else:
                v_lo = v_hi = v
        lo_t = v_lo.amin(dim=(0, 1)) if lo is None else torch.tensor(lo, dtype=torch.float32, device=self.device)
        hi_t = v_hi.amax(dim=(0, 1)) if hi is None else torch.tensor(hi, dtype=torch.float32, device=self.device)
        span = hi_t - lo_t
        ok = torch.isfinite(span) & (span > 0) & torch.isfinite(lo_t)
        return torch.where(ok, lo_t, 0.0).contiguous(), torch.where(ok, 1.0 / span, 0.0).contiguous()

    # ---- unsupervised segmentation: spherical k-means over patch features (csrc/kmeans.hip) ----
    def _point_planes(self, x: torch.Tensor, plan, n_blocks: int) -> torch.Tensor:
        """The unit patch rows of every frame as fp16 hi + lo planes [B, 2, n, D]: the backbone in batches of ``plan.chunk``, each
        batch normalised into its slice of one buffer."""
        n, D = plan.hp * plan.wp, self.cfg.embed_dim
        planes = torch.empty((plan.B, 2, n, D), dtype=torch.float16, device=self.device)
        for c0 in range(0, plan.B, plan.chunk):
            tokens = self.features(x[c0:c0 + plan.chunk], n_blocks)
            capi.check(capi.lib().dinoseg_op_normalize_tokens(tokens.data_ptr(), tokens.shape[0], n, D, planes[c0:].data_ptr(),
                                                              self._stream()))
        return planes

    def _cluster_labels(self, scores: torch.Tensor, plan) -> torch.Tensor:
        labels = torch.empty((plan.B, plan.OH, plan.OW), dtype=torch.int32, device=self.device)
        capi.check(capi.lib().dinoseg_op_upsample_argmax(scores.data_ptr(), plan.B, plan.hp, plan.wp, plan.k, plan.OH, plan.OW,
                                                         labels.data_ptr(), None, self._stream()))
        return labels

    @torch.no_grad()
    def cluster(self, x: torch.Tensor, k: int, iters: int = 10, init="sample", seed: int = 0, n_init: int = 1, size=None,
                n_blocks: int = 0, chunk: int = 32, want_scores: bool = False) -> "ClusterResult":
        """Unsupervised segmentation: spherical k-means over the patch tokens of a batch or clip (the k-means baseline of STEGO and
        of "Deep ViT Features as Dense Visual Descriptors").  ``x`` uint8 [B,H,W,3] or fp32 [B,3,H,W], H and W multiples of the
        patch size -> ``ClusterResult(labels int32 [B,OH,OW], centroids fp32 [k,D], counts int32 [k], objective fp32 [iters+1],
        moved int32 [iters+1], scores fp32 [B,n,k] or None)``.  All B n cells are clustered jointly, so a cluster id means the same
        thing in every frame.  Every cell goes to the centroid with the largest cosine (the lowest id on an exact tie); a centroid
        becomes the unit row of the sum of its cells; an empty cluster keeps its centroid (the rule: include/dinoseg.h,
        dinoseg_op_kmeans_assign).  ``init="sample"`` starts from ``k`` distinct cells drawn on the host from ``seed``; an fp32
        [k, D] tensor starts from its rows, normalised.  ``iters`` (assign, update) pairs run without a host synchronisation and
        without an early stop, then one final assignment against the final centroids gives the scores whose bilinear enlargement
        to ``size`` (default the frames' own) with the first maximum is ``labels``; ``iters=0`` labels by the initial centroids.
        ``objective[t]`` is the sum of the cells' best cosines in pass t, ``moved[t]`` the number of cells that changed cluster
        (all of them in pass 0), ``counts`` the cluster sizes of the last update (zeros for ``iters=0``).  With ``n_init > 1`` the
        runs use seeds ``seed, seed + 1, ...`` and the one with the largest final objective wins (the first on a tie).  No head
        weight is used.  Inference only."""
        plan = kmeans_plan(self.cfg.patch, self.cfg.embed_dim, x, k, iters, init, seed, n_init, size, chunk)
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._require_gpu()
        planes = self._point_planes(self._to_device(x, plan.kind), plan, n_blocks)
        runner = _KMeansRunner(self, plan, planes)
        best = None
        for r in range(plan.n_init):
            if plan.init == "sample":
                idx = sample_indices(plan.N, plan.k, plan.seed + r).to(self.device)
                flat = planes.permute(0, 2, 1, 3).reshape(plan.N, 2, -1)[idx].float()        # the sampled points: (hi + lo) 2^-10
                rows = ((flat[:, 0] + flat[:, 1]) * 2.0 ** -10).contiguous()
            else:
                rows = init.to(device=self.device, dtype=torch.float32).contiguous()
            run = runner.run(rows)
            final = float(run.objective[-1])                                                 # the run's one read of its records
            if best is None or final > best[0]:
                best = (final, run)
        run = best[1]
        labels = self._cluster_labels(run.scores, plan)
        scores = run.scores.view(plan.B, plan.hp * plan.wp, plan.k) if want_scores else None
        return ClusterResult(labels, run.centroids, run.counts, run.objective, run.moved, scores)

    @torch.no_grad()
    def assign_clusters(self, x: torch.Tensor, centroids: torch.Tensor, size=None, n_blocks: int = 0, want_scores: bool = False):
        """The streaming form of ``cluster`` for a camera: frames ``x`` (as in ``cluster``) and unit centroids fp32 [k, D], as
        ``cluster`` returns them -> (labels int32 [B,OH,OW], scores fp32 [B,n,k] or None).  Features, normalisation, one assignment
        launch, the enlargement.  The centroids are taken as they are (not normalised again), so ``cluster``'s own centroids give
        the labels of its final pass bit for bit.  Inference only."""
        plan = kmeans_plan(self.cfg.patch, self.cfg.embed_dim, x, None, 0, centroids, 0, 1, size, max(int(x.shape[0]), 1))
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._require_gpu()
        planes = self._point_planes(self._to_device(x, plan.kind), plan, n_blocks)
        runner = _KMeansRunner(self, plan, planes)
        scores = runner.assign_only(centroids.to(device=self.device, dtype=torch.float32).contiguous())
        labels = self._cluster_labels(scores, plan)
        return labels, (scores.view(plan.B, plan.hp * plan.wp, plan.k) if want_scores else None)

    # ---- unsupervised foreground masks: normalized cut on a 1-bit patch graph (csrc/ncut.hip) ----
    @torch.no_grad()
    def ncut(self, x: torch.Tensor, tau: float = 0.2, eps: float = 1e-5, iters: int = 64, seed: int = 0, size=None, n_blocks: int = 0,
             chunk: int = 32, want_graph: bool = False, split=False) -> "NcutResult":
        """Unsupervised foreground masks: the spectral bipartition of every frame's patch-similarity graph (TokenCut, "Deep
        Spectral Methods").  ``x`` uint8 [B,H,W,3] or fp32 [B,3,H,W], H and W multiples of the patch size -> ``NcutResult(labels
        int32 [B,OH,OW] with 1 = foreground, fg uint8 [B,n], eigvec fp32 [B,n] (foreground positive), seed_cell int32 [B], rho
        fp32 [B,iters], degree int32 [B,n], graph uint64 [B,n,ceil(n/64)] or None)``.  Every frame is its own graph; frames are
        independent.  Two cells are joined when the cosine of their tokens exceeds ``tau``; a joined pair weighs 1, any other pair
        ``eps``; ``iters`` lazy power iterations with the known top vector deflated approach the second eigenvector of the
        normalised graph (``rho`` records the Rayleigh quotient of every pass; nothing stops early), started from
        ``ncut_start(n, seed)``; the cells on the side of the cell with the largest entry are the foreground, and the bilinear
        enlargement of the signed margin to ``size`` (default the frames' own) gives ``labels`` (the rule:
        include/dinoseg.h, dinoseg_op_ncut_graph).  No n x n matrix of floats is formed: the graph is n^2 bits.  No head weight is
        used.  Inference only.  ``split`` (``True``, or the rows per workgroup) deals every frame's rows to many workgroups, one launch
        per pass: the same bits in every field, a fraction of the latency, and grids of up to ``NCUT_SPLIT_MAX_CELLS`` cells (960 x
        960 at patch 8 fits) where the default stops at ``NCUT_MAX_CELLS``."""
        return self._ncut(x, tau, eps, iters, seed, size, n_blocks, chunk, want_graph, split)[0]

    def _ncut(self, x, tau, eps, iters, seed, size, n_blocks, chunk, want_graph, split):
        """``ncut`` -> (its result, the signed margin fp32 [B, n] its labels were formed from, the plan)"""
        plan = ncut_plan(self.cfg.patch, x, tau, eps, iters, seed, size, chunk, split)
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._require_gpu()
        lib, dev, B, n, D = capi.lib(), self.device, plan.B, plan.hp * plan.wp, self.cfg.embed_dim
        planes = self._point_planes(self._to_device(x, plan.kind), plan, n_blocks)
        graph_bytes, graph_op = ((lib.dinoseg_ncut_split_graph_bytes, lib.dinoseg_op_ncut_graph_split) if plan.split else
                                 (lib.dinoseg_ncut_graph_bytes, lib.dinoseg_op_ncut_graph))
        nbytes = graph_bytes(B, n)
        if nbytes < 0:
            raise capi.DinosegError(f"dinoseg_ncut_graph_bytes refused {B} frames of {n} cells")
        graph = torch.empty((B, n, nbytes // (8 * B * n)), dtype=torch.int64, device=dev)
        degree = torch.empty((B, n), dtype=torch.int32, device=dev)
        capi.check(graph_op(planes.data_ptr(), B, n, D, plan.tau, graph.data_ptr(), degree.data_ptr(), self._stream()))
        z = ncut_start(n, plan.seed).to(dev).expand(B, n).contiguous()
        rho = torch.empty((B, plan.iters), dtype=torch.float32, device=dev)
        fg = torch.empty((B, n), dtype=torch.uint8, device=dev)
        eigvec = torch.empty((B, n), dtype=torch.float32, device=dev)
        margin = torch.empty((B, n), dtype=torch.float32, device=dev)
        seed_cell = torch.empty((B,), dtype=torch.int32, device=dev)
        if plan.split:
            scratch = torch.empty((lib.dinoseg_ncut_split_scratch_bytes(B, n),), dtype=torch.uint8, device=dev)
            capi.check(lib.dinoseg_op_ncut_iterate_split(graph.data_ptr(), degree.data_ptr(), B, n, plan.eps, z.data_ptr(), plan.iters,
                                                         max(plan.split, 0), z.data_ptr(), rho.data_ptr() if plan.iters else None,
                                                         fg.data_ptr(), eigvec.data_ptr(), margin.data_ptr(), seed_cell.data_ptr(),
                                                         scratch.data_ptr(), self._stream()))
        else:
            capi.check(lib.dinoseg_op_ncut_iterate(graph.data_ptr(), degree.data_ptr(), B, n, plan.eps, z.data_ptr(), plan.iters,
                                                   z.data_ptr(), rho.data_ptr() if plan.iters else None, fg.data_ptr(), eigvec.data_ptr(),
                                                   margin.data_ptr(), seed_cell.data_ptr(), self._stream()))
        labels = self._margin_labels(margin, plan.hp, plan.wp, plan.OH, plan.OW)
        return NcutResult(labels, fg, eigvec, seed_cell, rho, degree, graph.view(torch.uint64) if want_graph else None), margin, plan

    def _margin_labels(self, margin: torch.Tensor, hp: int, wp: int, OH: int, OW: int) -> torch.Tensor:
        """Pixel labels int32 [B, OH, OW] of a signed cell margin fp32 [B, hp wp]: the bilinear enlargement of the two-class map
        (0, margin) with the first maximum (ties go to background)."""
        B = margin.shape[0]
        two = torch.stack((torch.zeros_like(margin), margin), dim=2).contiguous()      # the two-class map [B, n, 2] = (0, margin)
        labels = torch.empty((B, OH, OW), dtype=torch.int32, device=self.device)
        capi.check(capi.lib().dinoseg_op_upsample_argmax(two.data_ptr(), B, hp, wp, 2, OH, OW, labels.data_ptr(), None, self._stream()))
        return labels

    # ---- connected components of a label map and their object table (csrc/components.hip) ----
    @torch.no_grad()
    def components(self, labels: torch.Tensor, connectivity: int = 4, ignore=None, max_objects: int = 256) -> "ComponentsResult":
        """Objects of a label map: its connected components, numbered in raster order of their first pixels, and per component
        the first pixel, the label, the area and the box.  ``labels``: a map [B,H,W] or [H,W] (taken as one frame) of any integer
        dtype whose values fit int32, on the device or on the host -- the ``labels`` of ``segment*``, ``cluster`` and ``ncut`` as
        they come -> ``ComponentsResult(ids int32 [B,H,W], count int32 [B], first int32 [B,M], label int32 [B,M], area int32
        [B,M], box int32 [B,M,4])`` with M = ``max_objects``.  A pixel is void (id -1) when its label is negative or equals
        ``ignore``; two pixels belong together when a path of 4-neighbours (``connectivity=8``: 8-neighbours) of one label joins
        them.  ``count`` is the true number of components, however large; the table describes the first ``min(count, M)`` of them
        (``box`` = (x0, y0, x1, y1), half-open) and holds first = label = -1, area = 0, box = 0 behind them (the rule:
        include/dinoseg.h, dinoseg_op_components).  The conversion to int32 and the copy to the device are torch's; nothing
        synchronises with the host.  Inference only."""
        plan = components_plan(labels, connectivity, ignore, max_objects)
        self._require_gpu()
        lib, dev, B, H, W, M = capi.lib(), self.device, plan.B, plan.H, plan.W, plan.max_objects
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        nbytes = lib.dinoseg_components_scratch_bytes(B, H, W)
        if nbytes < 0:
            raise capi.DinosegError(f"dinoseg_components_scratch_bytes refused {B} frames of {H} x {W}")
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
        count, status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2))
        first, label, area = (torch.empty((B, M), dtype=torch.int32, device=dev) for _ in range(3))
        box = torch.empty((B, M, 4), dtype=torch.int32, device=dev)
        capi.check(lib.dinoseg_op_components(lab.data_ptr(), B, H, W, plan.connectivity, plan.ignore, M, ids.data_ptr(), count.data_ptr(),
                                             first.data_ptr(), label.data_ptr(), area.data_ptr(), box.data_ptr(), status.data_ptr(),
                                             scratch.data_ptr(), self._stream()))
        return ComponentsResult(ids, count, first, label, area, box)

    @torch.no_grad()
    def discover(self, x: torch.Tensor, tau: float = 0.2, eps: float = 1e-5, iters: int = 64, seed: int = 0, size=None, n_blocks: int = 0,
                 chunk: int = 32, split=True, connectivity: int = 4) -> "DiscoverResult":
        """Unsupervised single-object discovery (TokenCut's ``detect_box``): ``ncut``, then the connected component of the
        foreground cells that holds the seed cell, its box and its mask.  Arguments as ``ncut`` -> ``DiscoverResult(labels int32
        [B,OH,OW] with 1 = the object, box int32 [B,4] = (x0, y0, x1, y1) half-open in the coordinates of the frame (H, W) whatever
        ``size`` is, found uint8 [B], cells uint8 [B,n], area int32 [B] in cells, ncut NcutResult)``.  ``cells`` is the component
        of ``ncut.fg`` on the patch grid (``connectivity=4``, scipy.ndimage.label's default, as TokenCut has it) around
        ``ncut.seed_cell``; ``box`` is the component's cell box times the patch size; ``labels`` is the enlargement of the margin
        with every cell outside ``cells`` pushed to the background side.  ``found`` is 0 where the seed cell itself is background
        (a one-cell grid, a constant vector): then ``cells`` is empty and ``box`` and ``area`` are 0.  No host synchronisation.
        Inference only."""
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
        res, margin, plan = self._ncut(x, tau, eps, iters, seed, size, n_blocks, chunk, False, split)
        return DiscoverResult(*self._discover_from(margin, res.fg, res.seed_cell, plan.hp, plan.wp, plan.OH, plan.OW, connectivity), res)

    def _discover_from(self, margin: torch.Tensor, fg: torch.Tensor, seed_cell: torch.Tensor, hp: int, wp: int, OH: int, OW: int,
                       connectivity: int = 4):
        """``discover`` from the cut on: (margin fp32 [B,n], fg uint8 [B,n], seed_cell int32 [B]) on the device -> (labels, box,
        found, cells, area)."""
        B, n, p = fg.shape[0], hp * wp, self.cfg.patch
        comp = self.components(fg.view(B, hp, wp), connectivity, ignore=0, max_objects=n)
        at = seed_cell.to(torch.int64).view(B, 1)
        k = torch.gather(comp.ids.view(B, n), 1, at)                                   # the seed's component, -1 on a background seed
        found = torch.gather(fg, 1, at).view(B)
        cells = (comp.ids.view(B, n) == k) & (k >= 0)
        row = k.clamp(min=0)
        hit = (k >= 0).view(B)
        box = torch.gather(comp.box, 1, row.view(B, 1, 1).expand(B, 1, 4)).view(B, 4) * p
        box = torch.where(hit.view(B, 1), box, torch.zeros_like(box))
        area = torch.where(hit, torch.gather(comp.area, 1, row).view(B), torch.zeros_like(comp.count))
        labels = self._margin_labels(torch.where(cells, margin, -margin.abs()), hp, wp, OH, OW)
        return labels, box, found, cells.to(torch.uint8), area

    # ---- multi-object discovery: recursive normalized cuts (csrc/maskcut.hip) ----
    @torch.no_grad()
    def discover_all(self, x: torch.Tensor, max_objects: int = 3, tau: float = 0.2, eps: float = 1e-5, iters: int = 64, seed: int = 0,
                     size=None, n_blocks: int = 0, chunk: int = 32, split=True, connectivity: int = 4,
                     want_graph: bool = False) -> "MaskCutResult":
        """Unsupervised multi-object discovery (MaskCut, the discovery step of CutLER): K = ``max_objects`` rounds of ``discover``
        on one graph, the cells of every found object painted out of the graph before the next cut.  Arguments as ``discover`` ->
        ``MaskCutResult(labels int32 [B,OH,OW] with 0 = background and t + 1 = the object of round t, count int32 [B], found uint8
        [B,K], box int32 [B,K,4] = (x0, y0, x1, y1) half-open in the coordinates of the frame, area int32 [B,K] in cells, cells
        uint8 [B,K,n], seed_cell int32 [B,K], rho fp32 [B,K,iters], graph uint64 [B,n,ceil(n/64)] or None)``.  Round 0 is
        ``discover(split=True)``.  A painted cell stays in the graph as a node joined to nothing (every pair with it weighs ``eps``);
        every round starts from ``ncut_start(n, seed)``; a round whose seed cell is background or already painted finds nothing
        (``found`` 0, empty ``cells``, ``box`` and ``area`` 0) and, since nothing stops early, every later round repeats it; ``count``
        is the number of rounds that found an object (the rule: include/dinoseg.h, dinoseg_op_maskcut).  The rounds run on the split
        launches only: ``split=False`` raises ``ValueError``.  ``want_graph`` returns the ORIGINAL graph (a copy: the rounds consume
        theirs).  MaskCut's corner reversal, its IoU and area rejections and its CRF are not done.  No host synchronisation.
        Inference only."""
        mplan = maskcut_plan(self.cfg.patch, x, max_objects, tau, eps, iters, seed, size, chunk, split, connectivity)
        plan, K = mplan.ncut, mplan.max_objects
        if not 0 <= n_blocks <= self.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {self.cfg.n_blocks}]")
        self._require_gpu()
        lib, dev, B, n, D = capi.lib(), self.device, plan.B, plan.hp * plan.wp, self.cfg.embed_dim
        planes = self._point_planes(self._to_device(x, plan.kind), plan, n_blocks)
        nbytes, sbytes = lib.dinoseg_ncut_split_graph_bytes(B, n), lib.dinoseg_maskcut_scratch_bytes(B, plan.hp, plan.wp, K)
        if nbytes < 0 or sbytes < 0:
            raise capi.DinosegError(f"dinoseg_maskcut_scratch_bytes refused {B} frames of {plan.hp} x {plan.wp} cells")
        graph = torch.empty((B, n, nbytes // (8 * B * n)), dtype=torch.int64, device=dev)
        degree = torch.empty((B, n), dtype=torch.int32, device=dev)
        capi.check(lib.dinoseg_op_ncut_graph_split(planes.data_ptr(), B, n, D, plan.tau, graph.data_ptr(), degree.data_ptr(), self._stream()))
        original = graph.clone().view(torch.uint64) if want_graph else None
        z = ncut_start(n, plan.seed).to(dev).expand(B, n).contiguous()
        scratch = torch.empty((sbytes,), dtype=torch.uint8, device=dev)
        cells, fg = (torch.empty((B, K, n), dtype=torch.uint8, device=dev) for _ in range(2))
        margin, eigvec = (torch.empty((B, K, n), dtype=torch.float32, device=dev) for _ in range(2))
        found = torch.empty((B, K), dtype=torch.uint8, device=dev)
        area, seed_cell = (torch.empty((B, K), dtype=torch.int32, device=dev) for _ in range(2))
        box = torch.empty((B, K, 4), dtype=torch.int32, device=dev)
        score = torch.empty((B, n, K + 1), dtype=torch.float32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        rho = torch.empty((B, K, plan.iters), dtype=torch.float32, device=dev)
        capi.check(lib.dinoseg_op_maskcut(graph.data_ptr(), degree.data_ptr(), B, plan.hp, plan.wp, plan.eps, z.data_ptr(), plan.iters,
                                          max(plan.split, 0), mplan.connectivity, K, cells.data_ptr(), found.data_ptr(), area.data_ptr(),
                                          box.data_ptr(), score.data_ptr(), count.data_ptr(), fg.data_ptr(), margin.data_ptr(),
                                          eigvec.data_ptr(), seed_cell.data_ptr(), rho.data_ptr() if plan.iters else None,
                                          scratch.data_ptr(), self._stream()))
        labels = torch.empty((B, plan.OH, plan.OW), dtype=torch.int32, device=dev)
        capi.check(lib.dinoseg_op_upsample_argmax(score.data_ptr(), B, plan.hp, plan.wp, K + 1, plan.OH, plan.OW, labels.data_ptr(), None,
                                                  self._stream()))
        return MaskCutResult(labels, count, found, box * self.cfg.patch, area, cells, seed_cell, rho, original)

    def predict_dense(self, img, size=None, scales=None, flip: bool = False, window=None, stride=None, guided=None) -> np.ndarray:
        """The pixel-resolution sibling of ``predict()``: the image (PIL.Image or HxWx3 uint8 array) is resized to r x r on the
        device exactly as ``predict()`` does, the log-probabilities are upsampled to ``size`` (default: the IMAGE's own (rows,
        cols)) and the per-pixel argmax comes back as an int64 map.  Eager launches (``predict()`` keeps its captured graph).
        With ``scales`` the labels are those of ``segment_multiscale(resized frame, scales, flip, size)`` instead.
        With ``window`` the image is NOT resized: it is segmented at its own size by ``segment_windows(image, window, stride)``
        (``size`` other than the image's own, and ``scales``, raise ``ValueError``).
        With ``guided`` (``True`` or a dict of ``radius`` / ``sigma_spatial`` / ``sigma_range``) the log-probabilities of the
        resized frame are enlarged by ``segment_guided``'s rule instead, guided by the ORIGINAL image at its own size (resized
        only if ``size`` asks for another); ``guided`` with ``window`` or ``scales`` raises ``ValueError``."""
        mode = dense_mode(scales, flip, window, stride, guided)
        raw = self._image_u8(img)
        own, r, guide = tuple(raw.shape[:2]), self.resolution, None
        with torch.no_grad():
            frames = torch.from_numpy(raw).unsqueeze(0)
            if mode.kind == "windows":
                if size is not None and tuple(int(v) for v in size) != own:
                    raise ValueError(f"with window the image is segmented at its own size {own}, got size={tuple(size)}")
            else:
                self._require_gpu()
                size = out_size(size, own)
                frames = orig = frames.to(self.device)
                if own != (r, r):                                                # Resize(r, r) of get_transforms, on the GPU
                    frames = self._resize_view(orig, capi.INPUT_U8_HWC, r, r)
                if mode.kind == "guided":
                    guide = orig if size == own else self._resize_view(orig, capi.INPUT_U8_HWC, size[0], size[1])
            labels = self._segment_mode(frames, mode, size, guide=guide)[0]
            return labels[0].cpu().numpy().astype(np.int64)

    def _segment_mode(self, x: torch.Tensor, mode, size, want_logp: bool = False, guide: Optional[torch.Tensor] = None):
        """The one place that maps a resolved ``dense_mode`` to its runner: (labels int32 [B,OH,OW], None, low-res log-probs).
        The log-probs are those a validation step reports as "probs" (bilinear: None unless ``want_logp``, which costs that mode
        an output buffer); sliding windows keep the frames' own size whatever ``size`` says; ``guide`` is the guided mode's."""
        if mode.kind == "guided":
            return self._guided(x, guide, size, mode.args)
        if mode.kind == "windows":
            return self._windows(x, *mode.args, False, 32)
        if mode.kind == "multiscale":
            labels, _, _, logp = self._multiscale(x, *mode.args, size, False, False)
            return labels, None, logp
        return self._bilinear(x, size, want_logp=want_logp)

    @staticmethod
    def _image_u8(img) -> np.ndarray:
        """A PIL.Image or array as a contiguous uint8 HxWx3 array (``predict`` / ``predict_dense``)."""
        raw = np.asarray(img)
        if raw.dtype != np.uint8 or not raw.flags.c_contiguous:
            raw = np.ascontiguousarray(raw, dtype=np.uint8)
        if raw.ndim != 3 or raw.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {raw.shape}")
        return raw

    def _predict_graph(self, r: int):
        """The single-frame forward of ``predict()`` as a captured HIP graph (one replay instead of ~150 launches: a 12-block
        forward is 1.33 ms of kernels that the eager launch path stretches to 1.50).  Static input / output buffers; captured once
        per (resolution, bound parameter storage) -- an in-place weight update re-packs into the same library buffers before the
        replay, new parameter storage (``.to()``, ``load_state_dict`` of new tensors) re-captures.  Returns None where capture is
        not possible (``predict_graph = False``, a capture already in progress, a failed capture: eager from then on)."""
        if not getattr(self, "predict_graph", True) or torch.cuda.is_current_stream_capturing():
            return None
        cache = self.__dict__.setdefault("_pred_graphs", {})
        ent = cache.get(r)
        if ent is not None and ent["key"] == self._ptr_key and capi.lib().dinoseg_state_generation(self._handle) == ent["gen"]:
            return ent
        try:
            dev = self.device
            static_in = torch.zeros((1, r, r, 3), dtype=torch.uint8, device=dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                self.forward_frames(static_in, want_logp=False)          # warm-up: workspace, resolution cache, packs
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    _, static_out = self.forward_frames(static_in, want_logp=False)
            torch.cuda.current_stream(dev).wait_stream(side)
            ent = {"key": self._ptr_key, "graph": g, "in": static_in, "out": static_out,
                   "gen": capi.lib().dinoseg_state_generation(self._handle)}
            cache.clear()           # (one resolution at a time: the library caches one resampled position embedding)
            cache[r] = ent
            return ent
        except Exception:
            self.predict_graph = False          # (e.g. a runtime without graph support for one of the calls): eager from now on
            return None

    def predict(self, x) -> np.ndarray:
        """Run inference on a single image (PIL.Image or HxWx3 uint8 array); returns the int64 map the
        reference returns: np.kron of the (r/8)x(r/8) argmax map with a (480//(r/8))^2 block of ones
        (pl_torch_modules.py:276-300, including the non-480 sizes it yields when 480 % (r/8) != 0).  A patch-16 model follows the
        same rule with 16 in place of 8: o = r // 16, blocks of 480 // o."""
        with torch.no_grad():
            raw = self._image_u8(x)
            r = self.resolution
            self._require_gpu()
            self._sync_weights()
            ent = self._predict_graph(r)
            frames = torch.from_numpy(raw).unsqueeze(0)                           # uint8 on the wire, whatever its size
            if raw.shape[0] != r or raw.shape[1] != r:                           # Resize(r, r) of get_transforms, on the GPU
                frames = self._resize_view(frames.to(self.device), capi.INPUT_U8_HWC, r, r, out=None if ent is None else ent["in"])
            elif ent is not None:
                ent["in"].copy_(frames, non_blocking=True)
            if ent is not None:
                ent["graph"].replay()
                amax = ent["out"]
            else:
                _, amax = self.forward_frames(frames.to(self.device), want_logp=False)
            output_size = self.resolution // self.cfg.patch
            low_res = amax.cpu().numpy().astype(np.int64).reshape((output_size, output_size))
            high_res_patch_size = 480 // output_size
            # == np.kron(low_res, np.ones((k, k), dtype=int)) of the reference (:297-298), 4x cheaper on the host
            k = high_res_patch_size
            return np.repeat(np.repeat(low_res, k, axis=0), k, axis=1)

    def debug_tokens(self, x: torch.Tensor, block: int) -> torch.Tensor:
        """Token matrix [B, N, D] after prepare_tokens (block=0) or after transformer block `block`."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        _, _, tap = self._run(x, capi.INPUT_F32_CHW, x.shape[0], x.shape[2], x.shape[3], tap_block=block)
        return tap.reshape(x.shape[0], -1, self.cfg.embed_dim)

    def _mask_request(self, x: torch.Tensor, cls_mask: torch.Tensor, want_emb: bool, want_attn: bool):
        self._require_gpu()
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 3 or x.shape[2] % self.cfg.patch != 0 or x.shape[3] % self.cfg.patch != 0:
            raise ValueError(f"expected a single frame [1,3,H,W] with H % {self.cfg.patch} == W % {self.cfg.patch} == 0, got {tuple(x.shape)}")
        H, W = x.shape[2], x.shape[3]
        n = (H // self.cfg.patch) * (W // self.cfg.patch)
        m = cls_mask.to(device=self.device, dtype=torch.float32).reshape(cls_mask.shape[0], -1).contiguous()
        if m.shape[1] != n:
            raise ValueError(f"cls_mask must be [n_masks, {H // self.cfg.patch}, {W // self.cfg.patch}], got {tuple(cls_mask.shape)}")
        self._sync_weights()
        emb = torch.empty((m.shape[0], self.cfg.embed_dim), dtype=torch.float32, device=x.device) if want_emb else None
        att = torch.empty((1, self.cfg.num_heads, m.shape[0], n + 1), dtype=torch.float32, device=x.device) if want_attn else None
        capi.check(capi.lib().dinoseg_forward_mask_hw(self._handle, x.data_ptr(), capi.INPUT_F32_CHW, H, W, m.data_ptr(), m.shape[0],
                                                      capi.ptr(emb), capi.ptr(att), self._stream()))
        return emb, att

    def forward_mask(self, x: torch.Tensor, cls_mask: torch.Tensor) -> torch.Tensor:
        """One embedding per mask, [n_masks, embed_dim]: ``model.dino.forward_mask(x, cls_mask)`` of the reference
        (vision_transformer.py:250-271).  x: one frame fp32 [1,3,H,W]; cls_mask [n_masks, H/8, W/8]."""
        return self._mask_request(x, cls_mask, True, False)[0]

    def get_last_selfattention(self, x: torch.Tensor, cls_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Attention probabilities [B, heads, N, N] of the last block (reference: ``model.dino.get_last_selfattention(x)``,
        vision_transformer.py:273-280; used by visualize_attention.py:46).  x: fp32 [B,3,H,W], N = (H/8)*(W/8) + 1.  With
        cls_mask [n_masks, H/8, W/8]: the masked CLS attention [1, heads, n_masks, N] of one frame."""
        if cls_mask is not None:
            return self._mask_request(x, cls_mask, False, True)[1]
        self._require_gpu()
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % self.cfg.patch != 0 or x.shape[3] % self.cfg.patch != 0:
            raise ValueError(f"expected [B,3,H,W] with H % {self.cfg.patch} == W % {self.cfg.patch} == 0, got {tuple(x.shape)}")
        self._sync_weights()
        B, H, W = x.shape[0], x.shape[2], x.shape[3]
        N = (H // self.cfg.patch) * (W // self.cfg.patch) + 1
        out = torch.empty((B, self.cfg.num_heads, N, N), dtype=torch.float32, device=x.device)
        capi.check(capi.lib().dinoseg_last_selfattention_hw(self._handle, x.data_ptr(), capi.INPUT_F32_CHW, B, H, W, out.data_ptr(),
                                                            self._stream()))
        return out

    @torch.no_grad()
    def cls_attention(self, x: torch.Tensor, size=None, threshold: Optional[float] = None):
        """CLS attention maps of the last block at pixel resolution, ``(attn, keep)``: what the reference's visualize_attention.py
        draws, without the [B, heads, N, N] matrix of ``get_last_selfattention`` (csrc/cls_attention.hip, one launch behind the last
        block's qkv).  x: uint8 [B,H,W,3] or fp32 [B,3,H,W] frames.  ``attn`` fp32 [B, heads, OH, OW] is
        ``get_last_selfattention(x)[:, :, 0, 1:]`` on the (H/patch, W/patch) grid, enlarged to ``size = (OH, OW)`` (default the
        frames' own (H, W); any OH >= H/patch, OW >= W/patch) by nearest neighbour with exact integer coordinates -- for the default
        size ``F.interpolate(..., scale_factor=patch, mode="nearest")``, so the script's enlarged maps are ``cls_attention(x)[0]``.
        ``keep`` is None without a threshold, else uint8 [B, heads, OH, OW]: 1 where the patch is in the top ``threshold`` share of
        the patches' attention mass (0 < threshold < 1).  ``dt_utils.process_attentions(model.dino.get_last_selfattention(x),
        threshold)`` for frame 0 is ``cls_attention(x, size=(hp, wp), threshold=threshold)``: its ``keep`` when a threshold is given,
        its ``attn`` otherwise.  The threshold is the reference's sort / cumulative-sum rule in exact integers (include/dinoseg.h,
        dinoseg_op_cls_attention): a tied group is kept or dropped whole.  Inference only."""
        p = self.cfg.patch
        kind, B, H, W = frame_layout(x, p, multiple=True, one_patch=True, non_empty=True)
        hp, wp = H // p, W // p
        OH, OW = out_size(size, (H, W))
        if OH < hp or OW < wp:
            raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
        if threshold is not None:
            threshold = float(np.float32(threshold))       # the value the library sees
            if not 0.0 < threshold < 1.0:
                raise ValueError(f"threshold must be inside (0, 1), got {threshold}")
        limit = capi.lib().dinoseg_cls_attention_max_tokens()
        if hp * wp + 1 > limit:
            raise ValueError(f"a {H}x{W} frame has {hp * wp + 1} tokens, more than the {limit} one launch holds")
        self._require_gpu()
        x = self._to_device(x, kind)
        self._sync_weights()
        heads = self.cfg.num_heads
        attn = torch.empty((B, heads, OH, OW), dtype=torch.float32, device=x.device)
        keep = torch.empty((B, heads, OH, OW), dtype=torch.uint8, device=x.device) if threshold is not None else None
        capi.check(capi.lib().dinoseg_cls_attention_hw(self._handle, x.data_ptr(), kind, B, H, W, OH, OW,
                                                       0.0 if threshold is None else threshold, attn.data_ptr(), capi.ptr(keep),
                                                       self._stream()))
        return attn, keep

    # ---- validation metrics (pl_torch_modules.py:302-345) ------------------------------------------
    def validation_step(self, batch, batch_idx=0):
        """Reference: probs = self(x); pred = argmax.  Here the per-batch confusion matrix is accumulated on device."""
        x, y = batch
        with torch.no_grad():
            xx, kind, B, H, W = self._prep_batch(x)
            logp, amax, _ = self._run(xx, kind, B, H, W, want_logp=True, want_argmax=True)
            return self._score(amax, y, logp)

    def _score(self, pred: torch.Tensor, y: torch.Tensor, probs: torch.Tensor) -> dict:
        """A validation step's output: the confusion matrix of int32 predictions against the labels, counted on the device."""
        y = y.to(self.device).reshape(-1).long().contiguous()
        cm = torch.zeros((self.cfg.n_classes, self.cfg.n_classes), dtype=torch.int64, device=self.device)
        capi.check(capi.lib().dinoseg_op_confusion(pred.data_ptr(), y.data_ptr(), y.numel(), self.cfg.n_classes,
                                                   cm.data_ptr(), self._stream()))
        return {"pred": pred, "gt": y, "probs": probs, "confusion": cm}

    def validation_step_dense(self, batch, batch_idx=0, scales=None, flip: bool = False, window=None, stride=None, guided=None):
        """``validation_step`` scored per pixel: ``y`` is [B, OH, OW] pixel labels, the prediction is ``segment`` at y's size and
        the confusion matrix counts pixels.  Labels outside [0, n_classes) -- 255 or -100 "void" -- are skipped by the confusion
        kernel.  Same keys as ``validation_step`` ("pred": the pixel labels, "probs": the low-res log-probs), so
        ``validation_epoch_end`` takes its outputs unchanged.  With ``scales`` the prediction is ``segment_multiscale(x, scales,
        flip, size=y's)`` and "probs" the low-res log-probs of the unflipped scale-1.0 view (the first view's without one).
        With ``window`` the prediction is ``segment_windows(x, window, stride)`` on frames of any size, ``y`` has the frames' own
        H x W, and "probs" is the windows' low-res log-probs [B*G, n, C]; ``window`` with ``scales`` raises ``ValueError``.
        With ``guided`` (``True`` or a dict of ``radius`` / ``sigma_spatial`` / ``sigma_range``) the prediction is
        ``segment_guided(x, size=y's)`` on uint8 frames; ``guided`` with ``window`` or ``scales`` raises ``ValueError``."""
        x, y = batch
        mode = dense_mode(scales, flip, window, stride, guided)
        _, B, H, W = frame_layout(x, self.cfg.patch)
        size = label_size(y, B, own=(H, W) if mode.kind == "windows" else None)
        with torch.no_grad():
            labels, _, logp = self._segment_mode(x, mode, size, want_logp=True)
            return self._score(labels, y, logp)

    def validation_epoch_end(self, outputs, prefix="val"):
        """Balanced accuracy, macro F1 and macro IoU over all patches of the split, from the summed confusion matrices
        (same definitions as sklearn's balanced_accuracy_score / f1_score(macro) / jaccard_score(macro), which the
        reference calls on the concatenated predictions, pl_torch_modules.py:317-319)."""
        cm = torch.stack([o["confusion"] for o in outputs]).sum(0).cpu().numpy().astype(np.float64)
        return metrics_from_confusion(cm, prefix)

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, batch_idx)

    def test_epoch_end(self, outputs):
        return self.validation_epoch_end(outputs, prefix="test")

    def profile(self, level: int) -> None:
        """Per-kernel-class HIP-event timing inside forward (0 off, 1 attention only, 2 all classes)."""
        self._sync_weights()
        capi.check(capi.lib().dinoseg_profile(self._handle, int(level)))

    def profile_read(self) -> Dict[str, tuple]:
        """{class name: (summed ms, launches)} since the last read; waits for the recorded events."""
        n = len(capi.PROF_CLASSES)
        ms, cnt = (C.c_float * n)(), (C.c_int32 * n)()
        capi.check(capi.lib().dinoseg_profile_read(self._handle, ms, cnt))
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(capi.PROF_CLASSES)}

    # ---- fine-tune step --------------------------------------------------------------------------
    @staticmethod
    def grad_stage(name: str, n_blocks: int) -> int:
        """Backward stage after which the gradient of parameter `name` is final: 0 = head, 1 + k = final norm and block
        n_blocks-1-k, n_blocks + 1 = embeddings (the order dinoseg_backward produces them; see dinoseg_stream_wait_grad_stage)."""
        if name.startswith("clf."):
            return 0
        if name.startswith("dino.norm."):
            return 1 if n_blocks > 0 else 1
        if name.startswith("dino.blocks."):
            return 1 + (n_blocks - 1 - int(name.split(".")[2]))
        return n_blocks + 1

    def _grad_buckets(self, slot: str, bucket_bytes: int = 8 << 20):
        """Flat fp32 gradient buckets (dino_amd.parallel.make_flat_buckets) of the trainable parameters, cached per slot until
        the trainable set, the device or the bucket size changes."""
        from .parallel import make_flat_buckets
        params = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        key = (bucket_bytes,) + tuple((n, p.numel(), str(p.device)) for n, p in params)
        cache = self.__dict__.setdefault("_grad_bucket_cache", {})
        if slot not in cache or cache[slot]["key"] != key:
            cache[slot] = make_flat_buckets(params, lambda n: self.grad_stage(n, self.cfg.n_blocks), bucket_bytes)
            cache[slot]["key"] = key
        return cache[slot]

    def grad_buckets(self, bucket_bytes: int = 8 << 20):
        """The flat buckets behind the parameters' ``.grad`` (list of {'flat', 'names', 'stage'}, reverse registration order)."""
        self._bucket_bytes = bucket_bytes
        return self._grad_buckets("grad", bucket_bytes)["buckets"]

    def stream_wait_grad_stage(self, stage: int, stream) -> None:
        """Make `stream` (a torch.cuda.Stream on the model's device) wait for backward stage `stage` of the last step."""
        self._use(True)
        if self._handle is None:      # (precision 'auto' before any training step: no backward has recorded a stage yet -- nothing to wait for)
            return
        capi.check(capi.lib().dinoseg_stream_wait_grad_stage(self._handle, int(stage), stream.cuda_stream))

    def _sync_grads(self, slot: str = "grad") -> dict:
        """Bind the gradient buffers of every trainable parameter to the native handle; parameters with requires_grad=False are
        unbound = frozen (freeze_bb / unfreeze_bb).  slot 'grad': the buffers ARE the parameters' ``.grad`` (views into the flat
        buckets); slot 'autograd': private buffers whose contents torch.autograd receives from DINOSeg.forward's backward."""
        lib = capi.lib()
        bk = self._grad_buckets(slot, getattr(self, "_bucket_bytes", 8 << 20))
        sig = [slot]
        for name, p in self.named_parameters():
            if p.requires_grad:
                view = bk["views"][name]
                if slot == "grad" and (p.grad is None or p.grad.data_ptr() != view.data_ptr()):
                    p.grad = view
                sig.append((name, view.data_ptr()))
            else:
                sig.append((name, None))
        sig = tuple(sig)
        if sig != self._grad_sig:
            for name, ptr in sig[1:]:
                capi.check(lib.dinoseg_bind_grad(self._handle, name.encode(), ptr))
            self._grad_sig = sig
        return bk

    def _prep_batch(self, x: torch.Tensor):
        """uint8 [B,H,W,3] or fp32 [B,3,H,W] -> (contiguous tensor on the model's device, input kind, B, H, W)."""
        kind, B, H, W = frame_layout(x, self.cfg.patch, multiple=True)
        return self._to_device(x, kind), kind, B, H, W

    def _to_device(self, x: torch.Tensor, kind: int) -> torch.Tensor:
        """Frames of a checked layout as a contiguous tensor on the model's device (fp32 unless they are uint8)."""
        return x.to(device=self.device, dtype=torch.uint8 if kind == capi.INPUT_U8_HWC else torch.float32).contiguous()

    def check_labels(self) -> None:
        """Raise IndexError if a training step since the last check saw a label outside [0, n_classes) other than the
        ignore_index -100 (F.nll_loss raises at the call; here the row is skipped on device and reported on request, so the
        step stays asynchronous).  Synchronises the stream; ``fit()`` calls it once per epoch."""
        self._use(True)
        if self._handle is None:
            return
        bad = C.c_int32(0)
        capi.check(capi.lib().dinoseg_train_status(self._handle, C.byref(bad), self._stream()))
        flags = self.__dict__.get("_dense_flags")       # (training_step_dense: the loss runs outside the handle)
        if flags is not None and int(flags.item()):
            flags.zero_()
            bad.value = 1
        if bad.value:
            raise IndexError(f"Target out of bounds: labels must be in [0, {self.cfg.n_classes}) or -100 (ignore_index)")

    def training_step(self, batch, batch_idx=0):
        """The reference's step verbatim (pl_torch_modules.py:261-268): ``probs = self(x); loss = F.nll_loss(probs, y)``.
        ``loss`` carries an autograd graph whose backward runs in the native library (``loss.backward()`` ACCUMULATES into
        ``.grad`` like any torch module, so zero_grad / optimizer.step around it work unchanged, Lightning included).
        ``fused_training_step`` is the same arithmetic without the autograd round trip."""
        x, y = batch
        probs = self(x)
        y = y.to(self.device).reshape((-1,)).long()
        loss = torch.nn.functional.nll_loss(probs, y)
        return {"loss": loss, "pred": probs.argmax(dim=-1).detach(), "gt": y, "probs": probs.detach()}

    def fused_training_step(self, batch, batch_idx=0):
        """zero_grad + forward + F.nll_loss + backward in one native call (``dinoseg_train_step``): on return every trainable
        parameter's ``.grad`` holds d loss / d parameter of THIS call (overwritten), so ``fused_adam_step`` -- or any torch
        optimiser -- can follow.  x: fp32 [B,3,H,W] (normalised) or uint8 [B,H,W,3]; y: int [B, (H/8)*(W/8)] (-100 = ignored)."""
        x, y = batch
        self._require_gpu()
        self._sync_weights(train=True)
        self._sync_grads("grad")
        x, kind, B, H, W = self._prep_batch(x)
        dev = self.device
        n = (H // self.cfg.patch) * (W // self.cfg.patch)
        y = y.to(dev).reshape(-1).long().contiguous()
        if y.numel() != B * n:
            raise ValueError(f"labels must have B*(H/{self.cfg.patch})*(W/{self.cfg.patch}) = {B * n} entries, got {y.numel()}")
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        logp = torch.empty((B * n, self.cfg.n_classes), dtype=torch.float32, device=dev)
        capi.check(capi.lib().dinoseg_train_step_hw(self._handle, x.data_ptr(), kind, B, H, W, y.data_ptr(), loss.data_ptr(),
                                                    logp.data_ptr(), self._stream()))
        self._fwd_epoch = getattr(self, "_fwd_epoch", 0) + 1
        return {"loss": loss, "pred": logp.argmax(dim=-1).detach(), "gt": y, "probs": logp}

    # ---- augmentation of a training batch on the device (csrc/augment.hip; the table: dino_amd/augment.py) ----
    @torch.no_grad()
    def augment(self, x: torch.Tensor, y: Optional[torch.Tensor], table: torch.Tensor, out=None, out_kind: str = "f32",
                labels: str = "pixel"):
        """Warp, colour-jitter and blur a batch of frames, and warp their label masks, by a per-frame parameter table
        (``dino_amd.augment.augment_table`` / ``draw_reference_augment``; the rule is stated at ``dinoseg_op_augment`` in
        ``include/dinoseg.h``): one launch, or two when a frame is blurred.  ``x``: uint8 [B,H,W,3]; ``y``: None or an integer
        [B,H,W] mask (uint8 and int64 are read as they are, other integer dtypes are widened); ``table``: int32 [B,36], checked on
        the host before it is uploaded; ``out`` = (OH, OW), default the frames' own size.  Returns ``(image, labels)``: the image
        is normalised fp32 [B,3,OH,OW] (``out_kind="f32"``) or uint8 [B,OH,OW,3] (``"u8"``) -- what ``forward`` /
        ``forward_frames`` and the training steps take; the labels are int64 [B,OH,OW] (``labels="pixel"``) or int64
        [B,(OH/p)*(OW/p)] (``"patch"``: the pixel label at every patch's first pixel, the reference's nearest resize to the patch
        grid; OH and OW must then be patch multiples), or None without ``y``.  Needs the device, not the weights.  The fp32
        scratch of the blur ([B,3,OH,OW]) is allocated only when a radius is non-zero."""
        from .augment import validate_table

        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"expected uint8 [B,H,W,3] frames, got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        if B < 1 or H < 1 or W < 1:
            raise ValueError("empty batch")
        if out_kind not in ("f32", "u8"):
            raise ValueError(f"out_kind must be 'f32' or 'u8', got {out_kind!r}")
        if labels not in ("pixel", "patch"):
            raise ValueError(f"labels must be 'pixel' or 'patch', got {labels!r}")
        OH, OW = (H, W) if out is None else _pair(out, "out")
        if min(OH, OW) < 1 or max(H, W, OH, OW) > 16384:
            raise ValueError(f"frame sides must be in 1..16384 (source {H} x {W}, output {OH} x {OW})")
        if y is not None:
            if not isinstance(y, torch.Tensor) or y.is_floating_point() or y.dtype == torch.bool or tuple(y.shape) != (B, H, W):
                raise ValueError(f"expected an integer mask [B={B}, {H}, {W}], got {getattr(y, 'dtype', type(y).__name__)} "
                                 f"{tuple(getattr(y, 'shape', ()))}")
            p = self.cfg.patch
            if labels == "patch" and (OH % p != 0 or OW % p != 0):
                raise ValueError(f"labels='patch' needs an output that is a multiple of the patch ({p}), got {OH} x {OW}")
        rmax = validate_table(table, B, OH, OW)
        self._require_gpu()
        dev = self.device
        x = x.to(dev).contiguous()
        table = table.to(dev).contiguous()
        mask_kind = 0
        if y is not None:
            y = y.to(dev)
            if y.dtype != torch.uint8:
                y, mask_kind = y.long(), 1
            y = y.contiguous()
        if out_kind == "u8":
            img = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device=dev)
        else:
            img = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=dev)
        lab = None
        if y is not None:
            shape = (B, OH, OW) if labels == "pixel" else (B, (OH // self.cfg.patch) * (OW // self.cfg.patch))
            lab = torch.empty(shape, dtype=torch.int64, device=dev)
        scratch = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=dev) if rmax > 0 else None
        capi.check(capi.lib().dinoseg_op_augment(
            x.data_ptr(), capi.ptr(y), mask_kind, B, H, W, table.data_ptr(), rmax, OH, OW,
            capi.INPUT_U8_HWC if out_kind == "u8" else capi.INPUT_F32_CHW, img.data_ptr(),
            capi.ptr(lab) if labels == "pixel" else None, capi.ptr(lab) if labels == "patch" else None, self.cfg.patch,
            capi.ptr(scratch), self._stream()))
        return img, lab

    # ---- the step on pixel labels (upsample + cross-entropy + its gradient, fused: csrc/upsample_loss.hip) ----
    def _dense_pred(self, logp: torch.Tensor, B: int, hp: int, wp: int, OH: int, OW: int) -> torch.Tensor:
        pred = torch.empty((B, OH, OW), dtype=torch.int32, device=logp.device)
        capi.check(capi.lib().dinoseg_op_upsample_argmax(logp.data_ptr(), B, hp, wp, self.cfg.n_classes, OH, OW, pred.data_ptr(), None,
                                                         self._stream()))
        return pred

    def training_step_dense(self, batch, batch_idx=0, ignore_index=255):
        """``training_step`` on pixel labels: ``probs = self(x); loss = dense_nll_loss(probs, y)`` with y int [B, OH, OW] (255 /
        -100 = ignored) -- the cross-entropy of the bilinearly upsampled log-probs, what ``validation_step_dense`` scores.
        ``loss.backward()`` reaches the native backward through ``DINOSeg.forward``'s autograd node and ACCUMULATES into ``.grad``.
        ``fused_training_step_dense`` is the same arithmetic in one native call."""
        x, y = batch
        self._require_gpu()
        label_size(y, x.shape[0])
        probs = self(x)
        _, _, H, W = frame_layout(x, self.cfg.patch)
        hp, wp = H // self.cfg.patch, W // self.cfg.patch
        y = y.to(self.device).long().contiguous()
        flags = self.__dict__.get("_dense_flags")
        if flags is None or flags.device != self.device:
            flags = self.__dict__["_dense_flags"] = torch.zeros((1,), dtype=torch.int32, device=self.device)
        loss = dense_nll_loss(probs, y, (hp, wp), ignore_index, flags)
        with torch.no_grad():
            pred = self._dense_pred(probs.detach(), y.shape[0], hp, wp, int(y.shape[1]), int(y.shape[2]))
        return {"loss": loss, "pred": pred, "gt": y.reshape(-1), "probs": probs.detach()}

    def fused_training_step_dense(self, batch, batch_idx=0, ignore_index=255):
        """``fused_training_step`` on pixel labels, one native call (``dinoseg_train_step_dense_hw``): zero_grad + forward +
        cross-entropy of the log-probs upsampled to the labels' size + backward; every trainable parameter's ``.grad`` is
        OVERWRITTEN.  x: fp32 [B,3,H,W] (normalised) or uint8 [B,H,W,3]; y: any integer dtype [B, OH, OW] with OH >= H/patch,
        OW >= W/patch; ``ignore_index`` (outside the classes) and -100 are skipped.  Returns {"loss", "pred": int32 [B, OH, OW]
        (the pixel argmax of the step's own log-probs), "gt": the flat int64 labels, "probs": the low-res log-probs}."""
        x, y = batch
        self._require_gpu()
        self._sync_weights(train=True)
        self._sync_grads("grad")
        x, kind, B, H, W = self._prep_batch(x)
        dev = self.device
        OH, OW = label_size(y, B)
        hp, wp = H // self.cfg.patch, W // self.cfg.patch
        y = y.to(dev).reshape(-1).long().contiguous()
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        logp = torch.empty((B * hp * wp, self.cfg.n_classes), dtype=torch.float32, device=dev)
        capi.check(capi.lib().dinoseg_train_step_dense_hw(self._handle, x.data_ptr(), kind, B, H, W, OH, OW, y.data_ptr(), int(ignore_index),
                                                          loss.data_ptr(), logp.data_ptr(), self._stream()))
        self._fwd_epoch = getattr(self, "_fwd_epoch", 0) + 1
        return {"loss": loss, "pred": self._dense_pred(logp, B, hp, wp, OH, OW), "gt": y, "probs": logp}

    def _autograd_forward(self, x: torch.Tensor, kind: int, B: int, H: int, W: int) -> torch.Tensor:
        self._sync_weights(train=True)
        n = (H // self.cfg.patch) * (W // self.cfg.patch)
        logp = torch.empty((B * n, self.cfg.n_classes), dtype=torch.float32, device=self.device)
        capi.check(capi.lib().dinoseg_train_forward_hw(self._handle, x.data_ptr(), kind, B, H, W, logp.data_ptr(),
                                                       self._stream()))
        self._fwd_epoch = getattr(self, "_fwd_epoch", 0) + 1
        return logp

    def _autograd_backward(self, dlogp: torch.Tensor, epoch: int, params):
        if epoch != getattr(self, "_fwd_epoch", 0):
            raise RuntimeError("DINOSeg.backward: the activations of this forward were overwritten by a later forward / "
                               "training step (one saved forward per model; call backward before the next forward)")
        self._use(True)          # (precision 'auto': an inference call may have run since the forward)
        bk = self._sync_grads("autograd")
        dlogp = dlogp.to(device=self.device, dtype=torch.float32).contiguous()
        capi.check(capi.lib().dinoseg_backward(self._handle, dlogp.data_ptr(), self._stream()))
        by_ptr = {p.data_ptr(): n for n, p in self.named_parameters()}
        # autograd may keep (not copy) what backward returns: hand out copies, the bound buffers are rewritten next time
        return tuple(bk["views"][by_ptr[p.data_ptr()]].clone() if p.requires_grad else None for p in params)

    def fused_adam_step(self, lr=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, grad_scale=1.0) -> None:
        """Fused Adam / AdamW update of every trainable parameter from its .grad (torch.optim semantics, bias-corrected with a
        step count kept PER PARAMETER like torch; the flavour follows self.optimizer: AdamW -> decoupled decay 0.01 by default,
        Adam -> none).  Other optimizer classes have no fused kernel: use ``configure_optimizers()`` and torch's step."""
        if self.optimizer is torch.optim.AdamW:
            decoupled = 1
        elif self.optimizer is torch.optim.Adam:
            decoupled = 0
        else:
            raise NotImplementedError(f"fused_adam_step implements torch.optim.Adam and AdamW, not {self.optimizer!r}; "
                                      "use model.configure_optimizers().step() on the .grad buffers instead")
        if weight_decay is None:
            weight_decay = 0.01 if decoupled else 0.0
        lr = self.lr if lr is None else lr
        state = self.__dict__.setdefault("_adam_state", {})
        groups = {}
        for name, p in self.named_parameters():
            if not p.requires_grad or p.grad is None:
                continue
            st = state.get(name)
            if st is None or st["m"].data_ptr() == 0 or st["m"].device != p.device:
                st = state[name] = {"m": torch.zeros_like(p), "v": torch.zeros_like(p), "step": 0}
            st["step"] += 1
            groups.setdefault(st["step"], []).append((p, st))
        for step, items in groups.items():      # one launch per distinct step count (one, unless tensors were unfrozen later)
            k = len(items)
            arr = lambda xs: (C.c_void_p * k)(*xs)
            capi.check(capi.lib().dinoseg_adam_step_multi(
                k, arr([p.data_ptr() for p, _ in items]), arr([p.grad.data_ptr() for p, _ in items]),
                arr([st["m"].data_ptr() for _, st in items]), arr([st["v"].data_ptr() for _, st in items]),
                (C.c_int64 * k)(*[p.numel() for p, _ in items]), lr, betas[0], betas[1], eps, weight_decay, decoupled, step,
                grad_scale, self._stream()))
        self.invalidate_weights()      # weights changed in place through raw pointers: re-pack on the next forward

    def training_epoch_end(self, outputs):
        """pl_torch_modules.py:343-345: the train-split metrics of an epoch (the reference computes and drops them).  Accepts the
        reference's step outputs ({'pred', 'gt', ...}) as well as this class's ({'confusion'})."""
        outs = []
        for o in outputs:
            if "confusion" not in o:
                pred = torch.as_tensor(o["pred"]).to(self.device).reshape(-1).to(torch.int32).contiguous()
                o = self._score(pred, torch.as_tensor(o["gt"]), None)
            outs.append(o)
        return self.validation_epoch_end(outs, prefix="train")

    def _no_dataset(self, what):
        raise NotImplementedError(
            f"DINOSeg.{what}(): the DuckieSegDataset file reader (pl_torch_modules.py:347-365) is not part of dino_amd (DESIGN.md "
            "section 6); pass dataloaders of raw uint8 frames and masks to fit(), or override this hook in a subclass.  The "
            "augmentations of get_augmented_transforms() run on the device: fit(augment=dino_amd.Augmenter(...))")

    def train_dataloader(self, sim=False):
        self._no_dataset("train_dataloader")

    def val_dataloader(self, sim=False):
        self._no_dataset("val_dataloader")

    def test_dataloader(self):
        self._no_dataset("test_dataloader")

    def _eval_step(self, batch, batch_idx, test=False):
        """fit()'s validation / test step: pixel labels ([B, OH, OW]) are scored per pixel, patch labels as before."""
        if batch[1].dim() == 3:
            return self.validation_step_dense(batch, batch_idx)
        return self.test_step(batch, batch_idx) if test else self.validation_step(batch, batch_idx)

    def _fit_phase(self, train_dataloader, val_dataloader, ck_path, max_epochs, step, augment=None):
        """One ``Trainer.fit`` of the reference: ``max_epochs`` epochs, validation after each, best ``val_acc`` checkpointed.
        Every phase starts from a FRESH optimizer (moments and per-parameter step counts dropped): the reference builds a new
        ``Trainer`` per phase and per ``fit()`` call, so ``configure_optimizers()`` runs again (pl_torch_modules.py:391-421)."""
        from .ckpt import save_checkpoint
        self.__dict__.pop("_adam_state", None)
        best, history = -1.0, []
        for epoch in range(max_epochs):
            cms, losses = [], []
            for bi, (x, y) in enumerate(train_dataloader):
                if augment is not None:
                    x, y = augment(self, x, y)
                out = self.fused_training_step_dense((x, y), bi) if y.dim() == 3 else self.fused_training_step((x, y), bi)
                self.fused_adam_step()
                losses.append(out["loss"])
                cm = torch.zeros((self.cfg.n_classes, self.cfg.n_classes), dtype=torch.int64, device=self.device)
                capi.check(capi.lib().dinoseg_op_confusion(out["pred"].to(torch.int32).contiguous().data_ptr(), out["gt"].data_ptr(),
                                                           out["gt"].numel(), self.cfg.n_classes, cm.data_ptr(), self._stream()))
                cms.append({"confusion": cm})
                step += 1
            self.check_labels()
            metrics = self.validation_epoch_end(cms, prefix="train") if cms else {}
            metrics["train_loss"] = float(torch.stack(losses).mean()) if losses else float("nan")
            metrics.update(self.validation_epoch_end([self._eval_step(b, i) for i, b in enumerate(val_dataloader)]))
            metrics["epoch"] = epoch
            history.append(metrics)
            if metrics["val_acc"] > best:
                best = metrics["val_acc"]
                save_checkpoint(self, ck_path, epoch=epoch, global_step=step)
        return history, step

    def fit(self, ck_file_name=None, train_dataloader=None, val_dataloader=None, test_dataloader=None, max_epochs=None,
            sim_dataloader=None, augment=None):
        """The reference's ``fit`` (pl_torch_modules.py:367-431) without Lightning: freeze / unfreeze the backbone, train
        ``max_epochs`` epochs with ``fused_training_step`` + the fused optimizer step, validate after every epoch
        (``check_val_every_n_epoch=1``), keep the checkpoint with the best ``val_acc`` (``ModelCheckpoint(monitor='val_acc',
        mode='max')``) at ``write_path/<ck_file_name>.ckpt`` in the PL-1.5 schema, then run the test split and set
        ``self.best_ck``.  With ``pretrain_on_sim=True`` (ctor kwarg, :391-401) a first phase of ``max_epochs`` epochs runs on
        ``sim_dataloader`` (validated on the REAL validation split, like the reference's ``val_dataloader(sim=False)``) before the
        main phase; each phase tracks its own best ``val_acc`` (the reference builds a fresh ``ModelCheckpoint`` per phase), the
        main phase's best is what ``best_ck`` names.  The dataset reader is out of scope,
        so the dataloaders are arguments (or the ``train_dataloader() / val_dataloader() / test_dataloader()`` hooks of a
        subclass): any iterables of ``(x, y)`` batches with x uint8 [B,H,W,3] or fp32 [B,3,H,W] and y int [B,(H/8)*(W/8)].
        A batch whose y is [B, OH, OW] PIXEL labels (255 / -100 = void) trains through ``fused_training_step_dense`` and is
        validated / tested through ``validation_step_dense``.
        ``augment``: None, or a callable ``(model, x, y) -> (x, y)`` -- a ``dino_amd.Augmenter``, the reference's
        ``get_augmented_transforms()`` recipe on the device (uint8 [B,H,W,3] frames and integer [B,H,W] masks in; its ``labels``
        choose patch or pixel labels out) -- that every TRAIN batch of both phases passes through before the step; validation
        and test batches are untouched.  With None, fit runs exactly the calls it ran without the argument.
        Returns {'history': [per-epoch metrics of the main phase], 'sim_history': [...] or None, 'test': test metrics or None}."""
        import os

        hooks = type(self).train_dataloader is not DINOSeg.train_dataloader
        if train_dataloader is None and hooks:
            train_dataloader = self.train_dataloader()
        if val_dataloader is None and type(self).val_dataloader is not DINOSeg.val_dataloader:
            val_dataloader = self.val_dataloader()
        if test_dataloader is None and type(self).test_dataloader is not DINOSeg.test_dataloader:
            test_dataloader = self.test_dataloader()
        if train_dataloader is None or val_dataloader is None:
            raise ValueError("fit() needs train_dataloader and val_dataloader (the DuckieSegDataset pipeline is not part of dino_amd)")
        if self.pretrain_on_sim and sim_dataloader is None:
            if hooks:
                sim_dataloader = self.train_dataloader(sim=True)
            else:
                raise ValueError("pretrain_on_sim=True needs fit(sim_dataloader=...): the simulation split's loader "
                                 "(pl_torch_modules.py:391-401 builds it from train_path_sim, which is not part of dino_amd)")
        if self.freeze_backbone:
            self.freeze_bb()
        else:
            self.unfreeze_bb()
        if ck_file_name is None:        # same naming rule as the reference
            ck_file_name = (str(self.n_blocks) + "_" + self.head + ("_frozen" if self.freeze_backbone else "_finetuned") +
                            ("_grayscale" if self.grayscale else ""))
        out_dir = self.write_path if self.write_path is not None else "."
        os.makedirs(out_dir, exist_ok=True)
        ck_path = os.path.join(out_dir, ck_file_name + ".ckpt")
        epochs = self.max_epochs if max_epochs is None else max_epochs
        sim_history, step = None, 0
        if self.pretrain_on_sim:
            sim_history, step = self._fit_phase(sim_dataloader, val_dataloader, ck_path, epochs, 0, augment)
        history, step = self._fit_phase(train_dataloader, val_dataloader, ck_path, epochs, 0, augment)
        self.best_ck = ck_path if history else None
        test = None
        if test_dataloader is not None:
            test = self.test_epoch_end([self._eval_step(b, i, test=True) for i, b in enumerate(test_dataloader)])
        if self.comet_logger is not None and self.best_ck is not None:
            self.comet_logger.experiment.log_asset(self.best_ck)
        return {"history": history, "sim_history": sim_history, "test": test}

    def freeze_bb(self):
        for p in self.dino.parameters():
            p.requires_grad = False

    def unfreeze_bb(self):
        for p in self.dino.parameters():
            p.requires_grad = True

    def configure_optimizers(self):
        return self.optimizer(self.parameters(), lr=self.lr)

    # ---- checkpoints ------------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, **overrides):
        from .ckpt import load_checkpoint
        return load_checkpoint(cls, checkpoint_path, map_location=map_location, **overrides)


# --------------------------------------------------------------------------- video label propagation
class _PropagateRunner:
    """The launches of label propagation for one clip or stream, shared by ``DINOSeg.propagate`` and ``LabelPropagator``: a device
    ring of plane and seg slots (frame 0's, ``n_context`` queued frames' and the one the target frame is written into, which then
    takes the oldest queued frame's place), the scratch, and the two host pointer tables of ``dinoseg_op_propagate``."""

    def __init__(self, model: "DINOSeg", plan):
        self.model, self.plan = model, plan
        n, D, dev = plan.hp * plan.wp, model.cfg.embed_dim, model.device
        slots = plan.n_context + 2
        self.planes = torch.empty((slots, 2, n, D), dtype=torch.float16, device=dev)
        self.segs = torch.empty((slots, n, plan.C), dtype=torch.float32, device=dev)
        lib = capi.lib()
        nbytes = lib.dinoseg_propagate_scratch_bytes(plan.hp, plan.wp, plan.n_context + 1, plan.topk)
        if nbytes < 0:
            raise capi.DinosegError(f"dinoseg_propagate_scratch_bytes refused grid {plan.hp}x{plan.wp}, {plan.n_context + 1} context "
                                    f"frames, k = {plan.topk}")
        self.scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.queue: list = []                       # slots of the queued frames, oldest first
        self.free = list(range(1, slots))           # slot 0 is frame 0's
        self.t = 0

    def _labels(self, seg: torch.Tensor, labels_out: torch.Tensor) -> None:
        p = self.plan
        capi.check(capi.lib().dinoseg_op_upsample_argmax(seg.data_ptr(), 1, p.hp, p.wp, p.C, p.OH, p.OW, labels_out.data_ptr(), None,
                                                         self.model._stream()))

    def _normalize(self, tokens: torch.Tensor, slot: int) -> None:
        p = self.plan
        capi.check(capi.lib().dinoseg_op_normalize_tokens(tokens.data_ptr(), 1, p.hp * p.wp, self.model.cfg.embed_dim,
                                                          self.planes[slot].data_ptr(), self.model._stream()))

    def seed(self, tokens: torch.Tensor, first: torch.Tensor, labels_out: torch.Tensor) -> torch.Tensor:
        """Frame 0: its planes, its seg from ``first`` (slot 0) and its labels; returns the seg [n, C] (the slot itself)."""
        p, dev = self.plan, self.model.device
        self._normalize(tokens, 0)
        if p.seed == "soft":
            self.segs[0].copy_(first.to(device=dev, dtype=torch.float32))
        else:
            kind = 0 if first.dtype == torch.uint8 else 1
            y = first.to(device=dev, dtype=torch.uint8 if kind == 0 else torch.int64).contiguous()
            capi.check(capi.lib().dinoseg_op_label_cells(y.data_ptr(), kind, y.shape[0], y.shape[1], p.hp, p.wp, p.C,
                                                         self.segs[0].data_ptr(), self.model._stream()))
        self._labels(self.segs[0], labels_out)
        self.t = 1
        return self.segs[0]

    def step(self, tokens: torch.Tensor, labels_out: torch.Tensor) -> torch.Tensor:
        """Target frame ``self.t`` from its context (``context_frames``): returns its seg [n, C], a ring slot that stays valid
        for the next ``n_context`` steps."""
        p = self.plan
        slot = self.free.pop()
        self._normalize(tokens, slot)
        ctx = [0] + self.queue                      # frame 0, then the queued frames oldest first
        assert len(ctx) == len(context_frames(self.t, p.n_context))
        planes = (C.c_void_p * len(ctx))(*[self.planes[s].data_ptr() for s in ctx])
        segs = (C.c_void_p * len(ctx))(*[self.segs[s].data_ptr() for s in ctx])
        capi.check(capi.lib().dinoseg_op_propagate(self.planes[slot].data_ptr(), planes, segs, len(ctx), p.hp, p.wp,
                                                   self.model.cfg.embed_dim, p.C, p.radius, p.topk, p.temperature,
                                                   self.segs[slot].data_ptr(), None, None, self.scratch.data_ptr(),
                                                   self.model._stream()))
        self._labels(self.segs[slot], labels_out)
        if p.n_context > 0:
            self.queue.append(slot)
            if len(self.queue) > p.n_context:
                self.free.append(self.queue.pop(0))
        else:
            self.free.append(slot)
        self.t += 1
        return self.segs[slot]


class LabelPropagator:
    """The streaming form of ``DINOSeg.propagate`` for a camera: ``LabelPropagator(model, first_frame, first, ...)`` seeds frame 0
    (``first_frame`` uint8 [H,W,3] or fp32 [3,H,W], or the same with a leading batch of one; ``first`` as in ``propagate``), then
    ``step(frame) -> (labels int32 [OH,OW], seg fp32 [n,C] or None)`` labels every later frame from frame 0 and the ``n_context``
    frames before it.  Frame 0's own labels are ``labels0``.  Device memory: a ring of ``n_context + 2`` plane and seg slots (the
    extra one receives the target frame) and the scratch of ``dinoseg_op_propagate``; a step allocates its frame's tokens and its
    outputs.  Frame by frame this gives what ``propagate(chunk=1)`` gives, bit for bit.  Inference only."""

    def __init__(self, model: DINOSeg, first_frame: torch.Tensor, first: torch.Tensor, n_classes: Optional[int] = None,
                 n_context: int = 7, radius: Optional[int] = 12, topk: int = 5, temperature: float = 0.1, size=None,
                 n_blocks: int = 0, want_seg: bool = False):
        x = self._one(first_frame)
        self.plan = propagate_plan(model.cfg.patch, x, first, n_classes, n_context, radius, topk, temperature, size, 1)
        if not 0 <= n_blocks <= model.cfg.n_blocks:
            raise ValueError(f"intermediate must be in [0, {model.cfg.n_blocks}]")
        model._require_gpu()
        self.model, self.n_blocks, self.want_seg = model, n_blocks, want_seg
        with torch.no_grad():
            self._runner = _PropagateRunner(model, self.plan)
            self.labels0 = torch.empty((self.plan.OH, self.plan.OW), dtype=torch.int32, device=model.device)
            seg0 = self._runner.seed(model.features(model._to_device(x, self.plan.kind), n_blocks), first, self.labels0)
            self.seg0 = seg0.clone() if want_seg else None

    @staticmethod
    def _one(frame) -> torch.Tensor:
        if not isinstance(frame, torch.Tensor) or frame.dim() not in (3, 4):
            raise ValueError(f"expected one frame, uint8 [H,W,3] or fp32 [3,H,W], got {getattr(frame, 'shape', type(frame).__name__)}")
        x = frame[None] if frame.dim() == 3 else frame
        if x.shape[0] != 1:
            raise ValueError(f"expected one frame, got a batch of {x.shape[0]}")
        return x

    @torch.no_grad()
    def step(self, frame: torch.Tensor):
        p = self.plan
        x = self._one(frame)
        kind, _, H, W = frame_layout(x, self.model.cfg.patch, multiple=True, one_patch=True)
        if (kind, H, W) != (p.kind, p.H, p.W):
            raise ValueError(f"the stream's frames are {'uint8' if p.kind == capi.INPUT_U8_HWC else 'fp32'} {p.H}x{p.W}, got "
                             f"{x.dtype} {H}x{W}")
        labels = torch.empty((p.OH, p.OW), dtype=torch.int32, device=self.model.device)
        seg = self._runner.step(self.model.features(self.model._to_device(x, kind), self.n_blocks), labels)
        return labels, (seg.clone() if self.want_seg else None)


# --------------------------------------------------------------------------- PCA of patch features (streaming fit)
class PCAFitter:
    """The streaming fit of a PCA of patch features: ``PCAFitter(model, n_blocks=0)``, any number of ``update(frames, keep=None,
    chunk=32)`` calls (frames uint8 [B,H,W,3] or fp32 [B,3,H,W], any H x W of patch multiples per call; ``keep`` bool / uint8
    [B, n]) and ``solve(q)`` -> ``FeaturePCA``.  The state is the device accumulators of ``dinoseg_op_token_moments``: ``sum`` fp64
    [D], ``outer`` fp64 [D, D], ``count`` int64 and the fp32 ``shift`` [D]; no token outlives its chunk.  The shift is fixed by
    the first chunk that has a kept row: the fp32 column mean of its kept rows, from a sums-only moments call (null shift, null
    outer) and one small read.  This is the shifted-data algorithm: the solve's ``sum sum^T / count`` then removes a small
    remainder, not the features' large common mean."""

    def __init__(self, model: DINOSeg, n_blocks: int = 0):
        if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or not 0 <= n_blocks <= model.cfg.n_blocks:
            raise ValueError(f"n_blocks must be an integer in 0..{model.cfg.n_blocks}, got {n_blocks!r}")
        self.model, self.n_blocks = model, int(n_blocks)
        self.shift = self.sum = self.outer = self.count = None
        self._scratch = None

    def _moments(self, tokens, keep, n, shift, sum_, outer, count) -> None:
        lib, D, Bc = capi.lib(), self.model.cfg.embed_dim, tokens.shape[0]
        nbytes = lib.dinoseg_pca_scratch_bytes(Bc, n, D)
        if nbytes < 0:
            raise capi.DinosegError(f"dinoseg_pca_scratch_bytes refused B = {Bc}, n = {n}, D = {D}")
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty((nbytes,), dtype=torch.uint8, device=self.model.device)
        capi.check(lib.dinoseg_op_token_moments(tokens.data_ptr(), capi.ptr(keep), Bc, n, D, capi.ptr(shift), sum_.data_ptr(),
                                                capi.ptr(outer), count.data_ptr(), self._scratch.data_ptr(), self.model._stream()))

    @torch.no_grad()
    def update(self, frames: torch.Tensor, keep: Optional[torch.Tensor] = None, chunk: int = 32) -> int:
        """Add the kept patch rows of ``frames`` to the moments -> the number of rows taken (``keep`` is counted where it lives: a
        host mask costs no device synchronisation, a device mask one small read)."""
        model = self.model
        plan = pca_plan(model.cfg.patch, model.cfg.embed_dim, model.cfg.n_blocks, frames, keep=keep, n_blocks=self.n_blocks, chunk=chunk)
        model._require_gpu()
        x = model._to_device(frames, plan.kind)
        dev, D, n = model.device, model.cfg.embed_dim, plan.hp * plan.wp
        keep_u8 = None if keep is None else keep.to(device=dev, dtype=torch.uint8).contiguous()
        taken = plan.B * n if keep is None else int(keep.ne(0).sum().item())
        if self.sum is None:
            self.sum = torch.zeros((D,), dtype=torch.float64, device=dev)
            self.outer = torch.zeros((D, D), dtype=torch.float64, device=dev)
            self.count = torch.zeros((1,), dtype=torch.int64, device=dev)
        for c0 in range(0, plan.B, plan.chunk):
            tokens = model.features(x[c0:c0 + plan.chunk], self.n_blocks)
            keep_c = None if keep_u8 is None else keep_u8[c0:c0 + plan.chunk]
            if self.shift is None:
                s0 = torch.zeros((D,), dtype=torch.float64, device=dev)
                n0 = torch.zeros((1,), dtype=torch.int64, device=dev)
                self._moments(tokens, keep_c, n, None, s0, None, n0)
                rows = int(n0.item())                                                   # the one small read
                if rows == 0:
                    continue
                self.shift = (s0 / rows).to(torch.float32)
            self._moments(tokens, keep_c, n, self.shift, self.sum, self.outer, self.count)
        return taken

    def solve(self, q: int) -> FeaturePCA:
        """The ``FeaturePCA`` of the rows taken so far (``pca_solve`` on the accumulators read back)."""
        if self.shift is None:
            raise ValueError("a PCA needs at least 2 rows, got count = 0")
        return pca_solve(self.sum.cpu(), self.outer.cpu(), int(self.count.item()), self.shift.cpu(), int(q), self.n_blocks)


# --------------------------------------------------------------------------- few-shot segmentation (k-NN from a memory bank)
class KnnResult(NamedTuple):
    """What ``DINOSeg.segment_knn`` returns: pixel labels int32 [B, OH, OW], and when asked for the soft map fp32 [B, n, C] and the
    selected bank rows int32 [B, n, k] in rank order (-1 beyond min(k, bank.size))."""
    labels: torch.Tensor
    seg: Optional[torch.Tensor]
    idx: Optional[torch.Tensor]


class MemoryBank:
    """A flat bank of labelled patch features for ``DINOSeg.segment_knn``: ``MemoryBank(model, n_classes, capacity, hard=False,
    n_blocks=0)`` allocates, once, the unit rows as fp16 hi + lo planes [2, capacity, D] and the label store (soft fp32 [capacity,
    n_classes], or with ``hard=True`` one uint8 per row, 255 = void, hence at most 255 classes); rows 0 .. ``size`` - 1 are live.
    ``add`` fills it in place, ``clear`` empties it, ``state_dict`` / ``load_state_dict`` carry it bit for bit (with ``frames``, the
    number of frames added, which ``per_frame`` seeds count from).  Rows are never evicted or replaced.  ``project``, a
    ``FeaturePCA`` whose number of components is a multiple of 64 and whose ``n_blocks`` is the bank's, makes the rows the unit
    PROJECTED features: ``dim`` is then its ``q``, ``add`` and ``segment_knn`` project the tokens before they normalise them, and
    the state carries the projection.  Without it every call runs the launches it ran before."""

    def __init__(self, model: DINOSeg, n_classes: int, capacity: int, hard: bool = False, n_blocks: int = 0,
                 project: Optional[FeaturePCA] = None):
        for what, v, hi in (("n_classes", n_classes, 256), ("capacity", capacity, 1 << 24)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= hi:
                raise ValueError(f"{what} must be an integer in 1..{hi}, got {v!r}")
        if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or not 0 <= n_blocks <= model.cfg.n_blocks:
            raise ValueError(f"n_blocks must be an integer in 0..{model.cfg.n_blocks}, got {n_blocks!r}")
        if hard and int(n_classes) > 255:
            raise ValueError("a hard bank stores void as 255, so it holds at most 255 classes; use soft labels for 256")
        if project is not None:
            pca_projection(project, model.cfg.embed_dim, "project", bank=True, blocks=int(n_blocks))
        model._require_gpu()
        self.model, self.n_classes, self.capacity, self.hard, self.n_blocks = model, int(n_classes), int(capacity), bool(hard), int(n_blocks)
        self.project = project
        self.dim = model.cfg.embed_dim if project is None else project.q
        self.planes = torch.zeros((2, self.capacity, self.dim), dtype=torch.float16, device=model.device)
        self.labels = torch.full((self.capacity,), 255, dtype=torch.uint8, device=model.device) if self.hard else \
            torch.zeros((self.capacity, self.n_classes), dtype=torch.float32, device=model.device)
        self.size = 0
        self.frames = 0                             # frames added so far: frame i of the bank draws its cells from seed + i

    def clear(self) -> None:
        self.size = 0
        self.frames = 0

    def _rows(self, tokens: torch.Tensor, n: int) -> torch.Tensor:
        """The rows the bank compares, in the token layout: the backbone's tokens, or with ``project`` their projection
        (``dinoseg_op_pca_project``: fp32 [B, 1 + n, q], the CLS rows zero)."""
        if self.project is None:
            return tokens
        mean, basis, _ = self.project.on(self.model.device)
        out = torch.empty((tokens.shape[0], n + 1, self.dim), dtype=torch.float32, device=self.model.device)
        capi.check(capi.lib().dinoseg_op_pca_project(tokens.data_ptr(), tokens.shape[0], n, self.project.dim, mean.data_ptr(),
                                                     basis.data_ptr(), None, self.dim, out.data_ptr(), self.model._stream()))
        return out

    @torch.no_grad()
    def add(self, frames: torch.Tensor, labels: torch.Tensor, per_frame: Optional[int] = None, seed: int = 0) -> int:
        """Add labelled frames: ``frames`` uint8 [B,H,W,3] or fp32 [B,3,H,W] (any H x W of patch multiples; frames of different
        shapes go in separate calls), ``labels`` integer [B,OH,OW] at least as large as the patch grid (a label outside [0,
        n_classes) such as 255 or -100 is void) -> the number of rows added.  A cell's row is its unit patch feature
        (``features`` after the bank's ``n_blocks``, ``dinoseg_op_normalize_tokens``) and its label the class shares of its pixels
        (``dinoseg_op_label_cells``); a hard bank keeps the first maximum of the shares, 255 where all are zero.  ``per_frame=m``
        keeps m cells per frame, those of ``sample_indices(n, m, seed + i)`` for the i-th frame the bank has seen, in that order.
        A call that would overflow ``capacity`` raises ``ValueError`` and adds nothing."""
        model = self.model
        p = bank_add_plan(model.cfg.patch, frames, labels, per_frame, seed, self.capacity - self.size)
        x = model._to_device(frames, p.kind)
        y = labels.to(device=model.device, dtype=torch.uint8 if p.mask_kind == 0 else torch.int64).contiguous()
        lib, n, D, C_ = capi.lib(), p.hp * p.wp, self.dim, self.n_classes
        planes = torch.empty((2, n, D), dtype=torch.float16, device=model.device)
        seg = torch.empty((n, C_), dtype=torch.float32, device=model.device)
        classes = torch.arange(C_, device=model.device)
        for c0 in range(0, p.B, 32):
            tokens = self._rows(model.features(x[c0:c0 + 32], self.n_blocks), n)
            for i in range(tokens.shape[0]):
                b = c0 + i
                capi.check(lib.dinoseg_op_normalize_tokens(tokens[i].data_ptr(), 1, n, D, planes.data_ptr(), model._stream()))
                capi.check(lib.dinoseg_op_label_cells(y[b].data_ptr(), p.mask_kind, p.OH, p.OW, p.hp, p.wp, C_, seg.data_ptr(),
                                                      model._stream()))
                keep = slice(None) if p.per_frame == n else sample_indices(n, p.per_frame, p.seed + self.frames).to(model.device)
                at = slice(self.size, self.size + p.per_frame)
                self.planes[:, at] = planes[:, keep]
                rows = seg[keep]
                if self.hard:
                    top = rows.max(dim=1, keepdim=True).values
                    first = torch.where(rows == top, classes, C_).min(dim=1).values        # the first maximum
                    self.labels[at] = torch.where(top[:, 0] > 0, first, 255).to(torch.uint8)
                else:
                    self.labels[at] = rows
                self.size += p.per_frame
                self.frames += 1
        return p.rows

    def state_dict(self) -> dict:
        state = {"planes": self.planes.clone(), "labels": self.labels.clone(), "size": self.size, "frames": self.frames,
                 "n_classes": self.n_classes, "hard": self.hard, "n_blocks": self.n_blocks}
        if self.project is not None:
            state["project"] = self.project.state_dict()
        return state

    def load_state_dict(self, state: dict) -> None:
        planes, labels = state["planes"], state["labels"]
        same = (int(state["n_classes"]), bool(state["hard"]), int(state["n_blocks"])) == (self.n_classes, self.hard, self.n_blocks)
        if not same or tuple(planes.shape) != tuple(self.planes.shape) or planes.dtype != self.planes.dtype or \
                tuple(labels.shape) != tuple(self.labels.shape) or labels.dtype != self.labels.dtype or \
                not 0 <= int(state["size"]) <= self.capacity:
            raise ValueError("the state is not that of a bank with this one's capacity, width, n_classes, hard and n_blocks")
        if ("project" in state) != (self.project is not None):
            raise ValueError("the state and this bank do not agree on whether the rows are projected")
        if self.project is not None:
            project = pca_projection(FeaturePCA.from_state_dict(state["project"]), self.model.cfg.embed_dim, "the state's projection",
                                     bank=True, blocks=self.n_blocks)
            if project.q != self.dim:
                raise ValueError(f"the state's projection has {project.q} components, this bank's rows have width {self.dim}")
            self.project = project
        self.planes.copy_(planes)
        self.labels.copy_(labels)
        self.size, self.frames = int(state["size"]), int(state.get("frames", 0))


# --------------------------------------------------------------------------- unsupervised segmentation (spherical k-means)
class ClusterResult(NamedTuple):
    """What ``DINOSeg.cluster`` returns: pixel labels int32 [B, OH, OW], unit centroids fp32 [k, D], the cluster sizes of the last
    update int32 [k], per pass the objective fp32 [iters + 1] and the number of cells that changed cluster int32 [iters + 1], and the
    final pass's scores fp32 [B, n, k] when asked for."""
    labels: torch.Tensor
    centroids: torch.Tensor
    counts: torch.Tensor
    objective: torch.Tensor
    moved: torch.Tensor
    scores: Optional[torch.Tensor]


class _KMeansRun(NamedTuple):
    centroids: torch.Tensor
    counts: torch.Tensor
    objective: torch.Tensor
    moved: torch.Tensor
    scores: torch.Tensor


class _KMeansRunner:
    """The launches of spherical k-means over one planes buffer, shared by ``DINOSeg.cluster`` and ``DINOSeg.assign_clusters``: the
    scratch of ``dinoseg_kmeans_scratch_bytes`` and the per-point outputs are allocated once; every run owns its centroids, records
    and scores."""

    def __init__(self, model: "DINOSeg", plan, planes: torch.Tensor):
        self.model, self.plan, self.planes = model, plan, planes
        self.n, self.D, dev = plan.hp * plan.wp, model.cfg.embed_dim, model.device
        nbytes = capi.lib().dinoseg_kmeans_scratch_bytes(plan.B, self.n, plan.k, self.D)
        if nbytes < 0:
            raise capi.DinosegError(f"dinoseg_kmeans_scratch_bytes refused {plan.B} frames of {self.n} cells, k = {plan.k}, "
                                    f"width {self.D}")
        self.scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        self.assign = torch.empty((plan.N,), dtype=torch.int32, device=dev)
        self.best = torch.empty((plan.N,), dtype=torch.float32, device=dev)

    def _init(self, rows: torch.Tensor, normalize: bool):
        k, dev = self.plan.k, self.model.device
        cent = torch.empty((k, self.D), dtype=torch.float32, device=dev)
        cplanes = torch.empty((2, k, self.D), dtype=torch.float16, device=dev)
        capi.check(capi.lib().dinoseg_op_kmeans_init(rows.data_ptr(), k, self.D, int(normalize), cent.data_ptr(), cplanes.data_ptr(),
                                                     self.model._stream()))
        return cent, cplanes

    def _assign(self, cplanes, prev, scores, objective, moved, t: int) -> None:
        p = self.plan
        capi.check(capi.lib().dinoseg_op_kmeans_assign(
            self.planes.data_ptr(), p.B, self.n, cplanes.data_ptr(), p.k, self.D, capi.ptr(prev), self.assign.data_ptr(),
            self.best.data_ptr(), capi.ptr(scores), None if objective is None else objective[t:].data_ptr(),
            None if moved is None else moved[t:].data_ptr(), self.scratch.data_ptr(), self.model._stream()))

    def run(self, rows: torch.Tensor) -> _KMeansRun:
        """init, ``iters`` times (assign, update), the final assign with scores; no host synchronisation in between"""
        p, dev = self.plan, self.model.device
        cent, cplanes = self._init(rows, True)
        counts = torch.zeros((p.k,), dtype=torch.int32, device=dev)
        objective = torch.empty((p.iters + 1,), dtype=torch.float32, device=dev)
        moved = torch.empty((p.iters + 1,), dtype=torch.int32, device=dev)
        scores = torch.empty((p.N, p.k), dtype=torch.float32, device=dev)
        for t in range(p.iters):
            self._assign(cplanes, self.assign if t > 0 else None, None, objective, moved, t)
            capi.check(capi.lib().dinoseg_op_kmeans_update(
                self.planes.data_ptr(), p.B, self.n, self.assign.data_ptr(), cent.data_ptr(), cplanes.data_ptr(), p.k, self.D,
                cent.data_ptr(), cplanes.data_ptr(), counts.data_ptr(), self.scratch.data_ptr(), self.model._stream()))
        self._assign(cplanes, self.assign if p.iters > 0 else None, scores, objective, moved, p.iters)
        return _KMeansRun(cent, counts, objective, moved, scores)

    def assign_only(self, centroids: torch.Tensor) -> torch.Tensor:
        """one assignment against centroids taken as they are -> scores [N, k]"""
        p = self.plan
        _, cplanes = self._init(centroids, False)
        scores = torch.empty((p.N, p.k), dtype=torch.float32, device=self.model.device)
        self._assign(cplanes, None, scores, None, None, 0)
        return scores


# --------------------------------------------------------------------------- unsupervised foreground masks (normalized cut)
class NcutResult(NamedTuple):
    """What ``DINOSeg.ncut`` returns: pixel labels int32 [B, OH, OW] (1 = foreground), the cell partition uint8 [B, n], the
    sign-fixed eigenvector fp32 [B, n] (foreground positive), the cell with the largest entry int32 [B], the Rayleigh record of
    every pass fp32 [B, iters], the set bits per row int32 [B, n], and the row-major bit graph uint64 [B, n, ceil(n / 64)] when asked
    for."""
    labels: torch.Tensor
    fg: torch.Tensor
    eigvec: torch.Tensor
    seed_cell: torch.Tensor
    rho: torch.Tensor
    degree: torch.Tensor
    graph: Optional[torch.Tensor]


# --------------------------------------------------------------------------- objects of a label map (connected components)
class ComponentsResult(NamedTuple):
    """What ``DINOSeg.components`` returns: per pixel the number of its component int32 [B, H, W] (-1 on void pixels), the number of
    components int32 [B], and the table of the first M of them: the first pixel's linear index, the label, the area, and the half-open
    box (x0, y0, x1, y1), int32 [B, M] / [B, M, 4]; rows behind the last component hold first = label = -1, area = 0, box = 0."""
    ids: torch.Tensor
    count: torch.Tensor
    first: torch.Tensor
    label: torch.Tensor
    area: torch.Tensor
    box: torch.Tensor


class DiscoverResult(NamedTuple):
    """What ``DINOSeg.discover`` returns: pixel labels int32 [B, OH, OW] (1 = the object), its box int32 [B, 4] = (x0, y0, x1, y1)
    half-open in frame coordinates, whether the seed cell is foreground uint8 [B], the object's cells uint8 [B, n], their number int32
    [B], and the cut they were taken from."""
    labels: torch.Tensor
    box: torch.Tensor
    found: torch.Tensor
    cells: torch.Tensor
    area: torch.Tensor
    ncut: NcutResult


class MaskCutResult(NamedTuple):
    """What ``DINOSeg.discover_all`` returns for K = ``max_objects`` rounds: pixel labels int32 [B, OH, OW] (0 = background, t + 1 =
    the object of round t), the number of rounds that found an object int32 [B], and per round whether it did uint8 [B, K], the
    object's box int32 [B, K, 4] = (x0, y0, x1, y1) half-open in frame coordinates, its cells' number int32 [B, K], the cells uint8
    [B, K, n], the cut's seed cell int32 [B, K] and Rayleigh record fp32 [B, K, iters]; the ORIGINAL bit graph uint64 [B, n,
    ceil(n / 64)] when asked for."""
    labels: torch.Tensor
    count: torch.Tensor
    found: torch.Tensor
    box: torch.Tensor
    area: torch.Tensor
    cells: torch.Tensor
    seed_cell: torch.Tensor
    rho: torch.Tensor
    graph: Optional[torch.Tensor]
