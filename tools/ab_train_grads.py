"""GPU box: digests of the fine-tune step for comparing two builds of the library.  A fixed list of small cases with option
deterministic = 1; per case the sha256 of the loss, of every gradient of the first step and of every parameter after two fused Adam
steps go into a JSON file.  Run it once per library, each run a process of its own (DINOSEG_LIB selects an older build, as in
tools/ab_bench.sh), then compare the files:
    python tools/ab_train_grads.py out_a.json;  DINOSEG_LIB=old.so python tools/ab_train_grads.py out_b.json
    python tools/ab_train_grads.py --diff out_a.json out_b.json"""
import hashlib, json, os, sys
sys.path.insert(0, os.getcwd())


def diff(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = [(c, k) for c in sorted(set(A) | set(B)) for k in sorted(set(A.get(c, {})) | set(B.get(c, {})))
           if A.get(c, {}).get(k) != B.get(c, {}).get(k)]
    for c, k in bad:
        print("DIFFERS", c, k)
    print(f"{len(A)} / {len(B)} cases, {sum(len(v) for v in A.values())} / {sum(len(v) for v in B.values())} digests, {len(bad)} differ")
    return 1 if bad or not A else 0


if len(sys.argv) == 4 and sys.argv[1] == "--diff":
    sys.exit(diff(sys.argv[2], sys.argv[3]))

import torch
import dino_amd
from dino_amd import DINOSeg, ViTConfig, procedural_state_dict
from dino_amd.weights import synthetic_frames, synthetic_labels

S8 = ViTConfig(n_blocks=2)
TINY = ViTConfig(embed_dim=128, num_heads=2, n_blocks=2)
VITB = ViTConfig(embed_dim=768, num_heads=12, n_blocks=1)
P16 = ViTConfig(patch=16, pos_grid=14, n_blocks=2, head="linear", n_classes=150)
NOBLOCK = ViTConfig(n_blocks=0)
WIDE = ViTConfig(n_blocks=2, n_classes=150)


def block_weight(n, p):
    return n.startswith("dino.blocks.") and n.endswith(".weight") and p.dim() == 2


# name: (config, precision, frame rows, frame columns, train_streams, which parameters train, through torch.autograd or "dense" = the
# fused step on pixel labels of the frame's size[, options set for the case only])
CASES = {
    "vits8 bf16": (S8, "bf16", 64, 64, 2, "all", False),
    "vits8 bf16x3": (S8, "bf16x3", 64, 64, 2, "all", False),
    "vits8 bf16x3 one stream": (S8, "bf16x3", 64, 64, 1, "all", False),
    "vits8 bf16 one stream": (S8, "bf16", 64, 64, 1, "all", False),
    "patch16 linear head C=150 64x128": (P16, "bf16x3", 64, 128, 2, "all", False),
    "tiny": (TINY, "bf16x3", 64, 64, 2, "all", False),
    "vitb one block": (VITB, "bf16", 64, 64, 2, "all", False),
    "frozen backbone": (S8, "bf16x3", 64, 64, 2, "head", False),
    "bias-only freeze": (S8, "bf16x3", 64, 64, 2, "no block weights", False),
    "bias-only freeze one stream": (S8, "bf16x3", 64, 64, 1, "no block weights", False),
    "autograd": (S8, "bf16x3", 64, 64, 2, "all", True),
    "autograd one stream bf16": (S8, "bf16", 64, 64, 1, "all", True),
    "no blocks": (NOBLOCK, "bf16x3", 64, 64, 2, "all", False),              # the final norm hands a null fc2 bias, the block loop is empty
    "gemm_ln=0 bf16": (S8, "bf16", 64, 64, 2, "all", False, {"gemm_ln": 0}),      # LayerNorm + GEMM fallback of the training forward
    "gemm_ln=0 bf16x3": (S8, "bf16x3", 64, 64, 2, "all", False, {"gemm_ln": 0}),
    "mlp head C=150": (WIDE, "bf16x3", 64, 64, 2, "all", False),             # the wide head's dz_ld
    "64x128": (S8, "bf16x3", 64, 128, 2, "all", False),                      # the rectangular pos-embed scratch in T2
    "dense": (S8, "bf16x3", 64, 64, 2, "all", "dense"),                      # the dws growth and the dlogp entry
    "splitk_tiles=1": (S8, "bf16x3", 64, 64, 2, "all", False, {"splitk_tiles": 1}),      # the two ends of the weight gradients' slice count
    "route_ab=4": (S8, "bf16x3", 64, 64, 2, "all", False, {"route_ab": 4}),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(cfg, prec, H, W, streams, train, autograd, opts={}):
    with dino_amd.options(deterministic=1, train_streams=streams, **opts):
        return run_case(cfg, prec, H, W, train, autograd)


def run_case(cfg, prec, H, W, train, autograd):
    sd = procedural_state_dict(cfg)
    m = DINOSeg(head=cfg.head, n_blocks=cfg.n_blocks, n_classes=cfg.n_classes, precision=prec, arch=cfg, optimizer=torch.optim.Adam, lr=1e-3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.to("cuda:0")
    for n, p in m.named_parameters():
        p.requires_grad_(train == "all" or (train == "head" and n.startswith("clf.")) or (train == "no block weights" and not block_weight(n, p)))
    n_patches = (H // cfg.patch) * (W // cfg.patch)
    fr = torch.from_numpy(synthetic_frames(2, H, seed=181, w=W)).cuda()
    lb = torch.from_numpy(synthetic_labels(2, n_patches, cfg.n_classes, seed=182)).cuda()
    px = torch.from_numpy(synthetic_labels(2, H * W, cfg.n_classes, seed=183)).reshape(2, H, W).cuda()
    out = {}
    for step in range(2):
        if autograd == "dense":
            loss = m.fused_training_step_dense((fr, px), step)["loss"]
        elif autograd:
            for p in m.parameters():
                p.grad = None
            loss = m.training_step((fr, lb), step)["loss"]
            loss.backward()
        else:
            loss = m.fused_training_step((fr, lb), step)["loss"]
        torch.cuda.synchronize()
        if step == 0:
            out["loss"] = sha(loss)
            out.update({"grad " + n: sha(p.grad) for n, p in m.named_parameters() if p.requires_grad})
        m.fused_adam_step()
    torch.cuda.synchronize()
    out["loss step 2"] = sha(loss)
    out.update({"param " + n: sha(p) for n, p in m.named_parameters()})
    return out


res = {}
for name, case in CASES.items():
    res[name] = run(*case)
    print(name, len(res[name]), "digests", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(res, open(sys.argv[1], "w"), indent=1, sort_keys=True)
print("ok", len(res), "cases")
