"""The gradient-stage events of the fine-tune backward (dinoseg_grad_stages / dinoseg_stream_wait_grad_stage), the part of the step
dino_amd/parallel.py builds its bucketed all-reduce on.  ViT-S/8 with 2 blocks and the MLP head, 2 frames of 64 x 64: 130 token rows, one
over a 128-row tile.  Option deterministic is on, so two steps from the same state write the same bits."""
import contextlib

import pytest
import torch

import dino_amd
from dino_amd import DINOSeg, ViTConfig, capi, procedural_state_dict
from dino_amd.weights import synthetic_frames, synthetic_labels

pytestmark = pytest.mark.gpu
CFG = ViTConfig(n_blocks=2)
CASES = [(p, s) for p in ("bf16", "bf16x3") for s in (1, 2)]


@contextlib.contextmanager
def stepping(precision, streams):
    """The model and its batch, with the options of the case set for the body."""
    with dino_amd.options(deterministic=1, train_streams=streams):
        sd = procedural_state_dict(CFG)
        m = DINOSeg(head=CFG.head, n_blocks=CFG.n_blocks, n_classes=CFG.n_classes, precision=precision, arch=CFG)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m.to("cuda:0")
        fr = torch.from_numpy(synthetic_frames(2, 64, seed=171)).cuda()
        lb = torch.from_numpy(synthetic_labels(2, 64, CFG.n_classes, seed=172)).cuda()
        yield m, (fr, lb)
        torch.cuda.synchronize()


@pytest.mark.parametrize("precision,streams", CASES)
def test_a_stage_per_block_plus_head_and_embeddings(cuda, precision, streams):
    with stepping(precision, streams) as (m, batch):
        m.fused_training_step(batch, 0)
        assert capi.lib().dinoseg_grad_stages(m._handle) == CFG.n_blocks + 2 == 4


@pytest.mark.parametrize("precision,streams", CASES)
def test_gradients_of_a_stage_are_final_behind_its_event(cuda, precision, streams):
    """A second stream waits for stage 0..3 of a step that nobody synchronised with and copies, behind each wait, the gradients
    DINOSeg.grad_stage assigns to that stage: every copy equals the final gradient, and the gradients equal those of a step nothing
    waited on.  A functional check of the API (the events exist, are recorded in order, and cover the parameters grad_stage names),
    not a race detector: a copy that ran too early would usually still read final values on a GPU this idle."""
    with stepping(precision, streams) as (m, batch):
        m.unfreeze_bb()
        m.fused_training_step(batch, 0)
        torch.cuda.synchronize()
        alone = {n: p.grad.clone() for n, p in m.named_parameters()}
        t = torch.cuda.Stream()
        m.fused_training_step(batch, 0)
        copies, seen = {}, set()
        for stage in range(4):
            m.stream_wait_grad_stage(stage, t)
            with torch.cuda.stream(t):
                for n, p in m.named_parameters():
                    if DINOSeg.grad_stage(n, CFG.n_blocks) == stage:
                        copies[n] = p.grad.clone()
                        seen.add(stage)
        torch.cuda.synchronize()
        assert seen == {0, 1, 2, 3} and set(copies) == set(alone)
        for n, p in m.named_parameters():
            assert torch.equal(copies[n], p.grad), (n, "copied behind its stage event")
            assert torch.equal(p.grad, alone[n]), (n, "against the step nothing waited on")


@pytest.mark.parametrize("precision,streams", CASES)
def test_frozen_backbone_records_the_head_stage_only(cuda, precision, streams):
    with stepping(precision, streams) as (m, batch):
        m.freeze_bb()
        m.fused_training_step(batch, 0)
        t = torch.cuda.Stream()
        m.stream_wait_grad_stage(0, t)
        with pytest.raises(capi.DinosegError, match=r"recorded 1 stage\(s\); stage 1 was not reached"):
            m.stream_wait_grad_stage(1, t)


@pytest.mark.parametrize("precision,streams", CASES)
@pytest.mark.parametrize("stage", [-1, 4])
def test_stage_outside_the_range_is_refused(cuda, precision, streams, stage):
    with stepping(precision, streams) as (m, batch):
        m.unfreeze_bb()
        m.fused_training_step(batch, 0)
        with pytest.raises(capi.DinosegError, match="stage out of range"):
            m.stream_wait_grad_stage(stage, torch.cuda.Stream())
