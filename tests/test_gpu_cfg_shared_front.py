"""The CFG-shared front of the pair pass (wan.cfg_front_form): block 0's front — norm1 + modulate, q / k / v, RMSNorm + RoPE, self-attention, the
o projection, norm3, the cross-attention q projection and its RMSNorm — runs once on one forward's rows, the residual stream fans out to the stacked
rows in block 0's cross-attention output projection (the GEMM epilogue's residual row period).  Every output row is computed from the same operands
by the same kernels in the same order as when both halves are computed, so noise predictions must be EQUAL: torch.equal, no tolerance.
wan-tiny (two layers), the pair pass forced through the config (`cfg_pair=True`), token counts that are no multiple of 256 and need padding to the
64-row slot: 90 (one query block) and 270 (two)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FP8_MM = {"mm_config": {"mm_type": "W-fp8-channel-sym-A-fp8-channel-sym-dynamic-Hip", "weight_auto_quant": True}}
SHAPES = (((16, 3, 12, 10), 9), ((16, 3, 20, 18), 9))  # 90 tokens (slot 128) / 270 tokens (slot 320)


def _to_dev(wd):
    return {k: v.cuda() for k, v in wd.items()}


def _loop(cfg, wd, lat, inputs, steps=2, patch=None):
    """(noise prediction of step 0, latents after `steps` steps, the front forms the transformer reported), through WanModel.infer."""
    from lightx2v_amd import scheduler, wan

    model = wan.WanModel(cfg, wd)
    if patch is not None:
        patch(model)
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    forms, pred = [], None
    for i in range(steps):
        sch.step_pre(i)
        model.transformer_infer.front_form = None
        model.infer(inputs)
        forms.append(model.transformer_infer.front_form)
        if i == 0:
            pred = sch.noise_pred.float().clone()
        sch.step_post()
    return pred, sch.latents.float().clone(), forms


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_shared_front_is_bit_identical_to_the_unshared_pair_pass_and_to_separate_forwards(fp8):
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    assert dims["num_layers"] == 2
    wd = _to_dev(synth.synth_wan_weights(dims, seed=1))
    extra = FP8_MM if fp8 else {}
    for ts, frames in SHAPES:
        lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
        inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
        base = dict(target_shape=ts, target_video_length=frames, infer_steps=3, **extra)
        on = _loop(wan.default_config(dims, cfg_pair=True, **base), wd, lat, inputs)  # cfg_shared_front: the default
        off = _loop(wan.default_config(dims, cfg_pair=True, cfg_shared_front=False, **base), wd, lat, inputs)
        sep = _loop(wan.default_config(dims, cfg_pair=False, cfg_branch_streams=False, **base), wd, lat, inputs)
        assert on[2] == ["shared", "shared"] and off[2] == ["unshared", "unshared"] and sep[2] == [None, None], (on[2], off[2], sep[2])
        assert torch.isfinite(on[1]).all()
        for name, other in (("the unshared pair pass", off), ("separate forwards", sep)):
            assert torch.equal(on[0], other[0]), f"{ts}: noise prediction differs from {name}: max |d| = {(on[0] - other[0]).abs().max().item():.3e}"
            assert torch.equal(on[1], other[1]), f"{ts}: latents differ from {name}"


def test_teacache_and_i2v_equal_the_unshared_pair_pass():
    """TeaCache keeps its per-branch forwards (its skipped and residual-replay steps are per branch; the pair pass is not taken at all) and i2v
    shares (the image cross-attention reads the same shared q): either way the result is that of `cfg_shared_front=False`."""
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    ts, frames = SHAPES[0]
    wd = _to_dev(synth.synth_wan_weights(dims, seed=1))
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    tea = dict(target_shape=ts, target_video_length=frames, infer_steps=4, cfg_pair=True, feature_caching="Tea", coefficients=[[0, 0, 0, 1.0, 0], [0, 0, 0.5, 1.0, 0]],
               use_ret_steps=False, teacache_thresh=0.2)
    on = _loop(wan.default_config(dims, **tea), wd, lat, inputs, steps=4)
    off = _loop(wan.default_config(dims, cfg_shared_front=False, **tea), wd, lat, inputs, steps=4)
    assert on[2] == [None] * 4  # no pair pass, so no shared front
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])

    dims = synth.WAN_DIMS["wan-tiny-i2v"]
    wd = _to_dev(synth.synth_wan_i2v_weights(dims, seed=0))
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    image = {k: v.cuda() for k, v in synth.synth_i2v_inputs(dims, ts).items()}
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}, "image_encoder_output": image}
    i2v = dict(task="i2v", in_dim=36, cross_attn_2_type="hip_flash", target_shape=ts, target_video_length=frames, infer_steps=3, cfg_pair=True)
    on = _loop(wan.default_config(dims, **i2v), wd, lat, inputs)
    off = _loop(wan.default_config(dims, cfg_shared_front=False, **i2v), wd, lat, inputs)
    assert on[2] == ["shared", "shared"] and off[2] == ["unshared", "unshared"]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_different_input_tensors_are_not_shared():
    """A driver that hands the two forwards different token inputs (here: the unconditional half perturbed in WanModel._pair_inputs) gets both halves
    computed although `cfg_shared_front` is on: the result equals that of `cfg_shared_front=False` with the same inputs, and differs from the
    unperturbed one — the unconditional half was really used."""
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    ts, frames = SHAPES[0]
    wd = _to_dev(synth.synth_wan_weights(dims, seed=1))
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    base = dict(target_shape=ts, target_video_length=frames, infer_steps=3, cfg_pair=True)

    def perturb(model):
        plain = model._pair_inputs

        def pair_inputs(inputs):
            embed, grid_sizes, (x, _), embed0, seq_lens, freqs, ctxs = plain(inputs)
            return embed, grid_sizes, (x, (x.float() * 1.5).to(x.dtype)), embed0, seq_lens, freqs, ctxs

        model._pair_inputs = pair_inputs

    def equal_copy(model):  # equal values in a tensor of its own: still not shared (the gate is identity, not equality)
        plain = model._pair_inputs

        def pair_inputs(inputs):
            embed, grid_sizes, (x, _), embed0, seq_lens, freqs, ctxs = plain(inputs)
            return embed, grid_sizes, (x, x.clone()), embed0, seq_lens, freqs, ctxs

        model._pair_inputs = pair_inputs

    on = _loop(wan.default_config(dims, **base), wd, lat, inputs, patch=perturb)
    off = _loop(wan.default_config(dims, cfg_shared_front=False, **base), wd, lat, inputs, patch=perturb)
    same = _loop(wan.default_config(dims, **base), wd, lat, inputs)
    copy = _loop(wan.default_config(dims, **base), wd, lat, inputs, patch=equal_copy)
    assert on[2] == ["unshared", "unshared"] and copy[2] == ["unshared", "unshared"] and same[2] == ["shared", "shared"]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert not torch.equal(on[0], same[0])
    assert torch.equal(copy[0], same[0]) and torch.equal(copy[1], same[1])
