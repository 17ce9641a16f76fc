"""The audio adapter (lightx2v_amd/audio.py) on the GPU against tests/audio_restatement.py: one layer on a tiny grid, weight = 0, and the Wan driver on
the tiny synthetic model with a two-layer adapter handed over as audio_dit_blocks."""
import pytest
import torch

from tests import audio_restatement as R

pytestmark = pytest.mark.gpu
HEADS, D = 2, 256


def make_adapter(layers, time_freq_dim=32, seed=0):
    from lightx2v_amd import audio

    torch.manual_seed(seed)
    a = audio.AudioAdapter(128, HEADS, layers, audio_feature_dim=64, num_tokens=32, mlp_dims=(64, 64, 32 * 64), time_freq_dim=time_freq_dim, projection_transformer_layers=1)
    if time_freq_dim > 0:
        with torch.no_grad():
            for ca in a.ca:  # gates around 1: the residual is as large as the stream it joins
                ca.shift_scale_gate[:, 2] += 1.0
    audio_feat = torch.randn(1, 30, 64).cuda()
    return a.to("cuda", torch.bfloat16).eval(), audio_feat


@pytest.mark.parametrize("time_freq_dim", [32, 0])
def test_one_layer_vs_restatement(time_freq_dim):
    f, hw, tail = 3, 40, 5
    adapter, audio_feat = make_adapter(1, time_freq_dim)
    blocks = adapter(audio_feat, torch.tensor([500.0], device="cuda"), f, weight=0.75)
    assert sorted(blocks) == [0] and sorted(blocks[0]["kwargs"]) == ["ca_block", "dtype", "t_emb", "weight", "x"]
    kw = blocks[0]["kwargs"]
    grid = torch.tensor([[f, 5, 8]])
    x = (0.125 * torch.randn(f * hw + tail, D, generator=torch.Generator().manual_seed(1))).to(torch.bfloat16).cuda()  # a stream of the residual's size
    ref, r = R.modify_hidden_states(x, (f, 5, 8), kw["x"][0], R.params(kw["ca_block"]), kw["t_emb"], 0.75, HEADS)
    got = blocks[0]["modify_func"](x.clone(), grid, **kw)
    assert torch.equal(got[f * hw :], x[f * hw :]), "tail rows changed"
    assert float(r.norm()) > 0.1 * float(ref.norm())  # the case has a residual worth checking
    R.check(got, ref, r, f"one layer time_freq_dim={time_freq_dim}")
    # weight = 0: the gate row is 0, x + bf16(t * 0) = x
    got0 = blocks[0]["modify_func"](x.clone(), grid, **{**kw, "weight": 0.0})
    assert torch.equal(got0, x)


def test_wan_driver_with_audio_blocks():
    from lightx2v_amd import scheduler, synth, wan

    dims, wl = synth.WAN_DIMS["wan-tiny"], synth.WORKLOADS["wan-tiny"]
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=0).items()}
    lat, ctx, _ = synth.synth_inputs(dims, wl["target_shape"])
    cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=4)
    model, sch = wan.WanModel(cfg, wd), scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    sch.step_pre(0)
    embed, grid_sizes, (x0, *rest) = model.pre_infer.infer(model.pre_weight, {"text_encoder_output": {"context": [c.cuda() for c in ctx]}}, positive=True)
    tr, W = model.transformer_infer, model.transformer_weights
    run = lambda blocks: tr.infer(W, grid_sizes, embed, x0.clone(), *rest, audio_dit_blocks=blocks)
    plain = run(None)
    assert torch.equal(plain, run([]))

    adapter, audio_feat = make_adapter(dims["num_layers"])
    f = int(grid_sizes[0][0])
    blocks = adapter(audio_feat, torch.tensor([500.0], device="cuda"), f, weight=1.0)
    seen = []  # (x into modify_func, x out of it) per block

    def recording(func):
        def wrapped(hidden, grid, **kw):
            before = hidden.clone()
            out = func(hidden, grid, **kw)
            seen.append((before, out.clone()))
            return out

        return wrapped

    got = run([{i: {"modify_func": recording(b["modify_func"]), "kwargs": b["kwargs"]} for i, b in blocks.items()}])
    assert len(seen) == dims["num_layers"] and not torch.equal(got, plain)
    x = x0.clone()
    for i, (before, after) in enumerate(seen):  # block by block: the driver without audio, plus the restated residual
        x = tr.infer_block(W.blocks[i], grid_sizes, embed, x, *rest)
        assert torch.equal(x, before), f"block {i}: the block stack itself changed under audio_dit_blocks"
        kw = blocks[i]["kwargs"]
        ref, r = R.modify_hidden_states(x, tuple(grid_sizes[0].tolist()), kw["x"][0], R.params(kw["ca_block"]), kw["t_emb"], 1.0, HEADS)
        R.check(after, ref, r, f"wan-tiny block {i}")
        x = after.clone()
    assert torch.equal(x, got)
