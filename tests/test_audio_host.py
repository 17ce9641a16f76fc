"""The audio model's host logic without a GPU: the combinations the Wan drivers refuse, and the adapter's step-invariant caches."""
import pytest
import torch


def test_audio_blocks_refused_where_unbuilt():
    from lightx2v_amd import synth, ulysses, wan

    tr = wan.WanTransformerInfer(wan.default_config(synth.WAN_DIMS["wan-tiny"]))
    blocks, args = [{0: {"modify_func": None, "kwargs": {}}}], (None,) * 8
    tr._pair = (48, 64)
    with pytest.raises(NotImplementedError, match="pair pass"):
        tr.infer(*args, audio_dit_blocks=blocks)
    tr._pair, tr.parallel_attention = None, object()
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        tr.infer(*args, audio_dit_blocks=blocks)

    class Stub:
        group = None

        def world(self):
            return 2, 0

    tr2 = wan.WanTransformerInfer(wan.default_config(synth.WAN_DIMS["wan-tiny"]))
    ulysses.shard_wan_block_stack(type("M", (), {"transformer_infer": tr2})(), Stub())
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        tr2.infer(*args, audio_dit_blocks=blocks)


def test_adapter_kv_computed_once_across_steps(monkeypatch):
    from lightx2v_amd import audio

    torch.manual_seed(0)
    adapter = audio.AudioAdapter(128, 2, 2, audio_feature_dim=64, num_tokens=32, mlp_dims=(64, 64, 32 * 64), time_freq_dim=32, projection_transformer_layers=1).eval()
    calls = []
    monkeypatch.setattr(audio.PerceiverAttentionCA, "compute_kv", lambda self, x: calls.append(self) or torch.zeros(x.shape[1] * x.shape[2], 512))
    audio_feat, tokens = torch.randn(1, 30, 64), []
    for step in range(2):
        blocks = adapter(audio_feat, torch.tensor([900.0 - 400 * step]), 3)
        assert sorted(blocks) == [0, 1]
        for b in blocks.values():
            k, v = b["kwargs"]["ca_block"].kv(b["kwargs"]["x"])
            assert k.shape == v.shape == (3 * 128, 256)
        tokens.append(blocks[0]["kwargs"]["x"])
    assert tokens[0] is tokens[1] and tokens[0].shape == (1, 3, 128, 64)
    assert len(calls) == 2 and calls[0] is adapter.ca[0] and calls[1] is adapter.ca[1]  # once per layer, not per step
    adapter(torch.randn(1, 30, 64), torch.tensor([100.0]), 3)[0]["kwargs"]["ca_block"].kv(adapter._tokens[3])
    assert len(calls) == 3  # another audio tensor: recomputed
