"""world_size-1 worker for tests/test_gpu_ring.py over the real RCCL backend ("nccl" on ROCm) on the one GPU of the box: a ring of one rank is a
single launch with neither carry bit, so the whole RingAttention call — the transposition, the launch through x2v_attn_fwd_bf16_vt_carry — equals the
single-GPU launch bit for bit, and the ring-wrapped Wan forward (shard, block stack, gather over RCCL on the communication stream) equals the plain one."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    from lightx2v_amd import lib, ring, scheduler, synth, wan

    lib.init(0)
    g = torch.Generator().manual_seed(2)
    S, H = 256 + 90, 3
    qkv = torch.randn(S, 3 * H * 128, generator=g).to(torch.bfloat16).cuda()  # views of a fused projection, as the driver hands them over
    q, k, v = qkv[:, : H * 128], qkv[:, H * 128 : 2 * H * 128], qkv[:, 2 * H * 128 :]
    pa = ring.RingAttention()
    for variant in (lib.ATTN_FAST | lib.ATTN_Q_PRESCALED, lib.ATTN_FAST):
        out = pa(q, k, v, H, 128, variant=variant)
        assert pa.launches == [(False, False)] and not pa._buffers and not pa._states and pa.bytes_sent == 0
        assert torch.equal(out, lib.attention(q, k, v, H, 128, variant=variant)), "a ring of one differs from the single-GPU launch"

    dims = dict(synth.WAN_DIMS["wan-tiny"], dim=384, num_heads=3, ffn_dim=1024, num_layers=2)
    ts = (16, 3, 12, 10)
    wd = synth.synth_wan_weights(dims, seed=3)
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    outs = {}
    for mode in ("single", "ring"):
        cfg = wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=4, parallel_attn_type=None if mode == "single" else "ring")
        model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
        sch = scheduler.WanScheduler(cfg, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        sch.step_pre(0)
        outs[mode] = model._forward(inputs, True).float().cpu()
        if mode == "ring":
            pa = model.transformer_infer.parallel_attention
            assert pa.calls == dims["num_layers"] and pa.launches == [(False, False)] and pa.comm_stream is not None  # the gather ran on the communication stream
    assert torch.isfinite(outs["single"]).all()
    assert torch.equal(outs["single"], outs["ring"]), "world-1 ring forward over RCCL differs from the plain forward"
    dist.barrier()
    torch.cuda.synchronize()
    print("DIST_GPU_RING_RCCL1_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
