"""world_size-1 worker for tests/test_gpu_dist.py: the Hunyuan Ulysses driver (ulysses.UlyssesHunyuanAttention.attend_blocked) over the real RCCL
backend on the one GPU of the box, as tests/_dist_gpu_worker_rccl1.py does for Wan's.  One `model.infer` of hunyuan-tiny (2 double + 3 single blocks:
5 joint attentions) plain, and one after `parallelize_hunyuan` with the head->seq exchange FORCED into its two-piece split-size form and a CommTimer
attached.  Spies on the two collectives record shapes, split arguments and the stream each call was issued under: per attention RCCL must have seen
3 seq->head exchanges, 2 head->seq pieces and the text rows' all-gather, plus the gather of the noise prediction, ALL on the one communication stream;
the copy-free path must have been taken; the timer must hold one `comm` bracket per enqueue and one `exposed` bracket per join."""
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
    from lightx2v_amd import hunyuan as hy, lib, synth, ulysses

    lib.init(0)
    dims = synth.HUNYUAN_DIMS["hunyuan-tiny"]
    ts = synth.HUNYUAN_WORKLOADS["hunyuan-tiny"]["target_shape"]
    n_attn = dims["double_blocks"] + dims["single_blocks"]
    assert n_attn == 5
    wd = {k: v.cuda() for k, v in synth.synth_hunyuan_weights(dims, seed=2).items()}
    lat, text_states, mask, ts2 = synth.synth_hunyuan_inputs(dims, ts, seed=5, valid_text=11)
    inputs = {"text_encoder_output": {"text_encoder_1_text_states": text_states.cuda(), "text_encoder_1_attention_mask": mask.cuda(), "text_encoder_2_text_states": ts2.cuda()}}
    a2a, gathers = [], []
    real_a2a, real_gather = dist.all_to_all_single, dist.all_gather_into_tensor

    def spy_a2a(out, inp, out_split=None, in_split=None, **kw):
        a2a.append((tuple(out.shape), tuple(inp.shape), out_split, in_split, torch.cuda.current_stream().cuda_stream))
        return real_a2a(out, inp, out_split, in_split, **kw)

    def spy_gather(out, inp, **kw):
        gathers.append((tuple(out.shape), tuple(inp.shape), None, None, torch.cuda.current_stream().cuda_stream))
        return real_gather(out, inp, **kw)

    outs = {}
    timer = ulysses.CommTimer()
    for mode in ("single", "ulysses"):
        cfg = hy.default_config(dims, infer_steps=4)
        model = hy.HunyuanModel(cfg, wd)
        sch = hy.HunyuanScheduler(cfg)
        sch.prepare(lat)
        model.set_scheduler(sch)
        if mode == "ulysses":
            ulysses.parallelize_hunyuan(model)
            pa = model.transformer_infer.parallel_attention
            pa.split_head2seq = "force"
            pa.comm_timer = timer
            dist.all_to_all_single, dist.all_gather_into_tensor = spy_a2a, spy_gather
        sch.step_pre(1)
        try:
            model.infer(inputs)
        finally:
            dist.all_to_all_single, dist.all_gather_into_tensor = real_a2a, real_gather
        outs[mode] = sch.noise_pred.float().cpu()
        assert sch.latents.shape == lat.shape
    assert pa.copies == 0 and pa._buffers, "the fused driver must take the copy-free blocked exchange path (double and single blocks)"
    streams = {c[4] for c in a2a + gathers}
    assert streams == {pa.comm_stream.cuda_stream} and streams != {torch.cuda.default_stream().cuda_stream}, f"collectives issued under {len(streams)} streams (the one communication stream expected)"
    plain = [c for c in a2a if c[2] is None]
    split = [c for c in a2a if c[2] is not None]
    print(f"collectives per forward: all_to_all_single {len(plain)} without / {len(split)} with split sizes, all_gather_into_tensor {len(gathers)}")
    assert len(plain) == 3 * n_attn and all(c[0] == c[1] and c[0][0] == 1 for c in plain), (len(plain), plain[:3])
    assert len(split) == 2 * n_attn and all(len(c[2]) == 1 and c[2] == c[3] and c[0][0] == c[2][0] == c[1][0] for c in split), (len(split), split[:4])
    assert len(gathers) == n_attn + 1, (len(gathers), gathers[:3])
    torch.cuda.synchronize()
    timer.enabled = False
    c_ms, e_ms, n_comm = timer.totals_ms()
    print(f"brackets: comm {n_comm} ({c_ms:.3f} ms), exposed {len(timer.exposed)} ({e_ms:.3f} ms)")
    # comm: per attention the seq->head group (1) + 2 head->seq pieces + the text gather, + the final gather; exposed: 2 joins per attention + the final one
    assert n_comm == 4 * n_attn + 1 and len(timer.exposed) == 2 * n_attn + 1 and c_ms > 0.0 and e_ms >= 0.0, (n_comm, len(timer.exposed), c_ms, e_ms)
    a, b = outs["single"], outs["ulysses"]
    assert a.shape == b.shape and torch.isfinite(a).all()
    rel = ((a - b).norm() / a.norm()).item()
    print(f"ulysses vs plain relative L2 {rel:.3e}")
    assert rel < 5e-3, f"ulysses over RCCL vs single-GPU relative L2 {rel:.3e}"
    dist.barrier()
    torch.cuda.synchronize()
    print(f"DIST_GPU_HUNYUAN_RCCL1_OK rel={rel:.2e}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
