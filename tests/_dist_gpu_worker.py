"""world_size-2 worker for tests/test_gpu_dist.py: BOTH ranks drive cuda:0 (the GPU box has one MI355X), so the
collectives cannot be RCCL; the process group is gloo and the two collective entry points ulysses.py uses are
wrapped (here, in the test only) to stage device tensors through host memory.  Everything else — the HIP
kernels, the sharded RoPE offsets, head splitting, padding, stream joins — is the product path.
Checks: the Ulysses-sharded Wan CFG step against the CPU ORACLE's noise prediction for the same weights and inputs (wan/model.py:197-226
restated; tolerance of tests/test_gpu_model.py's CFG step), the conditional forward alone against the oracle's forward at the model-level 2e-2 (the
tight oracle leg: no CFG amplification), and — a further leg, not a substitute — against the single-GPU HIP forward."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _host_staged(fn):
    def wrapped(out, inp, *a, **kw):
        if out.is_cuda:
            torch.cuda.current_stream().synchronize()
            o, i = torch.empty(out.shape, dtype=out.dtype), inp.detach().cpu()
            r = fn(o, i, *a, **kw)
            out.copy_(o)
            return r
        return fn(out, inp, *a, **kw)

    return wrapped


def main():
    dist.init_process_group("gloo")
    r, n = dist.get_rank(), dist.get_world_size()
    dist.all_to_all_single = _host_staged(dist.all_to_all_single)
    dist.all_gather_into_tensor = _host_staged(dist.all_gather_into_tensor)
    torch.cuda.set_device(0)
    from lightx2v_amd import lib, scheduler, synth, wan

    lib.init(0)
    # 4 heads so that H % 2 == 0 with 2 heads per rank; S = 3*6*5 = 90 tokens -> 45 per rank (ragged vs the 32/64 tiles).  World 4 (all ranks
    # on the one GPU): 4 heads, one per rank, 3*8*6 = 144 tokens -> 36 per rank.  (A token count the group does not divide is zero-padded
    # and — a reference quirk kept bit for bit, ulysses/attn.py:60-66 — the pad rows then take part in the attention as keys, so the sharded
    # forward legitimately differs from the single-GPU one: 2.9e-2 with 6 pad rows among 96.  The 720p grids divide by 8.)
    heads = max(4, n)
    dims = dict(synth.WAN_DIMS["wan-tiny"], dim=128 * heads, num_heads=heads, ffn_dim=1024, num_layers=2)
    ts = (16, 3, 12, 10) if n == 2 else (16, 3, 16, 12)
    wd = synth.synth_wan_weights(dims, seed=3)
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    outs, conds = {}, {}
    # X2V_WORKER_FP8=1: the same run with the w8a8 operator class (mm_weight.py:287-319 restated): its N-blocked output (x2v_gemm_fp8_blocked) writes the
    # seq->head send buffers, its quantisation pass de-blocks the head->seq receive buffer (x2v_quant_fp8_rowwise_blocked) — the copy-free path, round 5
    fp8 = os.environ.get("X2V_WORKER_FP8") == "1"
    extra = {"mm_config": {"mm_type": "W-fp8-channel-sym-A-fp8-channel-sym-dynamic-Hip", "weight_auto_quant": True}} if fp8 else {}
    for mode in ("single", "ulysses", "ulysses-sequential"):
        cfg = wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=4, parallel_attn_type=None if mode == "single" else "ulysses",
                                 cfg_branch_streams=(mode == "ulysses"), **extra)
        model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
        sch = scheduler.WanScheduler(cfg, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        sch.step_pre(0)
        if mode != "ulysses-sequential":
            conds[mode] = model._forward(inputs, True).float().cpu()  # one branch, no CFG amplification: the TIGHT oracle leg below
        model.infer(inputs)
        outs[mode] = sch.noise_pred.float().cpu()
        if mode.startswith("ulysses"):
            pa = model.transformer_infer.parallel_attention
            assert pa.copies == 0 and pa._buffers, "the fused driver must take the copy-free blocked exchange path"
            il = model._cfg_interleave
            assert (il._pa_b is not None and il._pa_b._buffers and il._pa_b.copies == 0) == (mode == "ulysses"), "CFG-branch interleave: wrong path taken"
        sch.step_post()
        assert torch.isfinite(sch.latents).all()
    # the two CFG branches interleaved on two compute streams (the default) against the sequential order: same kernels on the same operands
    assert torch.equal(outs["ulysses"], outs["ulysses-sequential"]), "CFG-branch interleave changed the result"
    if fp8:
        # per-token activation scales and per-channel weight scales do not depend on how rows are partitioned: the sharded w8a8 forward is the
        # single-GPU one on re-grouped tiles (the w8a8 forward itself is compared with the oracle in tests/test_gpu_model.py / test_gpu_full_size.py)
        rel = ((outs["single"] - outs["ulysses"]).norm() / outs["single"].norm()).item()
        relc = ((conds["single"] - conds["ulysses"]).norm() / conds["single"].norm()).item()
        assert rel < 5e-3 and relc < 5e-3, f"rank {r}: w8a8 ulysses vs single-GPU relative L2 {rel:.3e} (conditional forward {relc:.3e})"
        dist.barrier()
        if r == 0:
            print(f"DIST_GPU_OK rel={rel:.2e} (w8a8)")
        dist.destroy_process_group()
        return
    from oracle import wan_oracle as O

    ref = O.wan_model_infer(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx, ctx_null, cfg["sample_guide_scale"])
    for mode in ("single", "ulysses"):
        e = ((outs[mode] - ref).norm() / ref.norm()).item()
        assert e <= 5e-2, f"rank {r}: {mode} vs oracle relative L2 {e:.3e}"  # guide scale 6 amplifies the per-branch 1e-2 (as in smoke())
    # the tight oracle leg: the conditional forward alone — sharded over the ranks and on one GPU — against the oracle's forward
    # at the model-level forward tolerance (2e-2), and the sharded one no further from the oracle than the single-GPU one (x 1.25)
    ref_c = O.wan_forward(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx)
    ec = {m: ((conds[m] - ref_c).norm() / ref_c.norm()).item() for m in ("single", "ulysses")}
    assert ec["ulysses"] <= 2e-2 and ec["single"] <= 2e-2, f"rank {r}: conditional forward vs oracle {ec}"
    assert ec["ulysses"] <= 1.25 * ec["single"] + 1e-3, f"rank {r}: sharded conditional forward further from the oracle than the single-GPU one {ec}"
    a, b = outs["single"], outs["ulysses"]
    rel = ((a - b).norm() / a.norm()).item()
    # same kernels on re-partitioned rows: the GEMM/attention tiles see different row groupings, not different math
    assert rel < 5e-3, f"rank {r}: ulysses vs single-GPU relative L2 {rel:.3e}"
    e_u, e_s = ((b - ref).norm() / ref.norm()).item(), ((a - ref).norm() / ref.norm()).item()
    assert e_u <= 1.25 * e_s + 1e-3, f"rank {r}: the sharded forward is further from the oracle ({e_u:.3e}) than the single-GPU one ({e_s:.3e})"
    dist.barrier()
    if r == 0:
        print(f"DIST_GPU_OK rel={rel:.2e}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
