"""Worker for tests/test_gpu_ring.py (world 2 and 4): every rank drives cuda:0 (the GPU box has one MI355X), so the process group is gloo and the
collectives ring.py issues — dist.batch_isend_irecv for the ring hops, all_gather_into_tensor for the gather — are wrapped, here in the worker only, to
stage device tensors through host memory.  Everything else is the product path: the carry launches (x2v_attn_fwd_bf16_vt_carry), the V^T chunks, the
two receive buffer pairs, the communication stream and its joins, the sharded RoPE offsets, the padding.
Checks, with the bounds of tests/_dist_gpu_worker.py: the ring-sharded conditional forward against the CPU oracle (<= 2e-2) and no further from it than
the single-GPU HIP forward (x 1.25 + 1e-3), the CFG step against the oracle (<= 5e-2); N launches per attention with the carry bits of a chain whose
last launch writes bf16; no host synchronisation inside RingAttention.__call__ other than the shim's own.  The ring-vs-single-GPU relative L2 is
printed, not bounded.  World 2 also runs a 3-head model, which Ulysses refuses."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATE = {"in_call": False, "in_shim": False, "syncs": 0}


def _host_staged(fn):
    def wrapped(out, inp, *a, **kw):
        if out.is_cuda:
            STATE["in_shim"] = True
            torch.cuda.current_stream().synchronize()
            STATE["in_shim"] = False
            o, i = torch.empty(out.shape, dtype=out.dtype), inp.detach().cpu()
            r = fn(o, i, *a, **kw)
            out.copy_(o)
            return r
        return fn(out, inp, *a, **kw)

    return wrapped


class _Done:
    def wait(self):
        return True


def _host_staged_p2p(real):
    """dist.batch_isend_irecv on device tensors: the sends are copied to the host once the current stream has produced them, the batch runs over
    gloo to completion, the receives are copied back on the current stream (so the stream order the driver set up still holds)."""

    def wrapped(ops):
        if not any(op.tensor.is_cuda for op in ops):
            return real(ops)
        STATE["in_shim"] = True
        torch.cuda.current_stream().synchronize()
        STATE["in_shim"] = False
        host = [op.tensor.detach().cpu() if op.op is dist.isend else torch.empty(op.tensor.shape, dtype=op.tensor.dtype) for op in ops]
        for req in real([dist.P2POp(op.op, t, op.peer, group=op.group) for op, t in zip(ops, host)]):
            req.wait()
        for op, t in zip(ops, host):
            if op.op is dist.irecv:
                op.tensor.copy_(t)
        return [_Done()]

    return wrapped


def _count_host_syncs():
    def counted(fn):
        def wrapped(*a, **kw):
            if STATE["in_call"] and not STATE["in_shim"]:
                STATE["syncs"] += 1
            return fn(*a, **kw)

        return wrapped

    torch.cuda.synchronize = counted(torch.cuda.synchronize)
    torch.cuda.Stream.synchronize = counted(torch.cuda.Stream.synchronize)
    torch.cuda.Event.synchronize = counted(torch.cuda.Event.synchronize)


def run_model(heads, ts, n, r, with_oracle_cfg):
    from lightx2v_amd import lib, ring, scheduler, synth, wan

    dims = dict(synth.WAN_DIMS["wan-tiny"], dim=128 * heads, num_heads=heads, ffn_dim=1024, num_layers=2)
    wd = synth.synth_wan_weights(dims, seed=3)
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    S = synth.seq_len_of(ts)
    assert S % n == 0, "these grids divide by the group (a padded one differs from the single-GPU forward by design: the pad rows are keys)"
    outs, conds, log = {}, {}, []
    for mode in ("single", "ring"):
        cfg = wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=4, parallel_attn_type=None if mode == "single" else "ring")
        model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
        if mode == "ring":
            pa = model.transformer_infer.parallel_attention
            assert isinstance(pa, ring.RingAttention) and getattr(model, "_cfg_interleave", None) is None
            real_fn, real_call = pa.attn_fn, ring.RingAttention.__call__

            def spy(q, k, vt, num_heads, state=None, last=False, prescaled=False):
                steps = state.steps if state is not None else 0
                res = real_fn(q, k, vt, num_heads, state=state, last=last, prescaled=prescaled)
                log.append((steps, last, tuple(k.shape), tuple(vt.shape), res.dtype if last else res.acc.dtype, tuple(res.shape) if last else None, prescaled))
                return res

            def call(self, *a, **kw):
                STATE["in_call"] = True
                try:
                    return real_call(self, *a, **kw)
                finally:
                    STATE["in_call"] = False

            pa.attn_fn = spy
            ring.RingAttention.__call__ = call
        sch = scheduler.WanScheduler(cfg, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        sch.step_pre(0)
        conds[mode] = model._forward(inputs, True).float().cpu()
        model.infer(inputs)
        outs[mode] = sch.noise_pred.float().cpu()
        sch.step_post()
        assert torch.isfinite(sch.latents).all()
        if mode == "ring":
            ring.RingAttention.__call__ = real_call
            n_attn = 3 * dims["num_layers"]  # the conditional forward alone, then the two forwards of the CFG step
            s_loc = S // n
            assert pa.calls == n_attn and len(log) == n * n_attn, (pa.calls, len(log))
            for a in range(n_attn):
                for s in range(n):
                    steps, last, kshape, vtshape, dtype, oshape, pre = log[a * n + s]
                    assert steps == s and last == (s == n - 1) and pre, (a, s, log[a * n + s])  # CARRY_IN from step 1 on, CARRY_OUT until the last
                    assert kshape == (s_loc, heads * 128) and vtshape == (heads, (s_loc + 63) // 64, 128, 64)
                    assert dtype == (torch.bfloat16 if last else torch.float32) and (oshape == (s_loc, heads * 128)) == last
            assert pa.launches == [(s > 0, s < n - 1) for s in range(n)] and pa.host_syncs == 0
            assert pa.bytes_sent == (n - 1) * (s_loc * heads * 128 + heads * ((s_loc + 63) // 64) * 128 * 64) * 2
            assert len(pa._buffers) == 1 and len(pa._states) == 1, "receive buffers and the state are allocated once per shape"
            assert pa.comm_stream is not None and STATE["syncs"] == 0, f"{STATE['syncs']} host synchronisations inside RingAttention.__call__"
    from oracle import wan_oracle as O

    ref_c = O.wan_forward(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx)
    ec = {m: ((conds[m] - ref_c).norm() / ref_c.norm()).item() for m in ("single", "ring")}
    assert ec["ring"] <= 2e-2 and ec["single"] <= 2e-2, f"rank {r} H={heads}: conditional forward vs oracle {ec}"
    assert ec["ring"] <= 1.25 * ec["single"] + 1e-3, f"rank {r} H={heads}: ring conditional forward further from the oracle than the single-GPU one {ec}"
    e_cfg = None
    if with_oracle_cfg:
        ref = O.wan_model_infer(wd, dims, lat.to(torch.bfloat16), sch.timesteps[0].cpu(), ctx, ctx_null, cfg["sample_guide_scale"])
        e_cfg = {m: ((outs[m] - ref).norm() / ref.norm()).item() for m in ("single", "ring")}
        assert e_cfg["ring"] <= 5e-2 and e_cfg["single"] <= 5e-2, f"rank {r} H={heads}: CFG step vs oracle {e_cfg}"
    rel = ((outs["single"] - outs["ring"]).norm() / outs["single"].norm()).item()
    relc = ((conds["single"] - conds["ring"]).norm() / conds["single"].norm()).item()
    return f"H={heads} N={n} ring-vs-single relL2 cfg {rel:.3e} cond {relc:.3e} oracle cond {ec['ring']:.3e} (single {ec['single']:.3e}) cfg {e_cfg and round(e_cfg['ring'], 5)}"


def main():
    dist.init_process_group("gloo")
    r, n = dist.get_rank(), dist.get_world_size()
    dist.all_gather_into_tensor = _host_staged(dist.all_gather_into_tensor)
    dist.batch_isend_irecv = _host_staged_p2p(dist.batch_isend_irecv)
    _count_host_syncs()
    torch.cuda.set_device(0)
    from lightx2v_amd import lib

    lib.init(0)
    # world 2: grid 3 x 6 x 5 = 90 tokens, 45 per rank; world 4: 3 x 8 x 6 = 144, 36 per rank (both ragged against the 64-key tile and the 32-row wave)
    ts = (16, 3, 12, 10) if n == 2 else (16, 3, 16, 12)
    lines = [run_model(4, ts, n, r, True)]
    if n == 2:
        lines.append(run_model(3, ts, n, r, True))  # 3 heads on 2 ranks: num_heads % world_size != 0
    dist.barrier()
    if r == 0:
        for ln in lines:
            print("RING_GPU " + ln)
        print("DIST_GPU_RING_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
