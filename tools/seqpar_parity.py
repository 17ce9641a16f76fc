#!/usr/bin/env python3
"""What the sequence-parallel drivers (lightx2v_amd/ulysses.py, ring.py) ask of RCCL and of the streams, for comparing two versions of the package
(a refactor against its parent commit) at world size 1 over the real "nccl" backend on one GPU:

    python tools/seqpar_parity.py path/to/parent/tree > parent.jsonl      (the directory that holds that version's lightx2v_amd/; a fresh process each)
    python tools/seqpar_parity.py .                   > head.jsonl
    python tools/seqpar_parity.py --table parent.jsonl head.jsonl

Per configuration one denoise step (`model.infer`) on synth weights; recorded, in this process only, by wrapping the `torch.distributed` collectives
and `torch.cuda.Stream.wait_stream`: the sha256 of the noise prediction as float32 bytes, the ordered trace of every collective (name, argument
shapes, split sizes, the role of the stream it was issued under) and of every wait (waiter role <- waited-on role), and the number of CommTimer
brackets (event records, not waits: they are not part of the trace).  Roles: "comm" = the driver's communication stream, "default", and
"compute0", "compute1", ... for any other stream in order of first appearance (the CFG branches' streams)."""
import hashlib
import json
import os
import sys

COLLECTIVES = ("all_to_all_single", "all_gather_into_tensor", "all_reduce", "broadcast", "barrier", "batch_isend_irecv", "all_to_all", "all_gather", "reduce_scatter_tensor")
CONFIGS = ("wan ulysses blocked, split forced", "wan ulysses row-major", "wan ulysses cfg_branch_streams", "wan ring", "hunyuan ulysses blocked, split forced", "hunyuan ulysses row-major")


def table(parent, head):
    rows = [[json.loads(ln) for ln in open(p) if ln.startswith("{")] for p in (parent, head)]
    print(f"{'configuration':42s} {'output parent':17s} {'output head':17s} equal  events {'trace parent':17s} {'trace head':17s} equal  brackets parent  head (comm/exposed)")
    ok = True
    for a, b in zip(*rows):
        assert a["config"] == b["config"]
        eo, et = a["output"] == b["output"], a["trace"] == b["trace"] and a["events"] == b["events"]
        ok = ok and eo and et and len(rows[0]) == len(rows[1]) == len(CONFIGS)
        print(f"{a['config']:42s} {a['output'][:16]}  {b['output'][:16]}  {'yes' if eo else 'NO':5s} {b['events']:7d} {a['trace'][:16]}  {b['trace'][:16]}  {'yes' if et else 'NO':5s}  "
              f"{a['brackets'][0]:3d}/{a['brackets'][1]:<3d}         {b['brackets'][0]:3d}/{b['brackets'][1]:<3d}")
    print(f"\n{'All' if ok else 'NOT all'} {len(CONFIGS)} rows equal in both columns.")
    return 0 if ok else 1


def main(root):
    sys.path.insert(0, os.path.abspath(root))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29557"), ("RANK", "0"), ("WORLD_SIZE", "1")):
        os.environ.setdefault(k, v)
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    from lightx2v_amd import hunyuan as hy, lib, scheduler, synth, ulysses, wan

    lib.init(0)
    events = []
    sid = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    shapes = lambda a: [list(t.shape) if isinstance(t, torch.Tensor) else t for t in a if isinstance(t, (torch.Tensor, list)) or t is None]  # noqa: E731

    def wrap(name, real):
        def spy(*a, **kw):
            events.append(("coll", name, shapes(a), sorted(k for k in kw if k != "group"), sid()))
            return real(*a, **kw)

        return spy

    for name in COLLECTIVES:
        setattr(dist, name, wrap(name, getattr(dist, name)))
    real_wait = torch.cuda.Stream.wait_stream

    def wait_spy(self, other):
        events.append(("wait", self.cuda_stream, other.cuda_stream))
        return real_wait(self, other)

    torch.cuda.Stream.wait_stream = wait_spy

    def record(config, model, pa, inputs, noise):
        timer = pa.comm_timer = ulysses.CommTimer()
        events.clear()
        model.infer(inputs)
        torch.cuda.synchronize()
        roles = {torch.cuda.default_stream().cuda_stream: "default"}
        if pa.comm_stream is not None:
            roles[pa.comm_stream.cuda_stream] = "comm"
        role = lambda s: roles.setdefault(s, f"compute{sum(1 for r in roles.values() if r.startswith('compute'))}")  # noqa: E731
        trace = [[e[0], e[1], e[2], e[3], role(e[4])] if e[0] == "coll" else ["wait", role(e[1]), role(e[2])] for e in events]
        print(json.dumps({"config": config, "output": hashlib.sha256(noise().float().cpu().contiguous().numpy().tobytes()).hexdigest(), "events": len(trace),
                          "trace": hashlib.sha256(json.dumps(trace, default=str).encode()).hexdigest(), "brackets": [len(timer.comm), len(timer.exposed)],
                          "collectives": sum(1 for e in trace if e[0] == "coll"), "waits": sum(1 for e in trace if e[0] == "wait")}), flush=True)

    dims = dict(synth.WAN_DIMS["wan-tiny"], dim=512, num_heads=4, ffn_dim=1024, num_layers=2)
    ts = (16, 3, 12, 10)
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=3).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    for config, pat, kw, blocked in ((CONFIGS[0], "ulysses", {}, True), (CONFIGS[1], "ulysses", {}, False), (CONFIGS[2], "ulysses", {"cfg_branch_streams": True}, True), (CONFIGS[3], "ring", {}, True)):
        model = wan.WanModel(wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=4, parallel_attn_type=pat, **kw), wd)
        model.transformer_infer.blocked_exchange = blocked
        pa = model.transformer_infer.parallel_attention
        if pat == "ulysses":
            pa.split_head2seq = "force"
        sch = scheduler.WanScheduler(model.config, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        sch.step_pre(0)
        record(config, model, pa, inputs, lambda: sch.noise_pred)

    hdims = synth.HUNYUAN_DIMS["hunyuan-tiny"]
    hwd = {k: v.cuda() for k, v in synth.synth_hunyuan_weights(hdims, seed=2).items()}
    hlat, text_states, mask, ts2 = synth.synth_hunyuan_inputs(hdims, synth.HUNYUAN_WORKLOADS["hunyuan-tiny"]["target_shape"], seed=5, valid_text=11)
    hinputs = {"text_encoder_output": {"text_encoder_1_text_states": text_states.cuda(), "text_encoder_1_attention_mask": mask.cuda(), "text_encoder_2_text_states": ts2.cuda()}}
    for config, blocked in ((CONFIGS[4], True), (CONFIGS[5], False)):
        cfg = hy.default_config(hdims, infer_steps=4)
        model = hy.HunyuanModel(cfg, hwd)
        sch = hy.HunyuanScheduler(cfg)
        sch.prepare(hlat)
        model.set_scheduler(sch)
        ulysses.parallelize_hunyuan(model)
        pa = model.transformer_infer.parallel_attention
        pa.split_head2seq = "force"
        if not blocked:
            pa.blocked_ok = lambda hd, mlp: False  # the driver then takes the row-major entry (UlyssesHunyuanAttention.__call__)
        sch.step_pre(1)
        record(config, model, pa, hinputs, lambda: sch.noise_pred)
        assert (pa.copies == 0) == blocked
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--table":
        sys.exit(table(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
