"""Worker for tests/test_gpu_stream_order.py: the sequence-parallel drivers (ulysses.UlyssesAttention, ulysses.UlyssesHunyuanAttention,
ring.RingAttention, all on ulysses.CommStreams) and wan.CfgBranchStreams, on one GPU in one process, in a state where every stream wait decides a
result.  `torch.distributed`'s collectives are replaced by stand-ins that run on the CURRENT stream and never touch the host
(tests/stream_order.py); the group is gloo at world 1 and only has to exist.  X2V_STREAM_ORDER_CASE picks the case:

    wan-blocked    wan-tiny (dim 512, 4 heads, 2 layers, ts (16, 3, 12, 10)), 2 CFG steps, fused blocked path, head->seq forced into two pieces
    wan-cfg        the same with cfg_branch_streams=True: two compute streams feed one communication stream
    row-major      UlyssesAttention.__call__ on 96 rows x 4 heads with a begin_exchange'd v
    hunyuan        hunyuan-tiny with padded text: UlyssesHunyuanAttention.attend_blocked through the fused driver
    ring           RingAttention.__call__ as one rank of an emulated ring: (N, r) = (4, 0), (4, 2), (2, 1), 90 rows per rank, 3 heads
    cfg-single     wan.CfgBranchStreams without a process group

Two regimes.  "comm": every stand-in collective fills its receive tensor with NaN, runs a device-side delay, then copies.  "compute": the
stand-ins are immediate and a delay sits on the compute stream in front of the producers of every send buffer (the head of every block; every
carry launch of the ring; the operands of a direct call), and on the calling stream in front of `forward_pair` where there are branch streams.
The delay is 20 x the event-timed duration of the undelayed driver call, at least 2 ms.

Per case: (1) under both regimes the result equals, bit for bit, the driver run with overlap=False and no delay (and the plain single-GPU forward
for the Wan models); (2) with the waits of ONE role turned into no-ops, under the regime aimed at that role, the result differs or holds NaN — the
proof that the delay was long enough for (1) to have failed; (3) no host synchronisation inside a driver call.  Before every run the drivers'
buffers are filled with NaN and, for the models and the row-major call, the same pass runs once on OTHER inputs: a run repeats the allocations
of the one before it, so memory read too early would otherwise hold the previous run's correct data.  X2V_STREAM_ORDER_PROFILE names a
file that receives the measured durations and delays (profiles/seqpar_stream_order.txt is one run's)."""
import os
import sys

# The calling stream, the communication stream and two branch streams must each have a hardware queue of their own: streams that share one are
# ordered by the runtime whatever the driver waits for (Harness.require_independent checks that they are not).  Read when the runtime starts.
os.environ["GPU_MAX_HW_QUEUES"] = "8"

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import stream_order as so  # noqa: E402

FACTOR, FLOOR_MS = 20.0, 2.0
DECOY_SEED = 7
CALLING_UNITS = 2  # delays on the calling stream in front of forward_pair: it must outlast the one at the head of a branch, enqueued just behind it


class Harness:
    def __init__(self, case):
        self.case = case
        self.delay = so.Delay()
        self.coll = so.StandIns(self.delay)
        self.waits = so.WaitFilter()
        self.syncs = so.HostSyncs()
        self.delay_ms, self.regime = 0.0, None
        self.lines = [f"{case}: delay by {self.delay.kind}, a 2 ms request measured {self.delay.check_ms:.3f} ms"]
        self.coll.install()

    # -- hooks the cases place in front of producers ------------------------------------------------------------------------
    def compute_delay(self, units=1):
        if self.regime == "compute":
            for _ in range(units):
                self.delay(self.delay_ms)

    def arm(self, regime, role):
        torch.cuda.synchronize()
        self.regime = regime
        self.coll.comm_delay_ms = self.delay_ms if regime == "comm" else 0.0
        self.waits.role, self.waits.skipped = role, 0
        self.syncs.count = 0
        self.coll.calls.clear()

    def disarm(self):
        self.regime, self.coll.comm_delay_ms, self.waits.role = None, 0.0, None
        torch.cuda.synchronize()

    def say(self, line):
        self.lines.append(f"{self.case}: {line}")
        print("STREAM_ORDER " + self.lines[-1], flush=True)

    # -- the three assertions -------------------------------------------------------------------------------------------------
    def require_independent(self, name, streams):
        """streams: {role name: stream}.  Every pair must be able to run side by side: streams that share a hardware queue are ordered by the
        runtime, whatever the driver waits for, and a control on them could not fail."""
        shared = [f"{b} behind {a}" for a, x in streams.items() for b, y in streams.items() if a != b and so.serialized_behind(x, y, self.delay)]
        self.say(f"{name}: streams {', '.join(streams)}: " + ("pairwise independent" if not shared else "SERIALISED by the runtime: " + "; ".join(shared)))
        assert not shared, f"{name}: the runtime serialises {shared} (too few hardware queues for these streams): no delay can expose a missing wait between them"

    def check(self, name, run, ref, controls, regimes=("comm", "compute"), count_syncs=True, observe=None, streams=None):
        """run(regime, role) -> CPU tensor.  ref: the overlap=False result.  controls: (regime, role) pairs.  observe(out, ref) -> how many
        elements of a control's result show the missing wait (default: NaN or different).  streams() -> {role name: stream} once a run has made them."""
        assert torch.isfinite(ref).all(), f"{name}: the reference is not finite"
        self.delay_ms = 0.0
        out = run(None, None)  # streams, buffers and loaded kernels exist from here on: the timed run below measures the call alone
        assert torch.equal(out, ref), f"{name}: overlap=True without delays differs from overlap=False in {so.differing(out, ref)} elements"
        if streams is not None:
            self.require_independent(name, dict(calling=torch.cuda.default_stream(), **streams()))
        self.syncs.timing = True
        out = run(None, None)
        self.syncs.timing = False
        calls = self.syncs.take_durations_ms()
        assert calls, f"{name}: no driver call was timed"
        assert torch.equal(out, ref), f"{name}: overlap=True without delays differs from overlap=False in {so.differing(out, ref)} elements"
        call_ms = max(calls)
        self.delay_ms = max(FACTOR * call_ms, FLOOR_MS)
        self.say(f"{name}: {len(calls)} driver calls, longest {call_ms:.3f} ms -> delay {self.delay_ms:.3f} ms")
        for regime in regimes:
            out = run(regime, None)
            n = so.differing(out, ref)
            self.say(f"{name}: positive, slow {regime}: {n} of {ref.numel()} elements differ, host synchronisations in driver calls {self.syncs.count}, waits by role {dict(self.waits.seen)}")
            assert n == 0, f"{name}, slow {regime}: {n} of {ref.numel()} elements differ from the overlap=False result: a wait is missing or misplaced"
            if count_syncs:
                assert self.syncs.count == 0, f"{name}, slow {regime}: {self.syncs.count} host synchronisations inside driver calls"
        equal = []
        for regime, role in controls:
            out = run(regime, role)
            n = (observe or so.differing)(out, ref)
            self.say(f"{name}: control, slow {regime}, {role} made a no-op ({self.waits.skipped} waits): {n} of {ref.numel()} elements differ or are NaN")
            assert self.waits.skipped > 0, f"{name}: no wait has the role {role}"
            if n == 0:
                equal.append(f"without {role} the result is still bit-equal under slow {regime}")
        assert not equal, f"{name}: {'; '.join(equal)}: the regime does not reach that wait"

    def finish(self):
        path = os.environ.get("X2V_STREAM_ORDER_PROFILE")
        if path:
            try:
                with open(path, "a") as f:
                    f.write("\n".join(self.lines) + "\n")
            except OSError:
                pass


def comm_ids_of(*drivers):
    return lambda: {d.comm_stream.cuda_stream for d in drivers if d is not None and d.comm_stream is not None}


# ------------------------------------------------------------------------------------------------------------------- Wan
def wan_case(h, cfg_streams):
    from lightx2v_amd import scheduler, synth, ulysses, wan

    dims = dict(synth.WAN_DIMS["wan-tiny"], dim=512, num_heads=4, ffn_dim=1024, num_layers=2)
    ts = (16, 3, 12, 10)
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=3).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    for name in ("attend_blocked", "__call__"):
        h.syncs.watch(ulysses.UlyssesAttention, name, timed=True)
    for name in ("begin_exchange_blocked", "begin_exchange", "on_comm"):
        h.syncs.watch(ulysses.UlyssesAttention, name)

    def build(pat, streams):
        cfg = wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=4, parallel_attn_type=pat, cfg_branch_streams=streams)
        model = wan.WanModel(cfg, wd)
        if pat:
            model.transformer_infer.parallel_attention.split_head2seq = "force"
        return model

    def loop(model, lat=lat):
        sch = scheduler.WanScheduler(model.config, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        for i in range(2):
            sch.step_pre(i)
            model.infer(inputs)
            sch.step_post()
        return sch.latents.float().cpu()

    single = loop(build(None, False))
    plain = build("ulysses", False)
    plain.transformer_infer.parallel_attention.overlap = False
    ref = loop(plain)
    assert plain.transformer_infer.parallel_attention.comm_stream is None and plain.transformer_infer.parallel_attention.copies == 0
    assert torch.equal(ref, single), "world-1 Ulysses with overlap=False differs from the plain single-GPU forward"

    model = build("ulysses", cfg_streams)
    tr, il = model.transformer_infer, model._cfg_interleave
    pa = tr.parallel_attention
    h.waits.comm_ids = comm_ids_of(pa)
    real_block = tr.infer_block

    def infer_block(*a, **kw):
        h.compute_delay()  # on the stream the block runs under: the default stream, or a branch stream
        return real_block(*a, **kw)

    tr.infer_block = infer_block
    real_pair = il.forward_pair

    def forward_pair(inp):
        h.compute_delay(CALLING_UNITS)  # the pre_infer outputs arrive late
        return real_pair(inp)

    il.forward_pair = forward_pair

    decoy = torch.randn(lat.shape, generator=torch.Generator().manual_seed(DECOY_SEED), dtype=lat.dtype)

    def run(regime, role):
        # A run with other latents first.  Every run repeats the allocations of the one before it, so what a tensor's memory holds before its
        # producer has run is the previous run's tensor of the same role: after an identical run that is the CORRECT data, and a collective
        # issued too early (the gather of a forward's output, say) would copy the right values all the same.
        loop(model, decoy)
        h.syncs.take_durations_ms()
        so.poison([pa._buffers, il._pa_b._buffers if il._pa_b is not None else None])
        h.arm(regime, role)
        out = loop(model)
        h.disarm()
        return out

    S = synth.seq_len_of(ts)
    controls = [("compute", so.ROLES[0]), ("comm", so.ROLES[1])] + ([("compute", so.ROLES[2]), ("compute", so.ROLES[3])] if cfg_streams else [])
    h.check("wan-tiny 2 CFG steps" + (", CFG branch streams" if cfg_streams else ""), run, ref, controls,
            streams=lambda: dict(comm=pa.comm_stream, **(dict(branch_a=il._streams[0], branch_b=il._streams[1]) if cfg_streams else {})))
    assert pa.copies == 0 and pa._buffers, "the fused driver must take the copy-free blocked exchange path"
    n_attn = 2 * 2 * dims["num_layers"]
    names = [c[0] for c in h.coll.calls]
    assert names.count("all_to_all_single") == 5 * n_attn and names.count("all_gather_into_tensor") == 4, (len(names), S)  # v | q, k | two head->seq pieces; one gather per forward
    streams = {c[1] for c in h.coll.calls}
    assert streams == {pa.comm_stream.cuda_stream} and pa.comm_stream.cuda_stream != h.waits.calling, "every collective runs on the one communication stream"
    if cfg_streams:
        assert il._streams is not None and il._pa_b._buffers and il._pa_b.comm_stream is pa.comm_stream, "the two-stream path was not taken"
    else:
        assert il._streams is None


# ------------------------------------------------------------------------------------------------------------------- row-major entry
def row_major_case(h):
    from lightx2v_amd import ulysses

    rows, heads = 96, 4
    g = torch.Generator().manual_seed(11)
    data = [torch.randn(rows, heads * 128, generator=g).to(torch.bfloat16).cuda() for _ in range(3)]
    decoy = [torch.randn(rows, heads * 128, generator=g).to(torch.bfloat16).cuda() for _ in range(3)]
    q, k, v = (torch.empty_like(t) for t in data)
    pa = ulysses.UlyssesAttention(None)
    h.waits.comm_ids = comm_ids_of(pa)
    h.syncs.watch(ulysses.UlyssesAttention, "__call__", timed=True)
    h.syncs.watch(ulysses.UlyssesAttention, "begin_exchange")

    def call(src, overlap):
        pa.overlap = overlap
        h.compute_delay()  # in front of the producers of q, k and v
        for t, s in zip((q, k, v), src):
            t.copy_(s)
        pend = pa.begin_exchange(v)
        assert (pend is not None) == overlap
        return pa(q, k, v if pend is None else pend, heads).float().cpu()

    def run(regime, role, overlap=True):
        # what a run without one of its waits reads early is then the decoy's data or NaN, never this run's own from an earlier pass
        call(decoy, overlap)
        torch.cuda.synchronize()
        so.poison([q, k, v])
        h.syncs.take_durations_ms()
        h.arm(regime, role)
        out = call(data, overlap)
        h.disarm()
        return out

    ref = run(None, None, overlap=False)
    h.check("UlyssesAttention.__call__ 96 rows x 4 heads, v begun early", run, ref, [("compute", so.ROLES[0]), ("comm", so.ROLES[1])],
            streams=lambda: dict(comm=pa.comm_stream))
    calls = h.coll.calls
    assert [c[0] for c in calls] == ["all_to_all_single"] * 4, calls
    comm = pa.comm_stream.cuda_stream
    assert comm != h.waits.calling and [c[1] for c in calls] == [comm, comm, comm, h.waits.calling], \
        f"seq->head of v, q, k on the communication stream and the final head->seq on the calling stream expected, got {calls}"
    h.say("the final head2seq of the row-major entry ran on the calling stream, the three seq2head on the communication stream")


# ------------------------------------------------------------------------------------------------------------------- HunyuanVideo
def hunyuan_case(h):
    from lightx2v_amd import hunyuan as hy, synth, ulysses

    dims = synth.HUNYUAN_DIMS["hunyuan-tiny"]
    ts = synth.HUNYUAN_WORKLOADS["hunyuan-tiny"]["target_shape"]
    n_attn = dims["double_blocks"] + dims["single_blocks"]
    wd = {k: v.cuda() for k, v in synth.synth_hunyuan_weights(dims, seed=2).items()}
    lat, text_states, mask, ts2 = synth.synth_hunyuan_inputs(dims, ts, seed=5, valid_text=11)
    assert 0 < int(mask.sum()) < mask.numel(), "padded text: the second attention segment and the text gather must run"
    inputs = {"text_encoder_output": {"text_encoder_1_text_states": text_states.cuda(), "text_encoder_1_attention_mask": mask.cuda(), "text_encoder_2_text_states": ts2.cuda()}}
    h.syncs.watch(ulysses.UlyssesHunyuanAttention, "attend_blocked", timed=True)
    h.syncs.watch(ulysses.UlyssesHunyuanAttention, "on_comm")
    cfg = hy.default_config(dims, infer_steps=4)
    model = hy.HunyuanModel(cfg, wd)
    ulysses.parallelize_hunyuan(model)
    tr = model.transformer_infer
    pa = tr.parallel_attention
    pa.split_head2seq = "force"
    h.waits.comm_ids = comm_ids_of(pa)
    for name in ("infer_double_block", "infer_single_block"):

        def entry(*a, _real=getattr(tr, name), **kw):
            h.compute_delay()
            return _real(*a, **kw)

        setattr(tr, name, entry)

    decoy = torch.randn(lat.shape, generator=torch.Generator().manual_seed(DECOY_SEED), dtype=lat.dtype)

    def forward(latents):
        sch = hy.HunyuanScheduler(cfg)
        sch.prepare(latents)
        model.set_scheduler(sch)
        sch.step_pre(1)
        model.infer(inputs)
        return sch.noise_pred.float().cpu()

    def run(regime, role, overlap=True):
        pa.overlap = overlap
        forward(decoy)  # other latents first: what memory holds before its producer has run is then never this run's own, correct, data
        h.syncs.take_durations_ms()
        so.poison(pa._buffers)
        h.arm(regime, role)
        out = forward(lat)
        h.disarm()
        return out

    ref = run(None, None, overlap=False)
    h.check("hunyuan-tiny one forward, padded text", run, ref, [("compute", so.ROLES[0]), ("comm", so.ROLES[1])], streams=lambda: dict(comm=pa.comm_stream))
    assert pa.copies == 0 and pa._buffers, "the fused driver must take the copy-free blocked exchange path"
    names = [c[0] for c in h.coll.calls]
    assert names.count("all_to_all_single") == 5 * n_attn and names.count("all_gather_into_tensor") == n_attn + 1, names
    assert {c[1] for c in h.coll.calls} == {pa.comm_stream.cuda_stream} and pa.comm_stream.cuda_stream != h.waits.calling


# ------------------------------------------------------------------------------------------------------------------- ring
def ring_case(h):
    from lightx2v_amd import lib, ring
    from tests import attn_ref as A

    rows, heads = 90, 3
    h.syncs.watch(ring.RingAttention, "__call__", timed=True)
    row_major = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], heads * 128).contiguous().cuda()  # noqa: E731
    bar = A.Case("ring, emulated rank", record=False)
    for N, r in ((4, 0), (4, 2), (2, 1)):
        inp = A.Inputs("R", rows, N * rows, heads, "none", seed=900 + 10 * N + r)
        spike = ((r + 1) % N) * rows + 41  # one key four times as long, in another rank's chunk: it arrives through a receive buffer
        inp.k[:, spike] = inp.k[:, spike] * 4
        q_src, k_all, v_all = row_major(inp.q), row_major(inp.k), row_major(inp.v)
        k_tab = [k_all[c * rows : (c + 1) * rows].contiguous() for c in range(N)]
        v_tab = [v_all[c * rows : (c + 1) * rows].contiguous() for c in range(N)]
        vt_tab = [lib.transpose_heads(t, heads) for t in v_tab]
        # the expected result: the carry chain over the chunks r, r-1, ..., issued directly on the default stream
        st = lib.AttnCarryState.alloc(rows, heads, q_src.device)
        for s in range(N):
            c = (r - s) % N
            res = lib.attention_carry(q_src, k_tab[c], vt_tab[c], heads, state=st, last=s == N - 1)
        chain = res.float().cpu()
        if (N, r) == (4, 2):
            got = res.reshape(rows, heads, 128).permute(1, 0, 2).contiguous().cpu()
            rel, Y, worst = bar.check(got, A.expect(inp, "vt"), "direct chain")
            h.say(f"ring N={N} r={r}: direct chain vs float64 dense attention over {N * rows} keys: relL2 {rel:.3e} (Y {Y:.3e}), worst d/tol {worst:.3f}")

        pa = ring.RingAttention(None)
        pa.world = lambda N=N, r=r: (N, r)
        h.waits.comm_ids = comm_ids_of(pa)
        q, k, v = torch.empty_like(q_src), torch.empty_like(k_tab[r]), torch.empty_like(v_tab[r])
        sent_ok = torch.zeros(N - 1, dtype=torch.bool, device="cuda")
        hops = []

        def transfer(send, recv, to, frm, N=N, r=r, hops=hops, sent_ok=sent_ok, k_tab=k_tab, vt_tab=vt_tab):
            hop = len(hops) + 1
            hops.append(torch.cuda.current_stream().cuda_stream)
            assert (to, frm) == ((r + 1) % N, (r - 1) % N) and hop < N
            sc, rc = (r - hop + 1) % N, (r - hop) % N
            # the pair handed on must be chunk sc as a whole, checked on the stream: a pair forwarded while a receive overwrites it is not
            sent_ok[hop - 1] = (send[0] == k_tab[sc]).all() & (send[1] == vt_tab[sc]).all()
            h.coll.transfer("ring hop", [(recv[0], k_tab[rc]), (recv[1], vt_tab[rc])])

        pa._transfer = transfer
        real_carry = pa.attn_fn

        def carry(*a, _real=real_carry, **kw):
            h.compute_delay()  # in front of every carry launch
            return _real(*a, **kw)

        pa.attn_fn = carry

        def run(regime, role, overlap=True, pa=pa, q=q, k=k, v=v, r=r, hops=hops, sent_ok=sent_ok, q_src=q_src, k_tab=k_tab, v_tab=v_tab):
            pa.overlap = overlap
            so.poison([pa._buffers, q, k, v])
            sent_ok.zero_()
            hops.clear()
            h.arm(regime, role)
            h.compute_delay()  # in front of the producers of the local chunk
            q.copy_(q_src)
            k.copy_(k_tab[r])
            v.copy_(v_tab[r])
            out = pa(q, k, v, heads)
            res = out.float().cpu()
            h.disarm()
            run.sent = sent_ok.cpu().tolist()
            return res

        ref = run(None, None, overlap=False)
        assert run.sent == [True] * (N - 1) and len(hops) == N - 1
        assert torch.equal(ref, chain), f"ring N={N} r={r}: overlap=False differs from the direct carry chain in {so.differing(ref, chain)} elements"
        name = f"ring N={N} r={r}, 90 rows x 3 heads"

        def observe(out, ref, run=run, N=N):
            n = so.differing(out, ref)
            h.say(f"ring: pairs sent intact per hop {run.sent}")
            return n + (N - 1 - sum(run.sent) if N < 3 else 0)  # at N = 2 no receive overwrites a pair: a send issued too early shows in the send-side flag alone

        def positive(regime, role, run=run, N=N, pa=pa):
            out = run(regime, role)
            if role is None:
                assert run.sent == [True] * (N - 1), f"ring: a pair was forwarded while it was not the chunk it should be: {run.sent}"
                assert pa.launches == [(s > 0, s < N - 1) for s in range(N)] and pa.host_syncs == 0
                assert set(hops) == {pa.comm_stream.cuda_stream} and pa.comm_stream.cuda_stream != h.waits.calling
            return out

        h.check(name, positive, ref, [("compute", so.ROLES[0]), ("comm", so.ROLES[1])], observe=observe, streams=lambda pa=pa: dict(comm=pa.comm_stream))
        h.say(f"{name}: equal to the direct carry chain bit for bit under both regimes; the pair sent was intact on every one of the {N - 1} hops")
        if (N, r) == (4, 2):
            out = positive("comm", None)
            got = out.to(torch.bfloat16).reshape(rows, heads, 128).permute(1, 0, 2).contiguous()
            rel, Y, worst = bar.check(got, A.expect(inp, "vt"), "ring driver, slow communication")
            h.say(f"{name}: driver result vs float64: relL2 {rel:.3e} (Y {Y:.3e}), worst d/tol {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------- CFG branch streams, one GPU
def cfg_single_case(h):
    from lightx2v_amd import scheduler, synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    ts = (16, 3, 12, 10)
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=1).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    h.syncs.watch(wan.CfgBranchStreams, "forward_pair", timed=True)

    def build(streams):
        cfg = wan.default_config(dims, target_shape=ts, target_video_length=9, infer_steps=3, cfg_pair=False, cfg_branch_streams=streams)
        return wan.WanModel(cfg, wd)

    def loop(model, lat=lat):
        sch = scheduler.WanScheduler(model.config, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        for i in range(2):
            sch.step_pre(i)
            model.infer(inputs)
            sch.step_post()
        return sch.latents.float().cpu()

    ref = loop(build(False))
    model = build(True)
    il = model._cfg_interleave = wan.CfgBranchStreams(model)
    tr = model.transformer_infer
    real_block, real_pair = tr.infer_block, il.forward_pair

    def infer_block(*a, **kw):
        h.compute_delay()  # at the head of each branch (and of every later block)
        return real_block(*a, **kw)

    def forward_pair(inp):
        h.compute_delay(CALLING_UNITS)  # on the calling stream: the pre_infer outputs arrive late
        return real_pair(inp)

    tr.infer_block, il.forward_pair = infer_block, forward_pair

    decoy = torch.randn(lat.shape, generator=torch.Generator().manual_seed(DECOY_SEED), dtype=lat.dtype)

    def run(regime, role):
        loop(model, decoy)  # other latents first: what memory holds before its producer has run is then never this run's own, correct, data
        h.syncs.take_durations_ms()
        h.arm(regime, role)
        out = loop(model)
        h.disarm()
        return out

    h.check("wan-tiny 2 CFG steps, wan.CfgBranchStreams, no process group", run, ref, [("compute", so.ROLES[2]), ("compute", so.ROLES[3])],
            regimes=("compute",), count_syncs=False, streams=lambda: dict(branch_a=il._streams[0], branch_b=il._streams[1]))
    assert il._streams is not None and not h.coll.calls, "the two-stream path was not taken"


def main():
    case = os.environ["X2V_STREAM_ORDER_CASE"]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    grouped = case != "cfg-single"
    if grouped:
        dist.init_process_group("gloo")
        assert dist.get_world_size() == 1
    from lightx2v_amd import lib

    lib.init(0)
    h = Harness(case)
    with torch.no_grad():
        {"wan-blocked": lambda: wan_case(h, False), "wan-cfg": lambda: wan_case(h, True), "row-major": lambda: row_major_case(h),
         "hunyuan": lambda: hunyuan_case(h), "ring": lambda: ring_case(h), "cfg-single": lambda: cfg_single_case(h)}[case]()
    torch.cuda.synchronize()
    h.coll.restore()
    h.finish()
    print(f"STREAM_ORDER_OK {case}", flush=True)
    if grouped:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
