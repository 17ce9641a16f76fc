"""Ring sequence parallelism for the Wan self-attention (one process per GPU, `torch.distributed` point-to-point over RCCL/xGMI).

reference: lightx2v/attentions/distributed/ring/attn.py:25-63 (`_update_out_and_lse`), 99-193 (ring_attn), comm/ring_comm.py (RingComm),
ring/wrap.py:53-71 (parallelize_wan), utils/wan/processor.py:9-37 (pre/post_process, shared with Ulysses).

Same partitioning as Ulysses — tokens of the flattened (t,h,w) axis in N contiguous shards — but the heads are NOT split: every rank keeps
its query rows for all heads and the K / V chunks travel round the ranks (to rank r+1, from rank r-1), so the head count puts no limit on the
group (Wan-1.3B's 12 heads on 8 GPUs).  Step s attends the chunk of rank (r - s) mod N and the partial results are merged through their
log-sum-exp.  What the reference pays beyond that is removed:
  * the merge is the epilogue of the attention kernel (x2v_attn_fwd_bf16_vt_carry): the running output stays fp32 from the first chunk to the
    last and is rounded to bf16 once; the reference rounds every block output to bf16 and merges with four fp32 elementwise passes per step;
  * V travels pre-transposed: the local v is transposed once (1/N of the single-GPU transposition) and the V^T chunk [H, ceil(S/N / 64), 128, 64]
    circulates, so no rank transposes a chunk it received;
  * no host synchronisation in the loop (the reference waits for its requests on the host every step): the transfer for step s+1 runs on the
    communication stream under step s's attention, into the other of two buffer pairs allocated once per shape; the order is by stream
    joins in both directions — a receive buffer is overwritten only after the launch that read it has been ordered before the receive, and a
    launch reads a buffer only after joining the receive.
The stream discipline (one communication stream, `_enqueue` behind the compute stream, `_join` before a read, the CommTimer brackets) is
ulysses.CommStreams, shared with the Ulysses drivers and described there; the wrapper round the Wan block stack is ulysses.shard_wan_block_stack.
"""
import torch
import torch.distributed as dist

from . import lib
from .ulysses import CommStreams, shard_wan_block_stack


def _no_group():
    """No process group: a ring of one (the single launch), with nothing to shard or gather."""
    return not (dist.is_available() and dist.is_initialized())


def transpose_heads_host(v, num_heads):
    """lib.transpose_heads's layout in plain torch, for tensors that are not on a HIP device (the gloo tests drive RingAttention with an
    `attn_fn`): v [Sk, H*128] -> V^T [H, ceil(Sk/64), 128, 64], keys >= Sk zero-filled."""
    sk = v.shape[0]
    tiles = (sk + 63) // 64
    vp = torch.zeros((tiles * 64, num_heads, 128), dtype=v.dtype, device=v.device)
    vp[:sk] = v[:, : num_heads * 128].reshape(sk, num_heads, 128)
    return vp.view(tiles, 64, num_heads, 128).permute(2, 0, 3, 1).contiguous()


class RingAttention(CommStreams):
    """Callable injected as `transformer_infer.parallel_attention`, with UlyssesAttention.__call__'s signature.

    attn_fn(q, k, vt, num_heads, state=None, last=False, prescaled=False) replaces the launch chain: lib.attention_carry's contract (returns the
    state, or the [S/N, H*128] result when `last`).  Counters for the tests: `launches` (the (carry_in, carry_out) pair of every launch of the
    last call), `calls`, and `host_syncs` (host synchronisations the driver itself made inside a call: none)."""

    def __init__(self, group=None, attn_fn=None, overlap=True):
        super().__init__(group, overlap)
        self._default_attn = attn_fn is None
        self.attn_fn = attn_fn or lib.attention_carry
        self._states = {}
        self.launches, self.calls, self.host_syncs = [], 0, 0
        self.bytes_sent = 0  # by this rank in the last call

    def world(self):
        return (1, 0) if _no_group() else super().world()

    def buffers(self, k, vt):
        """Two (K chunk, V^T chunk) receive pairs, allocated once per shape and reused by every layer (stream order makes that safe: a call's
        first receive is issued behind everything the compute stream has enqueued, the previous call's launches included)."""
        key = (tuple(k.shape), tuple(vt.shape), k.dtype, str(k.device))
        b = self._buffers.get(key)
        if b is None:
            b = self._buffers[key] = [(torch.empty(k.shape, dtype=k.dtype, device=k.device), torch.empty_like(vt)) for _ in range(2)]
        return b

    def _state(self, q, num_heads):
        """The chain's (acc, lse), owned here, once per shape; None for an `attn_fn` that keeps its own."""
        if not (self._default_attn and q.is_cuda):
            return None
        key = (q.shape[0], num_heads, str(q.device))
        st = self._states.get(key)
        if st is None:
            st = self._states[key] = lib.AttnCarryState.alloc(q.shape[0], num_heads, q.device)
        return st.reset()

    def _peers(self, n, r):
        to, frm = (r + 1) % n, (r - 1) % n
        if self.group is not None:
            to, frm = dist.get_global_rank(self.group, to), dist.get_global_rank(self.group, frm)
        return to, frm

    def _transfer(self, send, recv, to, frm):
        """One hop of the ring for a (K, V^T) pair (RingComm.send_recv x 2, commit, wait).  `wait` on an RCCL request orders the current — the
        communication — stream behind the transfer; it does not block the host."""
        ops = []
        for s, d in zip(send, recv):
            ops.append(dist.P2POp(dist.isend, s, to, group=self.group))
            ops.append(dist.P2POp(dist.irecv, d, frm, group=self.group))
        for req in dist.batch_isend_irecv(ops):
            req.wait()
        self.bytes_sent += sum(s.numel() * s.element_size() for s in send)

    def __call__(self, q, k, v, num_heads, head_dim=128, timer=None, variant=0):
        n, r = self.world()
        if head_dim != 128:
            raise lib.X2VError(f"ring attention: head_dim={head_dim} (only 128 is built)")
        prescaled = bool(variant & lib.ATTN_Q_PRESCALED)
        self.calls += 1
        self.launches, self.bytes_sent = [], 0
        vt = lib.transpose_heads(v, num_heads) if v.is_cuda else transpose_heads_host(v, num_heads)
        state = self._state(q, num_heads) if n > 1 else None  # a ring of one is the single dense launch: no state

        def launch(kc, vtc, s):
            nonlocal state
            last = s == n - 1
            self.launches.append((s > 0, not last))
            fn = lambda: self.attn_fn(q, kc, vtc, num_heads, state=state, last=last, prescaled=prescaled)  # noqa: E731
            res = timer("self", fn) if timer is not None else fn()
            if not last:
                state = res
            return res

        if n == 1:
            return launch(k, vt, 0)
        to, frm = self._peers(n, r)
        kc = k if k.is_contiguous() else k.contiguous()  # a view of a fused projection: the message is the chunk alone
        pairs = self.buffers(kc, vt)
        # Each hop is enqueued one step ahead of the launch that reads it.  Enqueueing orders it behind what the compute stream holds: the local
        # chunk is complete, and so is every earlier launch that read the receive buffers.  Without streams (host tensors under gloo, or
        # overlap off) these are the same hops in the same order, each completed where it is enqueued.
        self._enqueue(lambda: self._transfer((kc, vt), pairs[0], to, frm), q)
        if self._streams(q):
            kc.record_stream(self.comm_stream)
            vt.record_stream(self.comm_stream)
        out = launch(k, vt, 0)
        for s in range(1, n):
            have, nxt = pairs[(s - 1) % 2], pairs[s % 2]
            self._join(q)  # the chunk of step s has arrived
            if s + 1 < n:  # launch s-1, the last reader of `nxt`, is ordered before the receive that overwrites it
                self._enqueue(lambda: self._transfer(have, nxt, to, frm), q)
            out = launch(have[0], have[1], s)
        return out


def parallelize_wan(wan_model, group=None, attn_fn=None):
    """reference: ring/wrap.py:53-71 — swap the attention, shard x around the block stack (the same wrapper as Ulysses).  With CFG the two
    forwards run one after the other: no CFG-branch interleave is installed for the ring."""
    return shard_wan_block_stack(wan_model, RingAttention(group, attn_fn), passthrough=_no_group)
