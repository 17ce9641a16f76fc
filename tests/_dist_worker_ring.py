"""gloo worker for tests/test_ring_host.py (CPU, world 2 and 3): lightx2v_amd.ring.RingAttention with the restated carry step in fp32 torch
(tests/attn_carry_ref.TorchCarry) as its `attn_fn`, against float64 dense attention over the padded sequence.  Checks the chunk order (step s attends
the chunk of rank (r - s) mod N), the carry bits per launch, a token count the group does not divide (the zero pad rows are keys, the quirk the
Ulysses path keeps as well), and a head count the group does not divide (3 heads at world 2)."""
import math
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    dist.init_process_group("gloo")
    r, n = dist.get_rank(), dist.get_world_size()
    from lightx2v_amd import ring, ulysses
    from tests import attn_carry_ref as C
    from tests import attn_ref as A

    for S, H in ((97, 3), (96, 2), (130, 1)):  # 97: padded to 98 / 99; 130 at world 3: 44 rows per rank, 132 keys (chunks that are no multiple of anything)
        gen = torch.Generator().manual_seed(11 * S + H)
        q, k, v = (torch.randn(S, H * 128, generator=gen).to(torch.bfloat16) for _ in range(3))
        # the shards as the wrapped driver makes them: zero-padded to a multiple of N, contiguous chunks
        ql, kl, vl = (ulysses.pre_process(t) for t in (q, k, v))
        s_loc = -(-S // n)
        assert ql.shape == (s_loc, H * 128)
        pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, n * s_loc - S))  # noqa: E731
        qp, kp, vp = pad(q), pad(k), pad(v)
        assert torch.equal(ql, qp[r * s_loc : (r + 1) * s_loc])

        fn = C.TorchCarry()
        pa = ring.RingAttention(attn_fn=fn, overlap=False)
        out = pa(ql, kl, vl, H, 128)
        assert out.shape == (s_loc, H * 128) and out.dtype == torch.bfloat16

        # N launches, carry bits, chunk order
        assert pa.launches == [(s > 0, s < n - 1) for s in range(n)], pa.launches
        assert pa.host_syncs == 0
        firsts = [float(kp[((r - s) % n) * s_loc, 0]) for s in range(n)]
        assert len(set(firsts)) == n, "the chunks' first elements must tell them apart"
        assert [e[3] for e in fn.log] == firsts, f"rank {r}: chunk order {[e[3] for e in fn.log]} vs {firsts}"
        assert [e[0] for e in fn.log] == [s_loc] * n and [e[1] for e in fn.log] == [s > 0 for s in range(n)] and [e[2] for e in fn.log] == [s == n - 1 for s in range(n)]
        assert pa.bytes_sent == (n - 1) * (kl.numel() + H * ((s_loc + 63) // 64) * 128 * 64) * 2

        # float64 dense attention over the PADDED sequence (pad rows are keys with score 0 and v = 0) for this rank's query rows
        hm = lambda t: t.reshape(t.shape[0], H, 128).permute(1, 0, 2)  # noqa: E731
        qh, kh, vh = hm(ql), hm(kp), hm(vp)
        s64 = A.scores(qh, kh, q_rounded=True)
        o, _ = C.dense(s64, vh)
        w = torch.exp2(s64 - s64.amax(-1, keepdim=True))
        Aabs = (w / w.sum(-1, keepdim=True)) @ vh.to(torch.float64).abs()
        # fp32 rounding: a score is a 128-term fp32 dot product, |ds| <= 128 * 2^-24 * sum_d |q_d k_d|, i.e. ds * ln 2 relative in its weight (numerator and
        # denominator: twice); sums of at most n * s_loc terms, the exp2 / log2 of the merge and its two multiplications: 2^-24 each; one rounding to bf16 (8 significand bits: unit roundoff 2^-8)
        qe = A.prescale_q(qh).to(torch.float64)
        eps_s = 128 * 2.0 ** -24 * float((qe.abs() @ kh.to(torch.float64).abs().transpose(-1, -2)).max())
        tol = 2.0 ** -8 * o.abs() + (2 * eps_s * math.log(2.0) + (n * s_loc + 8 * n) * 2.0 ** -24) * Aabs
        err = (hm(out).to(torch.float64) - o).abs()
        assert (err <= tol).all(), f"rank {r} S={S} H={H}: worst err/tol {float((err / tol.clamp_min(1e-300)).max()):.3f}"
        # without the pad rows as keys the result is another one: the check above can tell
        if n * s_loc != S:
            o_np, _ = C.dense(s64[..., :S], vh[:, :S])
            assert not ((o_np - o).abs() <= tol).all()

    dist.barrier()
    if r == 0:
        print("RING_DIST_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
