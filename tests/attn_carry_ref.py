"""Restatement of the carry arithmetic of x2v_attn_fwd_bf16_vt_carry (include/x2v.h, steps 1-6) in plain PyTorch on the CPU: attention over all
keys as a chain over key chunks with the running state (A, L) — the output so far and its base-2 log-sum-exp — handed from step to step.  In float64
it is the yardstick of tests/test_ring_host.py (a chain over ANY chunking equals dense attention: the formula itself) and of the LSE check in
tests/test_gpu_attn_carry.py; in float32 it is the `attn_fn` that the gloo workers hand to ring.RingAttention.  Nothing here imports the library.

Tensors are head-major as in tests/attn_ref.py: s [H, Sq, Sk_chunk] base-2 scores, v [H, Sk_chunk, 128], A [H, Sq, 128], L [H, Sq]."""
import math

import torch

from tests import attn_ref as A

F64, F32, BF16 = A.F64, A.F32, A.BF16
LN2 = math.log(2.0)


def walk(s, v):
    """What a launch's key walk leaves per row: the reference m (here the chunk's row maximum; the kernel's is its lazily updated running maximum — the
    arithmetic below holds for any m), l = sum 2^(s - m), a = sum 2^(s - m) v (unnormalised)."""
    m = s.amax(-1)
    p = torch.exp2(s - m.unsqueeze(-1))
    return m, p.sum(-1), p @ v.to(s.dtype)


def step(s, v, state=None):
    """One launch: x2v.h steps 1-5 in its order.  state = (A, L) or None (no CARRY_IN).  Returns (A', L')."""
    m, l, a = walk(s, v)
    Lb = m + torch.log2(l)  # 1
    if state is None:
        return a * (1.0 / l).unsqueeze(-1), Lb  # 2-4: L' = Lb, w = 1 / l, A' = a * w
    Aold, L = state
    M = torch.maximum(L, Lb)  # 2
    Ln = M + torch.log2(torch.exp2(L - M) + torch.exp2(Lb - M))  # 3
    wA, wa = torch.exp2(L - Ln), torch.exp2(m - Ln)  # 4
    return Aold * wA.unsqueeze(-1) + a * wa.unsqueeze(-1), Ln  # 5


def chain(s, v, chunks, dtype=F64):
    """The chain over consecutive key chunks of the given sizes (sum = Sk): (A, L) after the last step, in `dtype`."""
    assert sum(chunks) == s.shape[-1] == v.shape[1] and min(chunks) > 0
    state, j = None, 0
    for c in chunks:
        state = step(s[..., j : j + c].to(dtype), v[:, j : j + c].to(dtype), state)
        j += c
    return state


def dense(s, v):
    """float64 attention over all keys at once and its base-2 log-sum-exp."""
    s = s.to(F64)
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    return (p / l) @ v.to(F64), (m + torch.log2(l)).squeeze(-1)


def lse_bar(q, k, Sk, prescaled, scale=0.0):
    """Per-row bound [H, Sq] on |lse - log2 sum_j 2^s_j| of one launch over Sk keys, in base-2 units, from the fp32 operations x2v.h lists:
      * a score is a 128-term fp32 dot product of exact bf16 products, accumulated by the matrix unit in an order and rounding mode this bound does not
        assume: |ds| <= 128 * 2^-23 * sum_d |q_d k_d| (two units in the last place per term covers truncation); an error ds of every score moves the
        log-sum-exp by at most max |ds|;
      * P = exp2(s - m), 1 ulp (2^-23 relative); the row sum is eight fp32 chains of at most ceil(Sk / 8) additions joined by three more:
        (ceil(Sk / 8) + 3) * 2^-24 relative; each lazy rescale multiplies the sum by an exp2 (2^-23 + 2^-24), at most once per 64-key tile;
        a relative error r of l is r / ln 2 in log2(l);
      * log2(l), 1 ulp: 2^-23 * |log2 l| with |log2 l| <= 8 + log2(Sk) (the running reference m is a score the row has seen and trails the row maximum by at
        most the rescale threshold 8: the largest P is in [1, 2^8], the sum in [1, Sk * 2^8]); the final addition m + log2(l): 2^-24 * (|lse| + 2^-23), |lse| <= max |s| + log2(Sk).
    Computed from the inputs alone, never from a kernel's output."""
    kw = A.form_args("pre" if prescaled else "vt")
    qe, f = A._q_and_factor(q, scale, dtype=F64, **kw)
    assert f is None
    sabs = qe.abs() @ k.to(F64).abs().transpose(-1, -2)  # [H, Sq, Sk]: sum_d |q_d k_d|, an upper bound of |s| as well
    top = sabs.amax(-1)
    nt = (Sk + 63) // 64
    rel_l = (math.ceil(Sk / 8) + 3) * 2.0 ** -24 + 2.0 ** -23 + nt * 1.5 * 2.0 ** -23
    return 128 * 2.0 ** -23 * top + rel_l / LN2 + 2.0 ** -23 * (8 + math.log2(Sk)) + 2.0 ** -24 * (top + math.log2(Sk) + 1)


# ---------------------------------------------------------------------------------------------------------------- the gloo workers' attn_fn
def rows_of_vt(vt, Sk):
    """V^T [H, ceil(Sk/64), 128, 64] (lib.transpose_heads's layout) -> v [H, Sk, 128]."""
    H, T = vt.shape[0], vt.shape[1]
    return vt.permute(0, 1, 3, 2).reshape(H, T * 64, 128)[:, :Sk]


class TorchCarry:
    """lib.attention_carry's contract in fp32 torch on row-major host tensors: q [Sq, H*128], k [Sk, H*128], vt as transpose_heads lays it out.
    Records (keys seen, carry_in, last, k's first element) per launch for the order checks."""

    def __init__(self):
        self.log = []

    def __call__(self, q, k, vt, num_heads, state=None, last=False, prescaled=False):
        H, Sq, Sk = num_heads, q.shape[0], k.shape[0]
        qh = q[:, : H * 128].reshape(Sq, H, 128).permute(1, 0, 2)
        kh = k[:, : H * 128].reshape(Sk, H, 128).permute(1, 0, 2)
        s = A.scores(qh, kh, prescaled=prescaled, q_rounded=not prescaled, dtype=F32)
        self.log.append((Sk, state is not None, last, float(k[0, 0])))
        Anew, Lnew = step(s, rows_of_vt(vt, Sk).to(F32), state)
        if not last:
            return Anew, Lnew
        return Anew.permute(1, 0, 2).reshape(Sq, H * 128).to(BF16)
