"""The carry form of the ping-pong attention kernel (x2v_attn_fwd_bf16_vt_carry: include/x2v.h) on the GPU: a chain of launches over key chunks against
float64 attention over the concatenated keys at the dense kernel's own bar (attn_ref.Case.check — the carry adds fp32 operations only), the
bit-equalities of the one-launch chain, the LSE of a CARRY_OUT launch against float64, and the isolation of acc / lse / o.

Operands are views of the fused, over-allocated buffers of tests/test_gpu_attn_fp64.py (k / v rows past a chunk hold dominant keys: a chunk's launch
must not see the next chunk's rows either); outputs and states are windows of poisoned buffers."""
import os

import pytest
import torch

from tests import attn_carry_ref as C
from tests import attn_ref as A
from tests.test_gpu_attn_bsr import FAMILIES
from tests.test_gpu_attn_fp64 import POISON, fused, head_major, poison_intact, views, window

pytestmark = pytest.mark.gpu
CASE = A.Case("carry v9")
SQ, H, CHUNKS = 256 + 33, 3, (320, 65, 200)  # one full query block and a tail; every step ends in a partial 64-key tile, one of them a single key
LSE_ROWS = []


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_ATTN_CARRY_TABLE")  # where to write the measured figures (profiles/attn_carry_parity.txt is one run's)
    if not path:
        return
    try:
        with open(path, "w") as f:
            f.write(f"# {CASE.name}: {len(CASE.rows)} checks, largest relL2 / Y = {CASE.max_ratio:.3f}, largest d/tol = {max((r[4] for r in CASE.rows), default=0):.3f}\n")
            f.write("\n".join(CASE.table()) + "\n")
            f.write("# lse of a CARRY_OUT launch vs float64 log2 sum 2^s (base-2 units): case, worst |d|, smallest bar of the case, worst |d| / bar\n")
            f.write("\n".join(LSE_ROWS) + "\n")
    except OSError:
        pass


def state_windows(lib, rows, heads, ldlse_extra=0):
    """Poisoned fp32 buffers and the (acc, lse) windows inside them: acc [rows, heads * 128] with token stride heads * 128 + 4 starting two rows down,
    lse [heads, rows] with head stride rows + ldlse_extra starting one head down."""
    HD = heads * 128
    big_a = torch.full((rows + 4, HD + 4), POISON, dtype=torch.float32, device="cuda")
    big_l = torch.full((heads + 2, rows + ldlse_extra), POISON, dtype=torch.float32, device="cuda")
    acc, lse = big_a[2 : rows + 2, :HD], big_l[1 : heads + 1, :rows]
    assert acc.data_ptr() % 16 == 0
    return big_a, big_l, lib.AttnCarryState(acc, big_l[1 : heads + 1])


def state_intact(big_a, big_l, rows, heads):
    HD = heads * 128
    return bool((big_a[:2] == POISON).all() and (big_a[rows + 2 :] == POISON).all() and (big_a[2 : rows + 2, HD:] == POISON).all()
                and (big_l[0] == POISON).all() and (big_l[heads + 1 :] == POISON).all() and (big_l[1 : heads + 1, rows:] == POISON).all())


def chunk_buffers(inp, pre, chunks):
    """One fused buffer per key chunk (q | this chunk's k | v, dominant rows past the chunk)."""
    form, out, j = "pre" if pre else "vt", [], 0
    for c in chunks:
        out.append(fused(inp.q_for(form), inp.k[:, j : j + c], inp.v[:, j : j + c], inp.H)[0])
        j += c
    return out


def run_chain(lib, inp, pre, chunks, ldlse_extra=5, state=None):
    """The chain over `chunks` with every window checked after every launch.  Returns the bf16 output window [Sq, H * 128] (device)."""
    Sq, Hh = inp.Sq, inp.H
    bufs = chunk_buffers(inp, pre, chunks)
    big_a, big_l, st = state_windows(lib, Sq, Hh, ldlse_extra)
    big_o, out = window(Sq, Hh * 128)
    res = None
    for i, (buf, c) in enumerate(zip(bufs, chunks)):
        q, k, v = views(buf, Sq, c, Hh)
        last = i == len(chunks) - 1
        before = (big_a.clone(), big_l.clone()) if last else None
        res = lib.attention_carry(q, k, lib.transpose_heads(v, Hh), Hh, state=st if len(chunks) > 1 else None, last=last, prescaled=pre, out=out if last else None)
        assert state_intact(big_a, big_l, Sq, Hh), "wrote outside the acc / lse windows"
        if last:
            assert torch.equal(big_a, before[0]) and torch.equal(big_l, before[1]), "acc / lse written without CARRY_OUT"
            assert res.data_ptr() == out.data_ptr() and poison_intact(big_o, Sq, Hh * 128), "wrote outside the output window"
        else:
            assert res is st and (big_o == POISON).all(), "o written under CARRY_OUT"
            assert torch.isfinite(st.acc).all() and torch.isfinite(st.lse[:, :Sq]).all()
    return out


def spike_in_chunk(Sq, Sk, Hh, key):
    """Family R with one key four times as long at index `key`: attn_ref's spike, placed where the chunking needs it."""
    inp = A.Inputs("R", Sq, Sk, Hh, "none", seed=700 + key)
    inp.k[:, key] = inp.k[:, key] * 4
    return inp


@pytest.mark.parametrize("pre", [False, True])
def test_chain_vs_dense_float64(lib, pre):
    """Three launches (CARRY_OUT | CARRY_IN + CARRY_OUT | CARRY_IN) against float64 attention over all 585 keys at the dense kernel's bar.  The spike of
    family R sits in the first chunk (first: key 3, middle: key 292) or the last (key 584), and a further case puts it in the one-key-tile middle chunk
    (key 350): the carried state dominates the new chunk, is dominated by it, or is comparable (family N: all scores alike)."""
    Sk = sum(CHUNKS)
    inputs = [A.Inputs(fam, SQ, Sk, H, spike) for fam, spike in FAMILIES] + [spike_in_chunk(SQ, Sk, H, 350)]
    form = "pre" if pre else "vt"
    for inp in inputs:
        inp.assert_margins(form)
        got = head_major(run_chain(lib, inp, pre, CHUNKS), H)
        rel, Y, worst = CASE.check(got, A.expect(inp, form), f"chain {'+'.join(map(str, CHUNKS))} {form}")
        print(f"{inp.name} seed={inp.seed} {form}: relL2 {rel:.3e}  Y {Y:.3e}  worst d/tol {worst:.3f}")


def test_ring_shaped_chain(lib):
    """Sq = Sk = 90 per chunk, 4 chunks, 4 heads against dense attention over 360 keys: the shape tests/_dist_gpu_worker_ring.py runs at world 4."""
    for fam, spike in FAMILIES:
        inp = A.Inputs(fam, 90, 360, 4, spike)
        for pre in (False, True):
            form = "pre" if pre else "vt"
            got = head_major(run_chain(lib, inp, pre, (90, 90, 90, 90), ldlse_extra=0), 4)
            CASE.check(got, A.expect(inp, form), f"ring chain 4x90 {form}")


def test_bits(lib):
    """A chain of one chunk with neither bit set is the dense one-walk launch, bit for bit; two identical chains are bit-equal."""
    Sk = sum(CHUNKS)
    for fam, spike in FAMILIES[:2]:
        inp = A.Inputs(fam, SQ, Sk, H, spike)
        for pre in (False, True):
            buf = fused(inp.q_for("pre" if pre else "vt"), inp.k, inp.v, H)[0]
            q, k, v = views(buf, SQ, Sk, H)
            vt = lib.transpose_heads(v, H)
            one = lib.attention_carry(q, k, vt, H, last=True, prescaled=pre)
            dense = lib.attention(q, k, None, H, variant=lib.ATTN_FAST | lib.ATTN_ONE_WALK | (lib.ATTN_Q_PRESCALED if pre else 0), vt=vt)
            assert torch.equal(one, dense), "a chain of one launch differs from the dense one-walk launch"
            a, b = run_chain(lib, inp, pre, CHUNKS), run_chain(lib, inp, pre, CHUNKS)
            assert torch.equal(a, b), "two identical chains differ"


@pytest.mark.parametrize("pre", [False, True])
def test_lse_of_a_carry_out_launch(lib, pre):
    """lse of one CARRY_OUT launch against float64 log2 sum_j 2^s_j, per row within attn_carry_ref.lse_bar — derived from the fp32 operations x2v.h
    lists, from the inputs alone — and acc against float64 attention through its bf16 rounding (Case.check).  lib.attention_lse is the same launch
    in natural-log units."""
    form = "pre" if pre else "vt"
    for Sk in (65, 585):
        for fam, spike in FAMILIES:
            inp = A.Inputs(fam, SQ, Sk, H, spike)
            buf = fused(inp.q_for(form), inp.k, inp.v, H)[0]
            q, k, v = views(buf, SQ, Sk, H)
            big_a, big_l, st = state_windows(lib, SQ, H, 7)
            res = lib.attention_carry(q, k, lib.transpose_heads(v, H), H, state=st, prescaled=pre)
            assert res is st and st.steps == 1 and state_intact(big_a, big_l, SQ, H)
            s64 = A.scores(inp.q_for(form), inp.k, **A.form_args(form))
            _, lse64 = C.dense(s64, inp.v)
            bar = C.lse_bar(inp.q_for(form), inp.k, Sk, pre)
            d = (st.lse[:, :SQ].cpu().to(torch.float64) - lse64).abs()
            LSE_ROWS.append(f"{inp.name} {form}: worst |d| {float(d.max()):.3e}  smallest bar {float(bar.min()):.3e}  worst |d| / bar {float((d / bar).max()):.4f}")
            print(LSE_ROWS[-1])
            assert (d <= bar).all(), LSE_ROWS[-1]
            CASE.check(head_major(st.acc.to(torch.bfloat16), H), A.expect(inp, form), f"carry-out acc {form}")
            out, lse_nat = lib.attention_lse(q, k, v, H, prescaled=pre)
            assert torch.equal(out, st.acc.to(torch.bfloat16)) and torch.equal(lse_nat, st.lse[:, :SQ] * C.LN2)
