"""The head-dim-128 attention kernels of lightx2v_amd/csrc/attn.hip (attn_fwd_pipe_kernel, the ping-pong attn_fwd_v9_kernel, the persistent
attn_fwd_p9_kernel) against the float64 reference of tests/attn_ref.py at every edge of their dispatch: the key-tile count and the last-tile mask
(both exits of v9's x2-unrolled walk), the 16-row group / 32-row wave / 256-row block tails, the staggered walk and its wrap, the XCD remap with
nwg % 8 != 0, the batched entry, and p9's item stride and q-piece schedule for every nt = 4..32.

Acceptance is attn_ref.Case.check on every call: |got - o| <= 2^-7 |o| + 1.05 * 2^-8 * A on EVERY element, relL2 <= 1.5 * Y (Y from the
emulations of attn_ref, never from a kernel), and the one-hot (H) and uniform (U) families bit for bit.  tests/test_attn_ref_host.py shows which
subtly wrong kernels this rejects.

Every call reads q / k / v as views of one fused buffer (token stride 3 * H * 128 + 64) and writes a window of a poisoned buffer (token stride
H * 128 + 4: the ABI takes ldo % 4 == 0) whose surroundings are checked afterwards.  The rows of k and v past Sk inside the allocation hold keys
that dominate (row Sk + i is 16 * q[37 i mod Sq]: a score of ~260 base-2 units for its own query, beyond every real score for every query of
family N and for about four in ten of the others) with v = 1e4; the result must equal, bit for bit, the same call on a buffer whose extra rows
are zero.  Every test asserts lib.attn_vt_launch_plan for the form it claims to exercise; none sets X2V_ATTN_MAP / _ROT / _SHORT."""
import os

import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu
POISON = -1984.0  # exact in bf16; no output of these cases comes near it
BF16 = torch.bfloat16
BIG_V = 1.0e4
CASES = {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_ATTN_PARITY_TABLE")  # where to write the table of measured ratios (profiles/attn_fp64_parity.txt is one run's)
    if not path:
        return
    try:
        with open(path, "w") as f:
            for name in sorted(CASES):
                f.write(f"# {name}: {len(CASES[name].rows)} checks, largest relL2 / Y = {CASES[name].max_ratio:.3f}, largest d/tol = {max((r[4] for r in CASES[name].rows), default=0):.3f}\n")
            for name in sorted(CASES):
                f.write("\n".join(CASES[name].table()) + "\n")
    except OSError:
        pass


def case(name):
    return CASES.setdefault(name, A.Case(name))


# ------------------------------------------------------------------------------------------------------------------- buffers
def window(rows, HD, dtype=BF16):
    """A poisoned [rows + 4, HD + 4] buffer and its [rows, HD] window (two rows down: a 16-byte aligned start with an 8-byte aligned token stride)."""
    big = torch.full((rows + 4, HD + 4), POISON, dtype=dtype, device="cuda")
    return big, big[2 : rows + 2, :HD]


def poison_intact(big, rows, HD):
    return bool((big[:2] == POISON).all() and (big[rows + 2 :] == POISON).all() and (big[2 : rows + 2, HD:] == POISON).all())


def fused(q, k, v, H, heads=None, seq_rows=None, seed=0):
    """[rows, 3 * H * 128 + 64] on the device with q | k | v of the given heads side by side (q [Hc, Sq, 128], k / v [Hc, Sk, 128] on the CPU; the
    other heads, if any, hold seeded N(0, 1) noise) and its twin whose k / v rows past Sk are zero instead of dominant.  seq_rows: the slot
    height of a stacked sequence (a multiple of 64), else the smallest that leaves one whole key tile of extra rows."""
    (Hc, Sq, _), Sk, HD = q.shape, k.shape[1], H * 128
    heads = list(range(H)) if heads is None else heads
    rows = seq_rows or max(Sq, (Sk + 63) // 64 * 64 + 64)
    ld = 3 * HD + 64
    if len(heads) < H:
        buf = torch.randn(rows, ld, generator=torch.Generator(device="cuda").manual_seed(1000 + seed), device="cuda", dtype=torch.float32).to(BF16)
    else:
        buf = torch.zeros(rows, ld, dtype=BF16, device="cuda")
    parts = buf.as_strided((rows, 3, H, 128), (ld, HD, 128, 1))
    hs = torch.as_tensor(heads, device="cuda")
    parts[:Sq, 0, hs] = q.permute(1, 0, 2).cuda()
    parts[:Sk, 1, hs] = k.permute(1, 0, 2).cuda()
    parts[:Sk, 2, hs] = v.permute(1, 0, 2).cuda()
    buf[:, 3 * HD :] = BIG_V
    zero = buf.clone()
    if rows > Sk:
        idx = (37 * torch.arange(rows - Sk, device="cuda")) % Sq
        parts[Sk:, 1] = 16 * parts[idx, 0]
        parts[Sk:, 2] = BIG_V
        zero[Sk:, HD : 3 * HD] = 0
    return buf, zero


def views(buf, Sq, Sk, H):
    HD = H * 128
    return buf[:Sq, :HD], buf[:Sk, HD : 2 * HD], buf[:Sk, 2 * HD : 3 * HD]


def head_major(out, H, heads=None, rows=None):
    o = out.reshape(out.shape[0], H, 128)
    if heads is not None:
        o = o[:, torch.as_tensor(heads, device=o.device)]
    if rows is not None:
        o = o[rows.to(o.device)]
    return o.permute(1, 0, 2).contiguous().cpu()


def attend(lib, buf, Sq, Sk, H, variant, scale=0.0):
    q, k, v = views(buf, Sq, Sk, H)
    big, out = window(Sq, H * 128)
    assert out.data_ptr() % 16 == 0 and out.stride(0) % 8 == 4
    lib.attention(q, k, v, H, scale=scale, out=out, variant=variant)
    assert poison_intact(big, Sq, H * 128), "wrote outside the output window"
    return out


def attend_twice(lib, bufs, Sq, Sk, H, variant, scale=0.0):
    got = attend(lib, bufs[0], Sq, Sk, H, variant, scale)
    assert torch.equal(got, attend(lib, bufs[1], Sq, Sk, H, variant, scale)), "rows of k / v past Sk reached the result"
    return got


def fast(lib, pre=False, one_walk=True, stagger=False):
    return lib.ATTN_FAST | (lib.ATTN_Q_PRESCALED if pre else 0) | (lib.ATTN_ONE_WALK if one_walk else 0) | (lib.ATTN_STAGGER if stagger else 0)


def both_buffers(inp, H=None, heads=None, scale=0.0, seed=0):
    """{False: (dominant, zero) with q as is, True: the same with a prescaled q}"""
    H = H or inp.H
    return {pre: fused(inp.q_for("pre" if pre else "vt", scale), inp.k, inp.v, H, heads, seed=seed) for pre in (False, True)}


# ------------------------------------------------------------------------------------------------------------------- Sk / Sq sweeps
def sweep(lib, Sq, Sk, H):
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True) == (False, False, False)
    kernels = [("pipe v0", 0, "pipe", False), ("pipe v4 eager", 4, "pipe", False), ("pipe v5 thr4", 5, "pipe", False), ("pipe v6 thr8", 6, "pipe", False),
               ("v9", fast(lib), "vt", False), ("v9 prescaled", fast(lib, pre=True), "pre", True)]
    for fam, spike in A.sweep_families():
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        for form in A.FORMS:
            inp.assert_margins(form)
        bufs, outs = both_buffers(inp), {}
        for name, variant, form, pre in kernels:
            got = head_major(attend_twice(lib, bufs[pre], Sq, Sk, H, variant), H)
            case(name).check(got, A.expect(inp, form), "sweep")
            outs[name] = got
        assert torch.equal(outs["pipe v0"], outs["pipe v6 thr8"]), "variant 0 is variant 6"
        tol = A.expect(inp, "pipe").tol()
        for a, b in (("pipe v4 eager", "pipe v5 thr4"), ("pipe v4 eager", "pipe v6 thr8"), ("pipe v5 thr4", "pipe v6 thr8")):
            assert ((outs[a].double() - outs[b].double()).abs() <= tol).all(), f"{inp.name}: {a} and {b} differ by more than the bar"


@pytest.mark.parametrize("Sk", A.SK_SWEEP)
def test_sk_sweep(lib, Sk):
    """nt = 1..5 and 17: both exits of v9's unrolled walk, a last tile with and without the mask, left = 1 and 63."""
    sweep(lib, A.SK_SWEEP_SQ, Sk, A.SK_SWEEP_H)


@pytest.mark.parametrize("Sq", A.SQ_SWEEP)
@pytest.mark.parametrize("Sk", A.SQ_SWEEP_SK)
def test_sq_sweep(lib, Sk, Sq):
    """The 16-row group, the 32-row wave and the 256-row block tails."""
    sweep(lib, Sq, Sk, A.SQ_SWEEP_H)


def test_scale(lib):
    """A non-default scale on every entry that takes one, and scale = 0 selecting 1 / sqrt(128)."""
    Sq, Sk, H = A.SCALE_SHAPE
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True) == (False, False, False)
    for fam, spike in (("R", "middle"), ("H", "none"), ("U", "none")):
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        bufs = both_buffers(inp)[False]
        for name, variant, form in (("pipe v0", 0, "pipe"), ("pipe v4 eager", 4, "pipe"), ("pipe v5 thr4", 5, "pipe"), ("v9", fast(lib), "vt")):
            inp.assert_margins(form, A.ODD_SCALE)
            got = attend_twice(lib, bufs, Sq, Sk, H, variant, A.ODD_SCALE)
            case(name).check(head_major(got, H), A.expect(inp, form, A.ODD_SCALE), "scale=0.05")
            assert torch.equal(attend(lib, bufs[0], Sq, Sk, H, variant, 0.0), attend(lib, bufs[0], Sq, Sk, H, variant, A.DEFAULT_SCALE)), "scale = 0 is 1/sqrt(128)"
            if fam == "R":
                assert not torch.equal(got, attend(lib, bufs[0], Sq, Sk, H, variant, 0.0))


# ------------------------------------------------------------------------------------------------------------------- staggered walk
@pytest.mark.parametrize("Sk", A.STAGGER_SK)
def test_staggered_walk(lib, Sk):
    """Nine query blocks of one head: rot = 0..7 and the ninth block back at 0; nt = 16, 17, 17, 18, with and without a masked last tile (which
    must stay last).  Blocks 0 and 8 (rot = 0) equal the unstaggered launch bit for bit."""
    Sq, H = A.STAGGER_SQ, 1
    assert lib.attn_vt_launch_plan(Sq, Sk, H, stagger=True, one_walk=True) == (False, True)
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True) == (False, False)
    for fam, spike in A.P9_FAMILIES:
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        bufs = both_buffers(inp)
        for pre in (False, True):
            got = attend_twice(lib, bufs[pre], Sq, Sk, H, fast(lib, pre, stagger=True))
            case("v9 staggered" + (" prescaled" if pre else "")).check(head_major(got, H), A.expect(inp, "pre" if pre else "vt"), "stagger")
            plain = attend(lib, bufs[pre][0], Sq, Sk, H, fast(lib, pre))
            assert torch.equal(got[:256], plain[:256]) and torch.equal(got[2048:], plain[2048:]), "query blocks with rot = 0 differ from the unstaggered walk"


# ------------------------------------------------------------------------------------------------------------------- XCD remap
def per_head(lib, buf, Sq, Sk, H, variant):
    """H launches of one head each on column views of the fused buffer: the plain grid, the same summation order."""
    assert lib.attn_vt_launch_plan(Sq, Sk, 1, one_walk=True, with_short=True) == (False, False, False)
    HD = H * 128
    big, out = window(Sq, HD)
    for h in range(H):
        c = slice(h * 128, (h + 1) * 128)
        lib.attention(buf[:Sq, c], buf[:Sk, HD:][:, c], buf[:Sk, 2 * HD :][:, c], 1, out=out[:, c], variant=variant)
    assert poison_intact(big, Sq, HD)
    return out


@pytest.mark.parametrize("Sq,Sk,H", A.XCD_SHAPES)
def test_xcd_remap(lib, Sq, Sk, H):
    """nwg = 513 (nwg % 8 = 1: one XCD's range is one longer) and 576 (8 | nwg): every (head, query block) is computed exactly once."""
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True) == (True, False, False)
    assert (((Sq + 255) // 256) * H) % 8 == (1 if H == 57 else 0)
    for fam, spike in A.P9_FAMILIES:
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        bufs = both_buffers(inp)
        for pre in (False, True):
            got = attend_twice(lib, bufs[pre], Sq, Sk, H, fast(lib, pre))
            case("v9 xcd remap" + (" prescaled" if pre else "")).check(head_major(got, H), A.expect(inp, "pre" if pre else "vt"), "xcd")
            if not pre:
                assert torch.equal(got, per_head(lib, bufs[pre][0], Sq, Sk, H, fast(lib, pre))), "remapped grid differs from per-head launches"


def stacked(inps, rps, seq_len, H, heads=None, pre=False):
    """The fused buffers of B stacked sequences (slot height rps, keys the first seq_len rows of a slot, the rest of the slot dominant / v = 1e4)."""
    pairs = [fused(i.q_for("pre" if pre else "vt"), i.k, i.v, H, heads, seq_rows=rps, seed=b) for b, i in enumerate(inps)]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def attend_batched(lib, buf, B, rps, seq_len, H, pre, all_rows_query=True):
    HD = H * 128
    q, k, v = views(buf, B * rps, B * rps, H)
    vt = lib.transpose_heads(v, H)
    big, out = window(B * rps, HD)
    lib.attention_batched(q, k, vt, H, B, rps, seq_len, out=out, prescaled=pre, all_rows_query=all_rows_query, one_launch=True)
    assert poison_intact(big, B * rps, HD), "wrote outside the output window"
    if not all_rows_query:
        assert all(bool((out[b * rps + seq_len : (b + 1) * rps] == POISON).all()) for b in range(B)), "rows past seq_len written"
    return out


def test_xcd_remap_batched(lib):
    B, rps, Sk, H = A.XCD_BATCHED
    assert lib.attn_vt_launch_plan(rps, Sk, H, batch=B, with_short=True) == (True, False, False) and (((rps + 255) // 256) * H * B) % 8 == 2
    for fam, spike in A.P9_FAMILIES:
        inps = [A.Inputs(fam, rps, Sk, H, spike, seed=b) for b in range(B)]
        bufs = stacked(inps, rps, Sk, H)
        got = attend_batched(lib, bufs[0], B, rps, Sk, H, False)
        assert torch.equal(got, attend_batched(lib, bufs[1], B, rps, Sk, H, False)), "a slot's padding rows reached the result"
        for b, inp in enumerate(inps):
            rows = slice(b * rps, (b + 1) * rps)
            case("v9 xcd remap batched").check(head_major(got[rows], H), A.expect(inp, "vt"), f"seq {b}")
            assert torch.equal(got[rows], per_head(lib, bufs[0][rows], rps, Sk, H, fast(lib))), f"sequence {b}: remapped grid differs from per-head launches"


def test_batched(lib):
    """Three stacked sequences of 257 keys in slots of 320 rows; every row of a slot a query, or only the first 257."""
    B, rps, Sk, H = A.BATCHED
    for fam, spike in A.P9_FAMILIES:
        inps = [A.Inputs(fam, rps, Sk, H, spike, seed=b) for b in range(B)]
        for pre in (False, True):
            bufs = stacked(inps, rps, Sk, H, pre=pre)
            for all_rows in (True, False):
                Sq = rps if all_rows else Sk
                assert lib.attn_vt_launch_plan(Sq, Sk, H, batch=B, with_short=True) == (False, False, False)
                got = attend_batched(lib, bufs[0], B, rps, Sk, H, pre, all_rows)
                assert torch.equal(got, attend_batched(lib, bufs[1], B, rps, Sk, H, pre, all_rows)), "a slot's padding rows reached the result"
                for b, inp in enumerate(inps):
                    cut = inp if all_rows else inp.take(rows=torch.arange(Sk))
                    case("v9 batched" + (" prescaled" if pre else "")).check(head_major(got[b * rps : b * rps + Sq], H), A.expect(cut, "pre" if pre else "vt"), f"seq {b}")


# ------------------------------------------------------------------------------------------------------------------- persistent form
@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def p9_check(lib, Sq, Sk, H, pre, what):
    """The persistent form on all heads: bit-equal with the one-walk form, float64 on the checked heads and query blocks."""
    assert lib.attn_vt_launch_plan(Sq, Sk, H, with_short=True) == (False, False, True) and lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True)[2] is False
    heads, rows = A.checked_heads(H), A.checked_rows(Sq)
    for fam, spike in A.P9_FAMILIES:
        inp = A.Inputs(fam, Sq, Sk, len(heads), spike)
        bufs = fused(inp.q_for("pre" if pre else "vt"), inp.k, inp.v, H, heads, seed=Sk)
        got = attend_twice(lib, bufs, Sq, Sk, H, fast(lib, pre, one_walk=False))
        assert torch.equal(got, attend(lib, bufs[0], Sq, Sk, H, fast(lib, pre))), f"{what}: persistent and one-walk forms differ"
        cut = inp if rows.numel() == Sq else inp.take(rows=rows)
        case("p9" + (" prescaled" if pre else "")).check(head_major(got, H, heads, None if rows.numel() == Sq else rows), A.expect(cut, "pre" if pre else "vt"), what)


@pytest.mark.parametrize("nt", A.P9_NT)
def test_p9_every_walk_length(lib, cus, nt):
    """Two items per workgroup at every nt: every q-piece schedule qps = (12 + nt) / (nt - 3), those that do not divide 16 included."""
    p9_check(lib, A.P9_SQ, nt * A.TILE, cus, nt % 2 == 1, f"nt={nt}")


@pytest.mark.parametrize("i", range(5))
def test_p9_item_walk(lib, cus, i):
    label, Sq, Sk, H, pre = A.p9_walk_cases(cus)[i]
    p9_check(lib, Sq, Sk, H, pre, label)


def test_p9_batched(lib, cus):
    B, rps, Sk, _ = A.P9_BATCHED
    H = cus // 2
    assert lib.attn_vt_launch_plan(rps, Sk, H, batch=B, with_short=True) == (False, False, True)
    heads = A.checked_heads(H)
    for fam, spike in A.P9_FAMILIES:
        inps = [A.Inputs(fam, rps, Sk, len(heads), spike, seed=b) for b in range(B)]
        for pre in (False, True):
            bufs = stacked(inps, rps, Sk, H, heads, pre=pre)
            got = attend_batched(lib, bufs[0], B, rps, Sk, H, pre)
            assert torch.equal(got, attend_batched(lib, bufs[1], B, rps, Sk, H, pre)), "a slot's padding rows reached the result"
            for b, inp in enumerate(inps):
                slot = bufs[0][b * rps : (b + 1) * rps]
                assert torch.equal(got[b * rps : (b + 1) * rps], attend(lib, slot, rps, Sk, H, fast(lib, pre))), f"sequence {b}: persistent and one-walk forms differ"
                case("p9 batched" + (" prescaled" if pre else "")).check(head_major(got[b * rps : (b + 1) * rps], H, heads), A.expect(inp, "pre" if pre else "vt"), f"seq {b}")
