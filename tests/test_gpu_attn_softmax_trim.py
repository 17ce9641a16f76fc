"""The softmax half-step of the ping-pong attention kernels (A9_EXP_TILE / A9_SOFTMAX in lightx2v_amd/csrc/attn.hip: attn_fwd_v9_kernel and the
persistent attn_fwd_p9_kernel) with its sum chains started from the first P under no asm operand, against the float64
reference through the harness and the acceptance of tests/test_gpu_attn_fp64.py unchanged (attn_ref.expect / Case.check: every element within
2^-7 |o| + 1.05 * 2^-8 * A, relL2 <= 1.5 Y; fused q | k | v buffer with dominant rows past Sk, poisoned output window).

Shapes: H = 2; Sq = 256 (one workgroup) and 300 (a ragged second one); Sk = 64 * 3 + 17 (both unrolled loop copies and the masked last tile)
and 64 * 4 (whole tiles).  Inputs are attn_ref's 'R' family with the keys behind the first tile halved and a few K rows planted
(tests/attn_chain_guard_ref.build_arm), so that one key tile of one wave reaches one arm and every other tile stays on the hot path:
  hot            nothing crosses: the hot path only behind tile 0;
  chainGC-where  one key 9 .. 12 above the reference in chain C (key parity) of query group G, in tile 2 / in the last (masked) tile;
  eight-at-2^5   eight consecutive keys of one lane 5.2 .. 5.8 above the reference: the pair-sum guard fires without cause (a chain-max guard
                 would not) — the output must simply be right;
  inf            one key more than 140 binary orders above it: the hot path's P is +inf and is recovered in the cold branch;
  second-wave    the crossing key for the 33rd query row only.
Every expectation, and the proof that a construction lands in its arm (attn_chain_guard_ref.assert_lands, float64 margins), is computed on the
host before the launch.  The persistent form runs at its smallest legal shape (512 keys, Sq = 4096, H = 32) and must equal the one-walk form
bit for bit; a batched launch (z = 2) must equal its two single launches bit for bit."""
import pytest
import torch

from tests import attn_chain_guard_ref as C
from tests import attn_ref as A
from tests import test_gpu_attn_fp64 as F

pytestmark = pytest.mark.gpu
H = 2
SHAPES = [(256, 64 * 3 + 17), (300, 64 * 3 + 17), (256, 64 * 4), (300, 64 * 4)]
P9_SHAPE = (4096, 512, 32)
P9_ARMS = ("hot", "chain01-middle", "chain10-last", "eight-at-2^5", "inf")
CASES = {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def case(name):
    return CASES.setdefault(name, A.Case(name))


@pytest.mark.parametrize("Sq,Sk", SHAPES)
@pytest.mark.parametrize("arm", C.ARMS)
def test_v9_arm(lib, arm, Sq, Sk):
    inp, tile, wave, kind = C.build_arm(arm, Sq, Sk, H)
    C.assert_lands(inp, tile, wave, kind)
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True) == (False, False, False)
    bufs = F.both_buffers(inp)
    for pre in (False, True):
        got = F.head_major(F.attend_twice(lib, bufs[pre], Sq, Sk, H, F.fast(lib, pre)), H)
        rel, y, worst = case("v9 softmax trim" + (" prescaled" if pre else "")).check(got, A.expect(inp, "pre" if pre else "vt"), f"{arm} ({kind})")
        print(f"v9{' prescaled' if pre else ''} {arm} Sq={Sq} Sk={Sk}: relL2 {rel:.4e}  Y {y:.4e}  worst d/tol {worst:.3f}")


@pytest.mark.parametrize("arm", P9_ARMS)
def test_p9_smallest_shape(lib, arm):
    Sq, Sk, heads_all = P9_SHAPE
    assert lib.attn_vt_launch_plan(Sq, Sk, heads_all, with_short=True) == (False, False, True)
    assert lib.attn_vt_launch_plan(Sq, Sk, heads_all, one_walk=True, with_short=True)[2] is False
    heads, rows = A.checked_heads(heads_all), A.checked_rows(Sq)
    inp, tile, wave, kind = C.build_arm(arm, Sq, Sk, len(heads))
    C.assert_lands(inp, tile, wave, kind)
    assert wave * A.WAVE_ROWS in rows.tolist(), "the aimed wave is not among the checked rows"
    cut = inp.take(rows=rows)
    for pre in (False, True):
        bufs = F.fused(inp.q_for("pre" if pre else "vt"), inp.k, inp.v, heads_all, heads, seed=Sk)
        got = F.attend_twice(lib, bufs, Sq, Sk, heads_all, F.fast(lib, pre, one_walk=False))
        assert torch.equal(got, F.attend(lib, bufs[0], Sq, Sk, heads_all, F.fast(lib, pre))), f"{arm}: persistent and one-walk forms differ"
        rel, y, worst = case("p9 softmax trim" + (" prescaled" if pre else "")).check(F.head_major(got, heads_all, heads, rows), A.expect(cut, "pre" if pre else "vt"), f"{arm} ({kind})")
        print(f"p9{' prescaled' if pre else ''} {arm}: relL2 {rel:.4e}  Y {y:.4e}  worst d/tol {worst:.3f}")


@pytest.mark.parametrize("Sk", [64 * 3 + 17, 64 * 4])
def test_batched_equals_single_launches(lib, Sk):
    """z = 2: two stacked sequences in slots of 320 rows (every row of a slot a query), each with its own planted arm."""
    B, rps = 2, 320
    inps = [C.build_arm(arm, rps, Sk, H)[0] for arm in ("chain11-last", "chain00-middle")]
    assert lib.attn_vt_launch_plan(rps, Sk, H, batch=B, with_short=True) == (False, False, False)
    for pre in (False, True):
        bufs = F.stacked(inps, rps, Sk, H, pre=pre)
        got = F.attend_batched(lib, bufs[0], B, rps, Sk, H, pre)
        assert torch.equal(got, F.attend_batched(lib, bufs[1], B, rps, Sk, H, pre)), "a slot's padding rows reached the result"
        for b, inp in enumerate(inps):
            slot = slice(b * rps, (b + 1) * rps)
            assert torch.equal(got[slot], F.attend(lib, bufs[0][slot], rps, Sk, H, F.fast(lib, pre))), f"sequence {b}: batched and single launches differ"
            case("v9 softmax trim batched" + (" prescaled" if pre else "")).check(F.head_major(got[slot], H), A.expect(inp, "pre" if pre else "vt"), f"seq {b}")
