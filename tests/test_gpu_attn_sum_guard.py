"""Every arm of the softmax half-step of the ping-pong attention kernels (A9_SOFTMAX in lightx2v_amd/csrc/attn.hip: attn_fwd_v9_kernel, and
attn_fwd_p9_kernel, which instantiates the same macro) against the float64 reference, through the harness and the acceptance of
tests/test_gpu_attn_fp64.py unchanged (attn_ref.Inputs / expect / Case.check: every element within 2^-7 |o| + 1.05 * 2^-8 * A, relL2 <= 1.5 Y;
fused q | k | v buffer with dominant rows past Sk, poisoned output window).

The row-max search, the lane swaps and the rescale sit behind a guard on the lane's tile sums.  The inputs are attn_ref's 'R' family with a few K
rows overwritten (tests/attn_guard_ref.py) so that the aimed key tile reaches one arm:
  (a) no score more than 2 above the first tile's max: hot path only behind tile 0;
  (b) eight consecutive keys of one lane 5.2 .. 5.8 above the running reference in tile 2: the guard fires, the exact condition does not;
  (c) one key 9 .. 12 above it, in a middle tile / in the partly filled last tile: rescale and recompute;
  (d) one key more than 140 binary orders above it in tile 1 (the row's q eight times as long): the hot path's P is +inf and is recovered;
  (e) the key of (c) for the 33rd query row only: the second wave alone takes the branch.
Every expectation, and the proof that a construction lands in its arm (float64 margins, attn_guard_ref.assert_lands), is computed on the host
before the launch.  Sq = 33 (one full wave and one row of the next), Sk = 193 / 257 (4 / 5 tiles, the last of one key), H = 2, the plain and
the prescaled v9 entry; one persistent walk (nt = 4, Sq = 257) runs the cases that fit whole tiles."""
import pytest
import torch

from tests import attn_guard_ref as G
from tests import attn_ref as A
from tests import test_gpu_attn_fp64 as F

pytestmark = pytest.mark.gpu
SQ, H = 33, 2
CASES = {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def case(name):
    return CASES.setdefault(name, A.Case(name))


@pytest.mark.parametrize("Sk", [193, 257])
@pytest.mark.parametrize("which", G.CASES)
def test_v9_arm(lib, which, Sk):
    inp, tile, wave, arm = G.build_case(which, SQ, Sk, H)
    G.assert_lands(inp, tile, wave, arm)
    exp = {pre: A.expect(inp, "pre" if pre else "vt") for pre in (False, True)}
    assert lib.attn_vt_launch_plan(SQ, Sk, H, one_walk=True, with_short=True) == (False, False, False)
    bufs = F.both_buffers(inp)
    for pre in (False, True):
        got = F.head_major(F.attend_twice(lib, bufs[pre], SQ, Sk, H, F.fast(lib, pre)), H)
        rel, y, worst = case("v9 sum guard" + (" prescaled" if pre else "")).check(got, exp[pre], f"({which}) {arm}")
        print(f"v9{' prescaled' if pre else ''} ({which}) Sk={Sk}: relL2 {rel:.4e}  Y {y:.4e}  worst d/tol {worst:.3f}")


@pytest.mark.parametrize("which", ["a", "b", "c-middle", "d", "e"])
def test_p9_arm(lib, which):
    """The persistent form: nt = 4 whole tiles, two query blocks per head, on a head count that takes plan bit 9; float64 on the checked heads
    and bit-equal with the one-walk form on all."""
    Sq, Sk, heads_all = A.P9_SQ, 4 * A.TILE, torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.attn_vt_launch_plan(Sq, Sk, heads_all, with_short=True) == (False, False, True)
    heads = A.checked_heads(heads_all)
    inp, tile, wave, arm = G.build_case(which, Sq, Sk, len(heads))
    G.assert_lands(inp, tile, wave, arm)
    for pre in (False, True):
        exp = A.expect(inp, "pre" if pre else "vt")
        bufs = F.fused(inp.q_for("pre" if pre else "vt"), inp.k, inp.v, heads_all, heads, seed=Sk)
        got = F.attend_twice(lib, bufs, Sq, Sk, heads_all, F.fast(lib, pre, one_walk=False))
        assert torch.equal(got, F.attend(lib, bufs[0], Sq, Sk, heads_all, F.fast(lib, pre))), f"({which}): persistent and one-walk forms differ"
        rel, y, worst = case("p9 sum guard" + (" prescaled" if pre else "")).check(F.head_major(got, heads_all, heads), exp, f"({which}) {arm}")
        print(f"p9{' prescaled' if pre else ''} ({which}): relL2 {rel:.4e}  Y {y:.4e}  worst d/tol {worst:.3f}")
