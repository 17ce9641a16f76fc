"""The chain-max witness for the guard in front of the lazy rescale of the ping-pong attention kernels (A9_SOFTMAX, lightx2v_amd/csrc/attn.hip),
checked without a GPU in fp32 torch (tests/attn_chain_guard_ref.py) beside the pair-sum guard the kernels use.  A P above 2^8 sits in exactly
one of a lane's four chains, and a round-to-nearest sum of non-negative addends is never below its largest addend, so that chain's sum alone
reaches GUARD_T = 2^8 (1 - 2^-10): the chain-max guard fires whenever the exact condition (some score more than THR above the reference) holds.
A chain sum never exceeds chain 0 + chain 1, so it fires on a subset of the tiles the pair-sum guard fires on; the cold branch decides by the
exact condition either way, so the m_run / rescale sequence is the same under both.  (The chain-max form measured slower on the GPU and is not
what the kernels run: DESIGN.md §4.1.  These properties are what would make a later swap bit-exact.)"""
import math

import pytest
import torch

from tests import attn_chain_guard_ref as C
from tests import attn_guard_ref as G
from tests import attn_ref as A

F32 = torch.float32
TWO8 = 2.0 ** C.THR
ABOVE = float(torch.nextafter(torch.tensor(float(C.THR), dtype=F32), torch.tensor(math.inf, dtype=F32)))  # the smallest fp32 score above THR


def tile_guards(sc):
    """sc [n, 2 groups, 4 lanes, 16]: one wave's view of a tile for one query column -> (exact, chain guard, pair guard) per tile [n]."""
    p = torch.exp2(sc.to(F32))
    return (sc > C.THR).flatten(1).any(-1), C.guard16(p).flatten(1).any(-1), C.pair_guard16(p).flatten(1).any(-1)


def test_exp2_of_the_smallest_crossing_score_reaches_the_threshold():
    """The step from `sc > THR` to `P >= GUARD_T` with 2^-10 to spare (the kernel's v_exp_f32 is good to about an ulp, as torch's exp2 is)."""
    p = float(torch.exp2(torch.tensor(ABOVE, dtype=F32)))
    assert p >= TWO8 * (1.0 - 2.0 ** -22) > C.GUARD_T == 255.75


def test_random_tiles():
    g = torch.Generator().manual_seed(11)
    n = 1 << 13
    sc = torch.rand(n, 2, 4, 16, generator=g) * 29.0 - 20.0  # scores in [-20, 9)
    sc[torch.arange(n) % 3 == 1] -= 6.0  # a third with everything below THR
    third = torch.arange(n) % 3 == 0  # a third with one score set next to THR
    idx = torch.randint(0, 128, (n,), generator=g)
    near = C.THR + (torch.rand(n, generator=g) - 0.5) * 2.0 ** -6
    flat = sc.view(n, 128)
    flat[third, idx[third]] = near[third]
    ex, ch, pr = tile_guards(sc)
    assert int(ex.sum()) > n // 8 and int((~ex).sum()) > n // 8, "the draw does not sit around the threshold"
    assert bool((ch | ~ex).all()), f"{int((ex & ~ch).sum())} tiles hold a crossing score and do not fire the chain-max guard"
    assert bool((pr | ~ch).all()), f"{int((ch & ~pr).sum())} tiles fire the chain-max guard and not the pair-sum guard"
    assert int((pr & ~ch).sum()) > 0, "no tile on which the pair-sum guard over-reports and the chain-max guard does not: the subset is not shown to be proper"
    print(f"{n} tiles: exact {int(ex.sum())}, chain-max guard {int(ch.sum())}, pair-sum guard {int(pr.sum())}")


@pytest.mark.parametrize("qd", range(4))
@pytest.mark.parametrize("g,chain", C.CHAINS)
def test_one_crossing_score_per_chain_position(g, chain, qd):
    """A score one fp32 step above THR at every key of chain `chain` of query group g in lane qd, alone (every other P = 0), among addends the
    sum absorbs, and in a crowd of equal small values: the guard fires; one step below THR is not the exact condition."""
    for e in range(chain, 16, 2):
        for fill in (-1e30, -17.0, 2.0):
            sc = torch.full((1, 2, 4, 16), fill, dtype=F32)
            sc[0, g, qd, e] = ABOVE
            ex, ch, pr = tile_guards(sc)
            assert bool(ex) and bool(ch) and bool(pr), f"key {e} fill {fill}"
            c0, c1 = G.chain_sums(torch.exp2(sc[0, g, qd]))
            assert float((c0, c1)[chain]) >= C.GUARD_T, "the witness is the chain that holds the key"
        sc = torch.full((1, 2, 4, 16), -1e30, dtype=F32)
        sc[0, g, qd, e] = float(torch.nextafter(torch.tensor(float(C.THR), dtype=F32), torch.tensor(0.0, dtype=F32)))
        assert not bool(tile_guards(sc)[0])


def test_inf_and_equal_values():
    sc = torch.rand(1, 2, 4, 16, generator=torch.Generator().manual_seed(3)) - 3.0
    sc[0, 1, 2, 9] = 140.0  # P = +inf in fp32
    assert math.isinf(float(torch.exp2(sc[0, 1, 2, 9])))
    ex, ch, pr = tile_guards(sc)
    assert bool(ex) and bool(ch) and bool(pr)
    # all 16 P of a lane equal: at 2^4 each chain holds 2^7 and their sum 2^8 (a false positive of the pair-sum guard only); at 2^5 each chain holds
    # 2^8 and the chain-max guard over-reports as well; above 2^8 both must fire
    for level, want_chain, want_pair, want_exact in ((4.0, False, True, False), (5.0, True, True, False), (float(ABOVE), True, True, True)):
        sc = torch.full((1, 2, 4, 16), -1e30, dtype=F32)
        sc[0, 0, 3] = level
        ex, ch, pr = tile_guards(sc)
        assert (bool(ex), bool(ch), bool(pr)) == (want_exact, want_chain, want_pair), f"16 values at 2^{level}"
    eight = torch.full((1, 2, 4, 16), -1e30, dtype=F32)
    eight[0, 1, 2, 8:] = 5.0  # eight keys of a lane at 2^5: chain sums 2^7
    ex, ch, pr = tile_guards(eight)
    assert (bool(ex), bool(ch), bool(pr)) == (False, False, True)


GUARDED = [("R", "none"), ("R", "first"), ("R", "middle"), ("R", "last"), ("N", "none"), ("H", "none"), ("U", "none")]


@pytest.mark.parametrize("Sq,Sk", [(33, 193), (33, 257), (257, 1031)])
def test_same_decisions_under_both_guards(Sq, Sk):
    fired = 0
    for fam, spike in GUARDED:
        inp = A.Inputs(fam, Sq, Sk, 2, spike)
        s, v = A.scores(inp.q, inp.k, q_rounded=True, dtype=F32), inp.v.to(F32)
        new, old = [], []
        out = C.emulate_guarded(s, v, trace=new, witness="chain")
        assert torch.equal(out, C.emulate_guarded(s, v, trace=old, witness="pair")), f"{inp.name}: outputs differ between the guards"
        assert torch.equal(out, G.emulate_guarded(s, v)) and torch.equal(out, A.emulate(s, v, "lazy8")), f"{inp.name}: not the max-on-every-tile outputs"
        for a, b in zip(new, old):
            assert torch.equal(a["fired"], b["fired"]) and torch.equal(a["m"], b["m"]), f"{inp.name}: m_run / rescale sequences differ"
            assert bool((a["guard"] | ~a["exact"]).all()) and bool((b["guard"] | ~a["guard"]).all())
            fired += int(a["fired"].sum())
    assert fired > 0, "no tile of these inputs rescales: the comparison shows nothing"


@pytest.mark.parametrize("Sk", [64 * 3 + 17, 64 * 4])
@pytest.mark.parametrize("arm", C.ARMS)
def test_gpu_arms_land(arm, Sk):
    """The inputs of tests/test_gpu_attn_softmax_trim.py reach the arm they are built for, in float64 and in fp32."""
    inp, tile, wave, kind = C.build_arm(arm, 64, Sk, 2)
    t64 = C.assert_lands(inp, tile, wave, kind)
    s, v = A.scores(inp.q, inp.k, q_rounded=True, dtype=F32), inp.v.to(F32)
    t32 = []
    assert torch.equal(C.emulate_guarded(s, v, trace=t32), A.emulate(s, v, "lazy8"))
    for a, b in zip(t64, t32):
        assert torch.equal(a["guard"], b["guard"]) and torch.equal(a["exact"], b["exact"])
