"""The sum guard in front of the lazy rescale of the ping-pong attention kernels (A9_SOFTMAX, lightx2v_amd/csrc/attn.hip), checked without a GPU
in fp32 torch (tests/attn_guard_ref.py): a lane's tile sum, added as the kernel adds it, reaches GUARD_T = 2^8 (1 - 2^-10) whenever one of its
sixteen P values exceeds 2^8 — so the max search, the lane swaps and the rescale may sit behind it — and the guard is allowed to fire without
cause.  The walk with the decision taken guard-then-max gives the outputs of attn_ref.emulate(..., 'lazy8') bit for bit; the inputs of
tests/test_gpu_attn_sum_guard.py land in the arms they are built for."""
import math

import pytest
import torch

from tests import attn_guard_ref as G
from tests import attn_ref as A

F32 = torch.float32
TWO8 = 2.0 ** G.THR


def exact16(p16):
    """The condition the guard stands in front of, on P: some score above THR <=> some P above 2^THR."""
    return (p16 > TWO8).any(-1)


def test_threshold_value():
    """Strictly below 2^8 by far more than v_exp_f32's error there (about one ulp = 2^-23 relative), and an fp32 number."""
    assert G.GUARD_T == 255.75 and G.GUARD_T == float(torch.tensor(G.GUARD_T, dtype=F32))
    assert G.GUARD_T < TWO8 * (1.0 - 2.0 ** -20)


def test_guard_fires_whenever_a_value_exceeds_the_threshold():
    g = torch.Generator().manual_seed(7)
    n = 1 << 14
    # sixteen non-negative values around the threshold: magnitudes 2^u, u in [-20, 9], a third of the vectors with one value set next to 2^8
    p = torch.exp2(torch.rand(n, 16, generator=g) * 29.0 - 20.0).to(F32)
    near = TWO8 * (1.0 + (torch.rand(n, generator=g) - 0.5) * 2.0 ** -8).to(F32)
    slot = torch.randint(0, 16, (n,), generator=g)
    third = torch.arange(n) % 3 == 0
    p[third, slot[third]] = near[third]
    p[torch.arange(n) % 3 == 1] *= 2.0 ** -6  # a third with everything small
    ex, gd = exact16(p), G.guard16(p)
    assert int(ex.sum()) > n // 8 and int((~ex).sum()) > n // 8, "the draw does not sit around the threshold"
    assert bool((gd | ~ex).all()), f"{int((ex & ~gd).sum())} vectors hold a value above 2^8 and do not fire the guard"
    print(f"guard: {n} vectors, {int(ex.sum())} with a value above 2^8 (all fire), {int((gd & ~ex).sum())} fire without one")


@pytest.mark.parametrize("slot", range(16))
def test_guard_on_single_values(slot):
    zeros = torch.zeros(16, dtype=F32)
    above, below = zeros.clone(), zeros.clone()
    above[slot] = torch.nextafter(torch.tensor(TWO8, dtype=F32), torch.tensor(math.inf, dtype=F32))
    below[slot] = torch.nextafter(torch.tensor(TWO8, dtype=F32), torch.tensor(0.0, dtype=F32))  # the fp32 neighbours of 2^8
    assert bool(exact16(above)) and bool(G.guard16(above))
    assert not bool(exact16(below))  # (the guard may fire here: it does, 2^8 (1 - 2^-24) >= GUARD_T)
    tiny = zeros.clone()
    tiny[slot] = TWO8 * (1.0 + 2.0 ** -22)
    assert float(tiny[slot]) > TWO8 and bool(exact16(tiny)) and bool(G.guard16(tiny))
    inf = torch.rand(16, generator=torch.Generator().manual_seed(slot)).to(F32)
    inf[slot] = math.inf
    assert bool(exact16(inf)) and bool(G.guard16(inf))
    # just above among values that an fp32 sum absorbs or rounds: the sum of non-negative addends never falls below its largest
    crowd = torch.full((16,), 2.0 ** -17, dtype=F32)
    crowd[slot] = above[slot]
    assert bool(G.guard16(crowd))


def test_false_positive_by_construction():
    """Sixteen values of 2^4: both chains reach 2^7, the lane's sum is 2^8 >= GUARD_T, and no value is anywhere near 2^8."""
    p = torch.full((16,), 2.0 ** 4, dtype=F32)
    c0, c1 = G.chain_sums(p)
    assert float(c0) == float(c1) == 2.0 ** 7
    assert bool(G.guard16(p)) and not bool(exact16(p))
    eight = torch.zeros(16, dtype=F32)
    eight[8:] = 2.0 ** 5.5  # case (b) of the GPU module
    assert bool(G.guard16(eight)) and not bool(exact16(eight))


def test_lane_map():
    """lane qd owns keys 32 j + 8 qd + e, in (j, e) order."""
    keys = torch.arange(64, dtype=F32)
    lanes = G.lane_values(keys)
    for qd in range(4):
        assert lanes[qd].tolist() == [32 * j + 8 * qd + e for j in range(2) for e in range(8)]
    c0, c1 = G.chain_sums(lanes)
    assert c0.tolist() == [sum(32 * j + 8 * qd + e for j in range(2) for e in range(0, 8, 2)) for qd in range(4)]
    assert c1.tolist() == [sum(32 * j + 8 * qd + e for j in range(2) for e in range(1, 8, 2)) for qd in range(4)]


GUARDED = [("R", "none"), ("R", "first"), ("R", "middle"), ("R", "last"), ("N", "none"), ("H", "none"), ("U", "none")]


@pytest.mark.parametrize("Sq,Sk", [(33, 193), (33, 257), (257, 1031)])
def test_guard_then_max_is_the_max_decision(Sq, Sk):
    """Same decisions by construction (the guard includes every tile on which the exact condition holds), pinned on the emulation's outputs."""
    fired = 0
    for fam, spike in GUARDED:
        inp = A.Inputs(fam, Sq, Sk, 2, spike)
        s, v = A.scores(inp.q, inp.k, q_rounded=True, dtype=F32), inp.v.to(F32)
        trace = []
        assert torch.equal(G.emulate_guarded(s, v, trace=trace), A.emulate(s, v, "lazy8")), f"{inp.name}: guard-then-max and max-only outputs differ"
        for tr in trace:
            assert bool((tr["guard"] | ~tr["exact"]).all()), f"{inp.name}: the exact condition holds on a tile whose guard is silent"
            fired += int(tr["exact"].sum())
    assert fired > 0, "no tile of these inputs rescales: the comparison shows nothing"


@pytest.mark.parametrize("Sk", [193, 257])
@pytest.mark.parametrize("case", G.CASES)
def test_gpu_cases_land_in_their_arm(case, Sk):
    inp, tile, wave, arm = G.build_case(case, 33, Sk, 2)
    trace = G.assert_lands(inp, tile, wave, arm)
    s, v = A.scores(inp.q, inp.k, q_rounded=True, dtype=F32), inp.v.to(F32)
    t32 = []
    assert torch.equal(G.emulate_guarded(s, v, trace=t32), A.emulate(s, v, "lazy8"))
    for a, b in zip(trace, t32):  # the fp32 walk takes the branches the float64 walk takes
        assert torch.equal(a["guard"], b["guard"]) and torch.equal(a["exact"], b["exact"])
    if case == "d":  # the hot path's P of the aimed key is +inf in fp32: the guard must fire on it
        top = float(trace[tile - 1]["top"][0, wave])
        assert top > 128.0 and math.isinf(float(torch.exp2(torch.tensor(top, dtype=F32))))
    if case == "e":  # the first wave never leaves the hot path
        assert not any(bool(tr["guard"][:, 0].any()) for tr in trace)
