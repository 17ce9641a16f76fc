"""The yardstick of tests/test_gpu_vae_attn16_fp64.py checked without a GPU: both emulations of a correct kernel pass tests/vae_attn16_ref.py's
acceptance on every case the GPU module runs, every subtly wrong kernel (vae_attn16_ref.MUTATIONS) is rejected at every shape where it can differ,
by the criterion named in REJECTED_BY, and the float64 reference agrees with a direct torch.softmax restatement."""
import math

import pytest
import torch

from tests import vae_attn16_ref as V

# mutation -> (family that must reject it, the criteria that may do so).  A wrong prefix limit is read out by family U ('finite' where the only key of a
# row is the one hidden: 0 / 0); a skipped rescale is an error of a power of two on a ladder that moves the reference maximum.
REJECTED_BY = {"see_one_more": ("U", {"readout"}), "hide_last_visible": ("U", {"readout", "finite"}), "block_first_row_limit": ("U", {"readout"}),
               "pad_keys_leak": ("U", {"readout"}), "skip_o_rescale": ("L", {"element"}), "skip_l_rescale": ("L", {"element"})}


@pytest.fixture(scope="module")
def inputs():
    return {c: V.case_inputs(*c) for c in V.CASES}


@pytest.mark.parametrize("case", V.CASES, ids=str)
def test_both_emulations_pass_the_acceptance(inputs, case):
    chk = V.Case("emulation", record=False)
    for inp in inputs[case]:
        exp = V.Expect(inp, keep=True)
        for kind, out in exp.emulated.items():
            chk.check(out, exp, kind)
    assert chk.max_worst <= 1 and chk.max_ratio <= 1 + 1e-12  # Y is the larger of the two by construction
    print(f"{case}: largest d/tol {chk.max_worst:.3f} over {len(chk.rows)} checks")


@pytest.mark.parametrize("mut", V.MUTATIONS)
def test_every_applicable_mutation_is_rejected_at_every_shape(inputs, mut):
    family, criteria = REJECTED_BY[mut]
    applied = 0
    for case in V.CASES:
        C, hw, frames = case
        if not V.mutation_applies(mut, hw * frames, hw):
            for inp in inputs[case]:  # where it does not apply it is no mutation: the same bits as the correct emulation
                assert torch.equal(V.emulate(inp.qkv, inp.n, C, hw, inp.scale, "lazy8", mut), V.emulate(inp.qkv, inp.n, C, hw, inp.scale, "lazy8")), (mut, inp.name)
            continue
        applied += 1
        seen = []
        for inp in inputs[case]:
            if inp.family != family:
                continue
            try:
                V.Case(mut, record=False).check(V.emulate(inp.qkv, inp.n, C, hw, inp.scale, "lazy8", mut), V.expect(inp))
            except V.Reject as r:
                seen.append((inp.name, r.criterion))
        assert seen, f"{mut} passes the acceptance on every family-{family} input of {case}"
        assert {c for _, c in seen} <= criteria, seen
        print(f"{mut} at {case}: rejected by {', '.join(f'{n} [{c}]' for n, c in seen)}")
    assert applied >= 4, f"{mut} applies at {applied} shapes only"


def test_ladders_move_the_rows_of_one_block_at_different_tiles():
    """Family L's premise on the 5-tile walk: in the first 16 rows of the last block some rows move their reference maximum at every tile, some at every
    second or third, some never after tile 0; the largest p of '+7.5' is about 2^7.5 and that of '+3' about 2^6; '+160' underflows the rescale factor
    to 0."""
    C, hw, frames = 128, 64, 5
    n = hw * frames
    moves = {}
    for variant in V.LADDERS:
        inp = V.Inputs("L", C, hw, frames, variant)
        q, k, _ = V._split16(inp.qkv, n, C, V.F32)
        s = (q @ k.t()) * V.scale_log2e(inp.scale)
        m, count, pmax, amin = torch.full((n,), -math.inf), torch.zeros(n, dtype=torch.int64), 0.0, 1.0
        for t0 in range(0, n, V.TILE):
            mt = s[:, t0 : t0 + V.TILE].amax(-1)
            move = mt > m + V.LAZY
            if t0:
                amin = min(amin, float(torch.exp2(m - torch.where(move, mt, m))[n - 16 :].min()))
            m = torch.where(move, mt, m)
            count += move
            pmax = max(pmax, float(torch.exp2(s[n - 16 :, t0 : t0 + V.TILE] - m[n - 16 :, None]).max()))
        moves[variant] = (sorted(set(count[n - 16 :].tolist())), pmax, amin)
    # moves per row with a = -1, 0.5, 1 (tile 0 counts): 8.5 per tile moves at every tile, 4.25 at every second; 7.5 at every second, 3.75 at every third
    # (tile 3 only); 3 at tile 3, 1.5 never; a descending ladder moves only the rows with a = -1
    assert moves["+8.5"][0] == [1, 3, 5] and moves["+7.5"][0] == [1, 2, 3] and moves["+3"][0] == [1, 2] and moves["-3"][0] == [1, 2], moves
    assert 2.0 ** 7 < moves["+7.5"][1] <= 2.0 ** 8 and 2.0 ** 5.5 < moves["+3"][1] <= 2.0 ** 6.5, moves  # 2^7.5 and 2^6, give or take the jitter
    assert moves["flat+160"][2] == 0.0 and 0.0 < moves["flat+40"][2] < 2.0 ** -39, moves


def test_ref64_agrees_with_a_softmax_restatement():
    for C, hw, frames in ((128, 5, 7), (128, 63, 3), (512, 33, 4)):
        inp = V.Inputs("R", C, hw, frames, 6.0)
        n = inp.n
        q, k, v = (t.half().double() for t in inp.qkv.split(C, dim=1))
        frame = torch.arange(n) // hw
        s = (q @ k.t()) * (float(V.scale_log2e(inp.scale)) * math.log(2.0))
        w = torch.where(frame[None, :] <= frame[:, None], s, torch.tensor(-math.inf, dtype=torch.float64)).softmax(-1)
        o, A = V.ref64(inp.qkv, n, C, hw, inp.scale)
        assert float((o - w @ v).abs().max()) <= 1e-12 and float((A - w @ v.abs()).abs().max()) <= 1e-12
        assert abs(float(V.scale_log2e(inp.scale)) * math.log(2.0) * math.sqrt(C) - 1) < 2.0 ** -22  # the base-2 factor is 1 / sqrt(C) to two fp32 roundings


def test_mutation_applies_states_the_shapes():
    table = {c: [m for m in V.MUTATIONS if V.mutation_applies(m, c[1] * c[2], c[1])] for c in V.CASES}
    assert table[(128, 64, 3)] == ["see_one_more", "hide_last_visible", "skip_o_rescale", "skip_l_rescale"]  # frames on tile edges: no padding, no spanning block
    assert table[(128, 129, 1)] == ["see_one_more", "hide_last_visible", "pad_keys_leak", "skip_o_rescale", "skip_l_rescale"]  # one frame: the key behind the limit is padding
    assert table[(128, 5, 7)] == ["see_one_more", "hide_last_visible", "block_first_row_limit", "pad_keys_leak"]  # one tile: nothing to rescale
    assert table[(512, 33, 4)] == list(V.MUTATIONS)
