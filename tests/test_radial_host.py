"""Radial attention, host side (no GPU): the block mask of lightx2v_amd/radial.py against the fixtures the unmodified reference wrote
(tests/golden/radial_masks.npz, tools/gen_radial_golden.py) and, where the reference checkout is present, against a live run of it; the launch plan
of lib.attn_block_plan; and the float64 yardstick of tests/radial_ref.py that tests/test_gpu_attn_bsr.py measures the kernel with."""
import contextlib
import inspect
import io
import os

import numpy as np
import pytest
import torch

from lightx2v_amd import lib, ops, radial
from oracle import ref_import
from tests import attn_ref as R
from tests import radial_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_masks.npz")
FIXTURES = RR.load_fixtures(GOLDEN)
FIXTURE_IDS = [f"{m['tokens_per_frame']}x{m['frames']}-{m['model_type']}-d{m['decay_factor']}" for m, _ in FIXTURES]


class _Rows:
    def __init__(self, n):
        self.shape = (n,)


def our_mask(tpf, frames, model_type, decay):
    S = tpf * frames
    return radial.MaskMap(S, frames).queryLogMask(_Rows((S + 127) // 128 * 128), "radial", block_size=128, decay_factor=decay, model_type=model_type)


def test_fixture_file_is_the_issue_s_list_and_small():
    want = [(200, 9, "wan", 1), (260, 11, "wan", 1), (96, 24, "wan", 1), (70, 4, "wan", 1), (384, 8, "wan", 1), (150, 16, "wan", 1), (1560, 13, "wan", 1), (1560, 21, "wan", 1),
            (3600, 21, "wan", 1), (200, 9, "hunyuan", 1), (200, 9, "wan", 0.5)]
    assert [(m["tokens_per_frame"], m["frames"], m["model_type"], m["decay_factor"]) for m, _ in FIXTURES] == want
    assert os.path.getsize(GOLDEN) < (1 << 20)
    dens = {(m["tokens_per_frame"], m["frames"]): float(mask.float().mean()) for m, mask in FIXTURES if m["model_type"] == "wan" and m["decay_factor"] == 1}
    assert round(dens[(3600, 21)], 3) == 0.379 and round(dens[(1560, 21)], 3) == 0.433 and round(dens[(1560, 13)], 3) == 0.550 and round(dens[(96, 24)], 3) == 0.108


@pytest.mark.parametrize("k", range(len(FIXTURES)), ids=FIXTURE_IDS)
def test_mask_equals_the_reference_fixture_bit_for_bit(k):
    md, want = FIXTURES[k]
    got = our_mask(md["tokens_per_frame"], md["frames"], md["model_type"], md["decay_factor"])
    assert got.dtype == torch.bool and got.shape == want.shape
    diff = got != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.numel()} blocks differ, first at {torch.nonzero(diff)[0].tolist()}"


def test_mask_is_cached_rejects_other_block_sizes_and_types():
    mm = radial.MaskMap(1800, 9)
    a = mm.queryLogMask(_Rows(1920), "radial", decay_factor=1, model_type="wan")
    assert mm.log_mask is not None
    b = mm.queryLogMask(torch.empty(1920, 1), "radial", decay_factor=0.25, model_type="hunyuan")  # cached: later arguments are ignored, as in the reference
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        radial.MaskMap(1800, 9).queryLogMask(_Rows(1920), "radial", block_size=64, model_type="wan")
    with pytest.raises(ValueError):
        radial.MaskMap(1800, 9).queryLogMask(_Rows(1920), "radial", model_type="cogvideo")
    with pytest.raises(ValueError):
        radial.MaskMap(1800, 9).queryLogMask(_Rows(1920), "log", model_type="wan")


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference checkout not present")
def test_mask_and_signatures_against_the_live_reference():
    import importlib.util

    path = os.path.join(ref_import.REFERENCE_ROOT, "lightx2v", "attentions", "common", "radial_attn.py")
    spec = importlib.util.spec_from_file_location("reference_radial_attn_live", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for tpf, frames, model_type, decay in ((130, 7, "wan", 1), (45, 12, "hunyuan", 0.5), (300, 5, "wan", 0.5)):
        S = tpf * frames
        with contextlib.redirect_stdout(io.StringIO()):
            want = mod.MaskMap(S, frames).queryLogMask(torch.empty((S + 127) // 128 * 128, 1), "radial", block_size=128, decay_factor=decay, model_type=model_type)
        assert torch.equal(our_mask(tpf, frames, model_type, decay), want), (tpf, frames, model_type, decay)
    for name in ("__init__", "queryLogMask"):
        ref_sig, our_sig = inspect.signature(getattr(mod.MaskMap, name)), inspect.signature(getattr(radial.MaskMap, name))
        assert [(p.name, p.default) for p in ref_sig.parameters.values()] == [(p.name, p.default) for p in our_sig.parameters.values()], name
    ref_import.patch_and_import()
    from lightx2v.common.ops.attn.attn_weight import RadialAttnWeight

    ref_sig, our_sig = inspect.signature(RadialAttnWeight.apply), inspect.signature(ops.HipRadialAttnWeight.apply)
    assert [(p.name, p.default) for p in ref_sig.parameters.values()] == [(p.name, p.default) for p in our_sig.parameters.values()]


def test_operator_is_registered_and_needs_a_mask_map():
    from lightx2v_amd.registry import ATTN_WEIGHT_REGISTER

    assert ATTN_WEIGHT_REGISTER["hip_radial"] is ops.HipRadialAttnWeight
    assert list(inspect.signature(ops.HipRadialAttnWeight.apply).parameters) == ["self", "q", "k", "v", "cu_seqlens_q", "cu_seqlens_kv", "max_seqlen_q", "max_seqlen_kv", "mask_map",
                                                                               "sparsity_type", "block_size", "decay_factor", "model_cls"]
    q = torch.zeros(256, 1, 128, dtype=torch.bfloat16)
    with pytest.raises(lib.X2VError, match="mask_map"):
        ops.HipRadialAttnWeight().apply(q, q, q, max_seqlen_q=256)


# ------------------------------------------------------------------------------------------------------------------- plan
def plan_pairs(plan, S):
    """{(query block row, key block)} a plan attends, with every structural property checked on the way."""
    nb, ntile = (S + 127) // 128, (S + 63) // 64
    recs = plan.records()
    assert sorted(q for q, _ in recs) == list(range((nb + 1) // 2)), "every 256-row query block exactly once"
    work = [len(e) for _, e in recs]
    assert work == sorted(work, reverse=True), "heaviest walk first"
    seen = {}
    for qblk, ents in recs:
        tiles = [t for t, _ in ents]
        assert tiles == sorted(set(tiles)) and tiles and 0 <= tiles[0] and tiles[-1] < ntile, "tiles ascend, in range, none twice"
        if S % 64 and (ntile - 1) in tiles:
            assert tiles[-1] == ntile - 1, "the partial tile ends its record"
        for t, bits in ents:
            assert bits in (1, 2, 3)
            for half in (0, 1):
                if bits >> half & 1:
                    assert 2 * qblk + half < nb, "the absent half of the last query block attends nothing"
                    seen.setdefault((2 * qblk + half, t // 2), set()).add(t)
    for (r, b), tiles in seen.items():
        assert tiles == {t for t in (2 * b, 2 * b + 1) if t < ntile}, "a block is both of its tiles"
    return set(seen)


def mask_pairs(mask):
    return {(int(r), int(c)) for r, c in torch.nonzero(torch.as_tensor(np.asarray(mask)))}


@pytest.mark.parametrize("k", range(len(FIXTURES)), ids=FIXTURE_IDS)
def test_plan_attends_exactly_the_fixture_mask(k):
    md, mask = FIXTURES[k]
    S = md["tokens_per_frame"] * md["frames"]
    plan = lib.attn_block_plan(mask, S, S)
    assert plan_pairs(plan, S) == mask_pairs(mask)
    assert plan.kept_blocks == int(mask.sum()) and plan.seq_len == S


def test_plan_attends_exactly_random_masks_and_csr():
    for seed in range(20):
        S = (257, 640, 1000, 1536 + 40, 2304)[seed % 5] + seed
        nb = (S + 127) // 128
        mask = RR.random_mask(nb, (0.1, 0.3, 0.7)[seed % 3], seed, diagonal=seed % 2 == 0)
        plan = lib.attn_block_plan(mask, S, S)
        assert plan_pairs(plan, S) == mask_pairs(mask), seed
        indptr = torch.cat([torch.zeros(1, dtype=torch.int32), mask.sum(1).cumsum(0).to(torch.int32)])
        indices = torch.nonzero(mask)[:, 1].to(torch.int32)
        assert np.array_equal(lib.attn_block_plan((indptr, indices), S, S).table, plan.table), seed


def test_plan_rejections():
    S = 640
    ok = torch.eye(5, dtype=torch.bool)
    lib.attn_block_plan(ok, S, S)
    with pytest.raises(lib.X2VError, match="Sq"):
        lib.attn_block_plan(ok, S, S + 128)
    with pytest.raises(lib.X2VError, match="must be bool"):
        lib.attn_block_plan(torch.eye(4, dtype=torch.bool), S, S)
    with pytest.raises(lib.X2VError, match="must be bool"):
        lib.attn_block_plan(torch.ones(5, 6, dtype=torch.bool), S, S)
    empty = ok.clone()
    empty[3, 3] = False
    with pytest.raises(lib.X2VError, match="block row 3 attends no block"):
        lib.attn_block_plan(empty, S, S)
    indptr = [0, 1, 2, 3, 4, 6]
    lib.attn_block_plan((indptr, [0, 1, 2, 3, 0, 4]), S, S)
    with pytest.raises(lib.X2VError, match="out of range"):
        lib.attn_block_plan((indptr, [0, 1, 2, 3, 0, 5]), S, S)
    with pytest.raises(lib.X2VError, match="out of range"):
        lib.attn_block_plan((indptr, [0, 1, 2, 3, -1, 4]), S, S)
    with pytest.raises(lib.X2VError, match="ascend"):
        lib.attn_block_plan((indptr, [0, 1, 2, 3, 4, 0]), S, S)
    with pytest.raises(lib.X2VError, match="ascend"):
        lib.attn_block_plan((indptr, [0, 1, 2, 3, 4, 4]), S, S)
    with pytest.raises(lib.X2VError, match="indptr"):
        lib.attn_block_plan(([0, 1, 2, 3, 6], [0, 1, 2, 3, 0, 4]), S, S)
    with pytest.raises(lib.X2VError, match="attends no block"):
        lib.attn_block_plan(([0, 1, 2, 3, 3, 5], [0, 1, 2, 0, 4]), S, S)


# ------------------------------------------------------------------------------------------------------------------- the float64 yardstick
def test_masked_ref64_equals_ref64_on_an_all_true_mask_and_respects_the_mask():
    inp = R.Inputs("R", 300, 300, 2, spike="middle")
    full = torch.ones(3, 3, dtype=torch.bool)
    for form in ("vt", "pre"):
        q, kw = inp.q_for(form), R.form_args(form)
        o, A = RR.masked_ref64(q, inp.k, inp.v, full, **kw)
        o0, A0 = R.ref64(q, inp.k, inp.v, **kw)
        assert torch.equal(o, o0) and torch.equal(A, A0)
    mask = torch.tensor([[True, False, False], [True, True, False], [False, False, True]])
    o, _ = RR.masked_ref64(inp.q, inp.k, inp.v, mask, q_rounded=True)
    o_first, _ = R.ref64(inp.q[:, :128], inp.k[:, :128], inp.v[:, :128], q_rounded=True)
    o_last, _ = R.ref64(inp.q[:, 256:], inp.k[:, 256:], inp.v[:, 256:], q_rounded=True)
    assert torch.equal(o[:, :128], o_first) and torch.equal(o[:, 256:], o_last)
    exp = RR.MaskedExpect(inp, "vt", mask)
    assert 0 < exp.Y < 1e-2 and set(exp.y) == set(R.EMULATIONS)


PAD_SHAPES = ((200, 9), (260, 11), (96, 24), (384, 8))


def padded_key_deviation():
    """The reference's zero-key padding against ours (keys >= S excluded), in float64 on the GPU module's fixture shapes: relative L2 over all rows
    and the largest element difference in units of the element tolerance."""
    rows = []
    for tpf, frames in PAD_SHAPES:
        S = tpf * frames
        mask = RR.fixture_mask(FIXTURES, tpf, frames)
        inp = R.Inputs("R", S, S, 1, spike="middle")
        o, A = RR.masked_ref64(inp.q, inp.k, inp.v, mask, q_rounded=True)
        op, _ = RR.masked_ref64(inp.q, inp.k, inp.v, mask, q_rounded=True, pad_keys=True)
        tol = R.ULP * o.abs() + R.P_ROUND * A
        rows.append((S, (-S) % 128, R.rel_l2(op, o), float(((op - o).abs() / tol).max())))
    return rows


def test_padded_keys_reproduce_the_reference_wrapper_and_the_difference_is_recorded():
    inp = R.Inputs("R", 200, 200, 1)
    mask = torch.ones(2, 2, dtype=torch.bool)
    op, _ = RR.masked_ref64(inp.q, inp.k, inp.v, mask, q_rounded=True, pad_keys=True)
    z = torch.zeros(1, 56, 128, dtype=torch.bfloat16)
    o_ref, _ = R.ref64(inp.q, torch.cat([inp.k, z], 1), torch.cat([inp.v, z], 1), q_rounded=True)  # what the wrapper computes on its padded k / v
    assert torch.allclose(op, o_ref, rtol=1e-12, atol=1e-14)
    rows = padded_key_deviation()
    for S, pad, rel, worst in rows:
        print(f"padded-key deviation S={S} ({pad} zero keys): relL2 {rel:.3e}, worst element difference {worst:.2f} x the element tolerance")
    by_S = {S: (pad, rel) for S, pad, rel, _ in rows}
    assert by_S[3072] == (0, 0.0), "no padding when S is a multiple of 128: the two forms are the same"
    assert all(rel > 0 for S, (pad, rel) in by_S.items() if pad), "padding changes the rows that attend the last block"
