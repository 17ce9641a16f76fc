"""Block-sparse self-attention (x2v_attn_bsr_fwd_bf16_vt, the list-driven form of attn_fwd_v9_kernel) against masked softmax in float64
(tests/radial_ref.py), through lib.attention_block_sparse, ops.HipRadialAttnWeight and the Wan driver with self_attn_1_type="hip_radial".

Acceptance is attn_ref.Case.check, constants from there: every element |got - o| <= 2^-7 |o| + 1.05 * 2^-8 * A with o, A from masked_ref64 (A the
softmax-weighted mean of |v| over the attended keys), and relL2 <= 1.5 * Y with Y from attn_ref.emulate on the attended keys of every block row.

Every call reads q / k as views of one fused buffer (token stride 3 * H * 128 + 64) whose k rows past S hold dominant keys, and writes a window of
a poisoned buffer whose surroundings are checked afterwards (the helpers of tests/test_gpu_attn_fp64.py)."""
import os

import pytest
import torch

from tests import attn_ref as A
from tests import radial_ref as RR
from tests.test_gpu_attn_fp64 import fused, head_major, poison_intact, views, window

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FIXTURES = RR.load_fixtures(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_masks.npz"))
CASE = A.Case("bsr v9")
S_ADV = 1536 + 40  # 13 block rows: seven query blocks, the last with one block row of 40 rows


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def launch(lib, buf, S, H, mask, pre, plan=None):
    """One sparse launch on the fused buffer; returns the [S, H * 128] output window (device)."""
    q, k, v = views(buf, S, S, H)
    vt = lib.transpose_heads(v, H)
    plan = plan or lib.attn_block_plan(mask, S, S)
    big, out = window(S, H * 128)
    got = lib.attention_block_sparse(q, k, vt, H, plan, prescaled=pre, out=out)
    assert got.data_ptr() == out.data_ptr() and poison_intact(big, S, H * 128), "wrote outside the output window"
    return out


def run(lib, inp, mask, pre, what, rows=None, exp_mask=None):
    form = "pre" if pre else "vt"
    buf, _ = fused(inp.q_for(form), inp.k, inp.v, inp.H)
    out = launch(lib, buf, inp.Sq, inp.H, mask, pre)
    exp = RR.expect(inp, form, mask if exp_mask is None else exp_mask)
    got = head_major(out, inp.H)
    if rows is not None:
        got, exp = got[:, rows], exp.rows(rows)
    rel, Y, worst = CASE.check(got, exp, what)
    print(f"{inp.name} {what} {form}: relL2 {rel:.3e}  Y {Y:.3e}  worst d/tol {worst:.3f}")
    return out


FAMILIES = (("R", "middle"), ("R", "first"), ("R", "last"), ("N", "none"))


def test_all_true_mask_is_dense_attention(lib):
    S, H = 1800, 2
    mask = torch.ones(RR.n_blocks(S), RR.n_blocks(S), dtype=torch.bool)
    for fam, spike in FAMILIES:
        inp = A.Inputs(fam, S, S, H, spike)
        for pre in (False, True):
            form = "pre" if pre else "vt"
            out = run(lib, inp, mask, pre, "all-true")
            buf, _ = fused(inp.q_for(form), inp.k, inp.v, H)
            q, k, v = views(buf, S, S, H)
            dense = lib.attention(q, k, v, H, variant=lib.ATTN_FAST | lib.ATTN_ONE_WALK | (lib.ATTN_Q_PRESCALED if pre else 0))
            tol = A.expect(inp, form).tol()
            d = (head_major(out, H).double() - head_major(dense, H).double()).abs()
            assert (d <= tol).all(), f"{inp.name} {form}: sparse on an all-true mask and the dense kernel differ by more than the bar ({float((d / tol).max()):.2f} x)"


@pytest.mark.parametrize("tpf,frames", [(200, 9), (260, 11), (96, 24), (384, 8)])
def test_fixture_masks(lib, tpf, frames):
    """S = 1800 (a last block of 8 rows), 2860 (23 block rows: the last query block holds one), 2304 (walks of one and two blocks), 3072 (no partial tile)."""
    S, H = tpf * frames, 2
    mask = RR.fixture_mask(FIXTURES, tpf, frames)
    for i, (fam, spike) in enumerate(FAMILIES):
        run(lib, A.Inputs(fam, S, S, H, spike), mask, pre=i % 2 == 0, what=f"radial {tpf}x{frames}")
    run(lib, A.Inputs("R", S, S, H, "middle"), mask, pre=False, what=f"radial {tpf}x{frames}")


def adversarial_mask():
    nb = RR.n_blocks(S_ADV)
    m = torch.zeros(nb, nb, dtype=torch.bool)
    m[0, [0, 3, 5]] = True  # rows 0 / 1 share exactly block 5
    m[1, [5, 8, 12]] = True
    m[2, 2] = True  # a single block beside a full row
    m[3, :] = True
    m[4, [4, 9]] = True  # the halves' first member tiles differ, either way round
    m[5, [1, 5]] = True
    m[6, [0, 6, 12]] = True
    m[7, [7, 12]] = True
    m[8:] = RR.random_mask(nb, 0.3, 77)[8:]
    return m


@pytest.mark.parametrize("which", ["hand-made", "density 0.3"])
def test_adversarial_masks(lib, which):
    mask = adversarial_mask() if which == "hand-made" else RR.random_mask(RR.n_blocks(S_ADV), 0.3, 5)
    for i, (fam, spike) in enumerate(FAMILIES):
        run(lib, A.Inputs(fam, S_ADV, S_ADV, 3, spike, seed=1), mask, pre=i % 2 == 1, what=which)


@pytest.mark.parametrize("row", [4, 5, 12])
def test_unlisted_blocks_do_not_leak(lib, row):
    """Every key block outside block row `row`'s list holds keys aligned to that row's queries (scores far above the attended ones) and |v| = 1e4;
    the row's output stays within the bar of the unpoisoned reference.  Rows 4 / 5: the two halves of a query block; row 12: the half-filled last one."""
    S, H = S_ADV, 2
    mask = RR.random_mask(RR.n_blocks(S), 0.3, 11)
    mask[row, 0] = False  # at least one unlisted block in front of the row's first member
    mask[row, row] = True
    inp = A.Inputs("R", S, S, H, "middle", seed=2)
    rows = torch.arange(row * 128, min((row + 1) * 128, S))
    poisoned = A.Inputs("R", S, S, H, "middle", seed=2)
    poisoned.seed = (2, "poison", row)
    poisoned.k, poisoned.v = inp.k.clone(), inp.v.clone()
    n_bad = 0
    for b in torch.nonzero(~mask[row]).flatten().tolist():
        keys = torch.arange(b * 128, min((b + 1) * 128, S))
        poisoned.k[:, keys] = 16 * inp.q[:, rows[keys % rows.numel()]]
        poisoned.v[:, keys] = 1.0e4 * (1 - 2 * (keys % 2)).to(BF16).view(1, -1, 1)
        n_bad += 1
    assert n_bad >= 2
    for pre in (False, True):
        form = "pre" if pre else "vt"
        buf, _ = fused(poisoned.q_for(form), poisoned.k, poisoned.v, H)
        got = head_major(launch(lib, buf, S, H, mask, pre), H)[:, rows]
        assert torch.isfinite(got).all()
        CASE.check(got, RR.expect(inp, form, mask).rows(rows), f"poison row {row}")


@pytest.mark.parametrize("S", [256 + 1, 384 + 31, 512 + 33])
def test_query_tails_strided_views_and_out(lib, S):
    """1, 31 and 33 rows past a block boundary; q / k strided views of the fused buffer and out= a strided window (launch() asserts both)."""
    mask = RR.random_mask(RR.n_blocks(S), 0.5, S)
    for i, (fam, spike) in enumerate(FAMILIES):
        inp = A.Inputs(fam, S, S, 3, spike)
        out = run(lib, inp, mask, pre=i % 2 == 0, what="tail")
        assert out.stride(0) == 3 * 128 + 4 and not out.is_contiguous()
    q, k, v = views(fused(inp.q, inp.k, inp.v, 3)[0], S, S, 3)
    assert q.stride(0) == k.stride(0) == 9 * 128 + 64
    fresh = lib.attention_block_sparse(q, k, lib.transpose_heads(v, 3), 3, lib.attn_block_plan(mask, S, S))  # out=None: a new contiguous tensor
    assert fresh.is_contiguous() and fresh.shape == (S, 3 * 128)
    CASE.check(head_major(fresh, 3), RR.expect(inp, "vt", mask), "out=None")


def test_bit_equal_launches_and_independent_block_rows(lib):
    S, H, row = S_ADV, 2, 5
    inp = A.Inputs("R", S, S, H, "middle", seed=3)
    buf, _ = fused(inp.q, inp.k, inp.v, H)
    m1 = RR.random_mask(RR.n_blocks(S), 0.3, 21)
    m2 = RR.random_mask(RR.n_blocks(S), 0.6, 22)
    m2[row] = m1[row]  # the same list for block row 5; its partner row 4 and every other row differ
    assert (m1[4] != m2[4]).any()
    a, b = launch(lib, buf, S, H, m1, False), launch(lib, buf, S, H, m1, False)
    assert torch.equal(a, b), "two launches on the same inputs differ"
    c = launch(lib, buf, S, H, m2, False)
    rows = slice(row * 128, (row + 1) * 128)
    assert torch.equal(a[rows], c[rows]), "a block row's result depends on the other rows' lists"
    assert not torch.equal(a[: 4 * 128], c[: 4 * 128])


def test_argument_errors_return_status_and_message(lib):
    S, H = 640, 2
    inp = A.Inputs("R", S, S, H)
    buf, _ = fused(inp.q, inp.k, inp.v, H)
    q, k, v = views(buf, S, S, H)
    vt = lib.transpose_heads(v, H)
    mask = torch.eye(5, dtype=torch.bool)
    plan = lib.attn_block_plan(mask, S, S)
    big, out = window(S, H * 128)
    tab = plan.device_table(q.device)

    def raw(q_, ldq, Sq, head_dim, plan_seq, plan_wgs):
        rc = lib._lib.x2v_attn_bsr_fwd_bf16_vt(q_.data_ptr(), ldq, k.data_ptr(), k.stride(0), vt.data_ptr(), vt.shape[1] * 64, out.data_ptr(), out.stride(0), Sq, Sq, H, head_dim, 0.0, 0,
                                               tab.data_ptr(), tab.numel(), plan_seq, plan_wgs, torch.cuda.current_stream().cuda_stream)
        return rc, lib._lib.x2v_last_error().decode()

    rc, msg = raw(q, q.stride(0), S, 64, S, plan.n_wgs)
    assert rc != 0 and "head_dim=64" in msg
    rc, msg = raw(q, q.stride(0), S - 128, 128, S, plan.n_wgs)  # the plan was built for another S
    assert rc != 0 and "plan was built for 640 rows" in msg
    rc, msg = raw(q, q.stride(0) + 4, S, 128, S, plan.n_wgs)  # rows not 16-byte aligned
    assert rc != 0 and "16-byte aligned" in msg
    other = lib.attn_block_plan(torch.eye(4, dtype=torch.bool), 512, 512)
    with pytest.raises(lib.X2VError, match="plan was built for 512 rows"):
        lib.attention_block_sparse(q, k, vt, H, other, out=out)
    with pytest.raises(lib.X2VError):
        lib.attention_block_sparse(q[:, : H * 64], k, vt, H, plan, out=out)
    torch.cuda.synchronize()
    assert poison_intact(big, S, H * 128) and (out == -1984.0).all(), "a refused call launched"
    assert raw(q, q.stride(0), S, 128, S, plan.n_wgs)[0] == 0


# ------------------------------------------------------------------------------------------------------------------- operator and driver
def test_operator_apply_on_a_radial_grid(lib):
    from lightx2v_amd import ops, radial

    tpf, frames, H = 200, 9, 2
    S = tpf * frames
    inp = A.Inputs("R", S, S, H, "middle", seed=4)
    q, k, v = (t.permute(1, 0, 2).contiguous().cuda() for t in (inp.q, inp.k, inp.v))  # [S, H, 128]
    mm = radial.MaskMap(S, frames)
    cu = torch.tensor([0, S], dtype=torch.int32)
    out = ops.HipRadialAttnWeight().apply(q, k, v, cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=S, max_seqlen_kv=S, mask_map=mm, model_cls="wan2.1")
    assert out.shape == (S, H * 128)
    mask = RR.fixture_mask(FIXTURES, tpf, frames)
    assert torch.equal(mm.queryLogMask(torch.empty(1920, 1), "radial", model_type="wan"), mask)
    CASE.check(head_major(out, H), RR.expect(inp, "vt", mask), "HipRadialAttnWeight.apply")
    with pytest.raises(lib.X2VError, match="mask_map"):
        ops.HipRadialAttnWeight().apply(q, k, v, max_seqlen_q=S)


def tiny_forward(target_shape, frames, sparse_fn=None, **overrides):
    from lightx2v_amd import lib as L
    from lightx2v_amd import scheduler, synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=3).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, target_shape)
    cfg = wan.default_config(dims, target_shape=target_shape, target_video_length=frames, infer_steps=3, **overrides)
    model = wan.WanModel(cfg, wd)
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    sch.step_pre(1)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    orig = L.attention_block_sparse
    if sparse_fn is not None:
        L.attention_block_sparse = sparse_fn
    try:
        return model._forward(inputs, True).float().cpu(), model
    finally:
        L.attention_block_sparse = orig


def torch_masked_attention(calls):
    """lib.attention_block_sparse's signature in fp32 torch on the GPU (prescaled q: P = 2^(q . k)); the token mask comes from the plan itself."""

    def fn(q, k, vt, num_heads, plan, prescaled=False, out=None, scale=0.0):
        assert prescaled
        S = q.shape[0]
        nb = RR.n_blocks(S)
        bm = torch.zeros(nb, nb, dtype=torch.bool)
        for qblk, ents in plan.records():
            for t, bits in ents:
                for half in (0, 1):
                    if bits >> half & 1:
                        bm[2 * qblk + half, t // 2] = True
        calls.append(bm)
        tok = bm.repeat_interleave(128, 0).repeat_interleave(128, 1)[:S, :S].cuda()
        qh = q.reshape(S, num_heads, 128).permute(1, 0, 2).float()
        kh = k.reshape(S, num_heads, 128).permute(1, 0, 2).float()
        vh = vt.permute(0, 1, 3, 2).reshape(num_heads, -1, 128)[:, :S].float()
        s = (qh @ kh.transpose(1, 2)).masked_fill(~tok, float("-inf"))
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        o = (p / p.sum(-1, keepdim=True)) @ vh
        return o.permute(1, 0, 2).reshape(S, num_heads * 128).to(BF16)

    return fn


def test_wan_driver_with_hip_radial_on_a_sparse_grid():
    """wan-tiny on a 9 x 10 x 20 token grid (200 tokens per frame, S = 1800: the (200, 9) fixture mask, density 0.769) against the same driver with
    the sparse launch replaced by masked attention in fp32 torch; the bound is tests/test_gpu_model.py's for a bf16 forward against its oracle (2e-2)."""
    from tests.util import assert_rel

    ts = (16, 9, 20, 40)
    got, model = tiny_forward(ts, 33, self_attn_1_type="hip_radial")
    calls = []
    ref, _ = tiny_forward(ts, 33, sparse_fn=torch_masked_attention(calls), self_attn_1_type="hip_radial")
    want = RR.fixture_mask(FIXTURES, 200, 9)
    assert len(calls) == 2 and all(torch.equal(c, want) for c in calls), "the driver's plan is not the (200, 9) radial mask"
    assert not want.all()
    assert model.transformer_infer.mask_map is not None and (model.transformer_infer.mask_map.video_token_num, model.transformer_infer.mask_map.num_frame) == (1800, 9)
    assert_rel(got, ref, 2e-2, "hip_radial forward vs fp32 masked attention")
    dense, _ = tiny_forward(ts, 33)
    assert not torch.equal(dense, got), "the radial forward is the dense forward"


def test_wan_driver_one_frame_grid_matches_hip_flash(lib):
    """One frame: the mask is all true, every self-attention output is within the pairwise bar of the dense kernel on the same operands."""
    from lightx2v_amd import lib as L

    seen = []
    orig = L.attention_block_sparse

    def spy(q, k, vt, num_heads, plan, prescaled=False, out=None, scale=0.0):
        o = orig(q, k, vt, num_heads, plan, prescaled=prescaled, out=out, scale=scale)
        dense = L.attention(q, k, None, num_heads, variant=L.ATTN_FAST | L.ATTN_Q_PRESCALED | L.ATTN_ONE_WALK, vt=vt)
        S = q.shape[0]
        assert plan.kept_blocks == RR.n_blocks(S) ** 2
        qh, kh = (head_major(t.contiguous(), num_heads) for t in (q, k))
        vh = vt.permute(0, 1, 3, 2).reshape(num_heads, -1, 128)[:, :S].cpu()
        o64, A64 = A.ref64(qh, kh, vh, prescaled=True)
        tol = A.ULP * o64.abs() + A.P_ROUND * A64
        seen.append(bool(((head_major(o, num_heads).double() - head_major(dense, num_heads).double()).abs() <= tol).all()))
        return o

    got, _ = tiny_forward((16, 1, 20, 40), 1, sparse_fn=spy, self_attn_1_type="hip_radial")
    flash, _ = tiny_forward((16, 1, 20, 40), 1)
    assert len(seen) == 2 and all(seen), "sparse and dense self-attention differ by more than the pairwise bar on an all-true mask"
    from tests.util import assert_rel

    assert_rel(got, flash, 2e-2, "one-frame hip_radial forward vs hip_flash forward")


def test_hip_radial_with_ulysses_raises():
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    cfg = wan.default_config(dims, target_shape=(16, 3, 8, 8), target_video_length=9, infer_steps=3, self_attn_1_type="hip_radial", parallel_attn_type="ulysses")
    with pytest.raises(NotImplementedError, match="hip_radial.*ulysses"):
        wan.WanModel(cfg, {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=3).items()})
