"""Block-scaled fp8 self-attention (x2v_attn_mx_*, lightx2v_amd/csrc/attn_mx.hip) against the restatement of tests/attn_mx_ref.py.

Every call reads q / k / v as views of one fused buffer (token stride 3 * H * 128 + 64) whose rows past Sk hold keys that dominate with v = 1e4, and
writes a window of a poisoned buffer whose surroundings are checked (the helpers of tests/test_gpu_attn_fp64.py); the result and every operand
buffer must equal, bit for bit, the same call on a buffer whose extra rows are zero.

Checks per case (H = 2; Sk = 1, 31, 32, 33, 127, 128, 129, 200, 296, 1576 with Sq = Sk and the plain q; Sq = 1, 33, 255, 256, 257 against Sk = 200
and 1576 with a prescaled q; families R with every spike position, N, H, U, sea, offset):
  * kmean within Sk * 2^-24 * mean|k| of the float64 mean (recursive fp32 summation of n terms is within (n - 1) u sum|x|, the division adds one u);
  * given the kernel's own kmean, the q, k and V^T codes and scale bytes equal the restatement's bit for bit, padding included;
  * element bound against exact float64 softmax over the dequantised DEVICE operands: |got - o| <= 2^-7 |o| + 1.05 * 2^-4 * A + F;
  * relL2 <= 1.5 * Y, Y the error of the restatement's emulation (P^ rounding emulated) on the same operands;
  * distance from exact attention on the bf16 inputs: relL2(GPU) <= 1.5 * relL2(restatement from the bf16 inputs); both figures and the dense v9
    kernel's go to the table (X2V_ATTN_MX_PARITY_TABLE names the file; profiles/attn_mx_parity.txt is one run's).

The element bound.  With w_j = P_j / l the exact weights (P_j = 2^(s_j - max s), l = sum P_j >= 1) the kernel forms sum_j P^_j v^_j / l' where P^_j is
P_j (relative to the running max of its tile, >= the final one, and scaled down afterwards in fp32) rounded to e4m3 after the 2^8 shift and l'
is the fp32 sum of the unrounded P.  A P whose code is normal (P * 2^8 >= 2^-6, i.e. P >= 2^-14) moves by at most its half-ulp, 2^-4 P: the sum of
those terms is within 2^-4 * A of exact, A = sum_j w_j |v^_jd|.  Below 2^-14 the codes are subnormal with spacing 2^-9 * 2^-8 = 2^-17 — the smallest
positive code stated in x2v.h — so such a P moves by at most 2^-18 absolutely (a P below 2^-18 is flushed to 0, which is that same bound); a key
that was normal when it was rounded but ends below 2^-14 after later rescales moved by at most 2^-4 * 2^-14 = 2^-18 too.  Those keys add
F_d = 2^-18 / l * sum_{j: P_j < 2^-14} |v^_jd|.  2^-7 |o| covers the final bf16 rounding and the fp32 effects on l and the scores; 1.05 is the
margin the d64 / d80 / d128 attention tests use on their P term."""
import os

import numpy as np
import pytest
import torch

from tests import attn_mx_ref as M
from tests import attn_ref as A
from tests.test_gpu_attn_fp64 import fused, head_major, poison_intact, views, window

pytestmark = pytest.mark.gpu
H = M.H_TEST
ROWS = []  # (case name, form, relL2 GPU, relL2 restatement, relL2 dense v9) against exact attention on the bf16 inputs
DRIVER = []  # further lines of the table: the smoothing comparison and the driver's figures


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_ATTN_MX_PARITY_TABLE")
    if not path:
        return
    try:
        with open(path, "w") as f:
            f.write("# relL2 against exact float64 attention on the bf16 inputs: hip_mxfp8 on the GPU | the restatement (tests/attn_mx_ref.py) | the dense v9 kernel\n")
            fams = sorted({r[0].split(" ", 1)[0] for r in ROWS})
            for fam in fams:
                rs = [r for r in ROWS if r[0].split(" ", 1)[0] == fam]
                f.write(f"# family {fam:<9} n={len(rs):<3} largest mx {max(r[2] for r in rs):.4e}  restatement {max(r[3] for r in rs):.4e}  dense {max(r[4] for r in rs):.4e}  "
                        f"largest mx / restatement {max((r[2] / r[3] if r[3] > 0 else 0.0) for r in rs):.3f}\n")
            for name, form, g, r, d in ROWS:
                f.write(f"{name:<34} {form:<18} mx {g:.4e}  restatement {r:.4e}  dense {d:.4e}\n")
            for line in DRIVER:
                f.write(line + "\n")
    except OSError:
        pass


def run(lib, inp, prescaled, smooth=True):
    """attention_mx_prepare + attention_mx on the dominant and on the zero-extended buffer: (out [Sq, H*128], operands) of the first, equal to the second."""
    q = A.prescale_q(inp.q) if prescaled else inp.q
    res = []
    for buf in fused(q, inp.k, inp.v, H):
        qv, kv, vv = views(buf, inp.Sq, inp.Sk, H)
        ops = lib.attention_mx_prepare(qv, kv, vv, H, prescaled=prescaled, smooth_k=smooth)
        big, out = window(inp.Sq, H * 128)
        assert lib.attention_mx(qv, kv, vv, H, out=out, prepared=ops) is out
        assert poison_intact(big, inp.Sq, H * 128), "wrote outside the output window"
        res.append((out, ops))
    (o0, p0), (o1, p1) = res
    assert torch.equal(o0, o1), "rows of k / v past Sk reached the result"
    for name in ("q_codes", "q_scales", "k_codes", "k_scales", "vt_codes", "vt_scales"):
        assert torch.equal(getattr(p0, name), getattr(p1, name)), f"rows past Sk reached {name}"
    return o0, p0


def check(lib, inp, prescaled, record=True):
    out, ops = run(lib, inp, prescaled)
    tag = f"{inp.name} {'prescaled' if prescaled else 'plain'}"
    q = A.prescale_q(inp.q) if prescaled else inp.q
    # ---- kmean
    k64 = inp.k.to(torch.float64)
    km = ops.kmean.cpu().numpy().reshape(H, 128)
    bound = inp.Sk * 2.0 ** -24 * k64.abs().mean(1).numpy()
    assert np.all(np.abs(km.astype(np.float64) - k64.mean(1).numpy()) <= bound), f"{tag}: kmean outside the fp32 summation bound"
    # ---- quantiser bits, given the kernel's own kmean
    r = M.restated(inp, prescaled)
    if not np.array_equal(r.kmean, km):
        r = M.Restated(q, inp.k, inp.v, prescaled, True, kmean=km)
    dev = {n: getattr(ops, n).cpu().numpy() for n in ("q_codes", "q_scales", "k_codes", "k_scales", "vt_codes", "vt_scales")}
    for n, want in (("q_scales", r.q_scales), ("q_codes", r.q_codes), ("k_scales", r.k_scales), ("k_codes", r.k_codes), ("vt_scales", r.vt_scales), ("vt_codes", r.vt_codes)):
        assert dev[n].shape == want.shape, f"{tag}: {n} shape {dev[n].shape} vs {want.shape}"
        assert np.array_equal(dev[n], want), f"{tag}: {n}: {int((dev[n] != want).sum())} of {want.size} bytes differ from the restatement"
    assert dev["vt_scales"].max() < 0xFF
    # ---- kernel against exact float64 attention over the dequantised DEVICE operands
    qd, kd, vd = M.deq_qk(dev["q_codes"], dev["q_scales"], inp.Sq), M.deq_qk(dev["k_codes"], dev["k_scales"], inp.Sk), M.deq_vt(dev["vt_codes"], dev["vt_scales"], inp.Sk)
    o, Aw, F = M.exact(qd, kd, vd)
    got = head_major(out, H)
    assert torch.isfinite(got.float()).all(), f"{tag}: non-finite output"
    err, tol = (got.to(torch.float64) - o).abs(), M.tol(o, Aw, F)
    worst = float((err / tol.clamp_min(1e-300)).max())
    Y = r.Y  # the emulation ran on these very operands: the device buffers equal the restatement's (asserted above)
    rel = A.rel_l2(got, o)
    print(f"attn_mx {tag}: relL2 {rel:.4e} Y {Y:.4e} worst d/tol {worst:.3f}")
    assert bool((err <= tol).all()), f"{tag}: {int((err > tol).sum())} of {err.numel()} elements outside 2^-7|o| + 1.05*2^-4*A + F; worst d/tol {worst:.3f}"
    assert rel <= M.TRIANGLE * Y, f"{tag}: relL2 {rel:.4e} > 1.5 * Y, Y = {Y:.4e}"
    # ---- distance from exact attention on the bf16 inputs: GPU, restatement (its own kmean), dense v9
    ex = A.ref64(q, inp.k, inp.v, prescaled=prescaled)[0]
    rs = M.restated(inp, prescaled)
    g_rel, r_rel = A.rel_l2(got, ex), A.rel_l2(rs.emulated, ex)
    bufs = fused(q, inp.k, inp.v, H)
    qv, kv, vv = views(bufs[0], inp.Sq, inp.Sk, H)
    dense = lib.attention(qv, kv, vv, H, variant=lib.ATTN_FAST | lib.ATTN_ONE_WALK | (lib.ATTN_Q_PRESCALED if prescaled else 0))
    d_rel = A.rel_l2(head_major(dense, H), ex)
    if record:
        ROWS.append((inp.name, "prescaled" if prescaled else "plain", g_rel, r_rel, d_rel))
    assert g_rel <= M.TRIANGLE * r_rel, f"{tag}: relL2 against exact attention on the bf16 inputs {g_rel:.4e} > 1.5 * the restatement's {r_rel:.4e}"
    return g_rel


@pytest.mark.parametrize("Sk", M.SK_SWEEP)
def test_sk_sweep(lib, Sk):
    """One tile with left = 1, 31, 32, 33, 127, 128; a masked second and third tile; 13 tiles (the sea holds most of the weight at 1576)."""
    for fam, spike in M.families():
        check(lib, M.MxInputs(fam, Sk, Sk, H, spike), prescaled=False)


@pytest.mark.parametrize("Sk", M.RECT_SK)
@pytest.mark.parametrize("Sq", M.RECT_SQ)
def test_rectangular(lib, Sq, Sk):
    """Sq != Sk: the 16-row group, the 32-row wave and the 256-row block tails, with a q that carries its scale."""
    for fam, spike in M.families():
        check(lib, M.MxInputs(fam, Sq, Sk, H, spike), prescaled=True)


@pytest.mark.parametrize("Sk", (200, 1576))
def test_smoothing_is_not_worse_on_the_offset_family(lib, Sk):
    inp = M.MxInputs("offset", 257, Sk, H)
    ex = A.ref64(inp.q, inp.k, inp.v)[0]
    on, _ = run(lib, inp, False, smooth=True)
    off, ops = run(lib, inp, False, smooth=False)
    assert ops.kmean is None
    e_on, e_off = A.rel_l2(head_major(on, H), ex), A.rel_l2(head_major(off, H), ex)
    DRIVER.append(f"{inp.name}: relL2 against exact attention on the bf16 inputs with smooth_k on {e_on:.4e} | off {e_off:.4e}")
    print(f"attn_mx offset Sk={Sk}: smoothing on {e_on:.4e} off {e_off:.4e}")
    assert e_on <= M.TRIANGLE * e_off
    # without smoothing the k operand is the restatement's without it, bit for bit
    r = M.restated(inp, False, smooth_k=False)
    assert np.array_equal(ops.k_codes.cpu().numpy(), r.k_codes) and np.array_equal(ops.k_scales.cpu().numpy(), r.k_scales)


def test_one_call_form_strides_and_empty_query(lib):
    inp = M.MxInputs("R", 257, 200, H, "middle")
    buf, _ = fused(inp.q, inp.k, inp.v, H)
    qv, kv, vv = views(buf, inp.Sq, inp.Sk, H)
    ops = lib.attention_mx_prepare(qv, kv, vv, H)
    a = lib.attention_mx(qv, kv, vv, H)
    assert torch.equal(a, lib.attention_mx(None, None, None, H, prepared=ops)) and torch.equal(a, lib.attention_mx(qv.contiguous(), kv.contiguous(), vv.contiguous(), H))
    assert lib.attention_mx(qv[:0], kv, vv, H).shape == (0, H * 128)  # Sq = 0: a no-op
    with pytest.raises(lib.X2VError, match="no keys"):
        lib.attention_mx(qv, kv[:0], vv[:0], H)
    with pytest.raises(lib.X2VError):
        lib.attention_mx(qv, kv, vv, H + 1)
    with pytest.raises(lib.X2VError):
        lib.attention_mx(qv, kv, vv, H, prepared=lib.attention_mx_prepare(qv, kv, vv, 1))


def test_operator_apply_equals_the_library_call(lib):
    from lightx2v_amd import ops

    inp = M.MxInputs("R", 300, 300, H, "last", seed=2)
    q, k, v = (t.permute(1, 0, 2).contiguous().cuda() for t in (inp.q, inp.k, inp.v))  # [S, H, 128]
    cu = torch.tensor([0, 300], dtype=torch.int32)
    out = ops.HipMxfp8AttnWeight().apply(q, k, v, cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=300, max_seqlen_kv=300, model_cls="wan2.1")
    assert out.shape == (300, H * 128)
    assert torch.equal(out, lib.attention_mx(q.reshape(300, -1), k.reshape(300, -1), v.reshape(300, -1), H))
    assert torch.equal(out, ops.hip_mxfp8(q, k, v))
    with pytest.raises(lib.X2VError, match="one sequence"):
        ops.HipMxfp8AttnWeight().apply(q, k, v, cu_seqlens_q=torch.tensor([0, 100, 300], dtype=torch.int32), max_seqlen_q=300)
    with pytest.raises(lib.X2VError):
        ops.HipMxfp8AttnWeight().apply(q[:, :, :64], k[:, :, :64], v[:, :, :64])


# ------------------------------------------------------------------------------------------------------------------- driver
def tiny_model(**overrides):
    from lightx2v_amd import scheduler, synth, wan

    dims, wl = synth.WAN_DIMS["wan-tiny"], synth.WORKLOADS["wan-tiny"]
    wd = synth.synth_wan_weights(dims, seed=0)
    lat, ctx, ctx_null = synth.synth_inputs(dims, wl["target_shape"])
    cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=4, **overrides)
    model = wan.WanModel(cfg, {k: v.cuda() for k, v in wd.items()})
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    sch.timesteps[2] = 888
    model.set_scheduler(sch)
    sch.step_pre(2)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    return model, inputs, (wd, dims, lat, ctx)


def test_wan_driver_forward_against_the_oracle_with_restated_attention(lib):
    """wan-tiny with "self_attn_1_type": "hip_mxfp8": the forward's deviation from the oracle whose self-attention is the restatement (assigned here;
    cross-attention keeps the oracle's) is at most 1.5 x what that replacement alone moves the oracle's forward on the CPU."""
    from oracle import wan_oracle as O
    from tests.util import rel_l2

    model, inputs, (wd, dims, lat, ctx) = tiny_model(self_attn_1_type="hip_mxfp8")
    assert model.transformer_infer.mx_attn
    calls = []
    orig_mx = lib.attention_mx
    lib.attention_mx = lambda *a, **kw: (calls.append(1), orig_mx(*a, **kw))[1]
    try:
        got = model._forward(inputs, True).float().cpu()
    finally:
        lib.attention_mx = orig_mx
    assert len(calls) == dims["num_layers"], "the block driver did not take the hip_mxfp8 path once per block"
    t = torch.tensor(888)
    plain = O.wan_forward(wd, dims, lat.to(torch.bfloat16), t, ctx).float()
    orig = O.sdpa

    def sdpa_mx(q, k, v):
        if q.shape[0] != k.shape[0]:
            return orig(q, k, v)  # cross-attention stays bf16
        r = M.Restated(*(x.permute(1, 0, 2).contiguous().to(torch.bfloat16) for x in (q, k, v)))
        return r.emulated.permute(1, 0, 2).reshape(q.shape[0], -1).to(q.dtype)

    O.sdpa = sdpa_mx
    try:
        restated = O.wan_forward(wd, dims, lat.to(torch.bfloat16), t, ctx).float()
    finally:
        O.sdpa = orig
    moved, dev, from_plain = rel_l2(restated, plain), rel_l2(got, restated), rel_l2(got, plain)
    dense_model, dense_inputs, _ = tiny_model()
    dense = rel_l2(dense_model._forward(dense_inputs, True).float().cpu(), plain)
    DRIVER.append(f"wan-tiny forward: oracle with restated attention vs plain oracle {moved:.4e} | hip_mxfp8 forward vs oracle with restated attention {dev:.4e} | "
                  f"hip_mxfp8 forward vs plain oracle {from_plain:.4e} | hip_flash forward vs plain oracle {dense:.4e}")
    print(DRIVER[-1])
    assert torch.isfinite(got).all()
    assert dev <= M.TRIANGLE * moved, f"hip_mxfp8 forward is {dev:.4e} from the oracle with restated attention; the replacement alone moves the oracle by {moved:.4e}"


def test_refusals():
    from lightx2v_amd import synth, wan

    dims = synth.WAN_DIMS["wan-tiny"]
    cfg = wan.default_config(dims, target_shape=(16, 3, 8, 8), target_video_length=9, infer_steps=3, self_attn_1_type="hip_mxfp8", parallel_attn_type="ulysses")
    with pytest.raises(NotImplementedError, match="hip_mxfp8.*ulysses"):
        wan.WanModel(cfg, {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=3).items()})
    model, inputs, _ = tiny_model(self_attn_1_type="hip_mxfp8", cfg_pair=True)
    assert not model._pair_ok(inputs), "CFG runs two forwards with hip_mxfp8"
    tr = model.transformer_infer
    tr._pair = (48, 64)
    with pytest.raises(NotImplementedError, match="hip_mxfp8.*pair"):
        model._forward(inputs, True)
    tr._pair = None
    tr.radial = True
    with pytest.raises(NotImplementedError, match="hip_mxfp8.*radial"):
        model._forward(inputs, True)
    tr.radial = False
    tr.parallel_attention = lambda **kw: None
    with pytest.raises(NotImplementedError, match="hip_mxfp8.*Ulysses"):
        model._forward(inputs, True)
