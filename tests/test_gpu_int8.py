"""The w8a8 int8 operator on the GPU against tests/int8_restatement.py (which tests/test_int8_host.py pins to the reference class's fixture).

What must be EQUAL, and why: the quantiser is a chain of single correctly rounded fp32 operations on exactly representable inputs; the GEMM's
integer sum is exact, its conversion to fp32 one rounding, and with no bias and no activation the epilogue is two fp32 multiplications and one bf16
rounding — nothing a compiler may contract.  With a bias or an activation an FMA contraction may move one rounding: those cases take the project's
fp8 criterion (tests/test_gpu_ops.py::test_fp8_path_vs_oracle): assert_bf16_close(ulps=1, atol=4e-3, bad_frac=2e-3).

Both kernels run every GEMM case: the 128x128 one (variant 1) and the continuous 256x256 one (variant 5, gemm256c8.hip's int8 form), each at its own shape."""
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from tests import int8_restatement as R
from tests.util import assert_bf16_close

pytestmark = pytest.mark.gpu

KEY = "W-int8-channel-sym-A-int8-channel-sym-dynamic-Hip"
CRIT = dict(ulps=1, atol=4e-3, bad_frac=2e-3)
ZERO_ROW, OUTLIER_ROW, TIE_ROW = 3, 5, 7  # tools/gen_golden_int8.py


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


@pytest.fixture(scope="module")
def fx():
    return load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "int8_mm.safetensors"))


def _codes(shape, seed):
    return torch.randint(-128, 128, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int8)


def _bits_equal(got, want, name):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, name
    n = (got.view(torch.int16) != want.view(torch.int16)).sum().item() if got.dtype == torch.bfloat16 else (got != want).sum().item()
    print(f"{name}: {n} of {got.numel()} differ")
    assert n == 0, f"{name}: {n} of {got.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("K", [128, 2048, 5120, 13824])  # CH = 1, 1 (full), 3 (half-filled last chunk), 8 (7 chunks used)
def test_quantiser_equals_the_restatement(lib, fx, K):
    x = torch.randn(5, K, generator=torch.Generator().manual_seed(K)).to(torch.bfloat16) * 3
    x[1] = 0
    x[2, K // 2] = 900.0
    n = min(K, fx["x"].shape[1])
    x[3, :n], x[3, n:] = fx["x"][TIE_ROW, :n], 0  # the tie row: amax 127 (K = 128: 63.5), entries at x.5
    x[4, :n] = fx["x"][OUTLIER_ROW, :n]
    pad = torch.full((5, K + 16), 7.0, dtype=torch.bfloat16)  # rows strided inside a wider buffer
    pad[:, :K] = x
    want_q, want_s = R.quant_act(x)
    for name, xin in (("contiguous", x.cuda()), ("strided", pad.cuda()[:, :K])):
        q, s = lib.quant_int8_rowwise(xin)
        assert q.dtype == torch.int8 and s.dtype == torch.float32 and tuple(s.shape) == (5, 1)
        _bits_equal(s, want_s, f"K={K} {name} scales")
        _bits_equal(q, want_q, f"K={K} {name} codes")
    assert not q[1].any() and s[1].item() == 0.0
    for nb in (2, 4):  # the K-blocked form [B, M, K/B] reads the same row
        xb = x.cuda().reshape(5, nb, K // nb).permute(1, 0, 2).contiguous()
        qb, sb = lib.quant_int8_rowwise(xb)
        _bits_equal(qb, want_q, f"K={K} {nb} K-blocks codes")
        _bits_equal(sb, want_s, f"K={K} {nb} K-blocks scales")


def test_quantiser_on_the_fixture_rows(lib, fx):
    q, s = lib.quant_int8_rowwise(fx["x"].cuda())
    _bits_equal(q, fx["xq"], "fixture codes")
    _bits_equal(s, fx["sx"], "fixture scales")
    assert q[TIE_ROW, :6].tolist() == [0, 2, 2, 4, 4, 6]


@pytest.mark.parametrize("D", [520, 1536, 5120])
def test_layernorm_quant_is_the_two_kernels_in_sequence(lib, D):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(5, D, generator=g) * 2 + 0.3).to(torch.bfloat16).cuda()
    x[2] = 1.5  # a constant row: variance 0
    w, b, sc, sh = ((torch.randn(D, generator=g) * 0.5).to(torch.bfloat16).cuda() for _ in range(4))
    for name, kw in (("plain", {}), ("affine", dict(weight=w, bias=b)), ("modulate", dict(scale=sc, shift=sh)), ("both", dict(weight=w, bias=b, scale=sc, shift=sh))):
        q, s = lib.layernorm_quant_int8(x, **kw)
        q2, s2 = lib.quant_int8_rowwise(lib.layernorm(x, kw.get("weight"), kw.get("bias"), scale=kw.get("scale"), shift=kw.get("shift")))
        _bits_equal(q, q2, f"D={D} {name} codes")
        _bits_equal(s, s2, f"D={D} {name} scales")
        assert q.dtype == torch.int8 and q.abs().max().item() >= 100


# ------------------------------------------------------------------------------------------------ GEMM
KERNELS = pytest.mark.parametrize("variant", [1, 5], ids=["128x128", "continuous256"])


@KERNELS
def test_exact_integer_map(lib, variant):
    """One-hot weight rows: y[m, n] = x[m, k(n)] * c(n) exactly (|value| <= 256 is a bf16 number) — a wrong (lane, byte) -> k map, a row / column
    swap or an M / N tail error cannot hide."""
    M, N, K = (130, 136, 256) if variant == 1 else (300, 256, 512)
    xq = _codes((M, K), 1)
    xq[0, :4] = torch.tensor([-128, 127, -1, 0], dtype=torch.int8)
    kn = (37 * torch.arange(N) + 11) % K
    c = torch.tensor([1, -1, 2, -2], dtype=torch.int8)[torch.arange(N) % 4]
    wq = torch.zeros(N, K, dtype=torch.int8)
    wq[torch.arange(N), kn] = c
    prod = xq[:, kn].to(torch.int32) * c.to(torch.int32)  # in integers: 0 * -1 is 0, not the -0.0 a float product would give
    want = prod.to(torch.bfloat16)
    assert torch.equal(want.to(torch.int32), prod)  # representable
    got = lib.gemm_int8(xq.cuda(), torch.ones(M, 1, device="cuda"), wq.cuda(), torch.ones(N, 1, device="cuda"), variant=variant)
    _bits_equal(got, want, f"one-hot map, variant {variant}")


@KERNELS
@pytest.mark.parametrize("code", [127, -128])
def test_conversion_edge_beyond_2_pow_24(lib, code, variant):
    """|acc| = K * code^2 = 33 032 192 / 2^25 at K = 2048: beyond the fp32 integers' exact range, so the int32 -> fp32 conversion rounds."""
    M, N, K = (64, 64, 2048) if variant == 1 else (256, 256, 2048)
    xq, wq = torch.full((M, K), code, dtype=torch.int8), torch.full((N, K), code, dtype=torch.int8)
    sx = torch.tensor([2.0 ** -(10 + m % 3) for m in range(M)]).reshape(M, 1)
    sw = torch.tensor([2.0 ** -(9 + n % 5) for n in range(N)]).reshape(N, 1)
    assert K * code * code > 2**24
    want = R.gemm(xq, sx, wq, sw)
    got = lib.gemm_int8(xq.cuda(), sx.cuda(), wq.cuda(), sw.cuda(), variant=variant)
    _bits_equal(got, want, f"all-{code} x all-{code}, variant {variant}")


SHAPES = {1: (130, 136, 384, 40), 5: (300, 512, 1024, 256)}  # (M, N, K, residual row period: the continuous kernel wants a multiple of 8 that is >= 256)
_DATA = {}


def _data(variant):
    """Full-range codes, random positive scales, bias, residual and gate at the variant's shape; every restated result computed once."""
    if variant not in _DATA:
        M, N, K, P = SHAPES[variant]
        g = torch.Generator().manual_seed(11 + variant)
        t = dict(xq=_codes((M, K), 2), wq=_codes((N, K), 3), sx=torch.rand(M, 1, generator=g) * 0.02 + 1e-3, sw=torch.rand(N, 1, generator=g) * 0.004 + 1e-4,
                 b=(torch.randn(N, generator=g) * 0.5).to(torch.bfloat16), resid=torch.randn(M, N, generator=g).to(torch.bfloat16),
                 gate=torch.randn(N, generator=g).to(torch.bfloat16), rp=torch.randn(P, N, generator=g).to(torch.bfloat16))
        a = (t["xq"], t["sx"], t["wq"], t["sw"])
        ref = dict(plain=R.gemm(*a), bias=R.gemm(*a, t["b"]), gelu=R.gemm(*a, t["b"], R.EPI_GELU_TANH), silu=R.gemm(*a, t["b"], R.EPI_SILU),
                   resid_gate=R.gemm(*a, t["b"], R.EPI_RESIDUAL, resid=t["resid"], gate=t["gate"]), resid=R.gemm(*a, t["b"], R.EPI_RESIDUAL, resid=t["resid"]),
                   resid_nobias=R.gemm(*a, None, R.EPI_RESIDUAL, resid=t["resid"]),
                   resid_period=R.gemm(*a, t["b"], R.EPI_RESIDUAL, resid=t["rp"], gate=t["gate"], resid_period=P))
        _DATA[variant] = ({k: v.cuda() for k, v in t.items()}, ref, P)
    return _DATA[variant]


def _run(lib, d, P, case, variant):
    a = (d["xq"], d["sx"], d["wq"], d["sw"])
    if case == "plain":
        return lib.gemm_int8(*a, variant=variant)
    if case == "bias":
        return lib.gemm_int8(*a, d["b"], variant=variant)
    if case in ("gelu", "silu"):
        return lib.gemm_int8(*a, d["b"], epilogue=lib.EPI_GELU_TANH if case == "gelu" else lib.EPI_SILU, variant=variant)
    if case == "resid_period":
        return lib.gemm_int8(*a, d["b"], epilogue=lib.EPI_RESIDUAL, resid=d["rp"], gate=d["gate"], resid_period=P, variant=variant)
    r = d["resid"].clone()
    lib.gemm_int8(*a, None if case == "resid_nobias" else d["b"], epilogue=lib.EPI_RESIDUAL, resid=r, gate=d["gate"] if case == "resid_gate" else None, variant=variant)
    return r


CASES = ("plain", "bias", "gelu", "silu", "resid_gate", "resid", "resid_nobias", "resid_period")


@KERNELS
@pytest.mark.parametrize("case", CASES)
def test_random_data_vs_restatement(lib, case, variant):
    d, ref, P = _data(variant)
    got = _run(lib, d, P, case, variant)
    if case == "plain":
        _bits_equal(got, ref[case], f"EPI_NONE, no bias, variant {variant}")
    else:
        assert_bf16_close(got, ref[case], name=f"{case}, variant {variant}", **CRIT)


@pytest.mark.parametrize("case", CASES)
def test_the_two_kernels_give_the_same_bits(lib, case):
    """Same exact integer sum, same conversion, same epilogue statements: variant 5 == variant 1 at (300, 512, 1024), every epilogue."""
    d, _, P = _data(5)
    _bits_equal(_run(lib, d, P, case, 5), _run(lib, d, P, case, 1), f"variant 5 vs variant 1, {case}")


def test_variant_0_is_the_reported_kernel_and_the_others_are_refused(lib):
    d, _, P = _data(1)
    M, K = d["xq"].shape
    N = d["wq"].shape[0]
    assert lib.gemm_int8_kernel_choice(M, N, K, with_form=True) == (1, False)
    assert torch.equal(_run(lib, d, P, "bias", 0), _run(lib, d, P, "bias", 1))
    for v in (2, 3, 4, 5):  # no such kernels; 5: N % 256 != 0 and an odd number of K tiles
        with pytest.raises(lib.X2VError):
            lib.gemm_int8(d["xq"], d["sx"], d["wq"], d["sw"], variant=v)
    # a shape variant 0 gives to the continuous kernel (choose_kernel's rule: >= 192 tiles of 256 x 256, >= 8 K tiles); the last m-tile has 44 rows
    M, N, K = 192 * 256 - 212, 256, 1024
    assert lib.gemm_int8_kernel_choice(M, N, K, with_form=True) == (2, True)
    g = torch.Generator().manual_seed(4)
    xq, wq = _codes((M, K), 8).cuda(), _codes((N, K), 9).cuda()
    sx, sw = (torch.rand(M, 1, generator=g) * 0.01 + 1e-3).cuda(), (torch.rand(N, 1, generator=g) * 0.01 + 1e-3).cuda()
    b = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
    auto = lib.gemm_int8(xq, sx, wq, sw, b)
    assert torch.equal(auto, lib.gemm_int8(xq, sx, wq, sw, b, variant=5)), "variant 0 vs the reported kernel"
    assert torch.equal(auto, lib.gemm_int8(xq, sx, wq, sw, b, variant=1)), "continuous vs 128x128 kernel over 192 output tiles"
    # block-strided operands on the continuous kernel (gemm_int8_blocked runs variant 0)
    xb = xq.reshape(M, 2, K // 2).permute(1, 0, 2).contiguous()
    out = torch.empty((2, M, N // 2), dtype=torch.bfloat16, device="cuda")
    lib.gemm_int8_blocked(xb, sx, wq, sw, b, out=out)
    assert torch.equal(out.permute(1, 0, 2).reshape(M, N), auto), "K-blocked x, N-blocked y on the continuous kernel"


@pytest.mark.parametrize("nb", [2, 4])
def test_blocked_operands_equal_the_row_major_call(lib, nb):
    M, N, K = 130, 256, 512
    g = torch.Generator().manual_seed(5)
    xq, wq = _codes((M, K), 6).cuda(), _codes((N, K), 7).cuda()
    sx, sw = (torch.rand(M, 1, generator=g) * 0.01 + 1e-3).cuda(), (torch.rand(N, 1, generator=g) * 0.01 + 1e-3).cuda()
    b = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
    want = lib.gemm_int8(xq, sx, wq, sw, b)
    xb = xq.reshape(M, nb, K // nb).permute(1, 0, 2).contiguous()  # K-blocked codes [B, M, K/B]
    assert torch.equal(lib.gemm_int8_blocked(xb, sx, wq, sw, b), want), "K-blocked x"
    out = torch.full((nb, M + 2, N // nb), 3.0, dtype=torch.bfloat16, device="cuda")  # N-blocked y [B', M, N/B'] inside a taller buffer
    lib.gemm_int8_blocked(xq, sx, wq, sw, b, out=out[:, 1 : M + 1])
    assert torch.equal(out[:, 1 : M + 1].permute(1, 0, 2).reshape(M, N), want), "N-blocked y"
    assert (out[:, 0] == 3).all() and (out[:, M + 1] == 3).all()
    want_g = lib.gemm_int8(xq, sx, wq, sw, b, epilogue=lib.EPI_GELU_TANH)
    out2 = torch.empty((nb, M, N // nb), dtype=torch.bfloat16, device="cuda")
    lib.gemm_int8_blocked(xb, sx, wq, sw, b, epilogue=lib.EPI_GELU_TANH, out=out2)
    assert torch.equal(out2.permute(1, 0, 2).reshape(M, N), want_g), "K-blocked x, N-blocked y, GELU"
    r1, r2 = (torch.ones(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    lib.gemm_int8_blocked(xb, sx, wq, sw, b, epilogue=lib.EPI_RESIDUAL, resid=r1, gate=b)
    lib.gemm_int8(xq, sx, wq, sw, b, epilogue=lib.EPI_RESIDUAL, resid=r2, gate=b)
    assert torch.equal(r1, r2), "K-blocked x, gated residual"


# ------------------------------------------------------------------------------------------------ operator class
def _op(config=None):
    from lightx2v_amd import ops

    op = ops.MMWeightInt8Hip("w.weight", "w.bias")
    op.set_config(config or {})
    return op


@pytest.mark.parametrize("auto", [True, False], ids=["auto", "checkpoint"])
def test_operator_class_vs_fixture(lib, fx, auto):
    op = _op({"weight_auto_quant": auto})
    if auto:
        op.load({"w.weight": fx["w"].cuda(), "w.bias": fx["b"].cuda()})
    else:
        op.load({"w.weight": fx["auto_wq"].cuda(), "w.weight_scale": fx["auto_wscale"].cuda(), "w.bias": fx["b"].cuda()})
    _bits_equal(op.weight, fx["auto_wq"], "weight bytes")
    _bits_equal(op.weight_scale, fx["auto_wscale"], "weight scales")
    x = fx["x"].cuda()
    y = op.apply(x)
    assert_bf16_close(y, fx["auto_y" if auto else "ckpt_y"], name=f"int8 operator class (auto={auto})", **CRIT)
    assert torch.equal(op.apply(x, quantized=op.quantize_input(x)), y)
    sl = slice(16, 48)
    assert torch.equal(op.apply(x, row_slice=sl), y[:, sl])
    out = torch.empty((2, x.shape[0], y.shape[1] // 2), dtype=torch.bfloat16, device="cuda")  # an N-blocked `out`: x2v_gemm_int8_blocked
    op.apply(x, out=out)
    assert torch.equal(out.permute(1, 0, 2).reshape(y.shape), y)
    op.to_cpu()
    assert not op.weight.is_cuda
    op.to_cuda()
    assert torch.equal(op.apply(x), y)


def test_operator_class_keeps_the_w8a8_accuracy_class(lib):
    """Relative power error against the unquantised product < 1e-2: the project's fp8 bound, from the lightx2v_kernel test metric."""
    gen = torch.Generator().manual_seed(9)
    M, K, N = 700, 1536, 1280
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=gen) / math.sqrt(K)).to(torch.bfloat16)
    b = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    op = _op({"weight_auto_quant": True})
    op.load({"w.weight": w.cuda(), "w.bias": b.cuda()})
    got = op.apply(x.cuda()).float().cpu()
    full = x.float() @ w.float().t() + b.float()
    err = (((got - full) ** 2).sum() / (full**2).sum()).item()
    print(f"int8 relative power error {err:.3e}")
    assert err < 1e-2


# ------------------------------------------------------------------------------------------------ driver
def test_fused_driver_shares_quantised_pairs_bit_identically(lib, golden_model, monkeypatch):
    """Block 0 of wan-tiny under the int8 key: the fused driver quantises each LayerNorm output once (layernorm_quantize) and hands the pair to every
    projection; the same block with every projection quantising its own input through op.apply(x) must give the same bits."""
    from lightx2v_amd import ops, synth, wan

    dims, wl = synth.WAN_DIMS["wan-tiny"], synth.WORKLOADS["wan-tiny"]
    wd = {k: v.cuda() for k, v in synth.synth_wan_weights(dims, seed=0).items()}
    cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=4,
                             mm_config={"mm_type": KEY, "weight_auto_quant": True})
    model = wan.WanModel(cfg, wd)
    blk = model.transformer_weights.blocks[0]
    assert type(blk.compute_phases[1].self_attn_q) is ops.MMWeightInt8Hip and blk.compute_phases[3].ffn_0.weight.dtype == torch.int8
    lat, ctx, ctx_null = synth.synth_inputs(dims, wl["target_shape"])
    from lightx2v_amd import scheduler

    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=golden_model["latents0"])
    model.set_scheduler(sch)
    sch.step_pre(0)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}}
    embed, grid_sizes, (x, embed0, seq_lens, freqs, context) = model.pre_infer.infer(model.pre_weight, inputs, positive=True)
    tr = model.transformer_infer
    calls = []
    orig = ops.MMWeightInt8Hip.layernorm_quantize
    monkeypatch.setattr(ops.MMWeightInt8Hip, "layernorm_quantize", staticmethod(lambda *a, **k: (calls.append(1), orig(*a, **k))[1]))
    shared = tr.infer_block(blk, grid_sizes, embed, x.clone(), embed0, seq_lens, freqs, context)
    assert len(calls) >= 2, "the fused driver did not go through layernorm_quantize"
    monkeypatch.setattr(wan, "_ln_then_mm_input", lambda op, x, weight=None, bias=None, scale=None, shift=None, eps=1e-6: (lib.layernorm(x, weight, bias, scale=scale, shift=shift, eps=eps), {}))
    own = tr.infer_block(blk, grid_sizes, embed, x.clone(), embed0, seq_lens, freqs, context)
    assert torch.isfinite(shared.float()).all()
    _bits_equal(shared, own, "block 0: shared quantised pairs vs op.apply(x) per projection")
