"""Parity of each HIP operator (through the C-ABI) against (1) fixtures generated from the reference
(tests/golden/ops.*.safetensors) and (2) the CPU oracle on seeded inputs at sizes it finishes in seconds.

Tolerances (bf16 outputs; 1 ulp = 2^-7 relative, the widest bf16 spacing):
  * elementwise residual/gate: bit-exact (same rounding points as the reference chain)
  * GEMM, LayerNorm(+modulate), RMSNorm ref-chain mode, RoPE: <= 1 ulp (+ atol for cancellation), on all but a
    small stated fraction of elements whose fp32 sum landed on the other side of a rounding boundary
  * RMSNorm fp32 mode vs the reference's bf16-chain CPU fallback: 3 ulp (the chain itself rounds 5 times)
  * attention: |diff| <= 1e-3*|ref| + 4e-3 — the reference's own acceptance is allclose(rtol=1e-3, atol=1e-3)
    against flash-attn on N(0,1) data (attentions/distributed/ring/tests/test.py:97); ours additionally absorbs
    the bf16 rounding of the output (|o| <~ 1 → half-ulp 2e-3) and of P.
"""
import math

import pytest
import torch

from tests.util import assert_bf16_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def dev(t):
    return t.cuda()


def test_gemm_golden(lib, golden_ops):
    g = golden_ops
    y = lib.gemm(dev(g["mm_x"]), dev(g["mm_w"]), dev(g["mm_b"]))
    assert_bf16_close(y, g["mm_y"], ulps=1, atol=1e-3, bad_frac=1e-3, name="mm")
    y = lib.gemm(dev(g["mm_x"]), dev(g["mm_w"]))
    assert_bf16_close(y, g["mm_y_nobias"], ulps=1, atol=1e-3, bad_frac=1e-3, name="mm nobias")


def test_rmsnorm_golden(lib, golden_ops):
    g = golden_ops
    y = lib.rmsnorm(dev(g["rms_x"]), dev(g["rms_w"]), round_mode=lib.ROUND_REF)
    assert_bf16_close(y, g["rms_y"], ulps=1, bad_frac=2e-3, name="rmsnorm ref-chain")
    y = lib.rmsnorm(dev(g["rms_x"]), dev(g["rms_w"]), round_mode=lib.ROUND_FP32)
    assert_bf16_close(y, g["rms_y"], ulps=3, name="rmsnorm fp32 vs bf16 chain")
    from oracle import wan_oracle as O

    assert_bf16_close(y, O.rms_norm_fp32(g["rms_x"], g["rms_w"]), ulps=1, bad_frac=2e-3, name="rmsnorm fp32 vs fp32 oracle")


def test_layernorm_golden(lib, golden_ops):
    g = golden_ops
    x = dev(g["ln_x"])
    assert_bf16_close(lib.layernorm(x), g["ln_y"], ulps=1, atol=1e-3, bad_frac=2e-3, name="ln")
    y = lib.layernorm(x, scale=dev(g["ln_scale"]), shift=dev(g["ln_shift"]))
    assert_bf16_close(y, g["ln_mod_y"], ulps=1, atol=8e-3, bad_frac=2e-3, name="ln+modulate")
    y = lib.layernorm(x, weight=dev(g["ln_w"]), bias=dev(g["ln_b"]))
    assert_bf16_close(y, g["ln_affine_y"], ulps=1, atol=2e-3, bad_frac=2e-3, name="ln affine")


def test_residual_bit_exact(lib, golden_ops):
    g = golden_ops
    x = dev(g["res_x"]).clone()
    lib.gate_residual_(x, dev(g["res_y"]), dev(g["res_gate"]))
    assert torch.equal(x.cpu(), g["res_gated"])
    x = dev(g["res_x"]).clone()
    lib.gate_residual_(x, dev(g["res_y"]))
    assert torch.equal(x.cpu(), g["res_plain"])


def test_gelu_and_sinusoid_golden(lib, golden_ops):
    g = golden_ops
    assert_bf16_close(lib.activation(dev(g["gelu_x"]), lib.EPI_GELU_TANH), g["gelu_y"], ulps=1, atol=1e-6, bad_frac=2e-3, name="gelu")
    assert_bf16_close(lib.sinusoid_embed(dev(g["sin_t"]), 256), g["sin_y"], ulps=1, atol=1e-6, bad_frac=5e-3, name="sinusoid")


def test_rope_golden(lib, golden_ops):
    from lightx2v_amd.wan import rope_cos_sin_table

    g = golden_ops
    q = dev(g["rope_x"]).reshape(72, 256).clone()
    k = q.clone()
    grid = tuple(g["rope_grid"][0].tolist())
    lib.rmsnorm_rope_(q, k, None, None, rope_cos_sin_table(128, "cuda"), grid, 2)
    ref = g["rope_y"].reshape(72, 256)
    assert_bf16_close(q, ref, ulps=1, atol=2e-3, bad_frac=2e-3, name="rope q")
    assert torch.equal(q, k)


def test_attention_golden(lib, golden_ops):
    """The golden fixture at the oracle's tolerance; the tight criterion for these kernels is tests/test_gpu_attn_fp64.py (float64, every dispatch edge)."""
    g = golden_ops
    for variant in (0, 4, 5, 6):  # default and the three lazy-rescale thresholds (x2v.h)
        o = lib.attention(dev(g["attn_q"]), dev(g["attn_k"]), dev(g["attn_v"]), 2, variant=variant)
        assert_bf16_close(o, g["attn_o"], ulps=0.128, atol=4e-3, name=f"self attention variant {variant}")
        o = lib.attention(dev(g["attn_q"]), dev(g["xattn_k"]), dev(g["xattn_v"]), 2, variant=variant)
        assert_bf16_close(o, g["xattn_o"], ulps=0.128, atol=4e-3, name=f"cross attention variant {variant}")


def test_attention_fast_variants(lib, golden_ops):
    """The ping-pong kernel folds scale*log2(e) into q (one more bf16 rounding of q, relative 2^-9) — compared with the golden
    outputs at twice the default tolerance; it runs on the pre-transposed V (transposition checked exactly).  Both kernel bodies.
    The tight criterion for these kernels is tests/test_gpu_attn_fp64.py (float64, every dispatch edge)."""
    from oracle import wan_oracle as O

    g = golden_ops
    for variant in (lib.ATTN_FAST,):
        o = lib.attention(dev(g["attn_q"]), dev(g["attn_k"]), dev(g["attn_v"]), 2, variant=variant)
        assert_bf16_close(o, g["attn_o"], ulps=0.256, atol=8e-3, name=f"self attention variant {variant}")
        o = lib.attention(dev(g["attn_q"]), dev(g["xattn_k"]), dev(g["xattn_v"]), 2, variant=variant)
        assert_bf16_close(o, g["xattn_o"], ulps=0.256, atol=8e-3, name=f"cross attention variant {variant}")
    # ragged sizes: Sq, Sk not multiples of the tiles; strided (fused-qkv) views; many tiles
    gen = torch.Generator().manual_seed(77)
    for Sq, Sk, H in ((1, 1, 1), (33, 65, 2), (300, 1000, 3), (257, 4100, 1)):
        qkv_c = torch.randn(max(Sq, Sk), 3 * H * 128, generator=gen).to(torch.bfloat16)
        qkv = qkv_c.cuda()
        q, k, v = qkv[:Sq, : H * 128], qkv[:Sk, H * 128 : 2 * H * 128], qkv[:Sk, 2 * H * 128 :]
        # against the ORACLE (torch_sdpa, attn_weight.py:229-239), not against another kernel of this library: a defect shared by the two
        # kernels would pass a self-comparison
        ref = O.sdpa(qkv_c[:Sq, : H * 128].reshape(Sq, H, 128), qkv_c[:Sk, H * 128 : 2 * H * 128].reshape(Sk, H, 128), qkv_c[:Sk, 2 * H * 128 :].reshape(Sk, H, 128))
        assert_bf16_close(lib.attention(q, k, v, H), ref, ulps=0.128, atol=4e-3, name=f"default kernel vs oracle Sq={Sq} Sk={Sk} H={H}")
        for var in (lib.ATTN_FAST,):
            got = lib.attention(q, k, v, H, variant=var)
            assert_bf16_close(got, ref, ulps=0.256, atol=8e-3, name=f"ping-pong ({var}) vs oracle Sq={Sq} Sk={Sk} H={H}")
        vt = lib.transpose_heads(v, H)
        nt = (Sk + 63) // 64
        want = torch.zeros((H, 128, nt * 64), dtype=vt.dtype, device=vt.device)
        want[:, :, :Sk] = v.reshape(Sk, H, 128).permute(1, 2, 0)
        assert torch.equal(vt, want.reshape(H, 128, nt, 64).permute(0, 2, 1, 3))


# ---------------------------------------------------------------------------- oracle on seeded inputs
@pytest.mark.parametrize("M,K,N", [(1280, 1536, 1536), (1280, 1536, 8960), (333, 8960, 1536), (1, 256, 1536), (512, 4096, 1536), (700, 1536, 64)])
def test_gemm_vs_oracle(lib, M, K, N):
    """Against the oracle's bf16 addmm, by the dispatcher's own choice (these shapes take the 128x128 kernel).  Every kernel body forced at its
    edges against float64, with a bound on every element: tests/test_gpu_gemm_fp64.py."""
    from oracle import wan_oracle as O

    gen = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=gen) / math.sqrt(K)).to(torch.bfloat16)
    b = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    ref = O.mm(x, w, b)
    got = lib.gemm(dev(x), dev(w), dev(b))
    assert_bf16_close(got, ref, ulps=1, atol=2e-3, bad_frac=1e-3, name="gemm")
    # fused epilogues against the reference's separate ops
    ref_g = torch.nn.functional.gelu(ref, approximate="tanh")
    assert_bf16_close(lib.gemm(dev(x), dev(w), dev(b), epilogue=lib.EPI_GELU_TANH), ref_g, ulps=1, atol=2e-3, bad_frac=2e-3, name="gemm+gelu")
    res = torch.randn(M, N, generator=gen).to(torch.bfloat16)
    gate = (torch.randn(1, N, generator=gen) * 0.5).to(torch.bfloat16)
    ref_r = res.clone()
    ref_r.add_(ref * gate.squeeze(0))
    r = dev(res).clone()
    out = lib.gemm(dev(x), dev(w), dev(b), epilogue=lib.EPI_RESIDUAL, resid=r, gate=dev(gate))
    assert out.data_ptr() == r.data_ptr()
    assert_bf16_close(r, ref_r, ulps=1, atol=6e-3, bad_frac=2e-3, name="gemm+gate-residual")


def test_gemm_identity_and_linearity(lib):
    """Size-independent properties at a BASELINE-sized K: W = I reproduces x exactly; f(x1+x2) = f(x1)+f(x2) for
    inputs whose sum is exact in bf16."""
    K = 1536
    x = torch.randn(515, K, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    eye = torch.eye(K, dtype=torch.bfloat16, device="cuda")
    assert torch.equal(lib.gemm(x, eye), x)
    xi = torch.randint(-8, 8, (300, K), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).cuda()
    xj = torch.randint(-8, 8, (300, K), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    w = torch.randint(-2, 3, (256, K), generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    # integer data: every partial sum is exact in fp32, so the result must equal the exactly rounded product
    for xin in (xi, xj, xi + xj):
        ref = (xin.float() @ w.float().t()).to(torch.bfloat16)
        assert torch.equal(lib.gemm(xin, w), ref)


@pytest.mark.parametrize("Sq,Sk,H", [(1280, 1280, 12), (1000, 512, 12), (257, 1031, 2)])
def test_attention_vs_oracle(lib, Sq, Sk, H):
    from oracle import wan_oracle as O

    gen = torch.Generator().manual_seed(Sq + Sk)
    q = torch.randn(Sq, H, 128, generator=gen).to(torch.bfloat16)
    k = torch.randn(Sk, H, 128, generator=gen).to(torch.bfloat16)
    v = torch.randn(Sk, H, 128, generator=gen).to(torch.bfloat16)
    ref = O.sdpa(q, k, v)
    f32 = O.attention_fp32(q, k, v)
    got = lib.attention(dev(q), dev(k), dev(v), H)
    assert_bf16_close(got, ref, ulps=0.128, atol=4e-3, name="attention vs torch_sdpa")
    # triangle: we must be as close to exact fp32 attention as the reference's own CPU kernel is (x1.5 slack)
    e_ours = (got.float().cpu() - f32).abs().max().item()
    e_ref = (ref.float() - f32).abs().max().item()
    assert e_ours <= 1.5 * e_ref + 1e-3, (e_ours, e_ref)


def test_attention_persistent_short_walk(lib):
    """Cross-attention's launch form (x2v_attn_fwd_bf16_vt, plan bit 9: 4..32 whole key tiles, >= 512 query blocks x heads): a workgroup walks a
    range of (sequence, head, query block) items as one tile stream.  Against the ORACLE (torch_sdpa, attn_weight.py:229-239) at a size it finishes
    in seconds, and bit for bit against the one-walk form (X2V_ATTN_VT_ONE_WALK, itself oracle-tested above) at the shapes the oracle cannot reach:
    the minimum and maximum walk lengths, ragged last query blocks, ranges that cross heads (more heads than workgroup ranges and fewer), a
    strided q / out view, the model's shape (75 600 x 512 x 40), q prescaled or not, and two stacked sequences in one launch."""
    from oracle import wan_oracle as O

    gen = torch.Generator().manual_seed(4242)
    Sq, Sk, H = 3365, 512, 40  # 14 query blocks x 40 heads = 560 items; the last block of every head has 37 rows
    assert lib.attn_vt_launch_plan(Sq, Sk, H, with_short=True) == (False, False, True)
    assert lib.attn_vt_launch_plan(Sq, Sk, H, one_walk=True, with_short=True)[2] is False
    q = torch.randn(Sq, H, 128, generator=gen).to(torch.bfloat16)
    k = torch.randn(Sk, H, 128, generator=gen).to(torch.bfloat16)
    v = torch.randn(Sk, H, 128, generator=gen).to(torch.bfloat16)
    ref = O.sdpa(q, k, v)
    got = lib.attention(dev(q), dev(k), dev(v), H, variant=lib.ATTN_FAST)
    assert_bf16_close(got, ref, ulps=0.256, atol=8e-3, name="persistent short-walk form vs oracle")
    f32 = O.attention_fp32(q, k, v)
    e_ours, e_ref = (got.float().cpu() - f32).abs().max().item(), (ref.float() - f32).abs().max().item()
    assert e_ours <= 1.5 * e_ref + 2e-3, (e_ours, e_ref)

    gcu = torch.Generator(device="cuda").manual_seed(7)
    for Sq, Sk, H, pre in [(3365, 512, 40, False), (20000, 256, 12, False), (20000, 320, 12, True), (5000, 2048, 30, True), (131072 + 5, 384, 1, False), (75600, 512, 40, False), (75600, 512, 40, True),
                           (9450, 512, 40, True)]:
        assert lib.attn_vt_launch_plan(Sq, Sk, H, with_short=True)[2], (Sq, Sk, H)
        wide = torch.randn(Sq, H * 128 + 256, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
        q = wide[:, 128 : 128 + H * 128]  # token stride != H * 128
        k = torch.randn(Sk, H * 128, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
        v = torch.randn(Sk, H * 128, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
        k[Sk // 2] *= 4.0  # a late dominant key: the lazy rescale branch fires inside the walk
        vt = lib.transpose_heads(v, H)
        flags = lib.ATTN_FAST | (lib.ATTN_Q_PRESCALED if pre else 0)
        a = torch.full((Sq, H * 128 + 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        b = torch.full_like(a, float("nan"))
        lib.attention(q, k, None, H, out=a[:, : H * 128], variant=flags, vt=vt)
        lib.attention(q, k, None, H, out=b[:, : H * 128], variant=flags | lib.ATTN_ONE_WALK, vt=vt)
        assert torch.isfinite(a[:, : H * 128].float()).all(), (Sq, Sk, H)
        assert torch.equal(a[:, : H * 128], b[:, : H * 128]), f"persistent vs one-walk form Sq={Sq} Sk={Sk} H={H} prescaled={pre}"
        assert torch.isnan(a[:, H * 128 :].float()).all(), "columns behind the heads must not be written"
    # two stacked sequences (the CFG pair) in one launch: sequence b's keys are the first Sk rows of its slot
    Sp, Sk, H = 4096, 512, 40
    q = torch.randn(2 * Sp, H * 128, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    k = torch.randn(2 * Sp, H * 128, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    v = torch.randn(2 * Sp, H * 128, generator=gcu, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    vt = lib.transpose_heads(v, H)
    one = lib.attention_batched(q, k, vt, H, 2, Sp, Sk, one_launch=True)
    for b in range(2):
        rows = slice(b * Sp, (b + 1) * Sp)
        sep = lib.attention(q[rows], k[rows][:Sk], v[rows][:Sk], H, variant=lib.ATTN_FAST | lib.ATTN_ONE_WALK)
        assert torch.equal(one[rows], sep), f"stacked sequence {b}"


def test_attention_properties_full_size(lib):
    """At the BASELINE config-2 sequence length (S = 20280, where the CPU oracle is too slow): softmax rows sum to 1
    (V = 1 → O = 1), identical keys → O = mean(V), and a dominant key → O = its V row (online-softmax rescale path)."""
    S, H = 20280, 2
    gen = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(S, H * 128, generator=gen, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    k = torch.randn(S, H * 128, generator=gen, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    ones = torch.ones(S, H * 128, device="cuda", dtype=torch.bfloat16)
    o = lib.attention(q, k, ones, H)
    assert (o.float() - 1).abs().max().item() <= 2 ** -7
    v = torch.randn(S, H * 128, generator=gen, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    o = lib.attention(q, torch.zeros_like(k), v, H)
    mean_v = v.float().mean(0, keepdim=True)
    assert (o.float() - mean_v).abs().max().item() <= 2e-3
    k2 = k.clone()
    k2[12345] = (q[7].float() * 3).to(torch.bfloat16)  # q7·k ≈ 3*|q7|^2 ≈ 384*... dominates every other score
    o = lib.attention(q[:64].contiguous(), k2, v, H)
    assert (o[7].float() - v[12345].float()).abs().max().item() <= 2 ** -6


def test_fp8_path_vs_oracle(lib):
    from oracle import wan_oracle as O

    gen = torch.Generator().manual_seed(9)
    M, K, N = 700, 1536, 1280
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=gen) / math.sqrt(K)).to(torch.bfloat16)
    b = (torch.randn(N, generator=gen) * 0.1).to(torch.bfloat16)
    wq, sw = O.quant_fp8_weight_per_channel(w)
    xq_ref, sx_ref = O.quant_fp8_per_token(x)
    xq, sx = lib.quant_fp8_rowwise(dev(x))
    assert torch.allclose(sx.cpu(), sx_ref, rtol=1e-6, atol=0)
    mism = (xq.cpu().view(torch.uint8) != xq_ref.view(torch.uint8)).float().mean().item()
    assert mism <= 1e-3, f"{mism} of e4m3 codes differ"  # x/s ties at an e4m3 rounding boundary
    ref = O.mm_fp8(x, wq, sw, b)
    got = lib.gemm_fp8(xq, sx, dev(wq), dev(sw), dev(b))
    assert_bf16_close(got, ref, ulps=1, atol=4e-3, bad_frac=2e-3, name="fp8 scaled mm")
    # w8a8 keeps the reference's accuracy class vs bf16: relative-power error < 1e-2 (lightx2v_kernel test metric)
    full = O.mm(x, w, b).float()
    err = ((got.float().cpu() - full) ** 2).sum() / (full**2).sum()
    assert err < 1e-2


def test_fp8_vs_reference_class_fixture(lib):
    """tests/golden/fp8_mm.safetensors: the reference's own fp8 operator class (auto-quantised and checkpoint-loaded weights)."""
    import os

    from safetensors.torch import load_file

    from lightx2v_amd import ops

    g = load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp8_mm.safetensors"))
    xq, sx = lib.quant_fp8_rowwise(dev(g["x"]))
    assert torch.allclose(sx.cpu(), g["sx"], rtol=1e-6, atol=0), "per-token scales (incl. the floor of an all-zero token)"
    mism = (xq.cpu().view(torch.uint8) != g["xq"]).float().mean().item()
    assert mism <= 1e-3, f"{mism} of e4m3 codes differ"
    for auto in (True, False):
        op = ops.MMWeightFp8Hip("w.weight", "w.bias")
        op.set_config({"weight_auto_quant": auto})
        if auto:
            op.load({"w.weight": dev(g["w"]), "w.bias": dev(g["b"])})
            assert torch.equal(op.weight_scale.cpu(), g["auto_wscale"]) and torch.equal(op.weight.cpu().view(torch.uint8), g["auto_wq"])
        else:
            op.load({"w.weight": dev(g["auto_wq"]).view(torch.float8_e4m3fn), "w.weight_scale": dev(g["auto_wscale"].to(torch.bfloat16)), "w.bias": dev(g["b"])})
        y = op.apply(dev(g["x"]))
        assert_bf16_close(y, g["auto_y" if auto else "ckpt_y"], ulps=1, atol=4e-3, bad_frac=2e-3, name=f"fp8 operator class (auto={auto})")


def test_causal_conv3d_vs_torch(lib):
    """CausalConv3d.forward semantics (vae.py:19-44): left time padding 2 minus the cached frames, zero 'same'
    spatial padding, fp32."""
    gen = torch.Generator().manual_seed(3)
    for (T, H, W, Cin, Cout, kt, ks, nc) in [(2, 12, 20, 16, 24, 3, 3, 2), (1, 9, 7, 32, 3, 3, 3, 1), (3, 6, 6, 48, 96, 3, 3, 0), (2, 8, 8, 16, 16, 1, 3, 0), (2, 4, 6, 16, 32, 3, 1, 2)]:
        x = torch.randn(1, Cin, T, H, W, generator=gen)
        cache = torch.randn(1, Cin, nc, H, W, generator=gen) if nc else None
        w = torch.randn(Cout, Cin, kt, ks, ks, generator=gen) * 0.1
        b = torch.randn(Cout, generator=gen)
        xin = torch.cat([cache, x], dim=2) if nc else x
        p = ks // 2
        xin = torch.nn.functional.pad(xin, (p, p, p, p, (kt - 1) - nc, 0))
        ref = torch.nn.functional.conv3d(xin, w, b)  # [1,Cout,T,H,W]
        xc = x[0].permute(1, 2, 3, 0).contiguous().cuda()
        cc = cache[0].permute(1, 2, 3, 0).contiguous().cuda() if nc else None
        wc = w.permute(0, 2, 3, 4, 1).contiguous().cuda()
        got = lib.causal_conv3d(xc, wc, b.cuda(), cc).permute(3, 0, 1, 2).unsqueeze(0).cpu()
        assert torch.allclose(got, ref, rtol=1e-4, atol=2e-4), (got - ref).abs().max()
