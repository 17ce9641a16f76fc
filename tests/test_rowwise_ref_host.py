"""tests/rowwise_ref.py checked without a GPU: the float64 references of the row-wise operators against (1) the reference-generated fixtures
tests/golden/ops.*, (2) the CPU oracle on the seeded inputs of tests/test_gpu_rowwise_fp64.py at its smallest shapes, and (3) themselves —
for EVERY input set of the GPU module the same formula evaluated in fp32 torch (an independent fp32 evaluation standing in for any correct
fp32 kernel) must stay inside the hard bound, differ from bf16(ref64) in at most HALF the flip cap (1e-3 of 2e-3) and flag at most 1 % of the
rows as near a rounding boundary.  No kernel is compared here.

Measured with the committed seeds (share of elements whose fp32 result rounds to another bf16 than the float64 reference; flagged rows):
  RMSNorm (both modes, 15 D)      worst case 2.2e-5; no flagged row (after the D = 8 reseed, rowwise_ref.RMS_RESEED)
  LayerNorm (6 operand sets)      worst case 1.6e-5 with the mirrored mean-40 set (a plain N(40, 0.5) draw: up to 4.6e-3, see rowwise_ref.ln_inputs)
  RMSNorm + RoPE                  worst case 4.7e-5; no flagged row
  headnorm + RoPE                 0
  activations (65 280 patterns)   gelu-tanh 7.7e-5, SiLU 2.6e-4, exact GELU 0; sinusoid and gate-residual 0
"""
import math

import pytest
import torch

from tests import rowwise_ref as R
from tests.util import assert_bf16_close

HALF_CAP = R.FLIP_CAP / 2


def bf(t):
    return R.rne_bf16(t).to(torch.bfloat16)


def twin_check(case, fn, what=""):
    """fn(dtype=..., alt=...) -> Ref.  The fp32 evaluation, rounded once more to bf16 where the reference is exact, against the float64 one."""
    got = R.rne_bf16(fn(dtype=torch.float32, alt=-1).y).to(torch.float64)
    case.check(got, lambda alt: fn(dtype=torch.float64, alt=alt), what)


def finish(case):
    case.finish(cap=HALF_CAP, record=False)


# ------------------------------------------------------------------------------------------------------------------- the rounding itself
def test_rne_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 8)
    assert torch.equal(bf(x32.double()), x32.to(torch.bfloat16))  # fp32 values: torch's cast is the same RNE
    allb = R.all_finite_bf16()
    assert torch.equal(R.bf16_bits(R.rne_bf16(allb.double())), allb.view(torch.int16))  # idempotent on every pattern, signed zeros and subnormals included
    # ties go to even; a float64 just past the tie goes up although its fp32 cast is the tie itself (no double rounding)
    one = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40)], dtype=torch.float64)
    assert R.rne_bf16(one).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    gap, other = R.boundary_gap(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 - 2.0 ** -30, 1.5], dtype=torch.float64))
    assert gap[0] < R.FLAG_GAP and other[0] == 1.0 and gap[1] > 2.0 ** -11 and other[1] == 1.0 - 2.0 ** -8 and gap[2] > 2.0 ** -10


# ------------------------------------------------------------------------------------------------------------------- fixtures
def test_references_reproduce_the_fixtures(golden_ops):
    """Chain references rounded to bf16, within the tolerance tests/test_gpu_ops.py grants the kernels on the same fixtures; residual bit-exact."""
    g = golden_ops
    assert_bf16_close(bf(R.rmsnorm(g["rms_x"], g["rms_w"], mode=R.ROUND_REF).y), g["rms_y"], ulps=1, bad_frac=2e-3, name="rms_y")
    assert_bf16_close(bf(R.rmsnorm(g["rms_x"], g["rms_w"], mode=R.ROUND_FP32).y), g["rms_y"], ulps=3, name="rms_y fp32")
    x = g["ln_x"]
    assert_bf16_close(bf(R.layernorm(x).y), g["ln_y"], ulps=1, atol=1e-3, bad_frac=2e-3, name="ln_y")
    assert_bf16_close(bf(R.layernorm(x, scale=g["ln_scale"], shift=g["ln_shift"]).y), g["ln_mod_y"], ulps=1, atol=8e-3, bad_frac=2e-3, name="ln_mod_y")
    assert_bf16_close(bf(R.layernorm(x, w=g["ln_w"], b=g["ln_b"]).y), g["ln_affine_y"], ulps=1, atol=2e-3, bad_frac=2e-3, name="ln_affine_y")
    assert torch.equal(bf(R.gate_residual(g["res_x"], g["res_y"], g["res_gate"]).y), g["res_gated"])
    assert torch.equal(bf(R.gate_residual(g["res_x"], g["res_y"]).y), g["res_plain"])
    assert_bf16_close(bf(R.activation(g["gelu_x"], R.ACT_GELU_TANH).y), g["gelu_y"], ulps=1, atol=1e-6, bad_frac=2e-3, name="gelu_y")
    assert_bf16_close(bf(R.sinusoid(g["sin_t"], 256).y), g["sin_y"], ulps=1, atol=1e-6, bad_frac=5e-3, name="sin_y")
    grid = tuple(g["rope_grid"][0].tolist())
    ref = R.rmsnorm_rope(g["rope_x"].reshape(72, 256), None, _model_table(), 0, grid)
    assert_bf16_close(bf(ref.y), g["rope_y"].reshape(72, 256), ulps=1, atol=2e-3, bad_frac=2e-3, name="rope_y")


def _model_table():
    """The reference's `freqs` [1024, 64] (pre_infer.py:12-19) as the fp32 (cos, sin) table the C ABI takes."""
    from oracle import wan_oracle as O

    f = O.rope_freqs_table(128)
    return torch.stack([f.real, f.imag], dim=-1).float().contiguous()


# ------------------------------------------------------------------------------------------------------------------- the oracle
def _rows_match_torch_chain(got, want, x, name):
    """torch's CPU bf16 rsqrt is not the correctly rounded 1/sqrt (tests/test_gpu_hunyuan.py; a vectorised approximation, one bf16 ulp off on a
    sizeable share of inputs), so a whole row may be scaled by the neighbouring rstd.  Rows on which torch's rsqrt IS the correctly rounded
    one must agree bit for bit; no element of any row may be further than two ulps."""
    t = x.pow(2).mean(-1, keepdim=True) + 1e-6  # the torch chain up to rsqrt's argument
    exact = (torch.rsqrt(t).double() == R.rne_bf16(1.0 / torch.sqrt(t.double()))).reshape(-1)
    assert exact.any(), name
    assert torch.equal(got[exact], want[exact]), f"{name}: rows with a correctly rounded torch rsqrt differ"
    assert_bf16_close(got, want, ulps=2, name=name)


def test_references_agree_with_the_oracle():
    from oracle import hunyuan_oracle as HO
    from oracle import wan_oracle as O

    for D in R.NORM_D[:2]:
        x, w = R.rms_inputs(D, 9, "n01")
        ref = R.rmsnorm(x, w, mode=R.ROUND_REF)
        _rows_match_torch_chain(bf(ref.y), O.rms_norm(x, w), x, "rms_norm")
        assert_bf16_close(bf(R.rmsnorm(x, w, mode=R.ROUND_FP32).y), O.rms_norm_fp32(x, w), ulps=1, bad_frac=2e-3, name="rms_norm_fp32")
        xl, (lw, lb, sc, sh) = R.ln_inputs(D, 5, "n01")
        assert_bf16_close(bf(R.layernorm(xl).y), O.layer_norm(xl), ulps=1, atol=1e-3, bad_frac=2e-3, name="layer_norm")
        assert_bf16_close(bf(R.layernorm(xl, w=lw, b=lb).y), O.layer_norm(xl, lw, lb), ulps=1, atol=2e-3, bad_frac=2e-3, name="layer_norm affine")
        y = O.layer_norm(xl)
        y.mul_(1 + sc).add_(sh)
        assert_bf16_close(bf(R.layernorm(xl, scale=sc, shift=sh).y), y, ulps=1, atol=8e-3, bad_frac=2e-3, name="layer_norm + modulate")
    # RoPE: the model's table through the oracle's compute_freqs / compute_freqs_dist (ones padding past the grid) and apply_rotary_emb
    H, freqs, cs = 1, O.rope_freqs_table(128), _model_table()
    for gi, (grid, s0, S) in enumerate(R.ROPE_GRIDS):
        q = R.rope_inputs(H, gi)[0]
        fi = O.compute_freqs_dist(s0 + S, 64, grid, freqs, 0, 1)[s0:]  # one rank holding tokens [0, s0 + S): ones past the grid
        want = O.apply_rotary_emb(q.reshape(S, H, 128), fi).reshape(S, H * 128)
        assert_bf16_close(bf(R.rmsnorm_rope(q, None, cs, s0, grid).y), want, ulps=1, atol=2e-3, bad_frac=2e-3, name=f"rope grid#{gi}")
    for dim in R.SIN_DIMS:
        t = torch.tensor(R.SIN_T, dtype=torch.int64)
        assert_bf16_close(bf(R.sinusoid(t, dim).y), O.sinusoidal_embedding_1d(dim, t), ulps=1, atol=1e-6, bad_frac=2e-3, name=f"sinusoid {dim}")
    # HunyuanVideo rotary step (bf16 tensors: exact arithmetic between roundings, so bit-exact)
    Hh, L = R.HEAD_SHAPES[1]
    q, k, _, _, cos, sin = R.head_inputs(Hh, L)
    q2, k2 = HO.apply_rotary_emb(q.reshape(L, Hh, 128), k.reshape(L, Hh, 128), cos, sin)
    assert torch.equal(bf(R.headnorm_rope(q, None, cos, sin, Hh, L, mode=R.ROUND_REF).y), q2.reshape(L, -1))
    assert torch.equal(bf(R.headnorm_rope(k, None, cos, sin, Hh, L, mode=R.ROUND_REF).y), k2.reshape(L, -1))
    qn = O.rms_norm(q.reshape(L, Hh, 128), R.head_inputs(Hh, L)[2])
    ref = R.headnorm_rope(q, R.head_inputs(Hh, L)[2], cos, sin, Hh, 0, mode=R.ROUND_REF)
    _rows_match_torch_chain(bf(ref.y).reshape(L * Hh, 128), qn.reshape(L * Hh, 128), q.reshape(L * Hh, 128), "per-head rms_norm")


# ------------------------------------------------------------------------------------------------------------------- the caps, for the reference alone
@pytest.mark.parametrize("D", R.NORM_D)
def test_caps_hold_rmsnorm(D):
    cases = {m: R.Case(f"rmsnorm mode={m} D={D}") for m in (R.ROUND_FP32, R.ROUND_REF)}
    for what, x, w, mode, _ in R.rms_items(D):
        twin_check(cases[mode], lambda dtype, alt: R.rmsnorm(x, w, mode=mode, alt=alt, dtype=dtype), what)
    for c in cases.values():
        finish(c)


@pytest.mark.parametrize("D", R.NORM_D)
def test_caps_hold_layernorm(D):
    case = R.Case(f"layernorm D={D}")
    for what, x, kw, _, _ in R.ln_items(D):
        twin_check(case, lambda dtype, alt: R.layernorm(x, dtype=dtype, **kw), what)
    finish(case)


@pytest.mark.parametrize("H", R.ROPE_H)
def test_caps_hold_rmsnorm_rope(H):
    cs = R.rope_table()
    case = R.Case(f"rmsnorm_rope H={H}")
    for what, gi, q, k, wq, wk, mode in R.rope_items(H):
        grid, s0, _ = R.ROPE_GRIDS[gi]
        twin_check(case, lambda dtype, alt: R.rmsnorm_rope(q, wq, cs, s0, grid, mode=mode, out_scale=R.Q_SCALE, alt=alt, dtype=dtype), what + " q")
        twin_check(case, lambda dtype, alt: R.rmsnorm_rope(k, wk, cs, s0, grid, mode=mode, alt=alt, dtype=dtype), what + " k")
    finish(case)


@pytest.mark.parametrize("H,L", R.HEAD_SHAPES)
def test_caps_hold_headnorm_rope(H, L):
    case = R.Case(f"headnorm_rope H={H}")
    for what, q, k, wq, wk, cos, sin, l_rope, mode, scale in R.head_items(H, L):
        twin_check(case, lambda dtype, alt: R.headnorm_rope(q, wq, cos, sin, H, l_rope, mode=mode, out_scale=scale, alt=alt, dtype=dtype), what + " q")
        twin_check(case, lambda dtype, alt: R.headnorm_rope(k, wk, cos, sin, H, l_rope, mode=mode, alt=alt, dtype=dtype), what + " k")
    finish(case)


def test_caps_hold_elementwise():
    x = R.all_finite_bf16()
    for act in (R.ACT_GELU_TANH, R.ACT_SILU, R.ACT_GELU_ERF):
        case = R.Case(f"activation {act}")
        twin_check(case, lambda dtype, alt: R.activation(x, act, dtype=dtype))
        finish(case)
    for dim in R.SIN_DIMS:
        case = R.Case(f"sinusoid dim={dim}")
        twin_check(case, lambda dtype, alt: R.sinusoid(torch.tensor(R.SIN_T), dim, dtype=torch.float64))  # the kernel's contract is float64 then rounded: no fp32 twin
        finish(case)
    for D in (8, 1536, 5120):
        xr, yr, gate = R.residual_inputs(5, D)
        want = xr.clone()
        want.add_(yr * gate)
        assert torch.equal(bf(R.gate_residual(xr, yr, gate).y), want) and torch.equal(bf(R.gate_residual(xr, yr).y), xr + yr)
