"""The yardstick of the block-scaled fp8 attention (tests/attn_mx_ref.py) checked on the CPU, and the argument validation of the x2v_attn_mx_*
entries, which runs without a GPU.

  * the restated MXFP8 codes and scale bytes equal oracle/mx_oracle.py's on a shared case (two statements of one rule, written apart);
  * K smoothing is an identity in exact arithmetic;
  * on every input family the restatement's own emulation of the kernel stays inside the element bound and the 1.5 * Y bound the GPU test applies to
    the kernel (Y is that emulation's error, so the second holds by construction; the first is a property of the arithmetic, not of the code
    under test);
  * the flush term matters: an emulation that rounds P without the 2^8 shift leaves the bound on the sea family;
  * every new entry answers X2V_E_* before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attn_mx_ref as M
from tests import attn_ref as A

HOST_SHAPES = ((33, 33), (129, 129), (257, 200), (33, 1576))  # (Sq, Sk): one tile, a masked second tile, rectangular, the long sea


def test_restated_mxfp8_equals_the_oracle():
    from oracle import mx_oracle as O

    g = torch.Generator().manual_seed(11)
    x = (torch.randn(37, 256, generator=g) * torch.exp2(torch.randint(-20, 12, (37, 1), generator=g).float())).to(torch.bfloat16)
    x[3, :32] = 0  # an all-zero block
    x[5, 40] = 448.0 * 2.0 ** 3  # amax exactly 448 * 2^k: the scale's upper edge
    q, sc = O.quant_mxfp8(x)
    codes, byte = M.quant_rows(x.float().numpy())
    assert np.array_equal(byte, sc.numpy())
    assert np.array_equal(codes, q.view(torch.uint8).numpy())
    assert np.array_equal(M.deq_rows(codes, byte), O.dequant(q, sc).numpy())


def test_e4m3_round_trip_and_ties():
    codes = np.arange(256, dtype=np.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    vals = M.e4m3_values(codes)
    assert np.array_equal(M.e4m3_codes(vals), codes)
    assert abs(vals).max() == 448.0 and abs(vals[vals != 0]).min() == 2.0 ** -9
    # ties go to the even code: halfway between 2^-9 * {0, 1, 2}, and between 1.0 and 1.125
    assert list(M.e4m3_codes(np.array([2.0 ** -10, 3 * 2.0 ** -10, 1.0625, 1.1875]))) == [0, 2, 0x38, 0x3A]
    # the P operand: 1.0 is code value 256; 2^-17 is the smallest positive code; 2^-18 is flushed
    p = np.array([1.0, 2.0 ** -17, 2.0 ** -18, 1.5 * 2.0 ** -18])
    assert list(M.e4m3_values(M.e4m3_codes(p * 2.0 ** M.P_SHIFT)) * 2.0 ** -M.P_SHIFT) == [1.0, 2.0 ** -17, 0.0, 2.0 ** -17]


def test_smoothing_is_an_identity_in_exact_arithmetic():
    inp = M.MxInputs("offset", 65, 200, 2)
    q, k, v = (t.to(torch.float64) for t in (inp.q, inp.k, inp.v))
    mean = k.mean(1, keepdim=True)
    f = float(M.q_scale())
    soft = lambda s: torch.softmax(s * f * 0.6931471805599453, -1)
    a, b = soft(q @ k.transpose(1, 2)) @ v, soft(q @ (k - mean).transpose(1, 2)) @ v
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    # and the contract's fp32 mean is the float64 mean within the fp32 summation bound
    m32 = M.kmean32(inp.k)
    assert np.all(np.abs(m32 - mean[:, 0].numpy()) <= inp.Sk * 2.0 ** -24 * np.abs(k.numpy()).mean(1) + 2.0 ** -24 * np.abs(mean[:, 0].numpy()))


@pytest.mark.parametrize("Sq,Sk", HOST_SHAPES)
def test_restatement_stays_inside_its_own_bounds(Sq, Sk):
    for fam, spike in M.families():
        inp = M.MxInputs(fam, Sq, Sk, M.H_TEST, spike)
        for prescaled in (False, True):
            r = M.restated(inp, prescaled)
            err = (r.emulated.to(torch.float64) - r.o).abs()
            assert torch.isfinite(r.emulated.float()).all()
            assert bool((err <= r.tol()).all()), f"{inp.name} prescaled={prescaled}: worst d/tol {float((err / r.tol().clamp_min(1e-300)).max()):.3f}"
            assert A.rel_l2(r.emulated, r.o) <= M.TRIANGLE * r.Y


def test_padding_rules_of_the_restated_operands():
    inp = M.MxInputs("R", 33, 200, 2)
    r = M.restated(inp)
    assert r.k_codes.shape == (2, 256, 128) and not r.k_codes[:, 200:].any() and not r.k_scales[:, 200:].any()
    assert r.vt_codes.shape == (2, 2, 128, 128) and not r.vt_codes[:, 1, :, 72:].any()
    assert not r.vt_scales[:, 1, :, 3].any() and r.vt_scales.max() < 0xFF  # keys 224..255: a block with no key has byte 0
    # the partly filled block (keys 192..199 of 192..223) takes its amax from the real keys only
    blk = inp.v[:, 192:200].float().abs().amax(1).numpy()
    assert np.array_equal(r.vt_scales[:, 1, :, 2], M.e8m0_byte(blk))


def test_an_unshifted_p_operand_leaves_the_bound_on_the_sea():
    """The rejection this family is for: P rounded to e4m3 at scale 1 (smallest positive code 2^-9) flushes every sea key (P ~ 2^-10)."""
    inp = M.MxInputs("sea", 33, 1576, 2)
    r = M.restated(inp)
    s = (r.qd @ r.kd.transpose(1, 2))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ph = torch.from_numpy(M.e4m3_values(M.e4m3_codes(p.numpy())))
    bad = (ph @ r.vd) / p.sum(-1, keepdim=True)
    assert not bool(((bad - r.o).abs() <= r.tol()).all())
    w = p / p.sum(-1, keepdim=True)
    assert float(w[:, :, 1576 // 2].max()) < 0.5, "the sea must hold most of the weight"


def test_argument_validation_needs_no_gpu():
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    sizes = (ctypes.c_int64 * 7)()
    assert L.x2v_attn_mx_sizes(300, 200, 2, sizes) == 0
    assert list(sizes) == [2 * 300 * 128, 2 * 300 * 4, 2 * 256 * 128, 2 * 256 * 4, 2 * 2 * 16384, 2 * 2 * 512, (1 + 1) * 256 * 4]
    assert lib.attention_mx_sizes(300, 200, 2) == tuple(sizes)
    assert L.x2v_attn_mx_sizes(300, 200, 2, None) == -5
    assert L.x2v_attn_mx_sizes(-1, 200, 2, sizes) == -1 and L.x2v_attn_mx_sizes(1, 1 << 24, 2, sizes) == -1 and L.x2v_attn_mx_sizes(1, 1, 0, sizes) == -1
    with pytest.raises(lib.X2VError):
        lib.attention_mx_sizes(1, 1, 0)
    # x2v_attn_mx_kmean_f32(k, ldk, kmean, Sk, H, stream)
    assert L.x2v_attn_mx_kmean_f32(None, 256, a, 4, 2, None) == -5
    assert L.x2v_attn_mx_kmean_f32(a, 256, a, 0, 2, None) == -1
    assert L.x2v_attn_mx_kmean_f32(a, 255, a, 4, 2, None) == -2 and L.x2v_attn_mx_kmean_f32(a, 128, a, 4, 2, None) == -2  # odd stride; stride < H * 128
    # x2v_attn_mx_quant_qk(x, ldx, mean, smooth, scale, codes, scales, S, S_pad, H, stream)
    assert L.x2v_attn_mx_quant_qk(a, 256, None, 1, 1.0, a, a, 4, 4, 2, None) == -5  # smoothing without the mean
    assert b"mean" in L.x2v_last_error()
    assert L.x2v_attn_mx_quant_qk(a, 256, None, 0, 1.0, None, a, 4, 4, 2, None) == -5
    assert L.x2v_attn_mx_quant_qk(a, 256, None, 0, 1.0, a, a, 5, 4, 2, None) == -1  # S_pad < S
    assert L.x2v_attn_mx_quant_qk(a, 260, None, 0, 1.0, a, a, 4, 4, 2, None) == -2 and L.x2v_attn_mx_quant_qk(odd, 256, None, 0, 1.0, a, a, 4, 4, 2, None) == -2
    assert L.x2v_attn_mx_quant_qk(a, 256, None, 0, 1.0, a, a, 0, 0, 2, None) == 0  # no rows: nothing launched
    # x2v_attn_mx_quant_vt(v, ldv, codes, scales, Sk, H, stream)
    assert L.x2v_attn_mx_quant_vt(a, 256, None, a, 4, 2, None) == -5
    assert L.x2v_attn_mx_quant_vt(a, 256, a, a, 0, 2, None) == -1
    assert L.x2v_attn_mx_quant_vt(a, 252, a, a, 4, 2, None) == -2
    # x2v_attn_mx_fwd(q_codes, q_scales, k_codes, k_scales, vt_codes, vt_scales, o, ldo, Sq, Sk, H, stream)
    assert L.x2v_attn_mx_fwd(a, a, a, a, a, None, a, 256, 4, 4, 2, None) == -5
    assert L.x2v_attn_mx_fwd(a, a, a, a, a, a, a, 256, 4, 0, 2, None) == -1  # no keys
    assert b"no keys" in L.x2v_last_error()
    assert L.x2v_attn_mx_fwd(a, a, a, a, a, a, a, 258, 4, 4, 2, None) == -2 and L.x2v_attn_mx_fwd(a, a, a, a, a, a, a, 128, 4, 4, 2, None) == -2
    assert L.x2v_attn_mx_fwd(a, a, a, a, a, a, a, 256, 0, 4, 2, None) == 0  # no queries: a no-op
    assert L.x2v_attn_mx_fwd(a, a, a, a, a, a, a, 256, 4, 4, 2000, None) == -1


def test_operator_is_registered_under_its_own_key_only():
    from lightx2v_amd import ops, registry

    assert registry.ATTN_WEIGHT_REGISTER["hip_mxfp8"] is ops.HipMxfp8AttnWeight
    assert "sage_attn2" not in registry.ATTN_WEIGHT_REGISTER


def test_python_entries_refuse_host_tensors():
    """No CPU fall-back: a host tensor is an error whether or not a GPU is present."""
    from lightx2v_amd import lib

    x = torch.zeros(8, 256, dtype=torch.bfloat16)
    with pytest.raises(lib.X2VError):
        lib.attention_mx(x, x, x, 2)
    with pytest.raises(lib.X2VError):
        lib.attention_mx_prepare(x, x, x, 2)
