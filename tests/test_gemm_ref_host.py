"""tests/gemm_ref.py checked without a GPU: the float64 references against a row computed by hand, the premises of family I (exact fp32 sums,
enough inexact values in front of every rounding), both Lipschitz constants, an fp32 emulation of a correct kernel inside every check of both
families, and eleven emulations of a subtly WRONG kernel each rejected by the check named for it.  The rejections this module prints (pytest -s)
are the evidence that tests/test_gpu_gemm_fp64.py would fail on such a kernel: deliberately broken kernels are never run on a GPU."""
import pytest
import torch

from tests import gemm_ref as G

SHAPE = (300, 264, 256)  # M, N, K of the rejection tests: two m-tiles and two n-tiles of either tile size, both ragged


def test_round_bf16_is_one_rounding_to_nearest_even():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, 259.0, -257.0, 1.0 + 2.0 ** -8 + 2.0 ** -40, 0.0, 3.0e-5], dtype=G.F64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 256.0, 260.0, -256.0, 1.0 + 2.0 ** -7, 0.0, float(torch.tensor(3.0e-5).to(G.BF16))], dtype=G.F64)
    assert torch.equal(G.round_bf16(t), want)
    assert float(torch.tensor(1.0 + 2.0 ** -8 + 2.0 ** -40, dtype=G.F64).to(G.F32).to(G.BF16)) == 1.0  # what a detour through fp32 would give
    assert torch.equal(G.round_bf16(t[:6], "half_up"), torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, 258.0, 260.0, -256.0], dtype=G.F64))
    assert torch.equal(G.round_bf16(t[:6], "trunc"), torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -7, 256.0, 258.0, -256.0], dtype=G.F64))
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)).to(G.F64) * 37
    assert torch.equal(G.round_bf16(v.to(G.F32).to(G.F64)), v.to(G.F32).to(G.BF16).to(G.F64))  # on fp32 numbers it is torch's conversion


def test_reference_chain_by_hand():
    """One element through every epilogue with numbers small enough to follow: t = 3 * 43 + 2 * 64.5 + 0.5 = 258.5."""
    inp = G.Inputs("I", "bf16", 1, 8, 64)
    inp.x, inp.w = torch.zeros(1, 64, dtype=G.BF16), torch.zeros(8, 64, dtype=G.BF16)
    inp.x[0, 0], inp.x[0, 63], inp.w[0, 0], inp.w[0, 63] = 3.0, 2.0, 43.0, 64.5
    inp.acc = inp.x.double() @ inp.w.double().T
    inp.bias, inp.gate, inp.resid = torch.full((8,), 0.5, dtype=G.BF16), torch.full((8,), 1.5, dtype=G.BF16), torch.full((1, 8), 3.0, dtype=G.BF16)
    assert float(inp.t()[0, 0]) == 258.5
    assert float(G.Expect(inp, G.EPI_NONE).exact[0, 0]) == 258.0  # 8 bits: steps of 2 above 256; 258.5 -> 258
    assert float(G.Expect(inp, G.EPI_NONE, use_bias=False).exact[0, 0]) == 258.0
    assert float(G.Expect(inp, G.EPI_RESIDUAL).exact[0, 0]) == 392.0  # 258 * 1.5 = 387 -> 388 (tie to even, steps of 4: 384 | 388); 3 + 388 = 391 -> 392
    assert float(G.Expect(inp, G.EPI_RESIDUAL, use_gate=False).exact[0, 0]) == 260.0  # 3 + 258 = 261 -> 260 (tie to even)
    inp.family, inp.absacc = "R", inp.x.double().abs() @ inp.w.double().abs().T
    e = G.Expect(inp, G.EPI_NONE)
    assert float(e.f[0, 0]) == 258.5 and float(e.tol[0, 0]) == pytest.approx(2.0 ** -8 * 258.5 + (1 + 2.0 ** -8) * 65 * 2.0 ** -23 * 258.5, rel=1e-14)
    e = G.Expect(inp, G.EPI_RESIDUAL)
    e0 = 2.0 ** -8 * 258.5 + (1 + 2.0 ** -8) * 65 * 2.0 ** -23 * 258.5
    e1 = 1.5 * e0 + 2.0 ** -8 * (387.75 + 1.5 * e0)
    assert float(e.f[0, 0]) == 390.75 and float(e.tol[0, 0]) == pytest.approx(e1 + 2.0 ** -8 * (390.75 + e1), rel=1e-14)
    e = G.Expect(inp, G.EPI_SILU)
    tol = 1.10 * e0 + 2.0 ** -16 * 258.5
    assert float(e.f[0, 0]) == pytest.approx(258.5, rel=1e-14) and float(e.tol[0, 0]) == pytest.approx(tol + 2.0 ** -8 * (258.5 + tol), rel=1e-14)


def test_w8a8_reference_scales_rows_and_columns():
    inp = G.Inputs("R", "e4m3", 5, 16, 128)
    x, w = inp.x.float().double(), inp.w.float().double()
    t = torch.stack([torch.stack([(x[m] * w[n]).sum() * float(inp.sx[m]) * float(inp.sw[n]) + float(inp.bias[n]) for n in range(16)]) for m in range(5)])
    assert torch.allclose(inp.t(), t, rtol=1e-13, atol=1e-15)
    e = G.Expect(inp, G.EPI_NONE)
    S = torch.stack([torch.stack([(x[m] * w[n]).abs().sum() * float(inp.sx[m]) * float(inp.sw[n]) + abs(float(inp.bias[n])) for n in range(16)]) for m in range(5)])
    assert torch.allclose(e.tol, 2.0 ** -8 * t.abs() + (1 + 2.0 ** -8) * 131 * 2.0 ** -23 * S, rtol=1e-13)
    i = G.Inputs("I", "int8", 5, 16, 128)
    assert set(i.sx.tolist()) <= {0.5, 1.0, 2.0} and set(i.sw.tolist()) <= {0.25, 0.5, 1.0} and int(i.x.abs().max()) <= 8 and int(i.w.abs().max()) <= 4
    f = G.Inputs("I", "e4m3", 5, 16, 128)
    assert torch.equal(f.x.float(), f.x.float().round()) and float(f.x.float().abs().max()) <= 8


def test_lipschitz_constants():
    lg, ls = G.lipschitz(G.gelu64), G.lipschitz(G.silu64)
    print(f"max |gelu_tanh'| = {lg:.6f}, max |silu'| = {ls:.6f}")
    assert lg <= G.L_GELU < lg + 0.005 and ls <= G.L_SILU < ls + 0.005


@pytest.mark.parametrize("dtype,K", [(d, K) for d in G.DTYPES for K in (64, 128, 256, 1024, 13824) if K % G.KTILE[d] == 0])
def test_family_i_exercises_the_roundings(dtype, K):
    inp = G.Inputs("I", dtype, 257, 256, K)
    ft, fp = inp.assert_exercises_roundings()
    mid = G.Expect(inp, G.EPI_RESIDUAL).exact
    no_mid = G.round_bf16(inp.resid_rows() + G.round_bf16(inp.t()) * inp.gate.double()[None, :]).to(G.F32).to(G.BF16)
    diff = float((mid != no_mid).double().mean())
    print(f"{inp.name}: bias range {inp.bias_range}, acc + bias inexact {ft:.1%}, gated product inexact {fp:.1%}, chain differs from the chain without the middle rounding on {diff:.1%}")
    assert diff >= 0.01


def _emulation_passes(inp, case):
    for epi, use_bias, use_gate in G.EPILOGUES:
        if inp.family == "I" and epi not in (G.EPI_NONE, G.EPI_RESIDUAL):
            continue
        exp = G.Expect(inp, epi, use_bias, use_gate)
        for chunk in (0, 16):
            case.check(G.emulate(inp, epi, use_bias, use_gate, chunk=chunk), exp, f"emulation chunk={chunk}")


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_correct_emulation_passes_every_check(dtype):
    """fp32 accumulation, whole and in 16-wide k chunks, plus the contract's roundings: inside every bound of family R, equal to family I's chain."""
    case = G.Case("emulation", record=False)
    M, N, K = SHAPE
    for K_ in (K, 1024):
        for fam in ("I", "R"):
            _emulation_passes(G.Inputs(fam, dtype, M, N, K_), case)
    inp = G.Inputs("I", dtype, 600, 264, G.mid_k(dtype), resid_rows=264)
    for period in (7, 264):
        cut = G.Inputs("I", dtype, 600, 264, G.mid_k(dtype), resid_rows=period) if period != 264 else inp
        case.check(G.emulate(cut, G.EPI_RESIDUAL, period=period), G.Expect(cut, G.EPI_RESIDUAL, period=period), "emulation periodic")
    print(f"{dtype}: {len(case.rows)} checks, largest d/tol {case.worst_ratio:.3f}")
    assert 0.5 < case.worst_ratio <= 1.0  # the half-ulp term dominates: a correct kernel sits just under 1


def test_deep_k_family_i_emulation():
    inp = G.Inputs("I", "bf16", *G.DEEP)
    inp.assert_exercises_roundings()
    _emulation_passes(inp, G.Case("emulation", record=False))


def _rejected(inp, mut, epi, chunk=0):
    with pytest.raises(G.Reject) as r:
        G.Case("mutation", record=False).check(G.emulate(inp, epi, chunk=chunk, mut=mut), G.Expect(inp, epi), mut)
    print(f"{inp.name} {mut}: rejected by '{r.value.criterion}' — {r.value}")
    return r.value.criterion


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("mut", sorted(G.R_MUTATIONS))
def test_family_r_rejects(dtype, mut):
    """Family R at K = 256 rejects, with the epilogue named in gemm_ref.R_MUTATIONS: one k element dropped, two k columns of W swapped, bias or gate
    shifted by one column, the residual one row off, the accumulator rounded to bf16 before the bias add, truncation in place of round-to-nearest."""
    M, N, _ = SHAPE
    assert _rejected(G.Inputs("R", dtype, M, N, 256), mut, G.R_MUTATIONS[mut]) == "bound"


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("mut", sorted(G.I_MUTATIONS))
def test_family_i_rejects(dtype, mut):
    """Family I rejects: the residual without its middle rounding, round-half-up, one K tile of 64 read twice with its neighbour skipped, an output
    tile quadrant written 128 rows too low."""
    M, N, K = SHAPE
    inp = G.Inputs("I", dtype, M, N, K)
    inp.assert_exercises_roundings()
    assert _rejected(inp, mut, G.I_MUTATIONS[mut]) == "exact"


def test_gpu_lists():
    assert all(G.accepts("bf16", 5, 256, 64 * nk) for nk in G.K_TILES_CONT) and not any(G.accepts("bf16", 5, 256, 64 * nk) for nk in (1, 2, 3, 5))
    assert not G.accepts("e4m3", 5, 264, 1024) and G.accepts("int8", 5, 512, 512) and G.accepts("bf16", 4, 264, 64)
    for cus in (256, 304, 64):
        for ntn in (1, 2):
            a, b = G.persistent_ms(cus, ntn)
            assert -(-a // 256) * ntn >= cus + 1 > (-(-a // 256) - 1) * ntn and -(-b // 256) * ntn >= 2 * cus + 3 and a % 256 and b % 256
    assert (-(-G.VT_SHAPE[0] // 256)) * (G.VT_SHAPE[1] // 256) == 192 and G.VT_SHAPE[1] % 128 == 0 and G.VT_SHAPE[2] // 64 == 8 and G.VT_SHAPE[0] % 64
    assert -(-G.BLOCKED_M // 256) * 2 == 192
    assert -(-G.SCHED_MN[0] // 256) * (G.SCHED_MN[1] // 256) == 27
