"""The residual row period of the gated-residual GEMM epilogue (x2v_gemm_bf16_resid_period / x2v_gemm_fp8_resid_period): output row r combines with
row r mod resid_period of resid.  The bytes written must EQUAL those of the same GEMM given the residual materialised by concatenation — same MFMA,
same k order, same rounding point, only the address of the residual chunk differs — so every comparison here is torch.equal, no tolerance.

Shapes: the smallest at which each kernel that serves the epilogue can go wrong.
  continuous 256x256 (gemm256c / gemm256c8): >= 192 tiles and 8 K tiles; period 3200 = 12.5 tiles, so the period boundary falls inside a 256-row
      tile (between its two wave rows); period 3208, a multiple of 8 only, puts it inside a wave's part and inside a 16- / 32-row block of the
      epilogue walk, between two residual chunks; M = 2 periods; an odd last tile (M % 256 != 0).
  one tile per workgroup (gemm256s, bf16) / ping-pong (gemm256, w8a8): the same M and N at a K the continuous form does not take (an odd number of
      K tiles), and periods that are no multiple of 8 (an odd one included) at the continuous shape, which the dispatcher hands to them.
  128x128 (gemm.hip): M = 2 x 200, N = 256, one K tile.
y is a window of a larger poisoned buffer (rows behind M, columns behind N): nothing outside M x N may change."""
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0x7FC1  # a NaN pattern no kernel produces


def _operands(M, N, K, period, fp8, seed):
    from lightx2v_amd import lib

    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).cuda()
    bias = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
    gate = torch.randn(N, generator=g).to(torch.bfloat16).cuda()
    resid = torch.randn(period, N, generator=g).to(torch.bfloat16).cuda()
    if fp8:
        xq, sx = lib.quant_fp8_rowwise(x)
        wq, sw = lib.quant_fp8_rowwise(w)
        return (xq, sx, wq, sw), bias, gate, resid
    return (x, w), bias, gate, resid


def _window(t):
    """t as a window of a buffer with y's row stride (N + 8): the continuous kernels address the residual with y's offsets."""
    wide = torch.zeros((t.shape[0], t.shape[1] + 8), dtype=t.dtype, device=t.device)
    wide[:, : t.shape[1]].copy_(t)
    return wide[:, : t.shape[1]]


def _run(ops, bias, gate, resid, M, N, fp8, variant=0, resid_period=0):
    """The GEMM into an M x N window of a poisoned [M + 8, N + 8] buffer; returns (window copy, whole buffer as int16)."""
    from lightx2v_amd import lib

    resid = _window(resid)
    big = torch.full((M + 8, N + 8), POISON, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    out = big[:M, :N]
    if fp8:
        xq, sx, wq, sw = ops
        lib.gemm_fp8(xq, sx, wq, sw, bias, epilogue=lib.EPI_RESIDUAL, resid=resid, gate=gate, out=out, variant=variant, resid_period=resid_period)
    else:
        lib.gemm(ops[0], ops[1], bias, epilogue=lib.EPI_RESIDUAL, resid=resid, gate=gate, out=out, variant=variant, resid_period=resid_period)
    torch.cuda.synchronize()
    return out.clone(), big.view(torch.int16)


def _check(M, N, K, periods, fp8, variant=0, with_gate=True):
    for period in periods:
        ops, bias, gate, resid = _operands(M, N, K, period, fp8, seed=M + N + K + period)
        gate = gate if with_gate else None
        reps = (M + period - 1) // period
        cat = torch.cat([resid] * reps)[:M].contiguous()
        want, _ = _run(ops, bias, gate, cat, M, N, fp8, variant)  # the plain entry on the concatenated residual
        got, big = _run(ops, bias, gate, resid, M, N, fp8, variant, resid_period=period)
        assert torch.isfinite(want.float()).all()
        same = torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert same, f"M={M} N={N} K={K} period={period} fp8={fp8} variant={variant}: {(got.view(torch.int16) != want.view(torch.int16)).sum().item()} elements differ"
        assert (big[M:] == POISON).all() and (big[:, N:] == POISON).all(), f"period={period}: wrote outside M x N"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "w8a8"])
def test_continuous_kernels(fp8):
    from lightx2v_amd import lib

    N, K = 2048, 1024 if fp8 else 512
    M = 2 * 3200
    assert lib.gemm_kernel_choice(M, N, K, fp8=fp8, with_form=True) == (2 if fp8 else 3, True)
    _check(M, N, K, (3200, 3208, M), fp8)  # inside a tile / a multiple of 8 only / the plain call
    _check(M, N, K, (3200,), fp8, with_gate=False)
    _check(M - 56, N, K, (3200,), fp8)  # an odd last tile: M % 256 = 200, the second period cut short
    _check(M, N, K, (3200,), fp8, variant=5)  # the continuous form, forced


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "w8a8"])
def test_one_tile_per_workgroup_kernels(fp8):
    from lightx2v_amd import lib

    N, K = 2048, (1024 + 128) if fp8 else (512 + 64)  # an odd number of K tiles: not the continuous form
    M = 2 * 3200
    assert lib.gemm_kernel_choice(M, N, K, fp8=fp8, with_form=True) == (2 if fp8 else 3, False)
    _check(M, N, K, (3200, M), fp8)
    _check(M - 56, N, K, (3199,), fp8)  # an odd period: every row on its own
    # periods the continuous kernels do not take go to this form at the continuous shape too (bf16: forced as well)
    Kc = 1024 if fp8 else 512
    _check(M, N, Kc, (3204, 3199, 100), fp8)
    _check(M, N, Kc, (3200,), fp8, variant=2 if fp8 else 4)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "w8a8"])
def test_128_tile_kernel(fp8):
    from lightx2v_amd import lib

    M, N, K = 2 * 200, 256, 128
    assert lib.gemm_kernel_choice(M, N, K, fp8=fp8) == 1
    _check(M, N, K, (200, M, 7), fp8)
    _check(M - 3, N, K, (200,), fp8, with_gate=False)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "w8a8"])
def test_period_zero_is_the_plain_entry_and_bad_periods_are_refused(fp8):
    """resid_period = 0 through the new entry = the existing entry on the same inputs (the kernels of X2V_EPI_RESIDUAL are instruction-identical to
    their parents, profiles/gemm_resid_period_isa.txt); a y that overlaps resid and a forced continuous form with a period it cannot take are errors."""
    import ctypes

    from lightx2v_amd import lib

    M, N, K = 512, 256, 512
    ops, bias, gate, resid = _operands(M, N, K, M, fp8, seed=5)
    want, _ = _run(ops, bias, gate, resid, M, N, fp8)
    resid = _window(resid)
    L, st = lib._lib, lib._stream()
    big = torch.full((M + 8, N + 8), POISON, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    out = big[:M, :N]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    if fp8:
        xq, sx, wq, sw = ops
        call = lambda y, r, period, variant=0: L.x2v_gemm_fp8_resid_period(p(xq), K, p(sx), p(wq), K, p(sw), p(bias), p(y), y.stride(0), M, N, K, p(r), r.stride(0), period, p(gate), variant, st)
    else:
        call = lambda y, r, period, variant=0: L.x2v_gemm_bf16_resid_period(p(ops[0]), K, p(ops[1]), K, p(bias), p(y), y.stride(0), M, N, K, p(r), r.stride(0), period, p(gate), variant, st)
    assert call(out, resid, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert (big.view(torch.int16)[M:] == POISON).all() and (big.view(torch.int16)[:, N:] == POISON).all()
    assert call(resid, resid, 256) == -5 and b"overlap" in L.x2v_last_error()
    assert call(out, resid, 260, 5) == -1 and b"resid_period" in L.x2v_last_error()  # forced continuous form: multiples of 8 only
    assert call(out, resid, -1) == -1
