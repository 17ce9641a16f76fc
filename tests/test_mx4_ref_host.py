"""tests/mx4_ref.py checked without a GPU: the e2m1 element and its packing against values worked out by hand and against the rounding table of the
reference's fake quantiser, the divisor-6 argument against exact rational arithmetic, the premises of family I for every shape the GPU module uses, an
fp32 emulation of a correct kernel inside every check of both families, the emulations of a subtly WRONG kernel or quantiser each rejected, and the
argument validation of the new entries through ctypes (no device).  The rejections this module prints (pytest -s) are the evidence that
tests/test_gpu_mx4.py would fail on such a kernel: deliberately broken kernels are never run on a GPU."""
import ctypes
from fractions import Fraction

import pytest
import torch

from tests import gemm_ref as G
from tests import mx4_ref as R
from tests import mx_ref as X

SHAPE = (300, 264, 512)  # M, N, K of the rejection tests: mx_ref's host module's


# ------------------------------------------------------------------------------------------------------------------- element, packing, scale
def test_e2m1_by_hand():
    f = lambda *v: torch.tensor(v, dtype=G.F64)
    every = torch.arange(16, dtype=torch.uint8)
    vals = R.e2m1_values(every)
    assert torch.equal(R.e2m1_codes(vals), every)  # all 16 codes round-trip, -0 included
    assert vals[:8].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0] and vals[8:].tolist() == [-0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    # the reference's fake quantiser (lightx2v_kernel/test/nvfp4_nvfp4/fake_quant.py:10-21): ties at 0.25, 1.25, 2.5 and 5 go down, at 0.75, 1.75 and
    # 3.5 up; anything above 5 is 6
    got = R.e2m1_values(R.e2m1_codes(f(0.25, 1.25, 2.5, 5.0, 0.75, 1.75, 3.5, 0.26, 0.74, 1.24, 1.26, 2.49, 2.51, 3.49, 4.99, 5.01, 6.0, 7.0, 1000.0, -1000.0)))
    assert got.tolist() == [0.0, 1.0, 2.0, 4.0, 1.0, 2.0, 4.0, 0.5, 0.5, 1.0, 1.5, 2.0, 3.0, 3.0, 4.0, 6.0, 6.0, 6.0, 6.0, -6.0]
    assert R.e2m1_codes(f(-0.0, 0.0, -0.25, 1.0, -1.0, 6.0)).tolist() == [0x8, 0x0, 0x8, 0x2, 0xA, 0x7]
    assert R.e2m1_codes(f(5.9, 0.9, -0.4, 3.9), rnd="trunc").tolist() == [0x6, 0x1, 0x8, 0x5] and R.e2m1_codes(f(-0.0, -0.25, -1.0), neg_zero=False).tolist() == [0, 0, 0xA]
    # every e2m1 number is an e4m3 number (what emulate() relies on)
    assert torch.equal(X.e4m3_values(X.e4m3_codes(vals)), vals)
    # 6 * 2^k -> 2^k exactly; one bf16 step above needs the next power; the denormal quotient 2^-127 -> byte 0, above it byte 1
    assert R.e8m0_byte(f(0.0, 6.0, 6.03125, 5.96875, 1.0, 6 * 2.0 ** -127, 6.03125 * 2.0 ** -127, 6 * 2.0 ** -126, 2.0 ** -133, 3.0e38)).tolist() == \
        [0, 127, 128, 127, 125, 0, 1, 1, 0, 253]
    assert R.e8m0_byte(f(6.03125, 5.96875, 6.0), "floor").tolist() == [127, 126, 127] and R.e8m0_byte(f(6.0, 28.0, 448.0), divisor=28.0).tolist() == [125, 127, 131]


def test_divisor_6_quotient_rounds_as_the_exact_one():
    """mx4_ref.e8m0_byte takes max|x| / 6 in float64 and rounds it to fp32.  For EVERY positive finite bf16 number the result equals the exact
    rational quotient rounded once to fp32 (nearest-even, denormals kept): the double rounding never shows."""
    bits = torch.arange(1, 0x7F80, dtype=torch.int32)
    x = X.bf16_bits(bits).to(G.F32).to(G.F64)
    got = X.round_fp32(x / 6.0).tolist()
    bad = 0
    for xv, g in zip(x.tolist(), got):
        q = Fraction(xv) / 6
        e = q.numerator.bit_length() - q.denominator.bit_length()
        e = max(e - 1 if Fraction(2) ** e > q else e, -126)  # floor(log2 q), held at the least normal exponent
        step = Fraction(2) ** (e - 23)
        n = q / step
        fl = n.numerator // n.denominator
        rem = n - fl
        fl += 1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1) else 0
        bad += Fraction(g) != fl * step
    assert bad == 0, f"{bad} of {len(got)} bf16 numbers: the float64 quotient by 6 rounds to another fp32 number than the exact one"


def test_pack4_is_the_little_endian_nibble_string():
    g = torch.Generator().manual_seed(4)
    codes = torch.randint(0, 16, (7, 256), generator=g).to(torch.uint8)
    got = R.pack4(codes)
    assert got.shape == (7, 128) and got.dtype == torch.uint8 and torch.equal(R.unpack4(got), codes)
    row = got[0].to(torch.int64)
    bits = sum(int(row[i]) << (8 * i) for i in range(128))  # the row as one little-endian bit string: code j at bits 4 j .. 4 j + 3
    assert [(bits >> (4 * j)) & 15 for j in range(256)] == codes[0].tolist()
    assert int(got[0, 0]) == int(codes[0, 0]) | (int(codes[0, 1]) << 4)
    assert not torch.equal(R.pack4(codes, "high_first"), got) and torch.equal(R.unpack4(R.pack4(codes, "high_first")), codes[:, torch.arange(256) ^ 1])
    every = torch.arange(256, dtype=torch.uint8).reshape(1, 256)
    assert torch.equal(R.pack4(R.unpack4(every)), every)  # and the other way round, every byte


def test_quant4_by_hand_and_pins():
    x = torch.zeros(2, 128, dtype=G.BF16)
    x[0, 0], x[0, 1], x[0, 2], x[0, 33], x[1, 64:96] = 6.0, -5.0, 0.25, 3.0, -0.0
    q, sc = R.quant4(x)
    assert sc.tolist() == [[127, 126, 0, 0], [0, 0, 0, 0]] and q[0, :3].tolist() == [0x7, 0xE, 0x0] and int(q[0, 33]) == 0x7  # 3 / 6 -> 2^-1, 3 * 2 = 6
    assert bool((q[1, 64:96] == 0x8).all())
    assert torch.equal(R.dequant4(q, sc)[0, :3], torch.tensor([6.0, -4.0, 0.0], dtype=G.F64)) and float(R.dequant4(q, sc)[0, 33]) == 3.0
    assert len(R.PINS) == 15
    want = {"6*2^0": (127, 0x7), "6.03125*2^0": (128, None), "5.96875*2^0": (127, 0x7), "1.5*2^-125": (0, 0x7), "1.5*2^-125 + 1 step": (1, None), "2^-126": (0, 0x4),
            "least subnormal": (0, 0x0), "largest finite": (253, None)}
    for pin, (byte, code) in want.items():
        xs, n = X.sweep(R.PINS[pin])
        assert n == 2 * (R.PINS[pin] + 1) and bool(torch.isfinite(xs.float()).all())
        q, sc = R.quant4(xs)
        assert int(sc[0, 0]) == byte and (code is None or int(q[0, 0]) == code), (pin, int(sc[0, 0]), hex(int(q[0, 0])))
    for M, K in X.QUANT_LAYOUT:
        x = R.quant_input(M, K)
        q, sc = R.quant4(x)
        assert int(sc[0, 0]) == 127 and bool((q[0, :32] == 0x7).all())
        if M > 2:
            assert int(sc[M // 2, 1]) == 0 and int(sc[M // 2, 0]) > 0 and bool((q[M - 1, K - 32 :] == 0x8).all())
    for M, K in R.QUANT_GRID:
        assert M * K // 16 > 4096 * 256 and K % 128 == 0 and M % 64


@pytest.mark.parametrize("mut", sorted(R.QUANT4_MUTATIONS))
def test_quantiser_mutations_differ(mut):
    """Divisors 28 and 448, e8m0 floor instead of ceil, truncation instead of round-to-nearest-even and '-0 -> +0' each change bytes of the sweep
    under 5.96875 and of the first layout input: the bit-for-bit comparison of the GPU module rejects them.  So does the other nibble order."""
    for x in (X.sweep(R.PINS["5.96875*2^0"])[0], R.quant_input(5, 256)):
        q, sc = R.quant4(x)
        mq, ms = R.quant4(x, **R.QUANT4_MUTATIONS[mut])
        nq, ns = int((R.pack4(q) != R.pack4(mq)).sum()), int((sc != ms).sum())
        print(f"{mut} on {tuple(x.shape)}: {nq} packed bytes and {ns} scale bytes differ")
        assert nq > 0 and (ns > 0) == (mut in ("e8m0_floor", "divisor_28", "divisor_448"))
        assert int((R.pack4(q) != R.pack4(q, "high_first")).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------- inputs
def test_family_r_operands_are_the_parents():
    """The subclass draws the parent's ramped x and W again from the parent's seed: quantised with mx_ref.quant they are the parent's a and b."""
    M, N, K = 5, 16, 256
    p = X.Inputs("R", M, N, K)
    g = G._gen(77, 1, M, N, K, 0, 0)
    torch.randint(0, 2, (1,), generator=g)
    ramp = torch.logspace(-3, 3, K // 32).repeat_interleave(32)
    x = (torch.randn(M, K, generator=g).to(G.BF16).to(G.F32) * ramp).to(G.BF16)
    w = ((torch.randn(N, K, generator=g) / K ** 0.5).to(G.BF16).to(G.F32) / ramp).to(G.BF16)
    assert torch.equal(X.quant(x)[0], p.a) and torch.equal(X.quant(w)[0], p.b) and torch.equal(X.quant(w)[1], p.sb)
    c = R.Inputs("R", M, N, K)
    assert torch.equal(R.quant4(x)[0], c.a) and torch.equal(R.quant4(w)[0], c.b) and c.a_packed.shape == (M, K // 2) and c.b_packed.shape == (N, K // 2)
    assert torch.equal(c.bias, p.bias) and c.alpha == p.alpha
    assert torch.equal(c.acc0, R.dequant4(c.a, c.sa) @ R.dequant4(c.b, c.sb).T) and not torch.equal(c.acc0, p.acc0)
    assert set((c.sb.to(torch.int64) - p.sb.to(torch.int64)).unique().tolist()) <= {6, 7}  # 448 / 6 = 74.7, between 2^6 and 2^7: the same block maxima
    gv = R.given(x, w, c.bias)
    assert torch.equal(gv.acc0, c.acc0) and torch.equal(gv.absacc0, c.absacc0) and gv.scaled(False).name.startswith("R mxfp4 5x16x256")


def test_family_i_premises_for_every_gpu_shape():
    """Family I is the parent's construction on e2m1 integers: the premises (exact fp32 sums at every order, fp32 numbers in front of every rounding,
    each rounding exercised) hold for both inputs of every shape at which tests/test_gpu_mx4.py runs it."""
    shapes = R.family_i_shapes()
    assert len(shapes) >= 25 and all(K % 256 == 0 for _, _, K in shapes)
    for M, N, K in shapes:
        for flat in (False, True):
            if (M, N, K) in R.AUTO and flat:
                continue
            inp = R.Inputs("I", M, N, K, flat_a=flat)
            s, ft, fp, fr = inp.assert_premises()
            assert s < 0.9
            assert int(inp.a.max()) < 16 and int(inp.b.max()) < 16 and float(R.e2m1_values(inp.b).abs().max()) == 4.0 and inp.b_packed.shape == (N, K // 2)
            if M * K >= 1 << 12:
                assert set(R.e2m1_values(inp.a).unique().tolist()) == {-6.0, -4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 6.0}
            if M * N <= 1 << 17:
                assert torch.equal(inp.acc0, R.dequant4(inp.a, inp.sa) @ R.dequant4(inp.b, inp.sb).T)
            print(f"{inp.name}: spread {inp.spread}, sum |terms| {s:.2f} of 2^24, inexact: t {ft:.1%}, gated product {fp:.1%}, resid + p {fr:.1%}")


# ------------------------------------------------------------------------------------------------------------------- emulations
def _views(fam, M, N, K):
    if fam == "R":
        inp = R.Inputs("R", M, N, K)
        return [(inp.scaled(True), True), (inp.scaled(False), False)]
    out = []
    for flat in (False, True):
        inp = R.Inputs("I", M, N, K, flat_a=flat)
        inp.assert_premises()
        out += [(inp.scaled(u), flat) for u in (False, True)]
    return out


def test_correct_emulation_passes_every_check():
    """Block-ordered fp32 accumulation on e2m1 operands, rounding and truncating: equal to family I's chain, inside every bound of family R."""
    case = G.Case("emulation", record=False)
    for M, N, K in (SHAPE, (136, 136, 256)):
        for fam in ("I", "R"):
            for v, use_bias in _views(fam, M, N, K):
                for epi, use_gate in X.EPILOGUES:
                    if fam == "I" and epi not in (G.EPI_NONE, G.EPI_RESIDUAL):
                        continue
                    exp = G.Expect(v, epi, use_bias, use_gate)
                    for truncating in (False, True):
                        case.check(R.emulate(v, epi, use_bias, use_gate, truncating=truncating), exp, f"emulation truncating={truncating}")
    print(f"{len(case.rows)} checks, largest d/tol {case.worst_ratio:.3f}")
    assert 0.0 < case.worst_ratio <= 1.0


def _rejected_by(mut, epi):
    M, N, K = SHAPE
    hits = []
    for fam in ("I", "R"):
        for v, use_bias in _views(fam, M, N, K):
            if mut in ("alpha_after_bias", "bias_after_rounding") and not (use_bias and v.alpha_used):
                continue
            try:
                G.Case("mutation", record=False).check(R.emulate(v, epi, use_bias, mut=mut), G.Expect(v, epi, use_bias), mut)
            except G.Reject as r:
                hits.append(fam)
                print(f"{v.name} {mut}: rejected by '{r.criterion}' — {r}")
    return set(hits)


@pytest.mark.parametrize("mut", sorted(X.GEMM_MUTATIONS) + list(R.GEMM4_MUTATIONS))
def test_gemm_mutations_are_rejected(mut):
    """mx_ref's ten wrong kernels, and the three of the 4-bit operands — the two codes of a weight byte exchanged, the two 32-code pieces of a 64-wide
    step exchanged, the second scale dword of a 256-wide K-tile replaced by the first: each rejected by family I; those that change the product by
    every family."""
    hits = _rejected_by(mut, X.GEMM_MUTATIONS.get(mut, G.EPI_NONE))
    assert "I" in hits
    if mut in ("scale_bytes_swapped", "scale_dword_late", "drop_last_tile", "k_tile_twice", "alpha_after_bias", "rowmajor_table_read_as_tiled", "truncate") + R.GEMM4_MUTATIONS:
        assert hits == {"I", "R"}


def test_one_hot_walk_tells_the_code_order():
    """The GPU module's diagnostic walks: with one operand one-hot at k0(row) and distinct integers along k on the other, a kernel that exchanges the
    nibbles of a byte returns the value at k0 ^ 1, one that exchanges the 32-code pieces the value at k0 ^ 32 — different from the value at k0 for
    every row, and k0 visits both nibbles of every byte."""
    K = 256
    k0 = (37 * torch.arange(264) + 5) % K
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0, -1.0, -2.0, -3.0, -4.0, -6.0, 0.0])[(3 * torch.arange(K)[None, :] + torch.arange(5)[:, None]) % 11]
    assert len(set(k0.tolist())) == K and {k % 2 for k in k0.tolist()} == {0, 1}
    for other in (1, 32, 64, 128):
        assert bool((x[:, k0] != x[:, k0 ^ other]).any(0).all()), other
    assert torch.equal(R.e2m1_values(R.e2m1_codes(x.double())), x.double())


# ------------------------------------------------------------------------------------------------------------------- argument validation
def test_argument_validation_needs_no_gpu():
    """The new entries check their arguments before any HIP call, with the library's error codes (-1 shape, -2 alignment, -5 argument)."""
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert {"x2v_quant_mxfp4_bf16", "x2v_gemm_mxfp4", "x2v_gemm_mxfp4_epi", "x2v_gemm_mxfp4_variant"} <= set(lib.PROTOTYPES)
    # x2v_quant_mxfp4_bf16(x, ldx, q, ldq, scales, M, K, stream)
    assert L.x2v_quant_mxfp4_bf16(a, 96, a, 48, a, 4, 96, None) == -1 and b"K=96" in L.x2v_last_error()
    assert L.x2v_quant_mxfp4_bf16(None, 128, a, 64, a, 4, 128, None) == -5
    assert L.x2v_quant_mxfp4_bf16(a, 128, odd, 64, a, 4, 128, None) == -2
    assert L.x2v_quant_mxfp4_bf16(a, 128, a, 56, a, 4, 128, None) == -2  # ldq below K/2
    assert L.x2v_quant_mxfp4_bf16(a, 128, a, 64, a, 0, 128, None) == 0  # no rows: nothing launched
    # x2v_gemm_mxfp4(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, stream)
    P = L.x2v_gemm_mxfp4
    assert P(a, 192, a, a, 192, a, None, None, a, 64, 4, 64, 384, None) == -1 and b"K=384" in L.x2v_last_error()  # K % 256
    assert P(a, 128, a, None, 128, a, None, None, a, 64, 4, 64, 256, None) == -5  # null operand
    assert P(None, 128, a, a, 128, a, None, None, a, 64, 4, 64, 256, None) == -5
    assert P(a, 128, None, a, 128, a, None, None, a, 64, 4, 64, 256, None) == -5  # null scale table
    assert P(a, 128, a, a, 128, a, None, None, a, 64, 4, 60, 256, None) == -1  # N % 8
    assert P(a, 128, a, odd, 128, a, None, None, a, 64, 4, 64, 256, None) == -2  # b not 16-byte aligned
    assert P(a, 128, a, a, 136, a, None, None, a, 64, 4, 64, 256, None) == -2  # ldb % 16
    assert P(a, 112, a, a, 128, a, None, None, a, 64, 4, 64, 256, None) == -2  # lda below K/2 bytes
    assert P(a, 128, a, a, 128, a, None, None, odd, 64, 4, 64, 256, None) == -2  # y
    # x2v_gemm_mxfp4_variant(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream)
    V = L.x2v_gemm_mxfp4_variant
    assert V(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 256, 3, None) == -5 and b"unknown variant" in L.x2v_last_error()
    assert V(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 256, -1, None) == -5
    assert V(a, 1 << 24, a, a, 128, a, None, None, a, 64, 4, 64, 256, 2, None) == -1  # the 256x256 body's 32-bit tile addressing
    # x2v_gemm_mxfp4_epi(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, epilogue, resid, ldr, gate, stream)
    E = L.x2v_gemm_mxfp4_epi
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 256, 2, None, 0, None, None) == -5 and b"resid" in L.x2v_last_error()  # residual epilogue without resid
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 256, 2, a, 60, None, None) == -2  # ldr below N
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 384, 0, None, 0, None, None) == -1


def test_operator_class_is_registered():
    from lightx2v_amd import lib, mx, ops, plugin, registry

    cls = registry.MM_WEIGHT_REGISTER["W-mxfp4-A-mxfp4-dynamic-Hip"]
    assert cls is ops.MMWeightMxfp4Hip and issubclass(cls, ops.MMWeightMxfp8Hip)
    op = cls("a.weight", "a.bias")
    assert op.weight is None and cls._gemm is lib.gemm_mxfp4 and cls.quantize_input is not ops.MMWeightMxfp8Hip.quantize_input
    assert callable(mx.scaled_mxfp4_quant) and callable(mx.scaled_mxfp4_mm)
    assert not hasattr(mx, "scaled_fp4_quant") and not hasattr(mx, "cutlass_scaled_fp4_mm")  # NVFP4's names: another scale format (module docstring)
    assert "W-mxfp4-A-mxfp4-dynamic-Hip" in open(plugin.__file__).read()
    with pytest.raises(lib.X2VError):
        op.load({"a.weight": torch.zeros(8, 256)})  # quantised by the HIP kernel: a CPU tensor is an error
    with pytest.raises(lib.X2VError):  # the shared checks: a row of a holds K/2 bytes, K % 256 == 0
        lib.gemm_mxfp4(torch.zeros(4, 64, dtype=torch.uint8), None, torch.zeros(8, 64, dtype=torch.uint8), None)
