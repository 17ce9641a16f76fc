"""tests/mx6_ref.py checked without a GPU: the e3m2 element and its packing against values worked out by hand and against the byte formulas of the
reference's packing comment, the premises of family I for every shape the GPU module uses, an fp32 emulation of a correct kernel inside every check
of both families, the emulations of a subtly WRONG kernel or quantiser each rejected, and the argument validation of the new entries through ctypes
(no device).  The rejections this module prints (pytest -s) are the evidence that tests/test_gpu_mx6.py would fail on such a kernel: deliberately
broken kernels are never run on a GPU."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G
from tests import mx6_ref as R
from tests import mx_ref as X

SHAPE = (300, 264, 512)  # M, N, K of the rejection tests: mx_ref's host module's


# ------------------------------------------------------------------------------------------------------------------- element, packing, scale
def test_e3m2_by_hand():
    f = lambda *v: torch.tensor(v, dtype=G.F64)
    every = torch.arange(64, dtype=torch.uint8)
    vals = R.e3m2_values(every)
    assert torch.equal(R.e3m2_codes(vals), every)  # all 64 codes round-trip, -0 included
    assert vals[:8].tolist() == [0.0, 0.0625, 0.125, 0.1875, 0.25, 0.3125, 0.375, 0.4375] and float(vals[31]) == 28.0 and float(vals[63]) == -28.0
    assert sorted(set(vals.abs().tolist()))[-3:] == [20.0, 24.0, 28.0] and {float(i) for i in range(-7, 8)} <= set(vals.tolist())
    # ties to even: 26 -> 24, 2^-5 -> 0, 3 * 2^-5 -> 2 * 2^-4, 0.21875 -> 0.25 (into the normal range), 7.5 -> 8; saturation at +/-28; signed zero
    got = R.e3m2_values(R.e3m2_codes(f(26.0, 0.03125, 0.09375, 0.21875, 7.5, 6.5, 30.0, 1000.0, -1000.0, 27.9)))
    assert got.tolist() == [24.0, 0.0, 0.125, 0.25, 8.0, 6.0, 28.0, 28.0, -28.0, 28.0]
    assert R.e3m2_codes(f(-0.0, 0.0, -0.03125, 1.0, -1.0)).tolist() == [0x20, 0x00, 0x20, 0x0C, 0x2C]
    assert R.e3m2_codes(f(26.0, 27.9, -0.05), rnd="trunc").tolist() == [0x1E, 0x1E, 0x20] and R.e3m2_codes(f(-0.0, -0.03125, -1.0), neg_zero=False).tolist() == [0, 0, 0x2C]
    # the other 6-bit format decodes the same bits differently: 0x0C is 1.0 in e3m2 and 1.5 in e2m3
    assert float(R.e2m3_values(torch.tensor([0x0C]))) == 1.5 and float(R.e2m3_values(torch.tensor([0x1F]))) == 7.5
    # 28 * 2^k -> 2^k exactly; one bf16 step above needs the next power; the denormal quotient 2^-127 -> byte 0, above it byte 1
    assert R.e8m0_byte(f(0.0, 28.0, 28.125, 27.875, 1.0, 28 * 2.0 ** -127, 28.125 * 2.0 ** -127, 28 * 2.0 ** -126, 2.0 ** -133, 3.0e38)).tolist() == \
        [0, 127, 128, 127, 123, 0, 1, 1, 0, 251]
    assert R.e8m0_byte(f(28.125, 27.875, 28.0), "floor").tolist() == [127, 126, 127] and R.e8m0_byte(f(28.0, 448.0), divisor=448.0).tolist() == [123, 127]


def test_pack6_equals_the_reference_byte_formulas():
    """The reference packs codes a, b, c, d (one per byte of its converter's output) as byte0 = b << 6 | a, byte1 = c << 4 | b >> 2,
    byte2 = d << 2 | c >> 4, each truncated to 8 bits (mxfp6_quant_kernels_sm120.cu:74-99)."""
    g = torch.Generator().manual_seed(6)
    codes = torch.randint(0, 64, (7, 256), generator=g).to(torch.uint8)
    a, b, c, d = (codes.reshape(7, 64, 4)[..., i].to(torch.int64) for i in range(4))
    want = torch.stack([((b << 6) | a) & 255, ((c << 4) | (b >> 2)) & 255, ((d << 2) | (c >> 4)) & 255], -1).to(torch.uint8).reshape(7, 192)
    got = R.pack6(codes)
    assert torch.equal(got, want) and torch.equal(R.unpack6(got), codes)
    row = got[0].to(torch.int64)
    bits = sum(int(row[i]) << (8 * i) for i in range(192))  # the row as one little-endian bit string: code j at bits 6 j .. 6 j + 5
    assert [(bits >> (6 * j)) & 63 for j in range(256)] == codes[0].tolist()
    assert not torch.equal(R.pack6(codes, "big"), got) and not torch.equal(R.unpack6(R.pack6(codes, "big")), codes)


def test_quant6_by_hand_and_pins():
    x = torch.zeros(2, 128, dtype=G.BF16)
    x[0, 0], x[0, 1], x[0, 2], x[0, 33], x[1, 64:96] = 28.0, -26.0, 0.0625, 3.0, -0.0
    q, sc = R.quant6(x)
    assert sc.tolist() == [[127, 124, 0, 0], [0, 0, 0, 0]] and q[0, :3].tolist() == [0x1F, 0x3E, 0x01] and int(q[0, 33]) == 0x1E  # 3 / 28 -> 2^-3, 3 * 2^3 = 24
    assert bool((q[1, 64:96] == 0x20).all())
    assert torch.equal(R.dequant6(q, sc)[0, :3], torch.tensor([28.0, -24.0, 0.0625], dtype=G.F64)) and float(R.dequant6(q, sc)[0, 33]) == 3.0
    assert len(R.PINS) == 15
    want = {"28*2^0": (127, 0x1F), "28.125*2^0": (128, None), "27.875*2^0": (127, 0x1F), "1.75*2^-123": (0, 0x1F), "1.75*2^-123 + 1 step": (1, None), "2^-126": (0, 0x10),
            "least subnormal": (0, 0x00), "largest finite": (251, None)}
    for pin, (byte, code) in want.items():
        xs, n = X.sweep(R.PINS[pin])
        assert n == 2 * (R.PINS[pin] + 1) and bool(torch.isfinite(xs.float()).all())
        q, sc = R.quant6(xs)
        assert int(sc[0, 0]) == byte and (code is None or int(q[0, 0]) == code), (pin, int(sc[0, 0]), hex(int(q[0, 0])))
    for M, K in X.QUANT_LAYOUT:
        x = R.quant_input(M, K)
        q, sc = R.quant6(x)
        assert int(sc[0, 0]) == 127 and bool((q[0, :32] == 0x1F).all())
        if M > 2:
            assert int(sc[M // 2, 1]) == 0 and int(sc[M // 2, 0]) > 0 and bool((q[M - 1, K - 32 :] == 0x20).all())
    for M, K in R.QUANT_GRID:
        assert M * K // 16 > 4096 * 256 and K % 128 == 0 and M % 64


@pytest.mark.parametrize("mut", sorted(R.QUANT6_MUTATIONS))
def test_quantiser_mutations_differ(mut):
    """Divisor 448, e8m0 floor instead of ceil, truncation instead of round-to-nearest-even and '-0 -> +0' each change bytes of the sweep under 27.875
    and of the first layout input: the bit-for-bit comparison of the GPU module rejects them.  So does big-endian packing of correct codes."""
    for x in (X.sweep(R.PINS["27.875*2^0"])[0], R.quant_input(5, 256)):
        q, sc = R.quant6(x)
        mq, ms = R.quant6(x, **R.QUANT6_MUTATIONS[mut])
        nq, ns = int((R.pack6(q) != R.pack6(mq)).sum()), int((sc != ms).sum())
        print(f"{mut} on {tuple(x.shape)}: {nq} packed bytes and {ns} scale bytes differ")
        assert nq > 0 and (ns > 0) == (mut in ("e8m0_floor", "divisor_448"))
        assert int((R.pack6(q) != R.pack6(q, "big")).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------- inputs
def test_family_r_weights_are_the_parents():
    """The subclass draws the parent's ramped weights again from the parent's seed: quantised with mx_ref.quant they are the parent's b."""
    M, N, K = 5, 16, 256
    p = X.Inputs("R", M, N, K)
    g = G._gen(77, 1, M, N, K, 0, 0)
    torch.randint(0, 2, (1,), generator=g)
    torch.randn(M, K, generator=g)
    ramp = torch.logspace(-3, 3, K // 32).repeat_interleave(32)
    w = ((torch.randn(N, K, generator=g) / K ** 0.5).to(G.BF16).to(G.F32) / ramp).to(G.BF16)
    assert torch.equal(X.quant(w)[0], p.b) and torch.equal(X.quant(w)[1], p.sb)
    c = R.Inputs("R", M, N, K)
    assert torch.equal(c.a, p.a) and torch.equal(R.quant6(w)[0], c.b) and c.b_packed.shape == (N, K * 3 // 4) and torch.equal(c.bias, p.bias)
    assert torch.equal(c.acc0, X.dequant(c.a, c.sa) @ R.dequant6(c.b, c.sb).T) and not torch.equal(c.acc0, p.acc0)
    assert torch.equal(c.sb.to(torch.int64), p.sb.to(torch.int64) + 4)  # 448 / 28 = 2^4: same block maxima, the scale four powers up


def test_family_i_premises_for_every_gpu_shape():
    """Family I is the parent's product on e3m2 codes: the premises (exact fp32 sums at every order, fp32 numbers in front of every rounding, each
    rounding exercised) hold for both inputs of every shape at which tests/test_gpu_mx6.py runs it, and the product is the parent's."""
    shapes = X.family_i_shapes()
    assert len(shapes) >= 25
    for M, N, K in shapes:
        for flat in (False, True):
            if (M, N, K) in X.AUTO and flat:
                continue
            inp = R.Inputs("I", M, N, K, flat_a=flat)
            s, ft, fp, fr = inp.assert_premises()
            assert int(inp.b.max()) < 64 and float(R.e3m2_values(inp.b).abs().max()) == 4.0 and inp.b_packed.shape == (N, K * 3 // 4)
            if M * N <= 1 << 17:
                assert torch.equal(inp.acc0, X.dequant(inp.a, inp.sa) @ R.dequant6(inp.b, inp.sb).T)
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
    """Block-ordered fp32 accumulation on e3m2 weights, rounding and truncating: equal to family I's chain, inside every bound of family R."""
    case = G.Case("emulation", record=False)
    for M, N, K in (SHAPE, (136, 136, 128)):
        for fam in ("I", "R"):
            for v, use_bias in _views(fam, M, N, K):
                for epi, use_gate in X.EPILOGUES:
                    if fam == "I" and epi not in (G.EPI_NONE, G.EPI_RESIDUAL):
                        continue
                    exp = G.Expect(v, epi, use_bias, use_gate)
                    for truncating in (False, True):
                        case.check(R.emulate(v, epi, use_bias, use_gate, truncating=truncating), exp, f"emulation truncating={truncating}")
    print(f"{len(case.rows)} checks, largest d/tol {case.worst_ratio:.3f}")
    assert 0.3 < case.worst_ratio <= 1.0


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


@pytest.mark.parametrize("mut", sorted(X.GEMM_MUTATIONS) + list(R.GEMM6_MUTATIONS))
def test_gemm_mutations_are_rejected(mut):
    """mx_ref's ten wrong kernels, and the three of the 6-bit operand — the instruction's other 6-bit format, a big-endian weight string, the two
    16-code pieces of a fragment exchanged: each rejected by a family; those that change the product by every family."""
    hits = _rejected_by(mut, X.GEMM_MUTATIONS.get(mut, G.EPI_NONE))
    assert "I" in hits
    if mut in ("scale_bytes_swapped", "scale_dword_late", "drop_last_tile", "k_tile_twice", "alpha_after_bias", "rowmajor_table_read_as_tiled", "truncate") + R.GEMM6_MUTATIONS:
        assert hits == {"I", "R"}


def test_one_hot_walk_tells_the_fragment_order():
    """The GPU module's diagnostic walk: with W one-hot at k0(n) and distinct x along k, a kernel that exchanges the 16-code pieces of a fragment
    returns x[m, k0 ^ 32] — different from x[m, k0] for every n."""
    K = 256
    k0 = (37 * torch.arange(264) + 5) % K
    x = ((7 * torch.arange(K)[None, :] + torch.arange(5)[:, None]) % 15) - 7
    assert int(x.abs().max()) == 7 and bool((x[:, k0] != x[:, k0 ^ 32]).all()) and len(set(k0.tolist())) == K


# ------------------------------------------------------------------------------------------------------------------- argument validation
def test_argument_validation_needs_no_gpu():
    """The new entries check their arguments before any HIP call, with the library's error codes (-1 shape, -2 alignment, -5 argument)."""
    from lightx2v_amd import lib

    L = lib._lib
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    # x2v_quant_mxfp6_bf16(x, ldx, q, ldq, scales, M, K, stream)
    assert L.x2v_quant_mxfp6_bf16(a, 96, a, 72, a, 4, 96, None) == -1 and b"K=96" in L.x2v_last_error()
    assert L.x2v_quant_mxfp6_bf16(None, 128, a, 96, a, 4, 128, None) == -5
    assert L.x2v_quant_mxfp6_bf16(a, 128, odd, 96, a, 4, 128, None) == -2
    assert L.x2v_quant_mxfp6_bf16(a, 128, a, 92, a, 4, 128, None) == -2  # ldq below 3K/4
    assert L.x2v_quant_mxfp6_bf16(a, 128, a, 96, a, 0, 128, None) == 0  # no rows: nothing launched
    # x2v_gemm_mxfp6_mxfp8_variant(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream)
    V = L.x2v_gemm_mxfp6_mxfp8_variant
    assert V(a, 192, a, a, 144, a, None, None, a, 64, 4, 64, 192, 0, None) == -1 and b"K=192" in L.x2v_last_error()  # K % 128
    assert V(a, 128, a, a, 96, a, None, None, a, 64, 4, 60, 128, 0, None) == -1  # N % 8
    assert V(a, 128, a, None, 96, a, None, None, a, 64, 4, 64, 128, 0, None) == -5  # null b
    assert V(a, 128, None, a, 96, a, None, None, a, 64, 4, 64, 128, 0, None) == -5  # null scale table
    assert V(a, 128, a, odd, 96, a, None, None, a, 64, 4, 64, 128, 0, None) == -2  # b not 4-byte aligned
    assert V(a, 128, a, a, 98, a, None, None, a, 64, 4, 64, 128, 0, None) == -2  # ldb % 4
    assert V(a, 128, a, a, 92, a, None, None, a, 64, 4, 64, 128, 0, None) == -2  # ldb below 3K/4 bytes
    assert V(a, 128, a, a, 96, a, None, None, a, 64, 4, 64, 128, 3, None) == -5 and b"unknown variant" in L.x2v_last_error()
    assert V(a, 128, a, a, 96, a, None, None, a, 64, 4, 64, 128, -1, None) == -5
    # x2v_gemm_mxfp6_mxfp8_epi(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, epilogue, resid, ldr, gate, stream)
    E = L.x2v_gemm_mxfp6_mxfp8_epi
    assert E(a, 128, a, a, 96, a, None, None, a, 64, 4, 64, 128, 2, None, 0, None, None) == -5 and b"resid" in L.x2v_last_error()  # residual epilogue without resid
    assert E(a, 128, a, a, 96, a, None, None, a, 64, 4, 64, 128, 2, a, 60, None, None) == -2  # ldr below N
    assert E(a, 128, a, a, 96, a, None, None, a, 64, 4, 64, 96, 0, None, 0, None, None) == -1
    assert L.x2v_gemm_mxfp6_mxfp8(a, 128, a, a, 96, a, None, None, odd, 64, 4, 64, 128, None) == -2  # y
    assert {"x2v_quant_mxfp6_bf16", "x2v_gemm_mxfp6_mxfp8", "x2v_gemm_mxfp6_mxfp8_epi", "x2v_gemm_mxfp6_mxfp8_variant"} <= set(lib.PROTOTYPES)


def test_operator_class_is_registered():
    from lightx2v_amd import mx, ops, registry

    assert registry.MM_WEIGHT_REGISTER["W-mxfp6-A-mxfp8-dynamic-Hip"] is ops.MMWeightMxfp6Hip and issubclass(ops.MMWeightMxfp6Hip, ops.MMWeightMxfp8Hip)
    assert ops.MMWeightMxfp6Hip.quantize_input is ops.MMWeightMxfp8Hip.quantize_input  # the shared quantised activation of a fused driver
    assert mx.scaled_mxfp6_mxfp8_mm is mx.cutlass_scaled_mxfp6_mxfp8_mm and callable(mx.scaled_fp6_quant)
    with pytest.raises(lib_error()):
        ops.MMWeightMxfp6Hip("a.weight", None).load({"a.weight": torch.zeros(8, 128)})  # quantised by the HIP kernel: a CPU tensor is an error


def lib_error():
    from lightx2v_amd import lib

    return lib.X2VError
