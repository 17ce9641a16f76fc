"""tests/mx_ref.py checked without a GPU: the quantiser reference bit for bit against oracle/mx_oracle.py on finite inputs (every pin of the GPU
module's exhaustive sweep included) and against values worked out by hand, the premises of family I for every shape the GPU module lists, an fp32
emulation of a correct kernel (block-ordered accumulation, rounding or truncating when it aligns addends) inside every check of both families, and
the emulations of a subtly WRONG kernel or quantiser each rejected.  The rejections this module prints (pytest -s) are the evidence that
tests/test_gpu_mx_fp64.py would fail on such a kernel: deliberately broken kernels are never run on a GPU."""
import pytest
import torch

from tests import gemm_ref as G
from tests import mx_ref as X

SHAPE = (300, 264, 512)  # M, N, K of the rejection tests: two tiles of either size in both directions, both ragged, four K tiles


# ------------------------------------------------------------------------------------------------------------------- quantiser
def test_pieces_by_hand():
    f = lambda *v: torch.tensor(v, dtype=G.F64)
    assert X.e4m3_codes(f(0.0, -0.0, 1.0, -1.0, 448.0, 1000.0, 2.0 ** -6, 2.0 ** -9, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 17.0, 19.0, 15.5)).tolist() == \
        [0x00, 0x80, 0x38, 0xB8, 0x7E, 0x7E, 0x08, 0x01, 0x00, 0x80, 0x02, 0x58, 0x5A, 0x58]  # ties to even: 2^-10 -> 0, 3 * 2^-10 -> 2 * 2^-9, 17 -> 16, 19 -> 20, 15.5 -> 16
    assert X.e4m3_codes(f(17.0, 19.0, -(2.0 ** -10)), rnd="trunc").tolist() == [0x58, 0x59, 0x80] and X.e4m3_codes(f(-0.0, -(2.0 ** -10), -1.0), neg_zero=False).tolist() == [0, 0, 0xB8]
    every = torch.arange(256, dtype=torch.uint8)
    finite = (every & 0x7F) != 0x7F
    assert torch.equal(X.e4m3_values(every)[finite], every.view(torch.float8_e4m3fn).to(G.F32).to(G.F64)[finite])
    assert torch.equal(X.e4m3_codes(X.e4m3_values(every))[finite], every[finite])
    # 448 * 2^k -> 2^k exactly; one step above needs the next power; denormal quotients are not flushed: 448 * 2^-127 -> byte 0, above it byte 1
    assert X.e8m0_byte(f(0.0, 448.0, 450.0, 446.0, 1.0, 448 * 2.0 ** -127, 449 * 2.0 ** -127, 448 * 2.0 ** -126, 2.0 ** -133, 3.0e38, 448 * 2.0 ** 127)).tolist() == \
        [0, 127, 128, 127, 119, 0, 1, 1, 0, 247, 254]
    assert X.e8m0_byte(f(450.0, 446.0, 448.0), "floor").tolist() == [127, 126, 127]
    assert float(X.round_fp32(f(2.0 ** -149 * 1.5))) == 2.0 ** -148 and float(X.round_fp32(f(2.0 ** -149 * 2.5))) == 2.0 ** -148 and float(X.round_fp32(f(1 + 2.0 ** -24))) == 1.0
    sc = torch.arange(2 * 8, dtype=torch.uint8).reshape(2, 8)
    t = X.tiled(sc)
    assert t.shape == (2, 2, 4) and t[1, 0].tolist() == [4, 5, 6, 7] and t[0, 1].tolist() == [8, 9, 10, 11] and torch.equal(X.rowmajor(t), sc)


@pytest.mark.parametrize("pin", sorted(X.PINS))
def test_quantiser_equals_the_oracle_on_the_sweep(pin):
    """Every finite bf16 bit pattern under each pinned block maximum; the values the oracle gave when the issue was written."""
    from oracle import mx_oracle as MX

    x, n = X.sweep(X.PINS[pin])
    assert n == 2 * (X.PINS[pin] + 1) and bool(torch.isfinite(x.float()).all())
    q, sc = X.quant(x)
    rq, rs = MX.quant_mxfp8(x)
    assert torch.equal(sc, rs) and torch.equal(q, rq.view(torch.uint8))
    want = {"1.75*2^-119": (0, 0x7E), "1.75*2^-119 + 1 step": (1, None), "2^-126": (0, 0x40), "least subnormal": (0, 0x08), "largest finite": (247, None), "448*2^0": (127, 0x7E),
            "450*2^0": (128, None), "446*2^0": (127, 0x7E)}.get(pin)
    if want:
        assert int(sc[0, 0]) == want[0] and (want[1] is None or int(q[0, 0]) == want[1])
    if pin == "448*2^0":
        assert n == 34_754 and x.shape == (281, 128)


def test_quantiser_equals_the_oracle_on_the_layout_inputs():
    from oracle import mx_oracle as MX

    for M, K in X.QUANT_LAYOUT:
        x = X.quant_input(M, K)
        q, sc = X.quant(x)
        rq, rs = MX.quant_mxfp8(x)
        assert torch.equal(sc, rs) and torch.equal(q, rq.view(torch.uint8))
        if M > 2:
            assert int(sc[M // 2, 1]) == 0 and int(sc[M // 2, 0]) > 0 and bool((q[M - 1, K - 32 :] == 0x80).all())
    for M, K in X.QUANT_GRID:
        assert M * K // 8 > 8192 * 256 and K % 128 == 0
    assert X.QUANT_GRID[1][0] * X.QUANT_GRID[1][1] > 2.4 * X.QUANT_GRID[0][0] * X.QUANT_GRID[0][1] and X.QUANT_GRID[1][0] % 64


@pytest.mark.parametrize("mut", sorted(X.QUANT_MUTATIONS))
def test_quantiser_mutations_differ_on_the_sweep(mut):
    """e8m0 floor instead of ceil, truncation instead of round-to-nearest-even and '-0 -> +0' each change bytes of the sweep at 448 and of the first
    layout input: the bit-for-bit comparison of the GPU module rejects them."""
    for x in (X.sweep(X.PINS["446*2^0"])[0], X.quant_input(5, 256)):
        q, sc = X.quant(x)
        mq, ms = X.quant(x, **X.QUANT_MUTATIONS[mut])
        nq, ns = int((q != mq).sum()), int((sc != ms).sum())
        print(f"{mut} on {tuple(x.shape)}: {nq} codes and {ns} scale bytes differ")
        assert nq > 0 and (ns > 0) == (mut == "e8m0_floor")


# ------------------------------------------------------------------------------------------------------------------- GEMM reference
def test_gemm_reference_by_hand():
    """One output element: a = 3 in block 0 (byte 130) and 2 in block 3 (byte 126), b = 5 (byte 125) and 4 (byte 129); acc = 3 * 8 * 5 / 4 + 2 / 2 * 4 * 4
    = 30 + 16 = 46, alpha = 0.5, bias = 0.25."""
    inp = X.Inputs("R", 1, 8, 128)
    a, b = torch.zeros(1, 128, dtype=G.F64), torch.zeros(8, 128, dtype=G.F64)
    a[0, 0], a[0, 96], b[0, 0], b[0, 96] = 3.0, 2.0, 5.0, 4.0
    inp.a, inp.b = X.e4m3_codes(a), X.e4m3_codes(b)
    inp.sa, inp.sb = torch.tensor([[130, 127, 127, 126]], dtype=torch.uint8), torch.tensor([[125, 127, 127, 129]], dtype=torch.uint8).repeat(8, 1)
    assert float((X.dequant(inp.a, inp.sa) @ X.dequant(inp.b, inp.sb).T)[0, 0]) == 46.0
    inp.acc0, inp.absacc0, inp.alpha = X.dequant(inp.a, inp.sa) @ X.dequant(inp.b, inp.sb).T, X.dequant(inp.a, inp.sa).abs() @ X.dequant(inp.b, inp.sb).abs().T, 0.5
    inp.bias = torch.full((8,), 0.25, dtype=G.BF16)
    v = inp.scaled(True)
    e = G.Expect(v, G.EPI_NONE)
    assert float(e.f[0, 0]) == 23.25 and float(e.tol[0, 0]) == pytest.approx(2.0 ** -8 * 23.25 + (1 + 2.0 ** -8) * 131 * 2.0 ** -23 * 23.25, rel=1e-14)
    assert float(X.emulate(v, G.EPI_NONE)[0, 0]) == 23.25 and float(G.Expect(inp.scaled(False), G.EPI_NONE, use_bias=False).f[0, 0]) == 46.0


def test_family_i_premises_for_every_gpu_shape():
    """Exact fp32 sums at every accumulation order, fp32 numbers in front of every rounding, each rounding exercised: for both inputs (rows of a on
    their own bases without a bias, on one base with a bias) of every shape at which tests/test_gpu_mx_fp64.py runs family I."""
    shapes = X.family_i_shapes()
    for nk in X.K_TILES:
        assert (X.K_TILES_MN[0], X.K_TILES_MN[1], nk * 128) in shapes
    assert len(shapes) >= 25
    for M, N, K in shapes:
        for flat in (False, True):
            if (M, N, K) in X.AUTO and flat:
                continue  # the automatic choice runs without a bias
            inp = X.Inputs("I", M, N, K, flat_a=flat)
            s, ft, fp, fr = inp.assert_premises()
            print(f"{inp.name}: spread {inp.spread}, sum |terms| {s:.2f} of 2^24, bias range {inp.bias_range}, inexact: t {ft:.1%}, gated product {fp:.1%}, resid + p {fr:.1%}")
            assert int(inp.sa.min()) >= 107 and int(inp.sa.max()) <= 154 and inp.alpha in (0.5, 0.75) and X.spread(K) - 1 <= inp.spread <= X.spread(K)
    assert X.spread(128) == 7 and X.spread(1152) == 6 and X.spread(13824) == 3


def test_gpu_lists():
    assert [X.auto_body(*s) for s in X.AUTO] == [2, 1] and -(-X.AUTO[0][0] // 256) * (X.AUTO[0][1] // 256) == 208
    (m1, n1, k1), (m2, n2, k2) = X.SCHED
    assert (-(-m1 // 128), -(-n1 // 128), k1) == (9, 3, 128) and (-(-m2 // 256), -(-n2 // 256), k2) == (5, 2, 256)
    assert {1, 2} <= set(X.K_TILES) and {1, 127, 128, 129, 255, 256, 257} == set(X.M_TAILS) and {8, 120, 128, 136, 248, 256, 264} == set(X.N_TAILS)
    assert all(K == 13824 for _, _, K in X.DEEP) and len(X.PINS) == 15


# ------------------------------------------------------------------------------------------------------------------- emulations
def _views(fam, M, N, K):
    """(view, bias?) of every input of a shape: family I without a bias on per-row bases and with one on a flat base, each with and without alpha."""
    if fam == "R":
        inp = X.Inputs("R", M, N, K)
        return [(inp.scaled(True), True), (inp.scaled(False), False)]
    out = []
    for flat in (False, True):
        inp = X.Inputs("I", M, N, K, flat_a=flat)
        inp.assert_premises()
        out += [(inp.scaled(u), flat) for u in (False, True)]
    return out


def test_correct_emulation_passes_every_check():
    """Block-ordered fp32 accumulation, rounding and truncating: equal to family I's chain, inside every bound of family R."""
    case = G.Case("emulation", record=False)
    for M, N, K in (SHAPE, (136, 136, 128), (72, 136, 3456)):
        for fam in ("I", "R"):
            for v, use_bias in _views(fam, M, N, K):
                for epi, use_gate in X.EPILOGUES:
                    if fam == "I" and epi not in (G.EPI_NONE, G.EPI_RESIDUAL):
                        continue
                    exp = G.Expect(v, epi, use_bias, use_gate)
                    for truncating in (False, True):
                        case.check(X.emulate(v, epi, use_bias, use_gate, truncating=truncating), exp, f"emulation truncating={truncating}")
    print(f"{len(case.rows)} checks, largest d/tol {case.worst_ratio:.3f}")
    assert 0.5 < case.worst_ratio <= 1.0


def _rejected_by(mut, epi):
    M, N, K = SHAPE
    hits = []
    for fam in ("I", "R"):
        for v, use_bias in _views(fam, M, N, K):
            if mut in ("alpha_after_bias", "bias_after_rounding") and not (use_bias and v.alpha_used):
                continue
            try:
                G.Case("mutation", record=False).check(X.emulate(v, epi, use_bias, mut=mut), G.Expect(v, epi, use_bias), mut)
            except G.Reject as r:
                hits.append(fam)
                print(f"{v.name} {mut}: rejected by '{r.criterion}' — {r}")
    return set(hits)


@pytest.mark.parametrize("mut", sorted(X.GEMM_MUTATIONS))
def test_gemm_mutations_are_rejected(mut):
    """Scale bytes of a dword swapped, a scale dword one K tile late, the last K tile dropped, a K tile counted twice, alpha after the bias, the bias
    after the rounding, round-half-up, truncation, the gate product not rounded, a row-major table read as tiled: each rejected by a family; those
    that change the product by every family, the rounding ones at least by family I."""
    hits = _rejected_by(mut, X.GEMM_MUTATIONS[mut])
    assert "I" in hits
    if mut in ("scale_bytes_swapped", "scale_dword_late", "drop_last_tile", "k_tile_twice", "alpha_after_bias", "rowmajor_table_read_as_tiled", "truncate"):
        assert hits == {"I", "R"}


# ------------------------------------------------------------------------------------------------------------------- argument validation
def test_argument_validation_needs_no_gpu():
    """The MXFP8 entries check their arguments before any HIP call, with the library's error codes (-1 shape, -2 alignment, -5 argument) — the
    checks of the MXFP6 and MXFP4 entries (tests/test_mx6_ref_host.py, tests/test_mx4_ref_host.py): one body serves the three formats."""
    import ctypes

    from lightx2v_amd import lib

    L = lib._lib
    a, odd, two = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4098)
    assert {"x2v_quant_mxfp8_bf16", "x2v_gemm_mxfp8", "x2v_gemm_mxfp8_epi", "x2v_gemm_mxfp8_variant"} <= set(lib.PROTOTYPES)
    # x2v_quant_mxfp8_bf16(x, ldx, q, ldq, scales, M, K, stream)
    assert L.x2v_quant_mxfp8_bf16(a, 96, a, 96, a, 4, 96, None) == -1 and b"K=96" in L.x2v_last_error()
    assert L.x2v_quant_mxfp8_bf16(None, 128, a, 128, a, 4, 128, None) == -5
    assert L.x2v_quant_mxfp8_bf16(a, 128, odd, 128, a, 4, 128, None) == -2  # q not 8-byte aligned
    assert L.x2v_quant_mxfp8_bf16(a, 128, a, 120, a, 4, 128, None) == -2  # ldq below K
    assert L.x2v_quant_mxfp8_bf16(a, 128, a, 128, a, 0, 128, None) == 0  # no rows: nothing launched
    # x2v_gemm_mxfp8(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, stream)
    P = L.x2v_gemm_mxfp8
    assert P(a, 192, a, a, 192, a, None, None, a, 64, 4, 64, 192, None) == -1 and b"K=192" in L.x2v_last_error()  # K % 128
    assert P(a, 128, a, None, 128, a, None, None, a, 64, 4, 64, 128, None) == -5  # null operand
    assert P(None, 128, a, a, 128, a, None, None, a, 64, 4, 64, 128, None) == -5
    assert P(a, 128, None, a, 128, a, None, None, a, 64, 4, 64, 128, None) == -5  # null scale table
    assert P(a, 128, a, a, 128, a, None, None, a, 64, 4, 60, 128, None) == -1  # N % 8
    assert P(a, 128, a, odd, 128, a, None, None, a, 64, 4, 64, 128, None) == -2  # b not 16-byte aligned
    assert P(a, 128, a, a, 136, a, None, None, a, 64, 4, 64, 128, None) == -2  # ldb % 16
    assert P(a, 112, a, a, 128, a, None, None, a, 64, 4, 64, 128, None) == -2  # lda below K bytes
    assert P(a, 128, a, a, 128, a, None, None, odd, 64, 4, 64, 128, None) == -2  # y
    assert P(a, 128, a, a, 128, a, two, None, a, 64, 4, 64, 128, None) == -2  # a bias only 2-byte aligned: both bodies fetch it as 8-byte pairs
    # x2v_gemm_mxfp8_variant(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream)
    V = L.x2v_gemm_mxfp8_variant
    assert V(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 128, 3, None) == -5 and b"unknown variant" in L.x2v_last_error()
    assert V(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 128, -1, None) == -5
    assert V(a, 1 << 24, a, a, 128, a, None, None, a, 64, 4, 64, 128, 2, None) == -1  # the 256x256 body's 32-bit tile addressing
    assert V(a, 128, a, a, 1 << 24, a, None, None, a, 64, 4, 64, 128, 2, None) == -1 and b"leading dimension" in L.x2v_last_error()
    # x2v_gemm_mxfp8_epi(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, epilogue, resid, ldr, gate, stream)
    E = L.x2v_gemm_mxfp8_epi
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 128, 2, None, 0, None, None) == -5 and b"resid" in L.x2v_last_error()  # residual epilogue without resid
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 128, 2, a, 60, None, None) == -2  # ldr below N
    assert E(a, 1 << 24, a, a, 128, a, None, None, a, 64, 4, 64, 128, 1, None, 0, None, None) == -1  # every fused epilogue runs the 256x256 body
    assert E(a, 128, a, a, 128, a, None, None, a, 64, 4, 64, 192, 0, None, 0, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------- body rule
MX_FORMATS = ((8, 8, 128, 8), (8, 6, 128, 8), (4, 4, 256, 6))  # element bits of a and b, k-values per K-tile, K-tiles from which the 256x256 body runs


@pytest.mark.parametrize("bits_a,bits_b,ktile,nk_min", MX_FORMATS)
def test_kernel_choice_query(bits_a, bits_b, ktile, nk_min):
    """x2v_gemm_mx_kernel_choice (host arithmetic) is the rule variant 0 follows: the 256x256 body from 192 tiles of 256x256 and the format's least
    number of K-tiles on, with both leading dimensions below 2^24 bytes.  For the formats with e4m3 activations it is the w8a8 GEMM's rule, asked
    of x2v_gemm_kernel_choice over the edges; and it is the rule the GPU suites model (auto_body) at their AUTO shapes."""
    from lightx2v_amd import lib
    from tests import mx4_ref as R4

    ch = lambda M, N, K, **ld: lib.gemm_mx_kernel_choice(bits_a, bits_b, M, N, K, **ld)
    big = 1 << 24
    assert ch(3073, 4096, nk_min * ktile) == 2 and ch(3073, 4096, (nk_min - 1) * ktile) == 1  # 13 x 16 tiles
    assert ch(191 * 256, 256, 16 * ktile) == 1 and ch(191 * 256 + 1, 256, 16 * ktile) == 2 and ch(3072, 4096 - 256, 16 * ktile) == 1  # 191, 192, 180 tiles
    assert ch(3073, 4096, 16 * ktile, lda=big) == 1 and ch(3073, 4096, 16 * ktile, ldb=big) == 1 and ch(3073, 4096, 16 * ktile, lda=big - 16, ldb=big - 16) == 2
    ref = R4 if bits_a == 4 else X  # tests/mx6_ref.py takes mx_ref's AUTO shapes and auto_body
    assert [ch(*s) for s in ref.AUTO] == [ref.auto_body(*s) for s in ref.AUTO] == [2, 1]
    if bits_a == 8:
        n = 0
        for M in (1, 190 * 256, 191 * 256, 191 * 256 + 1, 3072, 3073):
            for N in (8, 256, 3848, 4096):
                for nk in (1, 7, 8, 9, 16):
                    for lda in (nk * 128, big - 16, big):
                        for ldb in (nk * 128 * bits_b // 8, big - 16, big):
                            w8a8 = lib.gemm_kernel_choice(M, N, nk * 128, ldx=lda, ldw=ldb if bits_b == 8 else lda, fp8=True) == 2
                            assert (ch(M, N, nk * 128, lda=lda, ldb=ldb) == 2) == (w8a8 and ldb < big), (M, N, nk, lda, ldb)
                            n += 1
        assert n == 6 * 4 * 5 * 9
    # a bad shape or format is an error, not a guess
    L = lib._lib
    assert L.x2v_gemm_mx_kernel_choice(0, 256, 256, 256, 256, 256) == -5 and L.x2v_gemm_mx_kernel_choice(4, 256, 256, 256, 256, 256) == -5
    fmt = MX_FORMATS.index((bits_a, bits_b, ktile, nk_min)) + 1
    assert L.x2v_gemm_mx_kernel_choice(fmt, 256, 256, ktile // 2 * 3, 512, 512) == -1 and L.x2v_gemm_mx_kernel_choice(fmt, 256, 252, ktile, 512, 512) == -1
    assert L.x2v_gemm_mx_kernel_choice(fmt, 256, 256, 2 * ktile, 2 * ktile * bits_a // 8 - 16, 512) == -1  # lda below the row's bytes
    with pytest.raises(lib.X2VError):
        ch(0, 256, ktile)
