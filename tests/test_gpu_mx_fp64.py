"""The MXFP8 path — quant_mx_kernel<1> of mx.hip and the MX instantiations of gemm.hip's 128x128 kernel and of gemm256.hip's 256x256 ping-pong kernel —
against the float64 references of tests/mx_ref.py, at the smallest shapes at which each edge exists.  tests/test_mx_ref_host.py shows which subtly
wrong kernels and quantisers this rejects.

Quantiser: codes and scale bytes BIT FOR BIT — every finite bf16 bit pattern under fifteen pinned block maxima (at and around 448 * 2^k, around the
denormal quotient 2^-127, bf16 subnormals, the largest finite bf16), rows that do not fill a wave with ldx > K and ldq > K inside poisoned
buffers, the grid-stride loop past the capped grid, and a NaN or an Inf element leaving every other block untouched.

GEMM: both bodies forced through `variant` (the fused epilogues through x2v_gemm_mxfp8_epi, which only the 256x256 body has).  Family I (integer
codes, scale bytes differing per row and per 32-wide block) is compared BIT FOR BIT with the float64 chain, family R (quantised N(0, 1) under a
per-block ramp of 10^6) on EVERY element with gemm_ref's derived bound; no share of elements is left out anywhere.  Operands are windows of loud
buffers (lda, ldb > K, the first row not the allocation's), scale tables 4-byte aligned slices of a byte buffer of 0xFF (an e8m0 NaN), the output
a window (ldy > N) of a poisoned buffer whose surroundings are checked after each call; resid and both tables must come back unchanged."""
import os

import pytest
import torch

from tests import gemm_ref as G
from tests import mx_ref as X

pytestmark = pytest.mark.gpu
POISON = -1984.0  # exact in bf16
QPOISON = 0xA5
BF16, U8, E4M3 = torch.bfloat16, torch.uint8, torch.float8_e4m3fn
CASES, QROWS, NOTES, _INPUTS, _EXPECT = {}, [], [], {}, {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_MX_PARITY_TABLE")  # where to write the table of measured ratios (profiles/mx_fp64_parity.txt is one run's)
    if not path:
        return
    try:
        with open(path, "w") as f:
            for name in sorted(CASES):
                f.write(CASES[name].header() + "\n")
            f.write(f"# quantiser: {len(QROWS)} checks (all bit for bit), {sum(r[2] + r[3] > 0 for r in QROWS)} with unequal bytes\n")
            for name in sorted(CASES):
                f.write("\n".join(CASES[name].table()) + "\n")
            for name, what, nq, ns, n in QROWS:
                f.write(f"{name:<24} {what:<60} exact unequal codes {nq} scale bytes {ns}  n={n}\n")
            for note in NOTES:
                f.write(f"# {note}\n")
    except OSError:
        pass


def case(name):
    return CASES.setdefault(name, G.Case(name, prefix="mx_fp64"))


# ------------------------------------------------------------------------------------------------------------------- buffers
def operand(codes):
    """Code bytes [rows, K] as an e4m3 window one row down in a buffer of 448s with 16 bytes more per row."""
    rows, K = codes.shape
    big = torch.full((rows + 2, K + 16), 0x7E, dtype=U8, device="cuda")
    win = big[1 : rows + 1, :K]
    win.copy_(codes)
    assert win.data_ptr() % 16 == 0 and win.stride(0) > K
    return win.view(E4M3)


def table(sc):
    """Scale bytes [rows, K / 32] as the kernels' table [K / 128][rows][4]: a contiguous, 4-byte aligned slice of a byte buffer of 0xFF, not at its
    start.  Returns (buffer, table)."""
    t = X.tiled(sc.cpu()).cuda()
    buf = torch.full((t.numel() + 256,), 0xFF, dtype=U8, device="cuda")
    win = buf[68 : 68 + t.numel()].view(t.shape)
    win.copy_(t)
    assert win.data_ptr() % 4 == 0 and win.is_contiguous()
    return buf, win


def out_window(M, N):
    """A poisoned buffer and its [M, N] window two rows down with ldy = N + 8."""
    big = torch.full((M + 4, N + 8), POISON, dtype=BF16, device="cuda")
    return big, big[2 : M + 2, :N]


def poison_intact(big, M, N, value=POISON):
    return bool((big[:2] == value).all() and (big[M + 2 :] == value).all() and (big[2 : M + 2, N:] == value).all())


class Dev:
    """The device side of an Inputs: operand windows and scale tables, made once."""

    def __init__(self, inp):
        self.inp = inp
        self.a, self.b = operand(inp.a.cuda()), operand(inp.b.cuda())
        (self.sa_buf, self.sa), (self.sb_buf, self.sb) = table(inp.sa), table(inp.sb)
        self.sa_copy, self.sb_copy = self.sa_buf.clone(), self.sb_buf.clone()
        self.bias = None if inp.bias is None else inp.bias.cuda().contiguous()
        self.gate = inp.gate.cuda().contiguous()
        self.alpha = torch.tensor([inp.alpha], dtype=torch.float32, device="cuda")
        self.resid_big = torch.full((inp.M + 4, inp.N + 8), POISON, dtype=BF16, device="cuda")
        self.resid = self.resid_big[2 : inp.M + 2, : inp.N]
        self.resid.copy_(inp.resid)
        self.resid_copy = self.resid_big.clone()


def inputs(family, M, N, K, flat_a=False):
    """(Inputs, Dev) of a shape, made once per module run; family I's premises are asserted here."""
    key = (family, M, N, K, flat_a)
    if key not in _INPUTS:
        big = M * N > (1 << 22)
        inp = X.Inputs(family, M, N, K, flat_a=flat_a, device="cuda" if big else "cpu")
        if family == "I":
            inp.assert_premises()
        if big:  # used by one test
            return inp, Dev(inp)
        _INPUTS[key] = (inp, Dev(inp))
    return _INPUTS[key]


def expect(view, epi, use_bias, use_gate=False):
    if view.M * view.N > (1 << 22):
        return G.Expect(view, epi, use_bias, use_gate)
    key = (view.name, epi, use_bias, use_gate)
    if key not in _EXPECT:
        _EXPECT[key] = G.Expect(view, epi, use_bias, use_gate)
    return _EXPECT[key]


def run(lib, d, epi, use_alpha, use_bias, use_gate=False, variant=0, entry="variant", in_place=False):
    """One call into a poisoned window; returns the window.  entry 'variant': x2v_gemm_mxfp8_variant (no epilogue), 'epi': x2v_gemm_mxfp8_epi."""
    inp = d.inp
    big, y = out_window(inp.M, inp.N)
    assert y.data_ptr() % 16 == 0 and y.stride(0) == inp.N + 8
    alpha, bias = d.alpha if use_alpha else None, d.bias if use_bias else None
    assert not use_bias or bias is not None
    if entry == "variant":
        assert epi == G.EPI_NONE
        lib.gemm_mxfp8(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, out=y, variant=variant)
    elif epi == G.EPI_NONE:  # the shim sends an epilogue-free call to the variant entry: call the epilogue entry itself
        p = lambda t: None if t is None else t.data_ptr()
        lib._check(lib._lib.x2v_gemm_mxfp8_epi(p(d.a), d.a.stride(0), p(d.sa), p(d.b), d.b.stride(0), p(d.sb), p(bias), p(alpha), p(y), y.stride(0), inp.M, inp.N, inp.K, epi, None,
                                               0, None, lib._stream()), "gemm_mxfp8_epi")
    elif epi == G.EPI_RESIDUAL and in_place:
        y.copy_(d.resid)
        out = lib.gemm_mxfp8(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, epilogue=epi, resid=y, gate=d.gate if use_gate else None)
        assert out.data_ptr() == y.data_ptr()
    else:
        kw = dict(resid=d.resid, gate=d.gate if use_gate else None) if epi == G.EPI_RESIDUAL else {}
        lib.gemm_mxfp8(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, epilogue=epi, out=y, **kw)
    assert poison_intact(big, inp.M, inp.N), "wrote outside the output window"
    assert torch.equal(d.resid_big, d.resid_copy), "resid was written"
    assert torch.equal(d.sa_buf, d.sa_copy) and torch.equal(d.sb_buf, d.sb_copy), "a scale table was written"
    return y


def views(family, M, N, K):
    """(view, Dev, bias?) with and without alpha, with and without bias: family R from one input, family I without a bias from the input whose rows
    of a have their own bases and with a bias from the one where they share it (tests/mx_ref.py says why)."""
    if family == "R":
        inp, d = inputs("R", M, N, K)
        return [(inp.scaled(ua), d, ub) for ua in (True, False) for ub in (True, False)]
    out = []
    for flat in (False, True):
        inp, d = inputs("I", M, N, K, flat)
        out += [(inp.scaled(ua), d, flat) for ua in (True, False)]
    return out


def check_bodies(lib, name, M, N, K, variants=(1, 2)):
    """NONE through both forced bodies, both families, every (alpha, bias) combination, against the one reference of each."""
    for family in ("I", "R"):
        for v, d, use_bias in views(family, M, N, K):
            exp = expect(v, G.EPI_NONE, use_bias)
            for variant in variants:
                got = run(lib, d, G.EPI_NONE, v.alpha_used is not None, use_bias, variant=variant)
                case(name).check(got, exp, X.BODY[variant])


# ------------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("nk", X.K_TILES)
def test_k_loop(lib, nk):
    """1..5 and 9 K tiles: the 128x128 body's ring parity and its last tile without a prefetch; the 256x256 body's prologue below LEAD half-tiles (one
    K tile), exactly one ring (two), the checked tail with its guarded scale prefetch, odd and even trip counts.  M = 257 and N = 264 leave a
    ragged tile in both directions for either tile size."""
    M, N = X.K_TILES_MN
    check_bodies(lib, "k loop", M, N, nk * X.KTILE)


@pytest.mark.parametrize("M", X.M_TAILS)
def test_m_tails(lib, M):
    """One row, one short of, exactly and one past the 128-row and the 256-row tile."""
    check_bodies(lib, "m tails", M, 136, X.TAIL_K)


@pytest.mark.parametrize("N", X.N_TAILS)
def test_n_tails(lib, N):
    """One 8-column group, one short of, exactly and one past 128 and 256 columns."""
    check_bodies(lib, "n tails", 129, N, X.TAIL_K)


@pytest.mark.parametrize("M,N,K", X.SCHED)
def test_scheduling_groups(lib, M, N, K):
    """9 x 3 tiles of 128 (groups of 8 m-tiles: a last group of 1, 27 tiles on 8 XCDs) and 5 x 2 tiles of 256 (groups of 4: a last group of 1): every
    tile computed once, and in its place."""
    check_bodies(lib, "scheduling groups", M, N, K)


@pytest.mark.parametrize("M,N,K", X.DEEP)
def test_deep_k(lib, M, N, K):
    """K = 13824 (108 K tiles): a K tile dropped, doubled or taken from the wrong stage, or a scale dword adopted late, anywhere in a long loop."""
    check_bodies(lib, "deep k", M, N, K)


@pytest.mark.parametrize("M,N,K", X.EPI_SHAPES)
def test_epilogues(lib, M, N, K):
    """x2v_gemm_mxfp8_epi: NONE (whichever body the shape gets), and on the 256x256 body GELU_TANH, SILU, RESIDUAL with a gate, without one and in
    place (out is resid), each with alpha and bias and without them, at a ragged tile, one short of a tile and one row of 8 columns — against the
    float64 chain, not against the body's own plain output."""
    for family in ("I", "R"):
        for v, d, use_bias in views(family, M, N, K):
            if (v.alpha_used is not None) != use_bias:
                continue
            for epi, use_gate in X.EPILOGUES:
                if family == "I" and epi not in (G.EPI_NONE, G.EPI_RESIDUAL):
                    continue
                exp = expect(v, epi, use_bias, use_gate)
                body = "epi entry, " + (X.BODY[X.auto_body(M, N, K)] if epi == G.EPI_NONE else X.BODY[2])
                case("epilogues").check(run(lib, d, epi, use_bias, use_bias, use_gate, entry="epi"), exp, body)
                if epi == G.EPI_RESIDUAL:
                    case("epilogues").check(run(lib, d, epi, use_bias, use_bias, use_gate, entry="epi", in_place=True), exp, body + " in place")


@pytest.mark.parametrize("M,N,K", X.AUTO)
def test_automatic_choice(lib, M, N, K):
    """variant = 0 just above and just below `tiles256 >= 192 && K / 128 >= 8` (13 x 16 = 208 tiles of 256; 8 K tiles -> the 256x256 body, 7 -> the
    128x128 body).  Family I: the result equals the float64 chain and the forced variant's output bit for bit.
    Family I cannot tell the bodies apart by their bits: this pins the correctness of whatever runs, not the choice — that is pinned on the host,
    through x2v_gemm_mx_kernel_choice (tests/test_mx_ref_host.py::test_kernel_choice_query).  The float64 side of this shape lives on the device."""
    inp, d = inputs("I", M, N, K)
    for use_alpha in (True, False):
        v = inp.scaled(use_alpha)
        exp = expect(v, G.EPI_NONE, False)
        got = run(lib, d, G.EPI_NONE, use_alpha, False, variant=0)
        case("automatic choice").check(got, exp, "variant 0")
        forced = run(lib, d, G.EPI_NONE, use_alpha, False, variant=X.auto_body(M, N, K))
        assert torch.equal(got.view(torch.int16), forced.view(torch.int16)), "variant 0 and the forced variant differ"
        case("automatic choice").check(forced, exp, X.BODY[X.auto_body(M, N, K)])


# ------------------------------------------------------------------------------------------------------------------- quantiser
def quant_call(lib, x):
    """x2v_quant_mxfp8_bf16 with ldx > K and ldq > K: x a window of a loud buffer, q and the scale table inside poisoned buffers whose surroundings
    are checked.  Returns (code bytes [M, K], scale bytes [M, K / 32]) on the CPU."""
    M, K = x.shape
    xbig = torch.full((M + 2, K + 8), 3.0e4, dtype=BF16, device="cuda")
    xw = xbig[1 : M + 1, :K]
    xw.copy_(x)
    xcopy = xbig.clone()
    qbig = torch.full((M + 4, K + 16), QPOISON, dtype=U8, device="cuda")
    q = qbig[2 : M + 2, :K]
    n = (K // 128) * M * 4
    tbuf = torch.full((n + 256,), QPOISON, dtype=U8, device="cuda")
    tab = tbuf[68 : 68 + n]
    assert xw.data_ptr() % 16 == 0 and q.data_ptr() % 8 == 0 and tab.data_ptr() % 4 == 0 and xw.stride(0) > K and q.stride(0) > K
    lib._check(lib._lib.x2v_quant_mxfp8_bf16(xw.data_ptr(), xw.stride(0), q.data_ptr(), q.stride(0), tab.data_ptr(), M, K, lib._stream()), "quant_mxfp8")
    assert poison_intact(qbig, M, K, QPOISON), "wrote outside q"
    assert bool((tbuf[:68] == QPOISON).all() and (tbuf[68 + n :] == QPOISON).all()), "wrote outside the scale table"
    assert torch.equal(xbig.view(torch.int16), xcopy.view(torch.int16)), "x was written"  # by bits: x may hold a NaN
    return q.cpu(), X.rowmajor(tab.view(K // 128, M, 4).cpu())


def check_quant(name, what, got, ref, keep=None):
    """Codes and scale bytes bit for bit; keep = (code mask [M, K], scale mask [M, K / 32]) of what is compared."""
    from tests.util import record

    (q, sc), (rq, rs) = got, ref
    assert q.shape == rq.shape and sc.shape == rs.shape and q.dtype == U8 and sc.dtype == U8
    dq, ds = q != rq, sc != rs
    if keep is not None:
        dq, ds = dq & keep[0], ds & keep[1]
    nq, ns = int(dq.sum()), int(ds.sum())
    QROWS.append((name, what, nq, ns, q.numel()))
    record(f"mx_fp64 {name} {what}", rule="exact", unequal_codes=nq, unequal_scale_bytes=ns, elements=q.numel())
    if nq or ns:
        i = int(dq.reshape(-1).to(torch.int32).argmax()) if nq else int(ds.reshape(-1).to(torch.int32).argmax()) * 32
        m, k = divmod(i, q.shape[1])
        raise AssertionError(f"{name} {what}: {nq} of {q.numel()} codes and {ns} of {sc.numel()} scale bytes differ; first at ({m}, {k}): code {int(q[m, k]):#04x} want "
                             f"{int(rq[m, k]):#04x}, scale byte {int(sc[m, k // 32])} want {int(rs[m, k // 32])}")


@pytest.mark.parametrize("pin", sorted(X.PINS))
def test_quant_sweep(lib, pin):
    """Slot 0 of every block pins the maximum; the other slots run through every finite bf16 bit pattern not above it, both signs, both zeros."""
    x, n = X.sweep(X.PINS[pin])
    q, sc = lib.quant_mxfp8(x.cuda())
    check_quant("quant sweep", f"pin {pin} ({n} patterns)", (q.view(U8).cpu(), X.rowmajor(sc.cpu())), X.quant(x))


@pytest.mark.parametrize("M,K", X.QUANT_LAYOUT)
def test_quant_layout_and_strides(lib, M, K):
    """Rows that do not fill a wave, ldx > K and ldq > K together, q and the table inside poisoned buffers, an all-zero block next to non-zero ones, a
    block of -0."""
    x = X.quant_input(M, K)
    check_quant("quant layout", f"{M}x{K} ldx={K + 8} ldq={K + 16}", quant_call(lib, x), X.quant(x))


@pytest.mark.parametrize("M,K", X.QUANT_GRID)
def test_quant_grid_stride(lib, M, K):
    """M K / 8 just above, and 2.5 times, the 8192 blocks x 256 lanes of the capped grid (the second with a ragged M): the second and third trip of
    the grid-stride loop, where the 14B workload lives."""
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-4, 4, M).unsqueeze(1)).to(BF16)
    q, sc = lib.quant_mxfp8(x.cuda())
    check_quant("quant grid stride", f"{M}x{K}", (q.view(U8).cpu(), X.rowmajor(sc.cpu())), X.quant(x))


@pytest.mark.parametrize("special", ("nan", "inf"))
def test_quant_isolation(lib, special):
    """One NaN / one +Inf element: every other block of its row and every other row has the codes and scale bytes of the same input with that
    element set to 0.  What the affected block holds is outside the contract (include/x2v.h): it is recorded, not asserted."""
    from tests.util import record

    M, K, r, k = 5, 256, 2, 72  # block 2 of row 2, next to that row's all-zero block
    b0 = k // 32 * 32
    x = X.quant_input(M, K)
    x[r, k] = 0.0
    ref = X.quant(x)
    xs = x.clone()
    xs[r, k] = float(special)
    q, sc = quant_call(lib, xs)
    keep_q, keep_s = torch.ones(M, K, dtype=torch.bool), torch.ones(M, K // 32, dtype=torch.bool)
    keep_q[r, b0 : b0 + 32], keep_s[r, k // 32] = False, False
    blk, rblk = q[r, b0 : b0 + 32], ref[0][r, b0 : b0 + 32]
    others = torch.arange(32) != k - b0
    others_as_ref = bool((blk[others] == rblk[others]).all())
    note = (f"quant isolation {special}: affected block has scale byte {int(sc[r, k // 32])} (with 0 in its place: {int(ref[1][r, k // 32])}), the element's code {int(blk[k - b0]):#04x}, "
            f"its other 31 codes {'equal' if others_as_ref else 'do not equal'} those with 0 in its place; distinct codes {sorted(set(blk.tolist()))[:8]}")
    print(note)
    NOTES.append(note)
    record(f"mx_fp64 quant isolation {special} affected block", scale_byte=int(sc[r, k // 32]), element_code=int(blk[k - b0]), others_as_with_zero=int(others_as_ref))
    check_quant("quant isolation", f"{special} at ({r}, {k}): all other blocks", (q, sc), ref, (keep_q, keep_s))
