"""MXFP4 (e2m1) x MXFP4 — quant_mx_kernel<3> of mx.hip and the fp4 modes of gemm.hip's 128x128 kernel and of gemm256.hip's 256x256 ping-pong kernel —
against the float64 references of tests/mx4_ref.py, at the smallest shapes at which each edge exists.  tests/test_mx4_ref_host.py shows which subtly
wrong kernels and quantisers this rejects.

Quantiser: packed codes and scale bytes BIT FOR BIT — every finite bf16 bit pattern under fifteen pinned block maxima (at and around 6 * 2^k, around
the denormal quotient 2^-127, bf16 subnormals, the largest finite bf16), rows that do not fill a wave with ldx > K and ldq > K/2 inside poisoned
buffers, the grid-stride loop past the capped grid, and a NaN or an Inf element leaving every other block untouched.

GEMM: both bodies forced through `variant` (the fused epilogues through x2v_gemm_mxfp4_epi, which only the 256x256 body has).  Family I is compared
BIT FOR BIT with the float64 chain, family R on EVERY element with gemm_ref's derived bound; no share of elements is left out.  Operands are windows
of loud buffers (lda, ldb > K/2, the first row not the allocation's), scale tables 4-byte aligned slices of a byte buffer of 0xFF, the output a
window (ldy > N) of a poisoned buffer whose surroundings are checked after each call; resid and both tables must come back unchanged.  Two diagnostic
walks (one-hot codes on either side) name the k a wrong code <-> k map reads, before the bit comparisons only say 'differs'."""
import os

import pytest
import torch

from tests import gemm_ref as G
from tests import mx4_ref as R
from tests import mx_ref as X

pytestmark = pytest.mark.gpu
POISON = -1984.0  # exact in bf16
QPOISON = 0xA5
BF16, U8 = torch.bfloat16, torch.uint8
BODY = R.BODY
CASES, QROWS, NOTES, _INPUTS, _EXPECT = {}, [], [], {}, {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_MX4_PARITY_TABLE")  # where to write the table of measured ratios (profiles/mx4_fp64_parity.txt is one run's)
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
    return CASES.setdefault(name, G.Case(name, prefix="mx4_fp64"))


# ------------------------------------------------------------------------------------------------------------------- buffers
def operand(codes, loud, pad=16):
    """Bytes [rows, W] as a window one row down in a buffer of `loud` bytes with `pad` bytes more per row."""
    rows, W = codes.shape
    big = torch.full((rows + 2, W + pad), loud, dtype=U8, device="cuda")
    win = big[1 : rows + 1, :W]
    win.copy_(codes)
    assert win.data_ptr() % 16 == 0 and win.stride(0) > W and win.stride(0) % 16 == 0
    return win


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
    big = torch.full((M + 4, N + 8), POISON, dtype=BF16, device="cuda")
    return big, big[2 : M + 2, :N]


def poison_intact(big, M, N, value=POISON):
    return bool((big[:2] == value).all() and (big[M + 2 :] == value).all() and (big[2 : M + 2, N:] == value).all())


class Dev:
    """The device side of an Inputs: a = packed e2m1 window in a buffer of 6s (0x77 bytes), b = packed e2m1 window in a buffer of -6s (0xFF), tables."""

    def __init__(self, inp):
        self.inp = inp
        self.a = operand(inp.a_packed.cuda(), 0x77)
        self.b = operand(inp.b_packed.cuda(), 0xFF, pad=32)
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
        inp = R.Inputs(family, M, N, K, flat_a=flat_a, device="cuda" if big else "cpu")
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
    """One call into a poisoned window; returns the window.  entry 'variant': x2v_gemm_mxfp4_variant (no epilogue), 'epi': x2v_gemm_mxfp4_epi."""
    inp = d.inp
    big, y = out_window(inp.M, inp.N)
    assert y.data_ptr() % 16 == 0 and y.stride(0) == inp.N + 8
    alpha, bias = d.alpha if use_alpha else None, d.bias if use_bias else None
    assert not use_bias or bias is not None
    if entry == "variant":
        assert epi == G.EPI_NONE
        lib.gemm_mxfp4(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, out=y, variant=variant)
    elif epi == G.EPI_NONE:  # the shim sends an epilogue-free call to the variant entry: call the epilogue entry itself
        p = lambda t: None if t is None else t.data_ptr()
        lib._check(lib._lib.x2v_gemm_mxfp4_epi(p(d.a), d.a.stride(0), p(d.sa), p(d.b), d.b.stride(0), p(d.sb), p(bias), p(alpha), p(y), y.stride(0), inp.M, inp.N, inp.K, epi,
                                               None, 0, None, lib._stream()), "gemm_mxfp4_epi")
    elif epi == G.EPI_RESIDUAL and in_place:
        y.copy_(d.resid)
        out = lib.gemm_mxfp4(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, epilogue=epi, resid=y, gate=d.gate if use_gate else None)
        assert out.data_ptr() == y.data_ptr()
    else:
        kw = dict(resid=d.resid, gate=d.gate if use_gate else None) if epi == G.EPI_RESIDUAL else {}
        lib.gemm_mxfp4(d.a, d.sa, d.b, d.sb, alpha=alpha, bias=bias, epilogue=epi, out=y, **kw)
    assert poison_intact(big, inp.M, inp.N), "wrote outside the output window"
    assert torch.equal(d.resid_big, d.resid_copy), "resid was written"
    assert torch.equal(d.sa_buf, d.sa_copy) and torch.equal(d.sb_buf, d.sb_copy), "a scale table was written"
    return y


def views(family, M, N, K):
    """(view, Dev, bias?) with and without alpha, with and without bias (tests/test_gpu_mx_fp64.py::views)."""
    if family == "R":
        inp, d = inputs("R", M, N, K)
        return [(inp.scaled(ua), d, ub) for ua in (True, False) for ub in (True, False)]
    out = []
    for flat in (False, True):
        inp, d = inputs("I", M, N, K, flat)
        out += [(inp.scaled(ua), d, flat) for ua in (True, False)]
    return out


def check_body(lib, name, M, N, K, variants=(1, 2)):
    """NONE through both forced bodies, both families, every (alpha, bias) combination, against the one reference of each."""
    for family in ("I", "R"):
        for v, d, use_bias in views(family, M, N, K):
            exp = expect(v, G.EPI_NONE, use_bias)
            for variant in variants:
                case(name).check(run(lib, d, G.EPI_NONE, v.alpha_used is not None, use_bias, variant=variant), exp, BODY[variant])


# ------------------------------------------------------------------------------------------------------------------- diagnostic walks
def _unit_tables(M, N, K):
    return (X.tiled(torch.full((M, K // 32), 127, dtype=U8)).cuda(), X.tiled(torch.full((N, K // 32), 127, dtype=U8)).cuda())


E2M1_INTS = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0, -1.0, -2.0, -3.0, -4.0, -6.0, 0.0], dtype=G.F64)


@pytest.mark.parametrize("side", ("b", "a"))
@pytest.mark.parametrize("variant", (1, 2))
def test_one_hot_walk_names_the_k_of_every_code(lib, variant, side):
    """K = 256, one operand one-hot (the code of 1.0 at k0(row) = (37 row + 5) mod 256: every k, so both nibbles of every byte), the other
    v[r, k] = E2M1_INTS[(3 k + r) mod 11], unit scales: y == v[:, k0] exactly.  A wrong code <-> k map fails here with the k it read instead.  (The same
    exchange of codes inside a scale block on BOTH operands leaves every product as it is: it cannot be seen, and does not matter.)"""
    H, D, K = 264, 136, 256  # rows of the one-hot operand, of the dense one
    k0 = (37 * torch.arange(H) + 5) % K
    hot = torch.zeros(H, K, dtype=U8)
    hot[torch.arange(H), k0] = int(R.e2m1_codes(torch.tensor([1.0], dtype=G.F64)))
    v = E2M1_INTS[(3 * torch.arange(K)[None, :] + torch.arange(D)[:, None]) % 11]
    dense = R.e2m1_codes(v)
    a, b = (dense, hot) if side == "b" else (hot, dense)
    sa, sb = _unit_tables(a.shape[0], b.shape[0], K)
    y = lib.gemm_mxfp4(R.pack4(a).cuda(), sa, R.pack4(b).cuda(), sb, variant=variant).float().cpu().double()
    y = y if side == "b" else y.T  # [dense row, one-hot row]
    want = v[:, k0]
    bad = (y != want).any(0).nonzero().flatten()
    if bad.numel():
        n = int(bad[0])
        reads = [k for k in range(K) if bool((v[:, k] == y[:, n]).all())]
        raise AssertionError(f"{BODY[variant]}, one-hot {side}: {bad.numel()} of {H} rows wrong; row {n}: its code sits at k = {int(k0[n])} (byte {int(k0[n]) // 2}, nibble {int(k0[n]) % 2}, "
                             f"16-byte chunk {int(k0[n]) // 32}), the kernel paired it with the other operand's k in {reads[:6] or 'no single k'}; "
                             f"y[0..3] = {y[:4, n].tolist()} want {want[:4, n].tolist()}")


@pytest.mark.parametrize("side", ("a", "b"))
def test_scale_byte_to_k_block_association(lib, side):
    """Across BOTH dwords of a 256-wide K-tile: scale byte j of a row's eight applies to k block j and to nothing else, on either operand and in
    either body (data only in block j: doubling byte i doubles the result iff i == j)."""
    M = N = 32
    K = 256
    one = int(R.e2m1_codes(torch.tensor([1.0], dtype=G.F64)))
    for j in range(8):
        a, b = torch.zeros(M, K, dtype=U8), torch.zeros(N, K, dtype=U8)
        if side == "a":
            a[:, 32 * j : 32 * j + 32], b[:] = one, one
        else:
            a[:], b[:, 32 * j : 32 * j + 32] = one, one
        ap, bp = R.pack4(a).cuda(), R.pack4(b).cuda()
        for i in range(8):
            sa, sb = torch.full((M, 8), 127, dtype=U8), torch.full((N, 8), 127, dtype=U8)
            (sa if side == "a" else sb)[:, i] = 128
            for variant in (1, 2):
                y = lib.gemm_mxfp4(ap, X.tiled(sa).cuda(), bp, X.tiled(sb).cuda(), variant=variant).float().cpu()
                assert (y == (64.0 if i == j else 32.0)).all(), (side, j, i, variant, y[0, 0].item())


# ------------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("nk", R.K_TILES)
def test_k_loop(lib, nk):
    """1..5 and 9 K tiles of 256: the 128x128 body's ring parity and its last tile without a prefetch; the 256x256 body's prologue below LEAD
    half-tiles (one K tile), exactly one ring (two), the checked tail, odd and even trip counts — two scale-table entries per K tile.  M = 257 and
    N = 264 leave a ragged tile in both directions for either tile size."""
    M, N = X.K_TILES_MN
    check_body(lib, "k loop", M, N, nk * R.KTILE4)


@pytest.mark.parametrize("M", R.M_TAILS)
def test_m_tails(lib, M):
    check_body(lib, "m tails", M, 136, R.TAIL_K)


@pytest.mark.parametrize("N", R.N_TAILS)
def test_n_tails(lib, N):
    """One 8-column group, one short of, exactly and one past 128 and 256 columns: clamped (128x128) or zero-filled (256x256) weight rows are read,
    never stored."""
    check_body(lib, "n tails", 129, N, R.TAIL_K)


@pytest.mark.parametrize("M,N,K", R.SCHED)
def test_scheduling_groups(lib, M, N, K):
    check_body(lib, "scheduling groups", M, N, K)


@pytest.mark.parametrize("M,N,K", R.DEEP)
def test_deep_k(lib, M, N, K):
    """K = 13824 (54 K tiles): a K tile dropped, doubled or taken from the wrong stage, or a scale dword adopted late, anywhere in a long loop."""
    check_body(lib, "deep k", M, N, K)


@pytest.mark.parametrize("M,N,K", R.EPI_SHAPES)
def test_epilogues(lib, M, N, K):
    """x2v_gemm_mxfp4_epi: NONE (whichever body the shape gets), and on the 256x256 body GELU_TANH, SILU, RESIDUAL with a gate, without one and in
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
                body = "epi entry, " + (BODY[R.auto_body(M, N, K)] if epi == G.EPI_NONE else BODY[2])
                case("epilogues").check(run(lib, d, epi, use_bias, use_bias, use_gate, entry="epi"), exp, body)
                if epi == G.EPI_RESIDUAL:
                    case("epilogues").check(run(lib, d, epi, use_bias, use_bias, use_gate, entry="epi", in_place=True), exp, body + " in place")


@pytest.mark.parametrize("M,N,K", R.AUTO)
def test_automatic_choice(lib, M, N, K):
    """variant = 0 just above and just below this mode's rule, MXFP8's on the K tiles of 256 with 6 in place of 8: `tiles256 >= 192 && K / 256 >= 6`
    (6 K tiles -> the 256x256 body, 5 -> the 128x128 body).  Family I: the result equals the float64 chain and the forced variant's output bit for bit (this pins the
    correctness of whatever runs, not the choice).  The float64 side of this shape lives on the device."""
    inp, d = inputs("I", M, N, K)
    for use_alpha in (True, False):
        v = inp.scaled(use_alpha)
        exp = expect(v, G.EPI_NONE, False)
        got = run(lib, d, G.EPI_NONE, use_alpha, False, variant=0)
        case("automatic choice").check(got, exp, "variant 0")
        forced = run(lib, d, G.EPI_NONE, use_alpha, False, variant=R.auto_body(M, N, K))
        assert torch.equal(got.view(torch.int16), forced.view(torch.int16)), "variant 0 and the forced variant differ"
        case("automatic choice").check(forced, exp, BODY[R.auto_body(M, N, K)])


# ------------------------------------------------------------------------------------------------------------------- quantiser
def quant_call(lib, x):
    """x2v_quant_mxfp4_bf16 with ldx > K and ldq > K/2: x a window of a loud buffer, q and the scale table inside poisoned buffers whose surroundings
    are checked.  Returns (codes [M, K] unpacked, scale bytes [M, K / 32]) on the CPU."""
    M, K = x.shape
    W = K // 2
    xbig = torch.full((M + 2, K + 8), 3.0e4, dtype=BF16, device="cuda")
    xw = xbig[1 : M + 1, :K]
    xw.copy_(x)
    xcopy = xbig.clone()
    qbig = torch.full((M + 4, W + 24), QPOISON, dtype=U8, device="cuda")
    q = qbig[2 : M + 2, :W]
    n = (K // 128) * M * 4
    tbuf = torch.full((n + 256,), QPOISON, dtype=U8, device="cuda")
    tab = tbuf[68 : 68 + n]
    assert xw.data_ptr() % 16 == 0 and q.data_ptr() % 8 == 0 and tab.data_ptr() % 4 == 0 and xw.stride(0) > K and q.stride(0) > W
    lib._check(lib._lib.x2v_quant_mxfp4_bf16(xw.data_ptr(), xw.stride(0), q.data_ptr(), q.stride(0), tab.data_ptr(), M, K, lib._stream()), "quant_mxfp4")
    assert poison_intact(qbig, M, W, QPOISON), "wrote outside q"
    assert bool((tbuf[:68] == QPOISON).all() and (tbuf[68 + n :] == QPOISON).all()), "wrote outside the scale table"
    assert torch.equal(xbig.view(torch.int16), xcopy.view(torch.int16)), "x was written"  # by bits: x may hold a NaN
    return R.unpack4(q.cpu()), X.rowmajor(tab.view(K // 128, M, 4).cpu())


def check_quant(name, what, got, ref, keep=None):
    """Codes (unpacked: unpack4 is a bijection of the packed bytes) and scale bytes bit for bit; keep = (code mask, scale mask) of what is compared."""
    from tests.util import record

    (q, sc), (rq, rs) = got, ref
    assert q.shape == rq.shape and sc.shape == rs.shape and q.dtype == U8 and sc.dtype == U8
    dq, ds = q != rq, sc != rs
    if keep is not None:
        dq, ds = dq & keep[0], ds & keep[1]
    nq, ns = int(dq.sum()), int(ds.sum())
    QROWS.append((name, what, nq, ns, q.numel()))
    record(f"mx4_fp64 {name} {what}", rule="exact", unequal_codes=nq, unequal_scale_bytes=ns, elements=q.numel())
    if nq or ns:
        i = int(dq.reshape(-1).to(torch.int32).argmax()) if nq else int(ds.reshape(-1).to(torch.int32).argmax()) * 32
        m, k = divmod(i, q.shape[1])
        raise AssertionError(f"{name} {what}: {nq} of {q.numel()} codes and {ns} of {sc.numel()} scale bytes differ; first at ({m}, {k}): code {int(q[m, k]):#03x} want "
                             f"{int(rq[m, k]):#03x}, scale byte {int(sc[m, k // 32])} want {int(rs[m, k // 32])}")


@pytest.mark.parametrize("pin", sorted(R.PINS))
def test_quant_sweep(lib, pin):
    """Slot 0 of every block pins the maximum; the other slots run through every finite bf16 bit pattern not above it, both signs, both zeros."""
    x, n = X.sweep(R.PINS[pin])
    q, sc = lib.quant_mxfp4(x.cuda())
    assert q.dtype == U8 and q.shape == (x.shape[0], 64) and sc.shape == (1, x.shape[0], 4)
    check_quant("quant sweep", f"pin {pin} ({n} patterns)", (R.unpack4(q.cpu()), lib.mx_scales_rowmajor(sc).cpu()), R.quant4(x))


@pytest.mark.parametrize("M,K", X.QUANT_LAYOUT)
def test_quant_layout_and_strides(lib, M, K):
    """Rows that do not fill a wave, ldx > K and ldq > K/2 together, q and the table inside poisoned buffers (the bytes past a row untouched), an
    all-zero block next to non-zero ones, a block of -0, a block at 6."""
    x = R.quant_input(M, K)
    check_quant("quant layout", f"{M}x{K} ldx={K + 8} ldq={K // 2 + 24}", quant_call(lib, x), R.quant4(x))


@pytest.mark.parametrize("M,K", R.QUANT_GRID)
def test_quant_grid_stride(lib, M, K):
    """M K / 16 just above the 4096 blocks x 256 lanes of the capped grid, with a ragged M: the second trip of the grid-stride loop."""
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-4, 4, M).unsqueeze(1)).to(BF16)
    q, sc = lib.quant_mxfp4(x.cuda())
    check_quant("quant grid stride", f"{M}x{K}", (R.unpack4(q.cpu()), X.rowmajor(sc.cpu())), R.quant4(x))


@pytest.mark.parametrize("special", ("nan", "inf"))
def test_quant_isolation(lib, special):
    """One NaN / one +Inf element: every other block of its row and every other row has the codes and scale bytes of the same input with that
    element set to 0.  What the affected block holds is outside the contract (include/x2v.h): it is recorded, not asserted."""
    from tests.util import record

    M, K, r, k = 5, 256, 2, 72  # block 2 of row 2, next to that row's all-zero block
    b0 = k // 32 * 32
    x = R.quant_input(M, K)
    x[r, k] = 0.0
    ref = R.quant4(x)
    xs = x.clone()
    xs[r, k] = float(special)
    q, sc = quant_call(lib, xs)
    keep_q, keep_s = torch.ones(M, K, dtype=torch.bool), torch.ones(M, K // 32, dtype=torch.bool)
    keep_q[r, b0 : b0 + 32], keep_s[r, k // 32] = False, False
    blk, rblk = q[r, b0 : b0 + 32], ref[0][r, b0 : b0 + 32]
    others = torch.arange(32) != k - b0
    others_as_ref = bool((blk[others] == rblk[others]).all())
    note = (f"quant isolation {special}: affected block has scale byte {int(sc[r, k // 32])} (with 0 in its place: {int(ref[1][r, k // 32])}), the element's code {int(blk[k - b0]):#03x}, "
            f"its other 31 codes {'equal' if others_as_ref else 'do not equal'} those with 0 in its place; distinct codes {sorted(set(blk.tolist()))[:8]}")
    print(note)
    NOTES.append(note)
    record(f"mx4_fp64 quant isolation {special} affected block", scale_byte=int(sc[r, k // 32]), element_code=int(blk[k - b0]), others_as_with_zero=int(others_as_ref))
    check_quant("quant isolation", f"{special} at ({r}, {k}): all other blocks", (q, sc), ref, (keep_q, keep_s))


# ------------------------------------------------------------------------------------------------------------------- acceptance
@pytest.mark.parametrize("m,k,n", R.ACCEPT)
def test_quantise_then_multiply(lib, m, k, n):
    """The usage pattern of the mirrored Python API at the reference's acceptance shapes: scaled_mxfp4_quant of a random activation and weight
    equals quant4 byte for byte, and scaled_mxfp4_mm of the two equals the float64 chain of the quantised operands under the family-R rule.  The
    distance to the product of the bf16 operands — the price of 4 bits — is recorded, not bounded."""
    from lightx2v_amd.mx import scaled_mxfp4_mm, scaled_mxfp4_quant
    from tests.util import record, rel_l2

    g = torch.Generator().manual_seed(m)
    x, w = torch.randn(m, k, generator=g).to(BF16), torch.randn(n, k, generator=g).to(BF16)
    bias = (torch.rand(n, generator=g) * 10).to(BF16)
    inp = R.given(x, w, bias, device="cuda")
    aq, asc = scaled_mxfp4_quant(x.cuda())
    wq, wsc = scaled_mxfp4_quant(w.cuda())
    assert aq.dtype == U8 and aq.shape == (m, k // 2) and wq.shape == (n, k // 2)
    check_quant("acceptance", f"activation {m}x{k}", (R.unpack4(aq).cpu(), X.rowmajor(asc.view(U8)).cpu()), (inp.a.cpu(), inp.sa.cpu()))
    check_quant("acceptance", f"weight {n}x{k}", (R.unpack4(wq).cpu(), X.rowmajor(wsc.view(U8)).cpu()), (inp.b.cpu(), inp.sb.cpu()))
    alpha = torch.tensor([1.0], device="cuda", dtype=torch.float32)
    pred = scaled_mxfp4_mm(aq, wq, asc, wsc, alpha=alpha, bias=bias.cuda().reshape(1, n))
    assert pred.shape == (m, n) and pred.dtype == BF16
    case("acceptance").check(pred, G.Expect(inp.scaled(False), G.EPI_NONE, True, False), "scaled_mxfp4_mm, " + BODY[R.auto_body(m, n, k)])
    real = torch.nn.functional.linear(x.cuda().float(), w.cuda().float(), bias.cuda().float())
    rel = rel_l2(pred.float().cpu(), real.cpu())
    NOTES.append(f"acceptance ({m}, {k}, {n}): rel_l2 of the MXFP4 product against the product of the bf16 operands {rel:.3e} (recorded, not bounded)")
    record(f"mx4 acceptance {m}x{k}x{n}", rel_l2_vs_bf16_operands=rel)


# ------------------------------------------------------------------------------------------------------------------- operator class
def test_operator_class(lib):
    """MMWeightMxfp4Hip: `load` quantises a [N, K] weight on the device to quant4's bytes; `apply` equals the float64 chain of quantise-then-multiply
    under the family-R rule; `row_slice` with a shared `quantized=` input equals the slice of the full product bit for bit; `state_dict` round-trips
    through `load` bit for bit; the fused epilogues reach the kernel."""
    from lightx2v_amd import ops

    N, K, M = 264, 512, 77
    g = torch.Generator().manual_seed(4)
    w, bias, x = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16), torch.randn(N, generator=g).to(BF16), torch.randn(M, K, generator=g).to(BF16)
    op = ops.MMWeightMxfp4Hip("blk.weight", "blk.bias")
    op.set_config({})
    op.load({"blk.weight": w.float().cuda(), "blk.bias": bias.cuda()})  # an fp32 checkpoint tensor
    inp = R.given(x, w, bias)
    assert op.weight.dtype == U8 and op.weight.shape == (N, K // 2) and op.weight_scale.shape == (K // 128, N, 4)
    assert torch.equal(op.weight.cpu(), inp.b_packed) and torch.equal(X.rowmajor(op.weight_scale.cpu()), inp.sb)
    xq = op.quantize_input(x.cuda())
    assert torch.equal(xq[0].cpu(), inp.a_packed) and torch.equal(X.rowmajor(xq[1].cpu()), inp.sa)
    full = op.apply(x.cuda())
    case("operator class").check(full, G.Expect(inp.scaled(False), G.EPI_NONE, True, False), "apply")
    case("operator class").check(op.apply(x.cuda(), epilogue=lib.EPI_GELU_TANH), G.Expect(inp.scaled(False), G.EPI_GELU, True, False), "apply, " + BODY[2])
    rs = slice(8, N - 16)
    part = op.apply(x.cuda(), row_slice=rs, quantized=xq)
    assert full.shape == (M, N) and torch.equal(part.view(torch.int16), full[:, rs].contiguous().view(torch.int16))
    sd = op.state_dict()
    assert set(sd) == {"blk.weight", "blk.weight_scale", "blk.bias"} and sd["blk.weight"].dtype == U8 and sd["blk.weight"].shape == (N, K // 2)
    assert sd["blk.weight_scale"].shape == (K // 128, N, 4)
    op2 = ops.MMWeightMxfp4Hip("blk.weight", "blk.bias")
    op2.set_config({})
    op2.load({k: v.cuda() for k, v in sd.items()})
    assert torch.equal(op2.weight, op.weight) and torch.equal(op2.weight_scale, op.weight_scale)
    assert torch.equal(op2.apply(x.cuda()).view(torch.int16), full.view(torch.int16))
    sd2 = op2.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(sd2[k], sd[k]) for k in sd)
