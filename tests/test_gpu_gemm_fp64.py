"""Every GEMM kernel body — gemm.hip's 128x128 kernel (bf16, e4m3, int8), gemm256.hip's ping-pong kernel (bf16, e4m3), gemm256s.hip's one-tile form
and its V^T form, gemm256c.hip and gemm256c8.hip (e4m3, int8) — forced through x2v_gemm_*_variant at the smallest shapes at which each edge exists,
against the float64 references of tests/gemm_ref.py: the K loop's prologue and tail at 1..9 K tiles, the M and N tails inside a tile, the scheduling
group and XCD remap with a ragged tile count, a persistent workgroup's second and third output tile, K = 13824, the blocked, periodic and V^T
entries.  Family I (integers) is compared BIT FOR BIT with the float64 chain, family R on EVERY element with the derived bound; no share of
elements is left out anywhere.  tests/test_gemm_ref_host.py shows which subtly wrong kernels this rejects.

Every call reads x, W and resid as windows of larger buffers filled with loud values (ldx > K, ldw > K, the first row not the allocation's, rows
16-byte aligned as the ABI asks) and writes a window of a poisoned buffer (ldy > N) whose surroundings are checked afterwards; resid must come
back unchanged.  One Inputs / Expect per (family, shape, dtype) serves every body that accepts the shape.  Variants are forced; where an entry has
no variant argument (the blocked entries, x2v_gemm_bf16_vt) the test asserts through gemm_kernel_choice / gemm_int8_kernel_choice which body runs.
None sets X2V_GEMM_CONTINUOUS / X2V_GEMM_FP8_CONTINUOUS."""
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
POISON = -1984.0  # exact in bf16
BF16 = torch.bfloat16
CASES, _INPUTS, _EXPECT = {}, {}, {}
I_EPILOGUES = tuple(e for e in G.EPILOGUES if e[0] in (G.EPI_NONE, G.EPI_RESIDUAL))


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_GEMM_PARITY_TABLE")  # where to write the table of measured ratios (profiles/gemm_fp64_parity.txt is one run's)
    if not path:
        return
    try:
        with open(path, "w") as f:
            for name in sorted(CASES):
                f.write(CASES[name].header() + "\n")
            for name in sorted(CASES):
                f.write("\n".join(CASES[name].table()) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def case(name):
    return CASES.setdefault(name, G.Case(name))


# ------------------------------------------------------------------------------------------------------------------- buffers
def loud(shape, dtype):
    """A device buffer of values that would show in any result they reached."""
    return torch.full(shape, {BF16: 3.0e4, G.E4M3: 448.0, G.I8: 127.0}[dtype], dtype=torch.float32, device="cuda").to(dtype)


def operand(t, blocks=0):
    """t [rows, cols] as a window one row down in a loud buffer with 16 bytes more per row; blocks = 2: the K-blocked form [2, rows, cols / 2] in a
    loud [2, rows + 2, cols / 2 + pad] buffer."""
    pad = 16 // t.element_size()
    rows, cols = t.shape
    if blocks:
        big = loud((blocks, rows + 2, cols // blocks + pad), t.dtype)
        win = big[:, 1 : rows + 1, : cols // blocks]
        win.copy_(t.reshape(rows, blocks, cols // blocks).permute(1, 0, 2))
    else:
        big = loud((rows + 2, cols + pad), t.dtype)
        win = big[1 : rows + 1, :cols]
        win.copy_(t)
    assert win.data_ptr() % 16 == 0 and win.stride(-2) > win.shape[-1]
    return win


def out_window(M, N, blocks=0):
    """A poisoned buffer and its [M, N] window two rows down with ldy = N + 8 (N-blocked: [2, M, N / 2] in [2, M + 4, N / 2 + 8])."""
    if blocks:
        big = torch.full((blocks, M + 4, N // blocks + 8), POISON, dtype=BF16, device="cuda")
        return big, big[:, 2 : M + 2, : N // blocks]
    big = torch.full((M + 4, N + 8), POISON, dtype=BF16, device="cuda")
    return big, big[2 : M + 2, :N]


def poison_intact(big, M, N):
    """Everything of `big` outside the window out_window cut from it."""
    n = N // big.shape[0] if big.dim() == 3 else N
    return bool((big[..., :2, :] == POISON).all() and (big[..., M + 2 :, :] == POISON).all() and (big[..., 2 : M + 2, n:] == POISON).all())


class Dev:
    """The device side of an Inputs: operand windows, made once."""

    def __init__(self, inp):
        self.inp = inp
        self.x, self.w = operand(inp.x.cuda()), operand(inp.w.cuda())
        self.bias, self.gate = inp.bias.cuda().contiguous(), inp.gate.cuda().contiguous()
        self.sx, self.sw = (None, None) if inp.sx is None else (inp.sx.cuda().contiguous(), inp.sw.cuda().contiguous())
        R = inp.resid.shape[0]
        self.resid_big = torch.full((R + 4, inp.N + 8), POISON, dtype=BF16, device="cuda")  # y's row stride: what the continuous forms ask of resid
        self.resid = self.resid_big[2 : R + 2, : inp.N]
        self.resid.copy_(inp.resid)
        self.resid_copy = self.resid_big.clone()
        self._xb = None

    @property
    def x_kblocked(self):
        if self._xb is None:
            self._xb = operand(self.inp.x.cuda(), blocks=2)
        return self._xb


def inputs(family, dtype, M, N, K, resid_rows=None):
    """(Inputs, Dev) of a shape, made once per module run; the float64 side of the large shapes lives on the device (rocBLAS's float64 matmul and
    torch's elementwise kernels are independent of the kernels under test), the small ones' on the CPU."""
    key = (family, dtype, M, N, K, resid_rows)
    if key not in _INPUTS:
        inp = G.Inputs(family, dtype, M, N, K, resid_rows=resid_rows, device="cuda" if M * N > (1 << 19) else "cpu")
        if family == "I":
            inp.assert_exercises_roundings()
        if M * N > (1 << 22):  # large cases are used by one test
            return inp, Dev(inp)
        _INPUTS[key] = (inp, Dev(inp))
    return _INPUTS[key]


def expect(inp, epi, use_bias=True, use_gate=True, period=0):
    key = (inp.family, inp.dtype, inp.M, inp.N, inp.K, inp.resid.shape[0], epi, use_bias, use_gate, period)
    if inp.M * inp.N > (1 << 22):
        return G.Expect(inp, epi, use_bias, use_gate, period)
    if key not in _EXPECT:
        _EXPECT[key] = G.Expect(inp, epi, use_bias, use_gate, period)
    return _EXPECT[key]


def run(lib, d, epi, use_bias, use_gate, variant, period=0):
    """One forced-variant call into a poisoned window; returns the window."""
    inp = d.inp
    big, y = out_window(inp.M, inp.N)
    assert y.data_ptr() % 16 == 0 and y.stride(0) == inp.N + 8
    kw = dict(bias=d.bias if use_bias else None, epilogue=epi, out=y, variant=variant)
    if epi == G.EPI_RESIDUAL:
        kw.update(resid=d.resid, gate=d.gate if use_gate else None, resid_period=period)
    if inp.dtype == "bf16":
        lib.gemm(d.x, d.w, **kw)
    else:
        (lib.gemm_fp8 if inp.dtype == "e4m3" else lib.gemm_int8)(d.x, d.sx, d.w, d.sw, **kw)
    assert poison_intact(big, inp.M, inp.N), "wrote outside the output window"
    assert torch.equal(d.resid_big, d.resid_copy), "resid was written"
    return y


def check_bodies(lib, name, family, dtype, M, N, K, variants, epilogues=None, group=0, resid_rows=None, period=0, what=""):
    """Every body of `variants` that accepts the shape against the one reference of (family, shape, dtype)."""
    inp, d = inputs(family, dtype, M, N, K, resid_rows)
    ran = 0
    for epi, use_bias, use_gate in epilogues or (I_EPILOGUES if family == "I" else G.EPILOGUES):
        exp = expect(inp, epi, use_bias, use_gate, period)
        for v in variants:
            if not G.accepts(dtype, v, N, K):
                continue
            got = run(lib, d, epi, use_bias, use_gate, v | (group << 8), period)
            case(name).check(got, exp, G.BODY[dtype, v] + (f" g={group}" if group else "") + what)
            ran += 1
    assert ran, "no body accepted the shape"


def tiles256(dtype):
    return tuple(v for v in G.VARIANTS[dtype] if v != 1)


def test_reference_rounding_on_the_device():
    """The float64 side of the large shapes runs on the device: its rounding must be the CPU's, ties included."""
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(1 << 16, generator=g, dtype=G.F64) * 300, torch.randint(-4096, 4096, (1 << 16,), generator=g).to(G.F64) / 8])
    for mode in ("rne", "half_up", "trunc"):
        assert torch.equal(G.round_bf16(v.cuda(), mode).cpu(), G.round_bf16(v, mode))


# ------------------------------------------------------------------------------------------------------------------- K loop
@pytest.mark.parametrize("nk", G.K_TILES)
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_k_loop(lib, dtype, nk):
    """1..9 K tiles through the 128x128, ping-pong and one-tile bodies: prologue only, prologue + tail, odd and even trip counts; M = 300 and N = 264
    leave a ragged tile in both directions for either tile size."""
    M, N = G.K_TILES_MN
    for family in ("I", "R"):
        check_bodies(lib, "k loop", family, dtype, M, N, nk * G.KTILE[dtype], [v for v in G.VARIANTS[dtype] if v != 5])


@pytest.mark.parametrize("nk", G.K_TILES_CONT)
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_k_loop_continuous(lib, dtype, nk):
    """4, 6 and 8 K tiles through the continuous forms (two output tiles at M = 300: the K loop runs on into the second)."""
    for family in ("I", "R"):
        check_bodies(lib, "k loop continuous", family, dtype, 300, 256, nk * G.KTILE[dtype], [5])


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_continuous_refuses_what_it_cannot_run(lib, dtype):
    for nk, N in ((3, 256), (5, 256), (4, 264)):
        inp, d = inputs("I", dtype, 300, N, nk * G.KTILE[dtype])
        with pytest.raises(lib.X2VError):
            run(lib, d, G.EPI_NONE, True, False, 5)
    inp, d = inputs("I", dtype, 600, 256, 4 * G.KTILE[dtype], resid_rows=7)
    with pytest.raises(lib.X2VError):
        run(lib, d, G.EPI_RESIDUAL, True, True, 5, period=7)


# ------------------------------------------------------------------------------------------------------------------- M and N tails
@pytest.mark.parametrize("M", G.M_TAILS)
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_m_tails(lib, dtype, M):
    """One row, one short of and one past the 128-row wave pair and the 256-row tile, on every body."""
    for family in ("I", "R"):
        check_bodies(lib, "m tails", family, dtype, M, 256, G.mid_k(dtype), G.VARIANTS[dtype])


@pytest.mark.parametrize("N", G.N_TAILS)
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_n_tails(lib, dtype, N):
    """One 8-column group, one group past 128, one short of and one past 256, one past 512."""
    for family in ("I", "R"):
        check_bodies(lib, "n tails", family, dtype, 129, N, G.mid_k(dtype), [v for v in G.VARIANTS[dtype] if v != 5])


# ------------------------------------------------------------------------------------------------------------------- tile order
SCHED_EPILOGUES = {"I": ((G.EPI_NONE, True, False), (G.EPI_RESIDUAL, True, True)), "R": ((G.EPI_NONE, True, False), (G.EPI_GELU, True, False), (G.EPI_RESIDUAL, True, True))}


@pytest.mark.parametrize("group", G.SCHED_GROUPS)
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_scheduling_groups(lib, dtype, group):
    """9 x 3 = 27 output tiles (no multiple of 8 XCDs) in groups of the default, 1 and 7 m-tiles (the last group ragged): every tile computed once,
    and in its place."""
    M, N = G.SCHED_MN
    for family in ("I", "R"):
        check_bodies(lib, "scheduling groups", family, dtype, M, N, G.mid_k(dtype), tiles256(dtype), SCHED_EPILOGUES[family], group=group)


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_scheduling_128(lib, dtype):
    """The 128x128 kernel's own grouping of 8 m-tiles at 9 x 3 tiles."""
    M, N = G.SCHED_128_MN
    for family in ("I", "R"):
        check_bodies(lib, "scheduling groups", family, dtype, M, N, G.mid_k(dtype), [1], SCHED_EPILOGUES[family])


@pytest.mark.parametrize("N", (256, 512))
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_persistent_later_tiles(lib, cus, dtype, N):
    """CUs + 1 and 2 CUs + 3 output tiles on the continuous forms: some workgroups run a second and a third tile, the others stop one earlier; the
    last m-tile is ragged."""
    for M in G.persistent_ms(cus, N // 256):
        assert -(-M // 256) * (N // 256) > cus and M % 256
        for family in ("I", "R"):
            check_bodies(lib, "persistent later tiles", family, dtype, M, N, 4 * G.KTILE[dtype], [5], SCHED_EPILOGUES[family])


# ------------------------------------------------------------------------------------------------------------------- deep K, periodic, blocked, V^T
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_deep_k(lib, dtype):
    """K = 13824 (216 / 108 K tiles), family I: a K tile dropped, doubled or taken from the wrong stage anywhere in a long loop changes the bits."""
    M, N, K = G.DEEP
    check_bodies(lib, "deep k", "I", dtype, M, N, K, G.VARIANTS[dtype])


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_resid_period(lib, dtype):
    """A residual of `period` rows under 600 output rows: 264 on the continuous forms (a multiple of 8 past one tile), 7 and 264 on the others."""
    K = 4 * G.KTILE[dtype]
    epi = ((G.EPI_RESIDUAL, True, True), (G.EPI_RESIDUAL, True, False))
    check_bodies(lib, "resid period", "I", dtype, 600, 256, K, [5], epi, resid_rows=264, period=264, what=" p=264")
    for period in (7, 264):
        check_bodies(lib, "resid period", "I", dtype, 600, 264, K, [v for v in G.VARIANTS[dtype] if v != 5], epi, resid_rows=period, period=period, what=f" p={period}")


def blocked_body(lib, dtype, M, N, K, y_blocked):
    """The body variant 0 gives a blocked call (gemm.hip dispatch_epi / dispatch_int8), read off the kernel-choice entries (which speak of a
    row-major x: ldx >= K there, and the strides used here are far from the span limits where they matter)."""
    pad = 8 if dtype == "bf16" else 16
    if dtype == "int8":
        fam, cont = lib.gemm_int8_kernel_choice(M, N, K, K + pad, K + pad, with_form=True)
    else:
        fam, cont = lib.gemm_kernel_choice(M, N, K, K + pad, K + pad, fp8=dtype != "bf16", with_form=True)
    cont = cont and (not y_blocked or (N // 2) % 128 == 0)
    return {1: 1, 2: 5 if cont else 2, 3: 5 if cont else 4}[fam]


@pytest.mark.parametrize("M,N,big", ((300, 272, False), (G.BLOCKED_M, 272, True), (G.BLOCKED_M, 512, True)))
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_blocked_entries(lib, dtype, M, N, big):
    """x in two K blocks and y in two N blocks (the Ulysses exchange buffers), family I, against the float64 chain — not against another kernel.  The
    blocked entries have no variant argument: a small shape reaches the 128x128 kernel, 192 output tiles with 8 K tiles the 256x256 bodies (N = 272:
    one-tile / ping-pong, N = 512: the continuous forms; int8 has no 256x256 body for N = 272 and stays on the 128x128 kernel)."""
    K = 8 * G.KTILE[dtype]
    inp, d = inputs("I", dtype, M, N, K)
    for y_blocked in (True, False):
        body = blocked_body(lib, dtype, M, N, K, y_blocked)
        want = 1 if not big or (dtype == "int8" and N == 272) else (5 if N == 512 else {"bf16": 4, "e4m3": 2}[dtype])
        assert body == want, f"variant 0 takes body {body} here, the test is written for {want}"
        blocked = {"bf16": lib.gemm_blocked, "e4m3": lib.gemm_fp8_blocked, "int8": lib.gemm_int8_blocked}[dtype]
        scales = () if dtype == "bf16" else (d.sx,)
        wscale = () if dtype == "bf16" else (d.sw,)
        if y_blocked:  # K-blocked x, N-blocked y, no residual there
            bigbuf, y = out_window(M, N, blocks=2)
            blocked(d.x_kblocked, *scales, d.w, *wscale, d.bias, G.EPI_NONE, out=y)
            assert poison_intact(bigbuf, M, N), "wrote outside the output blocks"
            got = y.permute(1, 0, 2).reshape(M, N)
            case("blocked entries").check(got, expect(inp, G.EPI_NONE), G.BODY[dtype, body] + " xK yN")
        else:  # K-blocked x into a row-major y with the gated residual
            bigbuf, y = out_window(M, N)
            if dtype == "bf16":
                lib.gemm(d.x_kblocked, d.w, d.bias, epilogue=G.EPI_RESIDUAL, resid=d.resid, gate=d.gate, out=y)
            else:
                blocked(d.x_kblocked, d.sx, d.w, d.sw, d.bias, G.EPI_RESIDUAL, out=y, resid=d.resid, gate=d.gate)
            assert poison_intact(bigbuf, M, N) and torch.equal(d.resid_big, d.resid_copy)
            case("blocked entries").check(y, expect(inp, G.EPI_RESIDUAL), G.BODY[dtype, body] + " xK")


def test_vt_entry(lib):
    """x2v_gemm_bf16_vt at the smallest shape it accepts (192 output tiles, 8 K tiles), family I: V^T [N / 128][ldvt / 64][128][64] equals the
    transposed float64 chain, rows M .. ldvt of the last 64-key tile are zero, and nothing around the array is written."""
    M, N, K = G.VT_SHAPE
    assert lib.gemm_kernel_choice(M, N, K, K + 8, K + 8) == 3 and lib.gemm_kernel_choice(M - 256, N, K, K + 8, K + 8) == 1 and M % 64
    inp, d = inputs("I", "bf16", M, N, K)
    ldvt, Hh = (M + 63) // 64 * 64, N // 128
    for use_bias in (True, False):
        flat = torch.full((Hh * ldvt * 128 + 128,), POISON, dtype=BF16, device="cuda")
        vt = flat[64 : 64 + Hh * ldvt * 128].view(Hh, ldvt // 64, 128, 64)
        lib._check(lib._lib.x2v_gemm_bf16_vt(d.x.data_ptr(), d.x.stride(0), d.w.data_ptr(), d.w.stride(0), d.bias.data_ptr() if use_bias else None, vt.data_ptr(), ldvt, M, N, K,
                                             lib._stream()), "gemm_bf16_vt")
        assert bool((flat[:64] == POISON).all() and (flat[-64:] == POISON).all()), "wrote outside V^T"
        rows = vt.permute(1, 3, 0, 2).reshape(ldvt, N)  # [tile, key, head, d] -> [token, head * 128 + d]
        assert bool((rows[M:] == 0).all()), "rows between M and the next multiple of 64 are not zero"
        case("vt entry").check(rows[:M], expect(inp, G.EPI_NONE, use_bias, False), "gemm256s V^T")
