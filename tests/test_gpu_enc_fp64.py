"""The kernels of the four encoder towers — gemm_rows_kernel (x2v_gemm_f16, x2v_gemm_rows_bf16), x2v_attn_f16_d80, x2v_attn_bf16_d64_relbias,
x2v_attn_f16_causal (d = 64, 128, 128 with the rotary tables), x2v_rmsnorm_f16, x2v_layernorm_f16, x2v_clip_embed_f16 — against the float64 yardstick
of tests/enc_ref.py, at the smallest shapes where each edge of their dispatch exists (the released widths stay with tests/test_gpu_clip.py,
test_gpu_t5.py and test_gpu_hunyuan_text.py).  The case lists are enc_ref's; tests/test_enc_ref_host.py shows which subtly wrong kernels the same rules
reject on the same lists.

Acceptance is enc_ref's on every call, no share of elements left out: attention |got - o| <= u |o| + 1.05 p A + F on every element, relL2 <= 1.5 Y,
families H / U / S bit for bit; GEMM family I bit for bit, family R inside the a-priori bound on every element; norms inside u |y| + atol on every
element with at most 2e-3 of a case's elements off T(y).

Every call reads its operands as views of over-allocated buffers and writes a window of a poisoned buffer whose surroundings are checked afterwards
(the helpers of tests/test_gpu_attn_fp64.py).  Attention runs twice, with 1e4 and with zeros in every row and column outside the sequences, and the two
results must be bit-equal; the GEMM and norm operands carry NaN outside their extents, so a read beyond them poisons the result.  ld* are distinct.
X2V_ENC_PARITY_TABLE names a path to write one run's table to (profiles/enc_fp64_parity.txt is one run's)."""
import os

import pytest
import torch

from tests import enc_ref as E
from tests.test_gpu_attn_fp64 import POISON, poison_intact, window

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
FILL = 1.0e4
CASES = {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    yield L
    path = os.environ.get("X2V_ENC_PARITY_TABLE")
    if not path:
        return
    try:
        with open(path, "w") as f:
            f.write("# kernel / case family: number of checks, worst d/tol (|got - ref| over the element bound), relL2 and Y of the family's largest relL2 / Y\n")
            for name in sorted(CASES):
                c = CASES[name]
                f.write("\n".join(c.table() if isinstance(c, E.AttnCase) else c.summary()) + "\n")
    except OSError:
        pass


def case(name, kind):
    return CASES.setdefault(name, kind(name))


# ------------------------------------------------------------------------------------------------------------------- attention
def attn_cols(K, H, Hkv):
    return (H + 2 * Hkv) * K.d


def attn_buffers(K, seqs, H, Hkv, row0, tail=64):
    """[row0 + sum(len) + tail, cols + 8] twice: the sequences packed from row `row0`, q | k | v side by side, every other row and the 8 pad columns
    holding 1e4 in the first and 0 in the second."""
    T, d = K.fmt.dtype, K.d
    total, cols = sum(s.n for s in seqs), attn_cols(K, H, Hkv)
    body = torch.cat([torch.cat([s.q.permute(1, 0, 2).reshape(s.n, H * d), s.k.permute(1, 0, 2).reshape(s.n, Hkv * d), s.v.permute(1, 0, 2).reshape(s.n, Hkv * d)], 1) for s in seqs], 0)
    out = []
    for fill in (FILL, 0.0):
        buf = torch.full((row0 + total + tail, cols + 8), fill, dtype=T)
        buf[row0 : row0 + total, :cols] = body
        out.append(buf.cuda())
    return out


def attn_call(lib, K, buf, cu, H, Hkv, bias, rope, rows=None):
    """One launch on the view buf[rows, :cols] into a poisoned window; returns the window (rows outside every sequence must still hold the poison)."""
    cols, HD = attn_cols(K, H, Hkv), H * K.d
    qkv = buf[:, :cols] if rows is None else buf[rows[0] : rows[1], :cols]
    n = qkv.shape[0]
    big, out = window(n, HD, K.fmt.dtype)
    assert qkv.stride(0) == cols + 8 and out.stride(0) == HD + 4 and out.data_ptr() % 16 == 0
    if K.name == "d80":
        lib.attention_f16_d80(qkv, len(cu) - 1, H, out=out)
    elif K.name == "t5":
        lib.attention_bf16_d64_relbias(qkv, bias, cu, H, out=out)
    else:
        lib.attention_f16_causal(qkv, cu, H, Hkv, K.d, rope=rope, out=out)
    assert poison_intact(big, n, HD), f"{K.name}: wrote outside the output window"
    assert bool((out[: cu[0]] == POISON).all() and (out[cu[-1] :] == POISON).all()), f"{K.name}: wrote rows outside every sequence"
    return out


def head_major(out, lo, n, H, d):
    return out[lo : lo + n].reshape(n, H, d).permute(1, 0, 2).contiguous().cpu()


def run_attention_launch(lib, kind, lens, H, Hkv, rope):
    K = E.KINDS[kind]
    row0 = 0 if kind == "d80" else 3  # the d80 entry takes batch * S rows from row 0; the packed entries start anywhere
    for fam, spike in E.attn_families(kind):
        seqs = E.attn_sequences(kind, lens, H, Hkv, fam, spike)
        for s in seqs:
            s.assert_margins()
        cu = [row0]
        for s in seqs:
            cu.append(cu[-1] + s.n)
        bias = None if seqs[0].bias is None else seqs[0].bias.cuda()  # pack() gives the sequences of a launch one table
        dom, zero = attn_buffers(K, seqs, H, Hkv, row0)
        rows = (0, cu[-1]) if kind == "d80" else None
        got = attn_call(lib, K, dom, cu, H, Hkv, bias, rope, rows)
        assert torch.equal(got, attn_call(lib, K, zero, cu, H, Hkv, bias, rope, rows)), f"{kind} {lens} {fam}: rows or columns outside the sequences reached the result"
        c = case(f"attn {kind}", E.AttnCase)
        for b, s in enumerate(seqs):
            c.check(head_major(got, cu[b] - (0 if rows is None else rows[0]), s.n, H, K.d), E.attn_expect(s), f"lens={lens}")
            if len(seqs) > 1:  # alone: the same bits as inside the packed launch
                if kind == "d80":
                    alone = attn_call(lib, K, dom, [0, s.n], H, Hkv, bias, rope, (cu[b], cu[b + 1]))
                    assert torch.equal(alone, got[cu[b] : cu[b + 1]]), f"{kind} {lens} {fam}: image {b} alone differs from the batched launch"
                else:
                    alone = attn_call(lib, K, dom, [cu[b], cu[b + 1]], H, Hkv, bias, rope)
                    assert torch.equal(alone[cu[b] : cu[b + 1]], got[cu[b] : cu[b + 1]]), f"{kind} {lens} {fam}: sequence {b} alone differs from the packed launch"


@pytest.mark.parametrize("kind", list(E.KINDS))
def test_attention(lib, kind):
    """Every launch of enc_ref.attn_launches() of this kernel, every family: d80 at S = 1 .. 272 and a batch of two; the relative-bias kernel at the
    edges of its 64 / 128 / 256 / 512-key bodies and two packed batches (one with two body sizes in one launch); the causal kernel at the edges of its
    64-key tiles, two packed batches, 4 / 1, 4 / 2 and 2 / 2 heads."""
    rope = tuple(t[:512].contiguous().cuda() for t in E.rope_tables()) if E.KINDS[kind].rope else None
    for k, lens, H, Hkv in E.attn_launches():
        if k == kind:
            run_attention_launch(lib, kind, lens, H, Hkv, rope)


# ------------------------------------------------------------------------------------------------------------------- GEMM
def padded(t, rows, ld, fill=float("nan")):
    """t [r, c] as the leading view of a [rows, ld] device buffer filled with `fill`."""
    big = torch.full((rows, ld), fill, dtype=t.dtype)
    big[: t.shape[0], : t.shape[1]] = t
    big = big.cuda()
    return big[: t.shape[0], : t.shape[1]]


def y_window(M, Ny, ldy, dtype):
    big = torch.full((M + 4, ldy), POISON, dtype=dtype, device="cuda")
    return big, big[2 : M + 2, :Ny]


def y_intact(big, M, Ny):
    return bool((big[:2] == POISON).all() and (big[M + 2 :] == POISON).all() and (big[2 : M + 2, Ny:] == POISON).all())


class GemmOperands:
    """The device side of one GemmInputs: x, w, resid as views of NaN-padded buffers with distinct leading dimensions, bias contiguous."""

    def __init__(self, inp):
        self.inp = inp
        self.ld = {gated: E.gemm_strides(inp.K, inp.Nw, inp.Nw // 2 if gated else inp.Nw) for gated in (False, True)}
        ldx, ldw, _, ldr = self.ld[False]
        self.x, self.w, self.resid = padded(inp.x, inp.M + 2, ldx), padded(inp.w, inp.Nw + 2, ldw), padded(inp.resid, inp.M + 1, ldr)
        self.bias = None if inp.bias is None else inp.bias.cuda()


def gemm_call(lib, ops, epi, rows=None, alias=False):
    """One launch of the entry for inp's element type on rows [lo, hi) of x (all by default) into a poisoned window; returns y [rows, Ny]."""
    inp, fmt = ops.inp, ops.inp.fmt
    lo, hi = rows or (0, inp.M)
    M, gated = hi - lo, epi in E.GATED
    Ny = inp.Nw // 2 if gated else inp.Nw
    ldx, ldw, ldy, ldr = ops.ld[gated]
    x, resid = ops.x[lo:hi], (ops.resid[lo:hi] if epi == E.EPI_RESIDUAL else None)
    if alias:  # y = resid: the window holds resid and is overwritten in place
        big, y = y_window(M, Ny, ldr, fmt.dtype)
        y.copy_(resid)
        resid = y
    else:
        big, y = y_window(M, Ny, ldy, fmt.dtype)
        lds = [x.stride(0), ops.w.stride(0), y.stride(0)] + ([resid.stride(0)] if resid is not None else [])
        assert len(set(lds)) == len(lds) and lds[:3] == [ldx, ldw, ldy]
    if fmt.name == "f16":
        code = {E.EPI_NONE: lib.EPI16_NONE, E.EPI_GELU_ERF: lib.EPI16_GELU_ERF, E.EPI_QUICK_GELU: lib.EPI16_QUICK_GELU, E.EPI_RESIDUAL: lib.EPI16_RESIDUAL, E.EPI_SWIGLU: lib.EPI16_SWIGLU}[epi]
        assert lib.gemm_f16_tile_choice(M, inp.Nw) == E.tile_choice(M, inp.Nw)
        lib.gemm_f16(x, ops.w, bias=None if gated else ops.bias, epilogue=code, resid=resid, out=y)
    else:
        code = {E.EPI_NONE: lib.EPIR_NONE, E.EPI_RESIDUAL: lib.EPIR_RESIDUAL, E.EPI_GEGLU: lib.EPIR_GEGLU}[epi]
        assert lib.gemm_rows_bf16_tile_choice(M, Ny, code) == E.tile_choice(M, inp.Nw)
        lib.gemm_rows_bf16(x, ops.w, epilogue=code, resid=resid, out=y)
    assert y_intact(big, M, Ny), f"{inp.name} {epi}: wrote outside the output window"
    return y


@pytest.mark.parametrize("tile", E.TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("fmt", list(E.FMT))
def test_gemm(lib, fmt, tile):
    """Every shape of enc_ref.gemm_shapes() that this tile takes (asserted through the entry's tile_choice on every call): K / 32 below, at and past the
    register ring, M from 1 to a partly filled second wave tile, N tails of 4 and 20 columns; every epilogue the entry admits, RESIDUAL also with
    y aliasing resid; family I bit for bit on NONE and RESIDUAL, family R inside the bound on every element."""
    c = case(f"gemm {fmt} {tile[0]}x{tile[1]}", E.GemmCase)
    shapes = [s for s in E.gemm_shapes() if s[3] == tile]
    assert shapes
    for M, Nw, K, _ in shapes:
        for fam in "IR":
            inp = E.gemm_inputs(fam, fmt, M, Nw, K)
            if fam == "I":
                inp.assert_exercises_roundings()
            ops = GemmOperands(inp)
            for epi in E.ENTRY_EPIS[fmt]:
                if fam == "I" and epi not in (E.EPI_NONE, E.EPI_RESIDUAL):
                    continue
                exp = E.GemmExpect(inp, epi)
                c.check(gemm_call(lib, ops, epi).cpu(), exp, f"{tile[0]}x{tile[1]}")
                if epi == E.EPI_RESIDUAL:
                    c.check(gemm_call(lib, ops, epi, alias=True).cpu(), exp, f"{tile[0]}x{tile[1]} in place")


@pytest.mark.parametrize("fmt", list(E.FMT))
def test_gemm_rows_batched_equal_rows_alone(lib, fmt):
    """Every output value is reduced in k order by one lane whatever the tile and M: the rows of a 128x64 launch equal the same rows computed by two
    64x64 launches, bit for bit, for every epilogue."""
    M, Nw, K, parts = E.GEMM_BATCHED
    tc = (lambda m: lib.gemm_f16_tile_choice(m, Nw)) if fmt == "f16" else (lambda m: lib.gemm_rows_bf16_tile_choice(m, Nw))
    assert tc(M) == (128, 64) and {tc(b - a) for a, b in parts} == {(64, 64)}
    ops = GemmOperands(E.gemm_inputs("R", fmt, M, Nw, K))
    for epi in E.ENTRY_EPIS[fmt]:
        full = gemm_call(lib, ops, epi)
        for a, b in parts:
            assert torch.equal(gemm_call(lib, ops, epi, rows=(a, b)), full[a:b]), f"{fmt} {epi}: rows {a}..{b} alone differ from the batched launch"


# ------------------------------------------------------------------------------------------------------------------- norms
def norm_window(M, D):
    big = torch.full((M + 4, D + 16), POISON, dtype=F16, device="cuda")
    return big, big[2 : M + 2, :D]


def test_rmsnorm_f16(lib):
    """D at both sides of the one-wave path's end (512) and of every chunk count of the four-wave path, M around the four rows per block."""
    c = case("rmsnorm_f16", E.NormCase)
    for D in E.RMS_D:
        for M in E.RMS_M:
            for which in E.RMS_SETS:
                x, w, _ = E.norm_inputs("rms", D, M, which)
                big, y = norm_window(M, D)
                xs = padded(x, M + 1, D + 8)
                assert xs.stride(0) != y.stride(0)
                lib.rmsnorm_f16(xs, w.cuda(), eps=E.NORM_EPS, out=y)
                assert y_intact(big, M, D)
                c.check(y.cpu(), E.rmsnorm64(x, w), f"D={D} M={M} {which}")
    c.finish()


def test_layernorm_f16_and_clip_embed(lib):
    """Strided rows at D = 8 .. 2048; the token assembly at batch 1 and 3, tokens 2 and 257."""
    c, ce = case("layernorm_f16", E.NormCase), case("clip_embed_f16", E.NormCase)
    for D in E.LN_D:
        for which in E.LN_SETS:
            x, w, b = E.norm_inputs("ln", D, E.LN_M, which)
            big, y = norm_window(E.LN_M, D)
            lib.layernorm_f16(padded(x, E.LN_M + 1, D + 8), w.cuda(), b.cuda(), eps=E.NORM_EPS, out=y)
            assert y_intact(big, E.LN_M, D)
            c.check(y.cpu(), E.layernorm64(x, w, b), f"D={D} {which}")
        for batch, tokens in E.EMBED_SHAPES:
            rows = batch * (tokens - 1)
            patches, w, b = E.norm_inputs("embed", D, rows, "n01")
            tp, _, _ = E.norm_inputs("embed", D, tokens + 1, "offset")
            cls, pos = tp[0].contiguous(), tp[1:].contiguous()
            big, y = norm_window(batch * tokens, D)
            lib.clip_embed(padded(patches, rows + 1, D + 8), cls.cuda(), pos.cuda(), w.cuda(), b.cuda(), batch, eps=E.NORM_EPS, out=y)
            assert y_intact(big, batch * tokens, D)
            ce.check(y.cpu(), E.clip_embed64(patches, cls, pos, w, b, batch), f"D={D} batch={batch} tokens={tokens}")
    c.finish()
    ce.finish()


def test_norm_refusals(lib):
    h = lambda M, D: torch.zeros(M, D, dtype=F16, device="cuda")
    f = lambda D: torch.zeros(D, device="cuda")
    with pytest.raises(lib.X2VError):
        lib.rmsnorm_f16(h(2, 8200), h(1, 8200)[0])
    with pytest.raises(lib.X2VError):
        lib.rmsnorm_f16(h(2, 12), h(1, 12)[0])
    with pytest.raises(lib.X2VError):
        lib.layernorm_f16(h(2, 2056), f(2056), f(2056))
    with pytest.raises(lib.X2VError):
        lib.layernorm_f16(h(2, 12), f(12), f(12))
    with pytest.raises(lib.X2VError):
        lib.clip_embed(h(2, 2056), h(1, 2056)[0], h(3, 2056), f(2056), f(2056), 1)
    with pytest.raises(lib.X2VError):
        lib.clip_embed(h(2, 12), h(1, 12)[0], h(3, 12), f(12), f(12), 1)
