"""The row-wise DiT kernels of lightx2v_amd/csrc/norm.hip against the float64 references of tests/rowwise_ref.py, at every dispatch edge:
D <= 512 (one wave, four rows per block), the CH = 1, 2, 3, 4 instantiations (D <= 2048, 4096, 6144, 8192), the CH = 8 instantiation with
dead chunks (8192 < D <= 16384, never streamed), rows whose D/8 is no multiple of 256, the scalar tail and the grid-stride loops.

Acceptance is rowwise_ref.Case for every case: the hard bound |got - ref| <= 2^-7 |ref| + atol on EVERY element (atol derived from the operands,
see Case.check), at most 2e-3 of a case's elements with other bits than bf16(ref) (tests/test_rowwise_ref_host.py shows a correct fp32
evaluation stays under half of that on the same inputs), and in the X2V_ROUND_REF chains a row whose mean / mean + eps / rstd lies within 2^-20
of a bf16 rounding boundary accepted against either neighbour (at most 1 % of a case's rows).  Bit-exact where the contract says so.
Every kernel runs on contiguous rows, on rows strided inside a wider poisoned buffer and in place where x2v.h allows aliasing; the poison
around every output window is checked after the call."""
import ctypes

import pytest
import torch

from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu
POISON = -1984.0  # exact in bf16; no output of these cases comes near it
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def window(M, D, right=64):
    """A poisoned [M + 2, D + right] buffer and its [M, D] window (rows 1 .. M, columns 0 .. D-1: 16-byte aligned rows, token stride D + right)."""
    big = torch.full((M + 2, D + right), POISON, dtype=BF16, device="cuda")
    return big, big[1 : M + 1, :D]


def poison_intact(big, M, D):
    return bool((big[0] == POISON).all() and (big[M + 1] == POISON).all() and (big[1 : M + 1, D:] == POISON).all())


def placed(x, right=64):
    big, v = window(x.shape[0], x.shape[1], right)
    v.copy_(x)
    return big, v


def run_rows(fn, x, layout):
    """fn(x_dev, out_dev) for one layout; returns the output on the CPU after checking the poison around it (and that the input stayed)."""
    M, D = x.shape
    if layout == "inplace":
        big, v = placed(x)
        fn(v, v)
        assert poison_intact(big, M, D), "in-place call wrote outside its window"
        return v.cpu()
    if layout == "strided":
        bigx, xin = placed(x, right=128)
    else:
        bigx, xin = None, x.cuda()
    big, out = window(M, D)
    fn(xin, out)
    assert poison_intact(big, M, D), f"{layout} call wrote outside its window"
    assert torch.equal(xin.cpu(), x) and (bigx is None or poison_intact(bigx, M, D)), "input touched"
    return out.cpu()


# ------------------------------------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("D", R.NORM_D)
def test_rmsnorm(lib, D):
    cases = {m: R.Case(f"rmsnorm mode={m} D={D}") for m in (R.ROUND_FP32, R.ROUND_REF)}
    for what, x, w, mode, kind in R.rms_items(D):
        wd = w.cuda()
        fn = lambda xin, out: lib.rmsnorm(xin, wd, out=out, round_mode=mode)
        got = run_rows(fn, x, "contiguous")
        cases[mode].check(got, lambda alt: R.rmsnorm(x, w, mode=mode, alt=alt), what)
        for layout in ("strided", "inplace"):  # y may alias x (x2v.h)
            assert torch.equal(run_rows(fn, x, layout), got), f"rmsnorm D={D} {what}: {layout} != contiguous"
        if kind == "zero_row":
            assert (got[x.shape[0] // 2] == 0).all(), "an all-zero row must come out exactly zero"
    for c in cases.values():
        c.finish()


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_kw(kw):
    return {{"w": "weight", "b": "bias"}.get(k, k): v.cuda() for k, v in kw.items()}


@pytest.mark.parametrize("D", R.NORM_D)
def test_layernorm(lib, D):
    variants = (0, 1, 2) if 512 < D <= 8192 else (0, 1)
    case = R.Case(f"layernorm D={D}")
    for what, x, kw, kind, combo in R.ln_items(D):
        ref, dkw = R.layernorm(x, **kw), _ln_kw(kw)
        for variant in variants:  # each form against the reference, not only against each other
            got = run_rows(lambda xin, out: lib.layernorm(xin, out=out, variant=variant, **dkw), x, ("strided", "contiguous", "strided")[variant])
            case.check(got, ref, f"{what} variant={variant}")
            if kind == "const_row":  # variance 0: the row is exactly b / shift (or what the modulate chain makes of b)
                row = got[x.shape[0] // 2].float()
                want = {"none": torch.zeros(D), "w": torch.zeros(D), "b": kw.get("b"), "wb": kw.get("b"), "mod": kw.get("shift")}.get(combo)
                assert torch.equal(row, R.rne_bf16(ref.y[x.shape[0] // 2]).float()) and (want is None or torch.equal(row, want.float())), f"constant row, {combo}"
    case.finish()


def test_layernorm_streams_long_inputs(lib):
    """M above twice any possible resident grid (8 blocks x 256 CUs) at D = 1536: variant 0 takes the streaming form by itself."""
    M, D = 2 * 8 * 256 + 37, 1536
    x, ops = R.ln_inputs(D, M, "n01")
    case = R.Case(f"layernorm streaming M={M} D={D}")
    for combo in ("mod", "all"):
        kw = R.ln_operands(ops, combo)
        got = run_rows(lambda xin, out: lib.layernorm(xin, out=out, variant=0, **_ln_kw(kw)), x, "strided")
        case.check(got, R.layernorm(x, **kw), combo)
        for variant in (1, 2):
            assert torch.equal(lib.layernorm(x.cuda(), variant=variant, **_ln_kw(kw)).cpu(), got), f"variant {variant} != by-shape form"
    case.finish()


@pytest.mark.parametrize("D", [520, 5120, 13824])
def test_layernorm_quant_fp8(lib, D):
    x, ops = R.ln_inputs(D, 5, "n01")
    for combo in ("none", "mod", "all"):
        kw = R.ln_operands(ops, combo)
        dkw = _ln_kw(kw)
        codes, sx = lib.layernorm_quant_fp8(x.cuda(), **dkw)
        y = lib.layernorm(x.cuda(), variant=1, **dkw)
        codes2, sx2 = lib.quant_fp8_rowwise(y)
        assert torch.equal(codes.view(torch.uint8), codes2.view(torch.uint8)) and torch.equal(sx, sx2), f"fused != layernorm + quant ({combo})"
        # the scale is amax|y| / 448 of a y that obeys the hard bound: it may be off by the largest bound of its row
        ref = R.layernorm(x, **kw)
        yb = R.rne_bf16(ref.y)
        tol = (R.ULP * yb.abs() + ref.atol).amax(-1, keepdim=True) / 448.0
        assert ((sx.cpu().double() - R.quant_fp8_scale(yb)).abs() <= tol).all(), f"per-token scales ({combo})"
        assert torch.allclose(sx, (y.float().abs().amax(-1, keepdim=True) / 448.0).clamp_min(1.0 / (448.0 * 512.0)), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------------------------- RMSNorm + 3-axis RoPE
def _rope_call(lib, q, k, wq, wk, cs, gi, H, mode, variant, layout):
    """Runs the in-place kernel on copies of q, k (CPU); 'fused' puts q | k side by side in one poisoned buffer (token stride 2D + 64)."""
    grid, s0, S = R.ROPE_GRIDS[gi]
    D = H * 128
    if layout == "fused":
        big, v = window(S, 2 * D)
        v[:, :D].copy_(q)
        v[:, D:].copy_(k)
        qd, kd, bigs = v[:, :D], v[:, D:], [(big, 2 * D)]
    else:
        (bq, qd), (bk, kd) = placed(q, right=0), placed(k, right=0)
        bigs = [(bq, D), (bk, D)]
    lib.rmsnorm_rope_(qd, kd, None if wq is None else wq.cuda(), None if wk is None else wk.cuda(), cs, grid, H, s0=s0, round_mode=mode, q_out_scale=R.Q_SCALE, variant=variant)
    assert all(poison_intact(b, S, d) for b, d in bigs), "rmsnorm_rope wrote outside its rows"
    return qd.cpu(), kd.cpu()


@pytest.mark.parametrize("H", R.ROPE_H)
def test_rmsnorm_rope(lib, H):
    cs_cpu = R.rope_table()
    cs = cs_cpu.cuda()
    case = R.Case(f"rmsnorm_rope H={H}")
    for what, gi, q, k, wq, wk, mode in R.rope_items(H):
        grid, s0, S = R.ROPE_GRIDS[gi]
        gq, gk = _rope_call(lib, q, k, wq, wk, cs, gi, H, mode, 1, "fused")
        case.check(gq, lambda alt: R.rmsnorm_rope(q, wq, cs_cpu, s0, grid, mode=mode, out_scale=R.Q_SCALE, alt=alt), what + " q")
        case.check(gk, lambda alt: R.rmsnorm_rope(k, wk, cs_cpu, s0, grid, mode=mode, alt=alt), what + " k")  # out_scale 1: k is not scaled
        if wq is None:  # no norm and the identity rotation past the grid: k rows come back untouched, q rows are x * q_out_scale rounded once
            past = s0 + torch.arange(S) >= grid[0] * grid[1] * grid[2]
            assert torch.equal(gk[past], k[past]) and torch.equal(gq[past], (q[past].float() * R.Q_SCALE).to(BF16))
        for variant in ((0, 2) if H <= 64 else (0,)):  # the streaming form covers D <= 8192
            aq, ak = _rope_call(lib, q, k, wq, wk, cs, gi, H, mode, variant, "separate")
            assert torch.equal(aq, gq) and torch.equal(ak, gk), f"H={H} {what}: variant {variant} != per-row form"
    case.finish()
    if H > 64:
        with pytest.raises(lib.X2VError):
            _rope_call(lib, q, k, wq, wk, cs, gi, H, mode, 2, "separate")


@pytest.mark.parametrize("H", [2, 40])
def test_rmsnorm_rope_blocked(lib, H):
    cs_cpu = R.rope_table()
    cs, D = cs_cpu.cuda(), H * 128
    case = R.Case(f"rmsnorm_rope_blocked H={H}")
    for what, gi, q, k, wq, wk, mode in R.rope_items(H):
        grid, s0, S = R.ROPE_GRIDS[gi]
        want_q, want_k = _rope_call(lib, q, k, wq, wk, cs, gi, H, mode, 1, "separate")
        for cb in (D // 2, 128):
            nb = D // cb
            (bq, qd), (bk, kd) = placed(q), placed(k, right=128)
            outs = [torch.full((nb + 1, S, cb), POISON, dtype=BF16, device="cuda") for _ in range(2)]  # one spare poisoned block behind the last
            lib.rmsnorm_rope_blocked(qd, kd, None if wq is None else wq.cuda(), None if wk is None else wk.cuda(), cs, grid, H, outs[0][:nb], outs[1][:nb], s0=s0,
                                     round_mode=mode, q_out_scale=R.Q_SCALE)
            assert torch.equal(qd.cpu(), q) and torch.equal(kd.cpu(), k) and poison_intact(bq, S, D) and poison_intact(bk, S, D), "blocked form touched its inputs"
            assert all(bool((o[nb] == POISON).all()) for o in outs), "blocked form wrote behind its last block"
            uq, uk = (o[:nb].permute(1, 0, 2).reshape(S, D).cpu() for o in outs)
            assert torch.equal(uq, want_q) and torch.equal(uk, want_k), f"H={H} {what} block_cols={cb}: un-blocked != in-place form"
        case.check(uq, lambda alt: R.rmsnorm_rope(q, wq, cs_cpu, s0, grid, mode=mode, out_scale=R.Q_SCALE, alt=alt), what + " q")
        case.check(uk, lambda alt: R.rmsnorm_rope(k, wk, cs_cpu, s0, grid, mode=mode, alt=alt), what + " k")
    case.finish()


# ------------------------------------------------------------------------------------------------------------------- per-head norm + RoPE
@pytest.mark.parametrize("H,L", R.HEAD_SHAPES)
def test_headnorm_rope(lib, H, L):
    D = H * 128
    case = R.Case(f"headnorm_rope H={H}")
    seen = {}
    for what, q, k, wq, wk, cos, sin, l_rope, mode, scale in R.head_items(H, L):
        dw = [None if t is None else t.cuda() for t in (wq, wk)]
        big, v = window(L, 3 * D)  # the q | k | v column blocks of a fused QKV output
        v[:, :D].copy_(q)
        v[:, D : 2 * D].copy_(k)
        lib.headnorm_rope_(v[:, :D], v[:, D : 2 * D], dw[0], dw[1], cos.cuda(), sin.cuda(), H, l_rope, round_mode=mode, q_out_scale=scale)
        assert poison_intact(big, L, 3 * D) and bool((v[:, 2 * D :] == POISON).all()), "headnorm_rope wrote outside q | k"
        gq, gk = v[:, :D].cpu(), v[:, D : 2 * D].cpu()
        case.check(gq, lambda alt: R.headnorm_rope(q, wq, cos, sin, H, l_rope, mode=mode, out_scale=scale, alt=alt), what + " q")
        case.check(gk, lambda alt: R.headnorm_rope(k, wk, cos, sin, H, l_rope, mode=mode, alt=alt), what + " k")
        if mode == R.ROUND_REF:  # q_out_scale is ignored with X2V_ROUND_REF (x2v.h): both scales give the same bits
            key = (l_rope, wq is None)
            assert key not in seen or torch.equal(seen[key], gq), f"{what}: q_out_scale changed a ROUND_REF result"
            seen[key] = gq
        for hpb in sorted({1, 3, H} & {d for d in (1, 3, H) if H % d == 0}):
            nb = H // hpb
            blk = [torch.full((nb + 1, L, hpb * 128), POISON, dtype=BF16, device="cuda") for _ in range(2)]
            for b, src in zip(blk, (q, k)):
                b[:nb].copy_(src.reshape(L, nb, hpb * 128).permute(1, 0, 2))
            lib.headnorm_rope_blocked_(blk[0][:nb], blk[1][:nb], dw[0], dw[1], cos.cuda(), sin.cuda(), H, l_rope, round_mode=mode, q_out_scale=scale)
            assert all(bool((b[nb] == POISON).all()) for b in blk), "head-blocked form wrote behind its last block"
            uq, uk = (b[:nb].permute(1, 0, 2).reshape(L, D).cpu() for b in blk)
            assert torch.equal(uq, gq) and torch.equal(uk, gk), f"{what}: heads_per_block={hpb} != row-major form"
    case.finish()


# ------------------------------------------------------------------------------------------------------------------- gate-residual
@pytest.mark.parametrize("D", [8, 1536, 5120])
def test_gate_residual(lib, D):
    M = 5
    x, y, gate = R.residual_inputs(M, D)
    case = R.Case(f"gate_residual D={D}")
    for g in (gate, None):
        want = x.clone()
        want.add_(y * g if g is not None else y)  # torch bf16 ops on the CPU: the contract is bit-exact
        for strided in (False, True):
            if strided:
                (bx, xd), (by, yd) = placed(x, right=64), placed(y, right=192)  # different row strides
            else:
                (bx, xd), (by, yd) = placed(x, right=0), placed(y, right=0)
            lib.gate_residual_(xd, yd, None if g is None else g.cuda())
            assert poison_intact(bx, M, D) and poison_intact(by, M, D) and torch.equal(yd.cpu(), y)
            assert torch.equal(xd.cpu(), want), f"gate={g is not None} strided={strided}"
        assert case.check(want, R.gate_residual(x, y, g)) == 0
    case.finish()


def test_gate_residual_grid_stride(lib):
    """M * D / 8 above 8192 x 256 vectors: the capped grid takes a second trip through its loop."""
    M, D = 4100, 5120
    assert M * D // 8 > 8192 * 256
    x, y, gate = R.residual_inputs(M, D, seed=1)
    want = x.clone()
    want.add_(y * gate)
    bx, xd = placed(x)
    lib.gate_residual_(xd, y.cuda(), gate.cuda())
    assert poison_intact(bx, M, D) and torch.equal(xd.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------- activations, sinusoid
def _act_raw(lib, x, n, act, room):
    """x2v_activation_bf16 on the first n elements of x into a poisoned buffer of n + room elements."""
    out = torch.full((n + room,), POISON, dtype=BF16, device="cuda")
    lib._check(lib._lib.x2v_activation_bf16(x.data_ptr(), out.data_ptr(), n, act, lib._stream()), "activation")
    assert bool((out[n:] == POISON).all()), f"activation wrote behind element {n}"
    return out[:n]


@pytest.mark.parametrize("act", [R.ACT_GELU_TANH, R.ACT_SILU, R.ACT_GELU_ERF])
def test_activation(lib, act):
    x = R.all_finite_bf16()
    xd = x.cuda()
    case = R.Case(f"activation act={act}")
    lut = _act_raw(lib, xd, x.numel(), act, 64)  # every finite bf16 bit pattern in one launch
    got = lut.cpu()
    case.check(got, R.activation(x, act), "all finite bf16")
    bits, gbits = x.view(torch.int16), got.view(torch.int16)
    assert gbits[bits == 0].item() == 0 and gbits[bits == -32768].item() == -32768, "act(+-0) must be exactly +-0"
    big = x.float().abs() > 1e30
    assert torch.isfinite(got.float()).all() and torch.equal(got[big & (x.float() > 0)], x[big & (x.float() > 0)]) and (got[big & (x.float() < 0)] == 0).all(), "limits at large |x|"
    case.finish()
    index = torch.arange(65536, dtype=torch.int64)
    index[bits.long() & 0xFFFF] = torch.arange(x.numel())
    index = index.cuda()
    for n in R.ACT_LENGTHS + (8192 * 256 * 8 + 2055,):  # the scalar tail; the last one takes the grid-stride loop round a second time
        xs = xd.repeat(-(-n // x.numel()))[:n].roll(3) if n > x.numel() else xd[20000 : 20000 + n].contiguous()
        out = _act_raw(lib, xs, n, act, 9)
        want = lut[index[xs.view(torch.int16).long() & 0xFFFF]]
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), f"n={n}"


@pytest.mark.parametrize("dim", R.SIN_DIMS)
def test_sinusoid(lib, dim):
    case = R.Case(f"sinusoid dim={dim}")
    for ts in (R.SIN_T, (727,), (1000,)):
        t = torch.tensor(ts, dtype=torch.int64)
        n = t.numel()
        out = torch.full((n + 1, dim), POISON, dtype=BF16, device="cuda")
        lib._check(lib._lib.x2v_sinusoid_embed_bf16(t.cuda().data_ptr(), out.data_ptr(), n, dim, lib._stream()), "sinusoid")
        assert bool((out[n] == POISON).all())
        case.check(out[:n].cpu(), R.sinusoid(t, dim), f"n={n}")
    case.finish()


# ------------------------------------------------------------------------------------------------------------------- argument edges
def test_argument_edges_return_codes(lib):
    """Return codes only, on a zeroed buffer large enough for every shape named: nothing here can fault.  Each raises X2VError and the next valid
    call works."""
    c, st = lib._lib, lib._stream()
    buf = torch.zeros(8, 16392 + 129 * 128, dtype=BF16, device="cuda")
    cs = R.rope_table().cuda()
    p, f32 = buf.data_ptr(), ctypes.c_float
    ld = buf.stride(0)
    t = torch.tensor([3], dtype=torch.int64, device="cuda")
    bad = {
        "rmsnorm D % 8": lambda: c.x2v_rmsnorm_bf16(p, ld, p, p, ld, 2, 12, f32(1e-6), 0, st),
        "rmsnorm D = 16392": lambda: c.x2v_rmsnorm_bf16(p, ld, p, p, ld, 2, 16392, f32(1e-6), 0, st),
        "layernorm D % 8": lambda: c.x2v_layernorm_bf16_variant(p, ld, None, None, None, None, p, ld, 2, 12, f32(1e-6), 0, st),
        "layernorm D = 16392": lambda: c.x2v_layernorm_bf16_variant(p, ld, None, None, None, None, p, ld, 2, 16392, f32(1e-6), 0, st),
        "layernorm variant 2, D = 512": lambda: c.x2v_layernorm_bf16_variant(p, ld, None, None, None, None, p, ld, 2, 512, f32(1e-6), 2, st),
        "layernorm variant 2, D = 8200": lambda: c.x2v_layernorm_bf16_variant(p, ld, None, None, None, None, p, ld, 2, 8200, f32(1e-6), 2, st),
        "layernorm scale without shift": lambda: c.x2v_layernorm_bf16_variant(p, ld, None, None, p, None, p, ld, 2, 512, f32(1e-6), 0, st),
        "layernorm_quant_fp8 scale without shift": lambda: c.x2v_layernorm_quant_fp8(p, ld, None, None, p, None, p, ld, p, 2, 1024, f32(1e-6), st),
        "layernorm_quant_fp8 D = 16392": lambda: c.x2v_layernorm_quant_fp8(p, ld, None, None, None, None, p, ld, p, 2, 16392, f32(1e-6), st),
        "rmsnorm_rope H = 129": lambda: c.x2v_rmsnorm_rope_scaled_bf16_variant(p, ld, p, ld, None, None, cs.data_ptr(), 2, 129, 0, 1, 1, 2, f32(1e-6), 0, f32(1.0), 0, st),
        "rmsnorm_rope variant 2, H = 72": lambda: c.x2v_rmsnorm_rope_scaled_bf16_variant(p, ld, p, ld, None, None, cs.data_ptr(), 2, 72, 0, 1, 1, 2, f32(1e-6), 0, f32(1.0), 2, st),
        "rmsnorm_rope wq without wk": lambda: c.x2v_rmsnorm_rope_scaled_bf16_variant(p, ld, p, ld, p, None, cs.data_ptr(), 2, 2, 0, 1, 1, 2, f32(1e-6), 0, f32(1.0), 0, st),
        "rmsnorm_rope q_out_scale = 0": lambda: c.x2v_rmsnorm_rope_scaled_bf16_variant(p, ld, p, ld, None, None, cs.data_ptr(), 2, 2, 0, 1, 1, 2, f32(1e-6), 0, f32(0.0), 0, st),
        "headnorm_rope q_out_scale < 0": lambda: c.x2v_headnorm_rope_bf16(p, ld, p, ld, None, None, None, None, 2, 2, 0, f32(1e-6), 0, f32(-1.0), st),
        "gate_residual D % 8": lambda: c.x2v_gate_residual_bf16(p, ld, p, ld, None, 2, 12, st),
        "activation unknown act": lambda: c.x2v_activation_bf16(p, p, 64, 2, st),
        "sinusoid odd dim": lambda: c.x2v_sinusoid_embed_bf16(t.data_ptr(), p, 1, 7, st),
    }
    x, w = R.rms_inputs(128, 3, "n01")
    want = lib.rmsnorm(x.cuda(), w.cuda())
    for name, call in bad.items():
        with pytest.raises(lib.X2VError):
            lib._check(call(), name)
        assert torch.equal(lib.rmsnorm(x.cuda(), w.cuda()), want), f"the call after '{name}' must work"
    assert (buf == 0).all()
