"""x2v_gemm_mid_f16 (csrc/gemm_mid.h: LDS tiles, split K, last-arriving workgroup reduces) against fp64 math with the entry's rounding points, the
ticket's workspace discipline, and the Llama driver's mid_gemm switch against the tiny tower's reference fixture.

Two rules on the kernel's numbers.  The share rule (_share_outside) counts the elements further than one ulp from the rounded fp64 result.  The
every-element rule (_every_element) bounds EACH element against the unrounded fp64 result f in the form of tests/gemm_ref.py: with t = x . W^T + bias,
S = |x| . |W|^T + |bias|, H = 2^-10 (one fp16 ulp, relative) and e0 = H |t| + (1 + H) (K + splits + 2) 2^-23 S - an fp32 accumulation of K exact
products in any order, the sum of the splits' partial tiles, the bias add and the fp16 round -
    NONE      |got - f| <= e0
    RESIDUAL  f = resid + t, tol = e0 + H (|f| + e0)
    SWIGLU    t holds the 2N Linear outputs (a, g) interleaved, f = silu(a) g:
              tol = L_SILU e0_a (|g| + e0_g) + |silu(a)| e0_g + 2^-16 |f|, then tol += H (|f| + tol)
L_SILU and the 2^-16 of the fp32 activation are gemm_ref's.  Family I (small integers: every partial sum an fp32 integer below 2^24 whatever the split
and the order) is compared bit for bit for NONE and RESIDUAL; its SWIGLU takes the two exactly known fp16 operands through the same chain in fp32
torch and allows that result the activation's 2^-16 and the last fp16 rounding.  None of these constants is fitted to the kernel's output."""
import functools

import pytest
import torch

from tests.gemm_ref import ACT_EVAL, L_SILU, UNIT

pytestmark = pytest.mark.gpu

ULP16 = 2.0**-10
POISON = -1984.0  # exact in fp16
FLIP_SHARE = 2e-3  # tests/test_gpu_clip.py::FLIP_SHARE
F16 = torch.float16
NONE, RESIDUAL, SWIGLU = 0, 2, 4
ROWS = 351


@functools.lru_cache(maxsize=None)
def _case(N, K, epi):
    """Operands of ROWS rows (x ~ N(0, 1), W ~ N(0, 1) / sqrt(K), resid ~ N(0, 1), bias ~ 0.1 N(0, 1), rounded to fp16) and the fp64 result with the
    entry's rounding points; smaller M take the first rows.  Shared by every test of the shape and never written."""
    g = torch.Generator().manual_seed(N * 7 + K + epi)
    x = torch.randn(ROWS, K, generator=g).half().cuda()
    w = (torch.randn(2 * N if epi == SWIGLU else N, K, generator=g) / K**0.5).half().cuda()
    bias = None if epi == SWIGLU else (torch.randn(N, generator=g) * 0.1).half().cuda()
    resid = torch.randn(ROWS, N, generator=g).half().cuda() if epi == RESIDUAL else None
    acc = x.double() @ w.double().t()
    if epi == SWIGLU:
        gate, up = acc[:, 0::2].to(F16).double(), acc[:, 1::2].to(F16).double()
        ref = gate * torch.sigmoid(gate) * up
    else:
        ref = (acc + bias.double()).to(F16).double()
        if epi == RESIDUAL:
            ref = resid.double() + ref
    return x, w, bias, resid, ref


def _share_outside(got, ref64, what):
    """tests/test_gpu_clip.py::_ulp_check: |got - fp16(ref64)| <= 1 ulp |ref| + 2^-23 except for FLIP_SHARE of the elements."""
    ref, got = ref64.to(F16).double(), got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = ((got - ref).abs() > ULP16 * ref.abs() + 2.0**-23).double().mean().item()
    print(f"{what}: share outside 1 ulp {bad:.2e}, max |d| {(got - ref).abs().max().item():.3e}")
    assert bad <= FLIP_SHARE, f"{what}: {bad:.2e} of elements outside 1 ulp + 2^-23; max |d| {(got - ref).abs().max().item():.3e}"
    return bad


def _tolerance(t, S, K, splits, epi, resid=None):
    """(f, tol) of the every-element rule (module docstring) from the float64 t and S of the Linear outputs; splits = the ranges the launch reduces."""
    e0 = ULP16 * t.abs() + (1 + ULP16) * (K + splits + 2) * UNIT * S
    if epi == NONE:
        return t, e0
    if epi == RESIDUAL:
        f = resid.double() + t
        return f, e0 + ULP16 * (f.abs() + e0)
    a, g, ea, eg = t[:, 0::2], t[:, 1::2], e0[:, 0::2], e0[:, 1::2]
    sa = a * torch.sigmoid(a)
    f = sa * g
    tol = L_SILU * ea * (g.abs() + eg) + sa.abs() * eg + ACT_EVAL * f.abs()
    return f, tol + ULP16 * (f.abs() + tol)


def _linear64(x, w, bias):
    t, S = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    return (t, S) if bias is None else (t + bias.double(), S + bias.double().abs())


def _splits_taken(M, w_rows, K, splits):
    from lightx2v_amd import lib

    return splits or lib.gemm_mid_choice(M, w_rows, K, torch.cuda.get_device_properties(0).multi_processor_count)[1]


def _every_element(got, f, tol, what):
    """|got - f| <= tol on every element; returns the largest d/tol."""
    from tests.util import record

    g = got.double()
    assert g.shape == f.shape and torch.isfinite(g).all(), f"{what}: shape {tuple(g.shape)} vs {tuple(f.shape)}, or non-finite values"
    ratio = (g - f).abs() / tol.clamp_min(1e-300)
    worst = ratio.max().item()
    print(f"{what}: largest d/tol {worst:.3f}")
    record(what, rule="bound", worst=worst, elements=g.numel())
    i = int(ratio.reshape(-1).argmax())
    assert worst <= 1.0, (f"{what}: {int((ratio > 1).sum())} of {g.numel()} elements outside the every-element bound; worst d/tol {worst:.3f} at ({i // g.shape[1]}, {i % g.shape[1]}): "
                          f"got {g.reshape(-1)[i].item():.9g} ref {f.reshape(-1)[i].item():.9g}")
    return worst


@functools.lru_cache(maxsize=None)
def _case64(N, K, epi):
    """t and S of _case(N, K, epi) in float64, computed once."""
    x, w, bias, _, _ = _case(N, K, epi)
    return _linear64(x, w, bias)


@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("epi", [NONE, RESIDUAL, SWIGLU], ids=["bias", "residual_in_place", "swiglu"])
@pytest.mark.parametrize("N, K", [(136, 2080), (256, 512)])
@pytest.mark.parametrize("M", [127, 128, 129, 351])
def test_gemm_mid_f16_vs_fp64(M, N, K, epi, splits):
    """Below, at and above a row tile and the workload's 351; a partial column tile with a K tail (33 K tiles, the last of 32 elements) and the plain
    case; one range, three, and the library's choice (16 uneven ranges at K = 2080, 4 at K = 512).  y is written into a NaN-poisoned oversized buffer;
    the residual epilogue runs in place.  CPU stand-in (fp32 accumulation of four K ranges summed in order) on these inputs: at most 4.4e-4 outside."""
    from lightx2v_amd import lib
    from tests.util import record

    x, w, bias, resid, ref = _case(N, K, epi)
    store = torch.full((M * N + 4096,), float("nan"), dtype=F16, device="cuda")
    out = store[: M * N].view(M, N)
    if epi == RESIDUAL:
        out.copy_(resid[:M])
    lib.gemm_mid_f16(x[:M], w, bias, epilogue=epi, resid=out if epi == RESIDUAL else None, out=out, splits=splits)
    torch.cuda.synchronize()
    assert torch.isnan(store[M * N :]).all(), "gemm_mid_f16 wrote past its output"
    what = f"gemm_mid_f16 M={M} N={N} K={K} epi={epi} splits={splits}"
    record(what, share_outside_1ulp=_share_outside(out, ref[:M], what))
    t, S = _case64(N, K, epi)
    f, tol = _tolerance(t[:M], S[:M], K, _splits_taken(M, w.shape[0], K, splits), epi, None if resid is None else resid[:M])
    _every_element(out, f, tol, what + " every element")


def test_gemm_mid_f16_ticket_leaves_the_workspace_reusable():
    """Two launches in a row on one workspace that is not cleared in between, three K ranges, residual epilogue, then a launch of another shape (other tile
    and slot counts) and the first once more: equal bits every time, and every counter word of the workspace (its first 4096 bytes, whatever the shape)
    is zero afterwards."""
    from lightx2v_amd import lib

    M, N, K = 351, 136, 2080
    x, w, bias, resid, ref = _case(N, K, RESIDUAL)
    outs = [lib.gemm_mid_f16(x, w, bias, epilogue=RESIDUAL, resid=resid, splits=3) for _ in range(2)]
    x2, w2, bias2, _, _ = _case(256, 512, NONE)
    lib.gemm_mid_f16(x2, w2, bias2, splits=0)
    outs.append(lib.gemm_mid_f16(x, w, bias, epilogue=RESIDUAL, resid=resid, splits=3))
    torch.cuda.synchronize()
    ws = lib.gemm_mid_workspace(x.device)
    assert ws.numel() * 4 >= lib._lib.x2v_gemm_mid_workspace_bytes(M, N, K, 3) and not ws[:1024].any(), "a tile counter was left non-zero"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _share_outside(outs[1], ref, "gemm_mid_f16 second launch on the same workspace")


# (M, N, K, splits, bias?): a single half K tile, one dead wave column (N = 8); a second K range that is only the half tile; one K tile per range, the
# last a half tile; the most ranges the kernel takes, uneven; five row tiles under the library's own split; no bias with the plain epilogue
EDGES = [(1, 8, 32, 1, True), (129, 8, 96, 2, True), (127, 136, 352, 6, True), (351, 264, 2080, 16, True), (513, 136, 512, 0, True), (130, 264, 64, 1, False)]


def _edge_operands(family, M, N, K, epi, use_bias):
    """x [M, K], w [N or 2N, K], bias [N] (None for SWIGLU or use_bias False), resid [M, N] (RESIDUAL) on the device, x / w / resid as column windows of
    wider NaN-filled buffers (ldx = K + 16, ldw = K + 24, ldr = N + 12 halves, each window 16 bytes in).  Family I: x in [-4, 4], w in [-2, 2], bias in
    [-64, 64], resid in [-200, 200], integers; family R: _case's distributions."""
    g = torch.Generator().manual_seed(((M * 1009 + N) * 1013 + K) * 8 + epi + (4 if family == "I" else 0))
    wn = 2 * N if epi == SWIGLU else N
    if family == "I":
        x, w = torch.randint(-4, 5, (M, K), generator=g), torch.randint(-2, 3, (wn, K), generator=g)
        bias, resid = torch.randint(-64, 65, (N,), generator=g), torch.randint(-200, 201, (M, N), generator=g)
    else:
        x, w = torch.randn(M, K, generator=g), torch.randn(wn, K, generator=g) / K**0.5
        bias, resid = torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g)

    def window(t, extra):
        buf = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=F16, device="cuda")
        buf[:, 8 : 8 + t.shape[1]] = t.to(F16).cuda()
        return buf[:, 8 : 8 + t.shape[1]]

    return window(x, 16), window(w, 24), bias.to(F16).cuda() if use_bias and epi != SWIGLU else None, window(resid, 12) if epi == RESIDUAL else None


def _run_window(x, w, bias, epi, resid, splits, in_place=False):
    """The kernel's y as the window [1 : M + 1, 8 : 8 + N] of a poisoned [M + 2, N + 16] buffer whose surroundings must come back untouched; in place the
    window holds resid beforehand.  After a split launch every counter word of the workspace is zero."""
    from lightx2v_amd import lib

    M, K, N = x.shape[0], x.shape[1], w.shape[0] // 2 if epi == SWIGLU else w.shape[0]
    buf = torch.full((M + 2, N + 16), POISON, dtype=F16, device="cuda")
    out = buf[1 : M + 1, 8 : 8 + N]
    if in_place:
        out.copy_(resid)
    lib.gemm_mid_f16(x, w, bias, epilogue=epi, resid=out if in_place else resid, out=out, splits=splits)
    torch.cuda.synchronize()
    got = out.clone()
    out.fill_(POISON)
    assert bool((buf == POISON).all()), f"gemm_mid_f16 M={M} N={N} K={K} epi={epi} splits={splits}: a store outside y[{M}, {N}]"
    if _splits_taken(M, w.shape[0], K, splits) > 1:
        assert not lib.gemm_mid_workspace(x.device)[:1024].any(), "a tile counter was left non-zero"
    return got


@pytest.mark.parametrize("epi", [NONE, RESIDUAL, SWIGLU], ids=["plain", "residual", "swiglu"])
@pytest.mark.parametrize("M, N, K, splits, use_bias", EDGES)
def test_gemm_mid_f16_integer_family_bit_for_bit(M, N, K, splits, use_bias, epi):
    """Family I through padded strides and the poison window.  NONE and RESIDUAL (out of place and in place) equal the float64 chain rounded at the entry's
    rounding points; SWIGLU stays within the fp32 chain's 2^-16 and the last fp16 rounding of it, overflow to the same infinity included."""
    x, w, bias, resid = _edge_operands("I", M, N, K, epi, use_bias)
    acc, S = _linear64(x, w, bias)
    assert float(S.max()) < 2.0**24  # every partial sum is an fp32 integer
    what = f"gemm_mid_f16 family I M={M} N={N} K={K} epi={epi} splits={splits}"
    if epi == SWIGLU:
        a, g = acc[:, 0::2].to(F16).float(), acc[:, 1::2].to(F16).float()
        f = (a * torch.sigmoid(a) * g).double()
        got = _run_window(x, w, None, epi, None, splits).double()
        tol = 2.0**-11 * f.abs() * (1 + ACT_EVAL) + ACT_EVAL * f.abs() + 2.0**-25
        same_inf = torch.isinf(got) & (got.sign() == f.sign()) & (f.abs() * (1 + ACT_EVAL) >= 65520.0)  # fp16 rounds 65520 and above to infinity
        bad = ~(((got - f).abs() <= tol) | same_inf)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside one rounding of the fp32 chain"
        return
    want = acc.to(F16)
    if epi == NONE:
        assert torch.equal(_run_window(x, w, bias, epi, None, splits), want), what
        return
    want = (resid.double() + want.double()).to(F16)
    assert torch.isfinite(want).all()
    for in_place in (False, True):
        got = _run_window(x, w, bias, epi, resid, splits, in_place)
        assert torch.equal(got, want), f"{what} in_place={in_place}: {int((got != want).sum())} of {want.numel()} elements differ from the float64 chain"


@pytest.mark.parametrize("epi", [NONE, RESIDUAL, SWIGLU], ids=["plain", "residual", "swiglu"])
@pytest.mark.parametrize("M, N, K, splits, use_bias", EDGES)
def test_gemm_mid_f16_every_element_at_the_edges(M, N, K, splits, use_bias, epi):
    """Family R at the edge shapes, through padded strides and the poison window: the share rule and the every-element rule."""
    x, w, bias, resid = _edge_operands("R", M, N, K, epi, use_bias)
    t, S = _linear64(x, w, bias)
    f, tol = _tolerance(t, S, K, _splits_taken(M, w.shape[0], K, splits), epi, resid)
    if epi == SWIGLU:
        a, g = t[:, 0::2].to(F16).double(), t[:, 1::2].to(F16).double()
        ref = a * torch.sigmoid(a) * g
    else:
        ref = t.to(F16).double() if epi == NONE else resid.double() + t.to(F16).double()
    for in_place in (False, True) if epi == RESIDUAL else (False,):
        what = f"gemm_mid_f16 family R M={M} N={N} K={K} epi={epi} splits={splits}{' in place' if in_place else ''}"
        got = _run_window(x, w, bias, epi, resid, splits, in_place)
        _every_element(got, f, tol, what)
        if got.numel() >= 4096:  # the share rule needs enough elements for a share of 2e-3 to mean something
            _share_outside(got, ref, what)


def test_llama_tower_mid_gemm_vs_reference_fixture():
    """The tiny tower with mid_gemm=True on the fixture's prompts of 130 and 136 valid tokens (>= 128 packed rows): tests/test_gpu_hunyuan_text.py's
    triangle against the reference's fp16 output, and the plan's four Linears per layer are x2v_gemm_mid_f16 launches; a 96-token prompt keeps x2v_gemm_f16."""
    from lightx2v_amd import lib, llama, synth
    from tests import llama_restatement as R
    from tests.test_gpu_hunyuan_text import _triangle
    from tests.util import load_golden

    gold = load_golden("llama_encoder_tiny")
    dims = synth.LLAMA_DIMS["llama-tiny"]
    sd = synth.synth_llama_weights(dims, seed=int(gold["seed"][0]))
    with torch.no_grad():
        truth = R.infer_ids(sd, dims, gold["ids"], gold["mask"], dtype=torch.float64)[0]
    m = llama.TextEncoderHFLlamaModel((sd, dims), "cuda", mid_gemm=True)
    lens = gold["mask"].sum(1).tolist()
    for b in (3, 2, 0):
        n = lens[b]
        states, _ = m.infer_ids(gold["ids"][b : b + 1], gold["mask"][b : b + 1])
        assert not states[0, n - 95 :].any()
        _triangle(states[0, : n - 95], gold["out_f16"][b, : n - 95], truth[b, : n - 95], f"llama tiny tower, mid_gemm, prompt {b} ({n} tokens)")
        names = [fn.__name__ for fn, _ in m._plan((n,), lib._stream())]
        want = "x2v_gemm_mid_f16" if n >= llama.MID_GEMM_ROWS else "x2v_gemm_f16"
        assert names.count(want) == 4 * m.num_layers and sum("gemm" in s for s in names) == 4 * m.num_layers, names
