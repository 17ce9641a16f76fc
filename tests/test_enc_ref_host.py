"""tests/enc_ref.py checked without a GPU: its float64 references against plain torch formulas where torch has one, its correct fp32 emulations against its
own acceptance rules on every case of the lists that tests/test_gpu_enc_fp64.py walks (imported from enc_ref, so the two cannot drift), the sharp cases
and family I bit for bit, and every subtly wrong emulation (enc_ref.ATTN_MUTATIONS, GEMM_MUTATIONS) rejected on at least one listed case where it applies.
The worst d / tol of the correct emulations is printed per kernel (run with -s) and written into enc_ref's docstring."""
import math

import pytest
import torch

from tests import enc_ref as E
from tests import gemm_ref

F64, F32, F16, BF16 = E.F64, E.F32, E.F16, E.BF16


def _all_sequences():
    for kind, lens, H, Hkv in E.attn_launches():
        for fam, spike in E.attn_families(kind):
            for inp in E.attn_sequences(kind, lens, H, Hkv, fam, spike):
                yield inp


# ------------------------------------------------------------------------------------------------------------------- the pieces
def test_rnd_is_one_rounding_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20000, generator=g, dtype=F64) * torch.exp2(torch.randint(-20, 14, (20000,), generator=g).to(F64))
    for name, T in (("f16", F16), ("bf16", BF16)):
        v = x.to(F32).to(T).to(F64)  # representable values stay
        assert torch.equal(E.rnd(v, name), v)
        r = E.rnd(x, name)
        assert torch.equal(r.to(F32).to(T).to(F64), r), "not a number of the format"
        up, down = torch.nextafter(r.to(F32).to(T), torch.tensor(math.inf, dtype=T)).to(F64), torch.nextafter(r.to(F32).to(T), torch.tensor(-math.inf, dtype=T)).to(F64)
        assert ((x - r).abs() <= (x - up).abs()).all() and ((x - r).abs() <= (x - down).abs()).all(), "not the nearest"
    # ties: 2049 lies between 2048 and 2050 in fp16 (to even: 2048), 2051 between 2050 and 2052 (2052); half-up takes the upper one; fp16 subnormals
    t = torch.tensor([2049.0, 2051.0, -2049.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -30], dtype=F64)
    assert E.rnd(t, "f16").tolist() == [2048.0, 2052.0, -2048.0, 0.0, 2.0 ** -23, 2.0 ** -24]
    assert E.rnd(t[:3], "f16", "half_up").tolist() == [2050.0, 2052.0, -2048.0]
    assert E.rnd(torch.tensor([257.0, 259.0], dtype=F64), "bf16").tolist() == [256.0, 260.0]
    # a float64 that double rounding through fp32 would get wrong: just above the tie 2049, by less than fp32 resolves
    assert float(E.rnd(torch.tensor([2049.0 + 2.0 ** -30], dtype=F64), "f16")) == 2050.0


def test_lipschitz_constants():
    for f, L in ((E.gelu_erf64, E.L_GELU_ERF), (E.quick_gelu64, E.L_QUICK_GELU), (gemm_ref.silu64, E.L_SILU), (gemm_ref.gelu64, E.L_GELU_TANH)):
        m = gemm_ref.lipschitz(f)
        assert L - 0.01 <= m <= L, f"{f.__name__}: max |f'| = {m:.5f}, constant {L}"


def test_activations_agree_with_torch():
    t = torch.linspace(-9, 9, 4001, dtype=F64)
    F = torch.nn.functional
    assert torch.allclose(E.gelu_erf64(t), F.gelu(t), rtol=0, atol=1e-14)
    assert torch.allclose(E.quick_gelu64(t), t * torch.sigmoid(1.702 * t), rtol=0, atol=1e-14)
    assert torch.allclose(gemm_ref.gelu64(t), F.gelu(t, approximate="tanh"), rtol=0, atol=1e-14)
    assert torch.allclose(gemm_ref.silu64(t), F.silu(t), rtol=0, atol=1e-14)


def test_rope_tables_and_rotation():
    cos, sin = E.rope_tables()
    assert cos.shape == (E.ROPE_ROWS, 64) and cos.dtype == F32 and float(cos[0].min()) == 1.0 and float(sin[0].abs().max()) == 0.0
    inv = E.ROPE_THETA ** (-torch.arange(0, 128, 2, dtype=F64) / 128)
    assert torch.allclose(cos[37].double(), torch.cos(37 * inv), atol=1e-7) and torch.allclose(sin[511].double(), torch.sin(511 * inv), atol=1e-7)
    t = torch.randn(2, 9, 128, generator=torch.Generator().manual_seed(1)).to(F16)
    pos = torch.arange(9) + 3
    r = E.rotate(t, pos, F64).double()
    c, s = cos[pos].double(), sin[pos].double()
    lo, hi = t[..., :64].double(), t[..., 64:].double()
    want = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)  # transformers' rotate_half form
    assert ((r - want).abs() <= 2.0 ** -11 * want.abs() + E.SUB16).all()
    assert (E.rotate(t, pos, F32) != E.rotate(t, pos, F64)).double().mean() < 1e-2  # the fp32 evaluation flips few roundings
    _, flag = E.rotate(t, pos, F64, True)
    assert ((E.rotate(t, pos, F32).double() - r).abs() <= flag).all(), "an fp32 rotation left the float64 one's grid point without being flagged"


@pytest.mark.parametrize("kind", list(E.KINDS))
def test_attention_reference_agrees_with_torch(kind):
    """ref64 against softmax(q k^T scale + bias + mask) v put together from torch's own softmax, on an R case with grouped heads where the kind has them."""
    K = E.KINDS[kind]
    H, Hkv = (4, 2) if K.causal else (3, 3)
    inp = E.AttnInputs(kind, "R", 70, H, Hkv, "middle")
    q, k, v = inp.q, inp.k, inp.v
    if K.rope:
        q, k = E.rotate(q, torch.arange(70), F64), E.rotate(k, torch.arange(70), F64)
    q, k, v = q.double(), k.double().repeat_interleave(H // Hkv, 0), v.double().repeat_interleave(H // Hkv, 0)
    s = torch.einsum("hid,hjd->hij", q, k) * K.scale
    i = torch.arange(70)
    if K.bias:
        s = s + inp.bias.double()[:, i[None, :] - i[:, None] + 511]
    if K.causal:
        s = s.masked_fill(i[None, :] > i[:, None], -math.inf)
    w = torch.softmax(s, -1)
    o, A, F = E.ref64(inp)
    assert torch.allclose(o, w @ v, rtol=0, atol=1e-13) and torch.allclose(A, w @ v.abs(), rtol=0, atol=1e-13)
    assert (F >= 0).all() and (K.fmt.name == "f16" or float(F.max()) == 0.0)
    assert abs(K.scale - K.d ** -0.5) < 1e-7 or kind == "t5"


def test_subnormal_term_counts_the_small_probabilities_only():
    """Family H: every key but the leader has P < 2^-14, so F = 2^-25 / l * (sum |v| - |v_leader|); family U: every P is 1 and F = 0."""
    inp = E.AttnInputs("d80", "H", 65, 2)
    s, v = E.operands(inp, F64)
    _, _, F = E.ref64(inp)
    want = E.SUB16 * (v.abs().sum(1, keepdim=True) - v.abs()[:, inp.j])
    assert torch.allclose(F, want, rtol=1e-9, atol=0)
    assert float(E.ref64(E.AttnInputs("d80", "U", 65, 2))[2].max()) == 0.0


def test_norm_references_agree_with_torch():
    F = torch.nn.functional
    x, w, b = E.norm_inputs("ln", 160, 5, "offset")
    y, atol = E.layernorm64(x, w, b)
    assert torch.allclose(y, F.layer_norm(x.double(), (160,), w.double(), b.double(), E._f32eps(E.NORM_EPS)), rtol=0, atol=1e-12) and (atol > 0).all()
    x, w, _ = E.norm_inputs("rms", 520, 3, "n01")
    y, _ = E.rmsnorm64(x, w)
    xd = x.double()
    assert torch.allclose(y, xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + E._f32eps(E.NORM_EPS)) * w.double(), rtol=0, atol=1e-12)
    g = torch.Generator().manual_seed(2)
    patches, cls, pos = torch.randn(6, 160, generator=g).half(), torch.randn(160, generator=g).half(), torch.randn(4, 160, generator=g).half()
    y, _ = E.clip_embed64(patches, cls, pos, w[:160].float(), b[:160], 2)
    tok = torch.cat([cls[None], patches[:3], cls[None], patches[3:]], 0)
    want = F.layer_norm((tok + pos.repeat(2, 1)).double(), (160,), w[:160].double(), b[:160].double(), E._f32eps(E.NORM_EPS))  # torch's own fp16 add
    assert torch.allclose(y, want, rtol=0, atol=1e-12)


def test_norm_rule_accepts_fp32_and_rejects_wrong_rows():
    """The same formulas in fp32, rounded once, pass; a row normalised with its neighbour's statistic, a dropped last chunk of 8 and a second rounding do not."""
    for kind, D, sets in (("rms", 520, E.RMS_SETS), ("ln", 160, E.LN_SETS)):
        case = E.NormCase(kind)
        for which in sets:
            x, w, b = E.norm_inputs(kind, D, 5, which)
            f = (lambda xx, dt: E.rmsnorm64(xx, w, dtype=dt)) if kind == "rms" else (lambda xx, dt: E.layernorm64(xx, w, b, dtype=dt))
            ref = f(x, F64)
            case.check(f(x, F32)[0].to(F16), ref, which)
            with pytest.raises(E.Reject):
                E.NormCase("shifted").check(f(x, F32)[0].roll(1, 0).to(F16), ref)
            short = x.clone()
            short[:, -8:] = 0
            with pytest.raises(E.Reject):
                E.NormCase("short").check(f(short, F32)[0].to(F16)[:, :], (ref[0], ref[1]))
        case.finish()
        assert case.worst <= 1.0
    twice = E.NormCase("two roundings")
    x, w, _ = E.norm_inputs("rms", 8192, 5, "n01")
    xn = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)).to(F16)  # LlamaRMSNorm's inner rounding, which the kernel does not do
    try:
        twice.check((xn.float() * w.float()).to(F16), E.rmsnorm64(x, w))
        twice.finish()
        rejected = False
    except E.Reject:
        rejected = True
    assert rejected, "a second rounding inside RMSNorm went unnoticed"


# ------------------------------------------------------------------------------------------------------------------- the case lists
def test_case_lists_cover_what_they_claim():
    launches = E.attn_launches()
    assert {l[1][0] for l in launches if l[0] == "d80" and len(l[1]) == 1} == set(E.D80_S) and ("d80", (257, 257), 3, 3) in launches
    assert {l[1][0] for l in launches if l[0] == "t5" and len(l[1]) == 1} == set(E.T5_LENS) and all(("t5", p) in {(l[0], l[1]) for l in launches} for p in E.T5_PACKS)
    for kind in E.CAUSAL_KINDS:
        got = {(l[1], l[2], l[3]) for l in launches if l[0] == kind}
        assert got == {(lens, H, Hkv) for lens in [(n,) for n in E.CAUSAL_LENS] + list(E.CAUSAL_PACKS) for H, Hkv in E.CAUSAL_HEADS}
    assert all(2 <= l[2] <= 4 for l in launches)
    shapes = E.gemm_shapes()  # asserts the tile of every shape
    assert {s[3] for s in shapes} == set(E.TILES)
    assert {s[2] for s in shapes if s[3] == (64, 16)} == set(E.GEMM_K) and all({s[2] for s in shapes if s[3] == t} >= set(E.GEMM_K3) for t in E.TILES)
    assert {s[0] for s in shapes} >= set(E.GEMM_M) and {s[1] % 64 for s in shapes} >= {4, 20}
    assert E.tile_choice(145, 6148) == (128, 64) and E.tile_choice(65, 6148) == (64, 64) and E.tile_choice(65, 3076) == (64, 32) and E.tile_choice(145, 132) == (64, 16)
    M, Nw, K, parts = E.GEMM_BATCHED
    assert len({E.tile_choice(M, Nw)} | {E.tile_choice(b - a, Nw) for a, b in parts}) == 2
    for K, Nw in ((128, 132), (32, 132), (256, 6148), (160, 148)):
        for Ny in (Nw, Nw // 2):
            ldx, ldw, ldy, ldr = E.gemm_strides(K, Nw, Ny)
            assert len({ldx, ldw, ldy, ldr}) == 4 and ldx > K and ldw > K and ldy > Ny and ldr > Nw and ldx % 8 == 0 and ldw % 8 == 0 and ldy % 4 == 0 and ldr % 4 == 0


def test_emulations_pass_every_listed_case(capsys):
    """Both correct attention emulations on every sequence of every launch and family, the GEMM emulation on every shape, family and epilogue: inside the
    acceptance rule, the sharp (S), one-hot (H), uniform (U) and integer (I) cases bit for bit (AttnCase.check / check_exact assert that)."""
    worst = {}
    for inp in _all_sequences():
        inp.assert_margins()
        exp = E.AttnExpect(inp, keep=True)
        for how, out in exp.emulated.items():
            _, _, w = E.AttnCase(inp.kind).check(out, exp, how)
            worst[inp.kind] = max(worst.get(inp.kind, 0.0), w)
            if inp.family in "SHU":
                assert torch.equal(out, inp.exact())
    for fmt in E.FMT:
        for M, Nw, K, _ in E.gemm_shapes():
            for fam in "IR":
                inp = E.gemm_inputs(fam, fmt, M, Nw, K)
                if fam == "I":
                    inp.assert_exercises_roundings()
                for epi in E.ENTRY_EPIS[fmt]:
                    if fam == "R" or epi in (E.EPI_NONE, E.EPI_RESIDUAL):
                        w = E.GemmCase(fmt).check(E.emulate_gemm(inp, epi), E.GemmExpect(inp, epi))
                        worst["gemm " + fmt] = max(worst.get("gemm " + fmt, 0.0), w)
    norms = {"rmsnorm": E.NormCase("rmsnorm"), "layernorm": E.NormCase("layernorm"), "clip_embed": E.NormCase("clip_embed")}
    for D in E.RMS_D:  # the same formulas in fp32, rounded once, on every norm case of the GPU module
        for M in E.RMS_M:
            for which in E.RMS_SETS:
                x, w, _ = E.norm_inputs("rms", D, M, which)
                norms["rmsnorm"].check(E.rmsnorm64(x, w, dtype=F32)[0].to(F16), E.rmsnorm64(x, w))
    for D in E.LN_D:
        for which in E.LN_SETS:
            x, w, b = E.norm_inputs("ln", D, E.LN_M, which)
            norms["layernorm"].check(E.layernorm64(x, w, b, dtype=F32)[0].to(F16), E.layernorm64(x, w, b))
        for batch, tokens in E.EMBED_SHAPES:
            patches, w, b = E.norm_inputs("embed", D, batch * (tokens - 1), "n01")
            tp, _, _ = E.norm_inputs("embed", D, tokens + 1, "offset")
            norms["clip_embed"].check(E.clip_embed64(patches, tp[0], tp[1:], w, b, batch, dtype=F32)[0].to(F16), E.clip_embed64(patches, tp[0], tp[1:], w, b, batch))
    for name, c in norms.items():
        c.finish()
        worst[name] = c.worst
    with capsys.disabled():
        print("\nworst d/tol of the correct emulations: " + " | ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def _first_rejection(mut):
    """The first listed sequence (shortest first) on which BOTH emulations carrying the mutation are rejected; the number of sequences where it applies."""
    applies = 0
    for inp in sorted(_all_sequences(), key=lambda s: s.n * s.H):
        if not E.mutation_applies(mut, inp):
            continue
        applies += 1
        exp = E.attn_expect(inp)
        hows = ("tiled",) if mut == "skip_o_rescale" else E.EMULATIONS
        crit = []
        for how in hows:
            try:
                E.AttnCase(mut).check(E.emulate_attn(inp, how, mut), exp)
                break
            except E.Reject as e:
                crit.append(e.criterion)
        else:
            return inp, crit, applies
    return None, None, applies


@pytest.mark.parametrize("mut", E.ATTN_MUTATIONS)
def test_attention_mutation_is_rejected(mut):
    inp, crit, applies = _first_rejection(mut)
    assert applies > 0, f"{mut}: no listed case where it applies"
    assert inp is not None, f"{mut}: accepted on all {applies} listed sequences where it applies"
    print(f"{mut}: rejected on {inp.name} ({', '.join(crit)})")


@pytest.mark.parametrize("kind, n, mut", [("t5", 512, "drop_last_key"), ("d80", 257, "leak_zero_key"), ("t5", 257, "leak_zero_key"), ("c128", 511, "leak_zero_key")])
def test_long_sequence_gaps_of_the_earlier_bars_are_closed(kind, n, mut):
    """A kernel that ignores key 511 of a 512-token T5 sequence, or lets the zero-filled key 257 into a 257-key softmax, stayed inside the max|v| bars
    of the tower tests on randn inputs; here each is rejected by at least two families of the listed launch of that length."""
    H, Hkv = next((h, hkv) for k, lens, h, hkv in E.attn_launches() if k == kind and lens == (n,))
    rejected = []
    for fam, spike in E.attn_families(kind):
        inp = E.AttnInputs(kind, fam, n, H, Hkv, spike)
        try:
            E.AttnCase(mut).check(E.emulate_attn(inp, "tiled" if E.KINDS[kind].causal else "global", mut), E.attn_expect(inp))
        except E.Reject as e:
            rejected.append((fam + spike, e.criterion))
    print(f"{kind} n={n} {mut}: rejected by {rejected}")
    assert len(rejected) >= 2, rejected


@pytest.mark.parametrize("kind", list(E.KINDS))
def test_sharp_cases_see_a_leaked_and_a_dropped_key_in_every_nonzero_element(kind):
    """The claim of family S: with len + 1 in the denominator, or one key missing from a column's count, no touched non-zero element keeps its bits in
    fp16 (a relative change of 1 / (len + 1) >= 2^-9 against a half spacing of at most 2^-11); bf16's half spacing reaches 2^-8, so there only most do."""
    n = 271 if kind == "d80" else 257 if kind == "t5" else 129
    inp = E.AttnInputs(kind, "S", n, 2)
    want = inp.exact()
    leaked = E.emulate_attn(inp, "global", "leak_zero_key")
    rows = slice((n - 1) // 64 * 64, n) if E.KINDS[kind].causal else slice(0, n)  # the rows that see the zero key
    same = ((leaked != want) == (want != 0))[:, rows]
    assert same.all() if kind != "t5" else (same.double().mean() > 0.5 and not (leaked != want)[want == 0].any())
    dropped = E.emulate_attn(inp, "global", "drop_last_key")
    col = (n - 1) % E.KINDS[kind].d
    rows = slice(n - 1, n) if E.KINDS[kind].causal else slice(0, n)
    assert (dropped != want)[:, rows, col].all()


@pytest.mark.parametrize("mut", list(E.GEMM_MUTATIONS))
def test_gemm_mutation_is_rejected_on_every_listed_shape(mut):
    fam, epi = E.GEMM_MUTATIONS[mut]
    for fmt in E.FMT:
        e = (E.EPI_SWIGLU if fmt == "f16" else E.EPI_GEGLU) if epi == "gated" else epi
        for M, Nw, K, _ in E.gemm_shapes():
            if M * Nw > 20000 and K != 160:  # the wide shapes once
                continue
            inp = E.gemm_inputs(fam, fmt, M, Nw, K)
            with pytest.raises(E.Reject):
                E.GemmCase(mut).check(E.emulate_gemm(inp, e, mut), E.GemmExpect(inp, e))
