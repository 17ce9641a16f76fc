"""tests/attn_ref.py checked without a GPU: the float64 reference against torch.softmax and a hand-computed row, the margins the N and H
families rest on, every emulation of a correct kernel inside the acceptance of Case.check on every family at every shape of
tests/test_gpu_attn_fp64.py, and five emulations of a subtly WRONG kernel rejected by at least one criterion at every shape where the defect
can occur.  The rejections this module prints (pytest -s) are the evidence that the GPU module would fail on such a kernel: deliberately
broken kernels are never run on a GPU."""
import math

import pytest
import torch

from tests import attn_ref as A

SHAPES = A.gpu_shapes()
SMALL = sorted({(Sq, Sk) for Sq, Sk, _, _ in SHAPES})


def test_ref64_is_softmax_attention():
    inp = A.Inputs("R", 33, 65, 2, "middle")
    o, a = A.ref64(inp.q, inp.k, inp.v)
    q, k, v = inp.q.double(), inp.k.double(), inp.v.double()
    w = torch.softmax(q @ k.transpose(-1, -2) * float(A.scale_log2e(0.0)) * math.log(2.0), -1)  # base e again
    assert torch.allclose(o, w @ v, rtol=1e-12, atol=1e-14) and torch.allclose(a, w @ v.abs(), rtol=1e-12, atol=1e-14)
    assert float(A.scale_log2e(0.0)) == pytest.approx(1.4426950408889634 / math.sqrt(128.0), rel=1e-7)
    o2, _ = A.ref64(inp.q, inp.k, inp.v, scale=0.05)
    w2 = torch.softmax(q @ k.transpose(-1, -2) * float(A.scale_log2e(0.05)) * math.log(2.0), -1)
    assert torch.allclose(o2, w2 @ v, rtol=1e-12, atol=1e-14) and not torch.allclose(o2, o, rtol=1e-3, atol=1e-5)


def test_q_rounding_chain_by_hand():
    """x2v_attn_fwd_bf16_vt re-rounds q: bf16(fp32(q) * fp32(scale * log2e)).  One row by hand: q = 1 + 2^-7 (a bf16 value) times 0.12751743 is
    0.128513..., which lies between the bf16 neighbours 0.12792969 (131 * 2^-10) and 0.12890625 (132 * 2^-10) and rounds to the second."""
    f = float(A.scale_log2e(0.0))
    assert f == pytest.approx(0.12751743, abs=1e-8)
    q = torch.full((1, 1, A.D), 1.0 + 2.0 ** -7, dtype=A.BF16)
    assert float(A.prescale_q(q)[0, 0, 0]) == 132 * 2.0 ** -10
    k = torch.zeros(1, 2, A.D, dtype=A.BF16)
    k[0, 0, 0], k[0, 1, 1] = 1.0, -1.0
    v = torch.zeros(1, 2, A.D, dtype=A.BF16)
    v[0, 0, 0], v[0, 1, 0] = 1.0, 3.0
    for kw, s in ((dict(q_rounded=True), 132 * 2.0 ** -10), (dict(), (1.0 + 2.0 ** -7) * f), (dict(prescaled=True), 1.0 + 2.0 ** -7)):
        w0 = 2.0 ** s / (2.0 ** s + 2.0 ** -s)  # scores +s and -s
        o, a = A.ref64(q, k, v, **kw)
        assert float(o[0, 0, 0]) == pytest.approx(w0 + 3.0 * (1.0 - w0), rel=1e-14) and float(a[0, 0, 0]) == pytest.approx(float(o[0, 0, 0]), rel=1e-14)
    assert torch.equal(A.scores(A.prescale_q(q), k, prescaled=True), A.scores(q, k, q_rounded=True))


@pytest.mark.parametrize("Sq,Sk", SMALL)
def test_family_margins(Sq, Sk):
    """N: every real score <= -12 base-2 units, so a leaked zero-score key takes the softmax.  H: the matched key leads by >= 40, so the output is its V row."""
    for form in A.FORMS:
        top = A.Inputs("N", min(Sq, 515), Sk, 2).assert_margins(form)
        h = A.Inputs("H", min(Sq, 515), Sk, 2)
        lead = h.assert_margins(form)
        assert {0, min(63, Sk - 1), min(64, Sk - 1), Sk - 1} <= set(h.j.tolist()) or Sq < 4
    print(f"margins Sq={Sq} Sk={Sk}: N top score {top:.1f}, H lead {lead:.1f}")


def _cases(Sq, Sk, H, families):
    for fam, spike in families:
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        for form in ("pipe", "vt"):  # 'pre' at the default scale is 'vt' (attn_ref.expect)
            yield inp, A.Expect(inp, form, keep=True)


@pytest.mark.parametrize("Sq,Sk,H,families", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_emulations_accepted_mutations_rejected(Sq, Sk, H, families):
    """The reference side alone stays inside both criteria at this shape (all emulations, every family, both score forms), and every mutation
    that applies at this Sk is rejected on at least one family."""
    case, wrong = A.Case("emulation", record=False), A.Case("mutation", record=False)
    rejected = {m: [] for m in A.MUTATIONS if A.mutation_applies(m, Sk)}
    for inp, exp in _cases(Sq, Sk, H, families):
        for kind, out in exp.emulated.items():
            case.check(out, exp, kind)
        for mut in rejected if exp.form == "vt" else ():  # the mutations act behind the scores: one score form shows them
            try:
                wrong.check(A.emulate(exp.s32, exp.v32, "lazy8", mut), exp, mut)
            except A.Reject as r:
                rejected[mut].append(f"{inp.family}{'' if inp.spike == 'none' else '-' + inp.spike}/{exp.form}:{r.criterion}")
    assert case.max_ratio <= 1.0 + 1e-12  # Y is the maximum over exactly these
    for mut, by in rejected.items():
        print(f"Sq={Sq} Sk={Sk} H={H} {mut}: rejected by {', '.join(by) if by else 'NOTHING'}")
        assert by, f"mutation {mut} passes every family at Sq={Sq} Sk={Sk}"


def test_scale_shape():
    Sq, Sk, H = A.SCALE_SHAPE
    case = A.Case("emulation", record=False)
    for fam, spike in (("R", "middle"), ("H", "none"), ("U", "none")):
        inp = A.Inputs(fam, Sq, Sk, H, spike)
        for form in A.FORMS:
            inp.assert_margins(form, A.ODD_SCALE)
            exp = A.Expect(inp, form, A.ODD_SCALE, keep=True)
            for kind, out in exp.emulated.items():
                case.check(out, exp, kind)


def test_subsets_keep_the_case():
    inp = A.Inputs("H", 2053, 129, 12)
    heads, rows = A.checked_heads(12), torch.arange(256, 768)
    cut = inp.take(heads=heads, rows=rows)
    full = A.Expect(inp, "vt")
    part = A.Expect(cut, "vt")
    assert torch.allclose(part.o, full.o[torch.as_tensor(heads)][:, rows], rtol=1e-13, atol=1e-15) and torch.equal(cut.exact(), inp.exact()[torch.as_tensor(heads)][:, rows])
    assert A.checked_heads(512) == [0, 73, 146, 219, 292, 365, 438, 511] and A.checked_heads(3) == [0, 1, 2]
    r = A.checked_rows(256 * 255 + 37)
    assert r.numel() == 7 * 256 + 37 and int(r[0]) == 0 and int(r[-1]) == 256 * 255 + 36
    for label, Sq, Sk, H, _ in A.p9_walk_cases(256):
        assert ((Sq + 255) // 256) * H >= 512 and Sk % 64 == 0, label
