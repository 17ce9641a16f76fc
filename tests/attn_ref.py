"""float64 reference, fp32 emulations, seeded inputs and the acceptance rule for the head-dim-128 attention kernels of lightx2v_amd/csrc/attn.hip
(attn_fwd_pipe_kernel, the ping-pong attn_fwd_v9_kernel and its persistent form attn_fwd_p9_kernel).  Plain PyTorch on the CPU; nothing here imports
the library or the oracle.  Shared by tests/test_attn_ref_host.py (the yardstick checked without a GPU) and tests/test_gpu_attn_fp64.py (the
kernels checked against it).

Tensors are head-major here: q [H, Sq, 128], k / v [H, Sk, 128], bf16.  Scores are in base 2: s = (q . k) * scale * log2(e), P = 2^(s - max).

The kernels' documented rounding model (x2v.h, attn.hip): fp32 scores; P rounded to bf16 as the operand of the PV product only, unrounded in the
row sum; O accumulated and normalised in fp32 and rounded to bf16 once.  The pre-transposed-V entry (x2v_attn_fwd_bf16_vt) without
X2V_ATTN_VT_PRESCALED first re-rounds q: q' = bf16(fp32(q) * fp32(scale * log2e)) — `ref64` reproduces that step exactly (a chain reference in
rowwise_ref's sense); with PRESCALED q enters as given; the row-major entry (x2v_attn_fwd_bf16_variant) multiplies the fp32 score.

Acceptance (Case.check), no share of elements left out:
  * every element: |got - o| <= 2^-7 |o| + 1.05 * 2^-8 * A, A = sum_j w_j |v_jd| the softmax-weighted mean of |v|: o' - o = sum_j w_j delta_j v_j
    with |delta_j| <= 2^-8 (P's rounding), plus the final rounding of O; the constants are those of the d64 / d80 attention tests;
  * aggregate: relL2(got - o) <= 1.5 * Y, Y the largest relative L2 error of three emulations of a correct kernel on the same inputs (global
    max; 64-key tiles with lazy rescale; eager rescale) — computed here, never from the code under test; 1.5 is the triangle factor of
    tests/test_gpu_ops.py::test_attention_vs_oracle."""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
D = 128
TILE = 64  # keys per tile (attn.hip AT_KV)
WAVE_ROWS = 32  # query rows that share one lazy-rescale decision (the branch is wave-uniform)
ULP = 2.0 ** -7
P_ROUND = 1.05 * 2.0 ** -8
TRIANGLE = 1.5
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=F32)
DEFAULT_SCALE = 0.08838834764831845  # 1 / sqrt(128): what scale <= 0 selects (x2v.h)
FORMS = ("pipe", "vt", "pre")  # x2v_attn_fwd_bf16_variant | x2v_attn_fwd_bf16_vt | the same with X2V_ATTN_VT_PRESCALED (q = prescale_q(q))
FAMILIES = ("R", "N", "H", "U")
SPIKES = ("none", "first", "middle", "last")
N_MARGIN, H_MARGIN = -12.0, 40.0  # base-2 units


def scale_log2e(scale):
    """The float the launchers hand to the kernels: (float)scale * 1.4426950408889634f."""
    s = torch.tensor(scale if scale > 0 else DEFAULT_SCALE, dtype=F32)
    return s * LOG2E_F32


def prescale_q(q, scale=0.0):
    """bf16(fp32(q) * fp32(scale * log2e)): the kernel's `(__bf16)((float)v * scale_log2e)`, and what a producer of a PRESCALED q hands over."""
    return (q.to(F32) * scale_log2e(scale)).to(BF16)


def _q_and_factor(q, scale, prescaled, q_rounded, dtype):
    if prescaled:
        return q.to(dtype), None
    if q_rounded:
        return prescale_q(q, scale).to(dtype), None
    return q.to(dtype), scale_log2e(scale).to(dtype)


def scores(q, k, scale=0.0, prescaled=False, q_rounded=False, dtype=F64):
    """Base-2 scores [H, Sq, Sk] of one entry's form, in `dtype`."""
    qe, f = _q_and_factor(q, scale, prescaled, q_rounded, dtype)
    s = qe @ k.to(dtype).transpose(-1, -2)
    return s if f is None else s * f


def form_args(form):
    return {"pipe": dict(prescaled=False, q_rounded=False), "vt": dict(prescaled=False, q_rounded=True), "pre": dict(prescaled=True, q_rounded=False)}[form]


def ref64(q, k, v, scale=0.0, prescaled=False, q_rounded=False):
    """float64 attention in base 2.  Returns (o, A): o [H, Sq, 128] unrounded, A = sum_j w_j |v_jd|."""
    s = scores(q, k, scale, prescaled, q_rounded, F64)
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    w = w / w.sum(-1, keepdim=True)
    vd = v.to(F64)
    return w @ vd, w @ vd.abs()


# ------------------------------------------------------------------------------------------------------------------- emulations
MUTATIONS = ("drop_last_key", "leak_zero_key", "swap_v_rows", "double_count", "skip_o_rescale")


def mutation_applies(mut, Sk):
    """drop / swap need a second key; the first key past Sk exists for a kernel only inside a partly filled last tile; a rescale needs a second tile."""
    return {"drop_last_key": Sk >= 2, "leak_zero_key": Sk % TILE != 0, "swap_v_rows": Sk >= 2, "double_count": True, "skip_o_rescale": Sk > TILE}[mut]


def _wave_any(need):
    """need [H, Sq] -> the same, every row replaced by the `any` over its 32-row wave (waves start at multiples of 32: 256-row blocks are whole waves)."""
    H, Sq = need.shape
    pad = (-Sq) % WAVE_ROWS
    n = torch.nn.functional.pad(need, (0, pad)).reshape(H, -1, WAVE_ROWS).any(-1, keepdim=True)
    return n.expand(-1, -1, WAVE_ROWS).reshape(H, -1)[:, :Sq]


def emulate(s, v, kind="lazy8", mut=None):
    """A correct kernel in fp32 torch on fp32 scores s [H, Sq, Sk] and v [H, Sk, 128]: kind 'global' (one pass, global row max), 'lazy8' / 'lazy4'
    (64-key tiles, online softmax; the first tile adopts its max, a later tile rescales when some row of the wave grew by more than 8 / 4) or
    'eager' (rescale on every tile).  P is rounded to bf16 for the PV product only, the row sum takes it unrounded, the division is fp32, O is
    rounded to bf16 once.  mut: one of MUTATIONS — a subtly WRONG kernel, for the host module's rejection tests."""
    s, v = s.to(F32), v.to(F32)
    dup = None
    if mut == "drop_last_key":
        s, v = s[..., :-1], v[:, :-1]
    elif mut == "leak_zero_key":  # its K row reads as zeros through the buffer descriptor: score 0; its V^T column is the zero padding
        s, v = torch.cat([s, torch.zeros_like(s[..., :1])], -1), torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    elif mut == "swap_v_rows":
        a, b = 0, min(TILE - 1, v.shape[1] - 1)
        v = v.clone()
        v[:, [a, b]] = v[:, [b, a]]
    elif mut == "double_count":
        dup = s.shape[-1] - 1
    H, Sq, Sk = s.shape
    if kind == "global":
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        l = p.sum(-1)
        if dup is not None:
            l = l + p[..., dup]
        return ((p.to(BF16).to(F32) @ v) / l.unsqueeze(-1)).to(BF16)
    thr = {"lazy8": 8.0, "lazy4": 4.0, "eager": None}[kind]
    m, l, o = None, torch.zeros(H, Sq), torch.zeros(H, Sq, D)
    for t0 in range(0, Sk, TILE):
        st = s[..., t0 : t0 + TILE]
        mt = st.amax(-1)
        if m is None:
            m = mt
        else:
            grow = torch.ones_like(mt, dtype=torch.bool) if thr is None else _wave_any(mt - m > thr)
            m_new = torch.where(grow, torch.maximum(m, mt), m)
            al = torch.exp2(m - m_new)
            l = l * al
            if mut != "skip_o_rescale":
                o = o * al.unsqueeze(-1)
            m = m_new
        p = torch.exp2(st - m.unsqueeze(-1))
        l = l + p.sum(-1)
        if dup is not None and t0 <= dup < t0 + TILE:
            l = l + p[..., dup - t0]
        o = o + p.to(BF16).to(F32) @ v[:, t0 : t0 + TILE]
    return (o / l.unsqueeze(-1)).to(BF16)


EMULATIONS = ("global", "lazy8", "lazy4", "eager")  # three kinds; the lazy one at both thresholds the kernels are built with


def rel_l2(got, o):
    n = o.norm()
    return float((got.to(F64) - o).norm() / n) if n > 0 else float((got.to(F64) - o).norm())


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 29) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def h_map(Sq, Sk):
    """j(i) = (37 i + Sk - 1) mod Sk, with keys 0, 63, 64 and Sk - 1 forced into the image when Sq >= 4 (clamped to Sk - 1)."""
    j = (37 * torch.arange(Sq, dtype=torch.int64) + Sk - 1) % Sk
    if Sq >= 4:
        j[0], j[1], j[2], j[3] = Sk - 1, 0, min(TILE - 1, Sk - 1), min(TILE, Sk - 1)
    return j


class Inputs:
    """One seeded case: q [H, Sq, 128], k, v [H, Sk, 128] bf16 on the CPU."""

    def __init__(self, family, Sq, Sk, H, spike="none", seed=0):
        assert family in FAMILIES and spike in SPIKES and (spike == "none" or family == "R")
        self.family, self.Sq, self.Sk, self.H, self.spike, self.seed = family, Sq, Sk, H, spike, seed
        g = _gen(FAMILIES.index(family), Sq, Sk, H, SPIKES.index(spike), seed)
        rn = lambda *shape: torch.randn(*shape, generator=g).to(BF16)
        if family == "R":
            q, k, v = rn(H, Sq, D), rn(H, Sk, D), rn(H, Sk, D)
            if spike != "none":  # a key four times as long: the lazy-rescale branch fires early, late, and inside the masked tile
                j = {"first": min(3, Sk - 1), "middle": Sk // 2, "last": Sk - 1}[spike]
                k[:, j] = k[:, j] * 4
        elif family == "N":  # every real score far below 0: a key past Sk (score 0) would take the whole softmax
            q = (torch.rand(H, Sq, D, generator=g) + 0.5).to(BF16)
            k = (-(torch.rand(H, Sk, D, generator=g) + 0.5)).to(BF16)
            v = rn(H, Sk, D)
        elif family == "H":  # one key decides each row: the output is that key's V row, bit for bit
            k = (torch.randint(0, 2, (H, Sk, D), generator=g) * 2 - 1).to(BF16)
            self.j = h_map(Sq, Sk)
            q = 8 * k[:, self.j]
            v = rn(H, Sk, D)
            v = torch.where(v.abs() < 2.0 ** -6, torch.where(v < 0, -(2.0 ** -6), 2.0 ** -6).to(BF16), v)
        else:  # U: all scores equal, v = 1: the output is the row sum over itself
            q, k, v = rn(H, Sq, D), torch.zeros(H, Sk, D, dtype=BF16), torch.ones(H, Sk, D, dtype=BF16)
        self.q, self.k, self.v = q, k, v

    @property
    def name(self):
        return f"{self.family}{'' if self.spike == 'none' else '-' + self.spike} Sq={self.Sq} Sk={self.Sk} H={self.H}"

    def take(self, heads=None, rows=None):
        """The same case cut to some heads / query rows (whole 256-row blocks: the waves of the lazy-rescale decision stay aligned)."""
        c = object.__new__(Inputs)
        c.__dict__.update(self.__dict__)
        if heads is not None:
            hs = torch.as_tensor(heads)
            c.q, c.k, c.v, c.H = self.q[hs], self.k[hs], self.v[hs], len(heads)
        if rows is not None:
            c.q, c.Sq = c.q[:, rows], int(rows.numel())
            if self.family == "H":
                c.j = self.j[rows]
        c.seed = (self.seed, None if heads is None else tuple(heads), None if rows is None else (int(rows[0]), int(rows.numel()), self.Sq))
        return c

    def q_for(self, form, scale=0.0):
        return prescale_q(self.q, scale) if form == "pre" else self.q

    def exact(self):
        """What the output must equal bit for bit (H, U), or None."""
        if self.family == "H":
            return self.v[:, self.j]
        if self.family == "U":
            return torch.ones(self.H, self.Sq, D, dtype=BF16)
        return None

    def assert_margins(self, form="vt", scale=0.0):
        """The property the family's argument rests on, checked in float64 on the scores of the form under test."""
        if self.family not in ("N", "H"):
            return None
        s = scores(self.q_for(form, scale), self.k, scale, **form_args(form))
        if self.family == "N":
            top = float(s.max())
            assert top <= N_MARGIN, f"{self.name} {form}: a real score of {top:.2f} base-2 units (must stay <= {N_MARGIN})"
            return top
        rows = torch.arange(self.Sq)
        lead = s[:, rows, self.j].clone()
        assert (s.argmax(-1) == self.j).all(), f"{self.name} {form}: a row is not led by its matched key"
        s[:, rows, self.j] = -math.inf
        margin = float((lead - s.amax(-1)).min()) if self.Sk > 1 else math.inf
        assert margin >= H_MARGIN, f"{self.name} {form}: matched key leads by only {margin:.1f} base-2 units (must lead by >= {H_MARGIN})"
        return margin


class Expect:
    """Reference side of one (inputs, form, scale): o, A in float64 and Y, all [H, Sq, 128] / a float; emulation outputs kept for the host module."""

    def __init__(self, inp, form, scale=0.0, keep=False):
        q, kw = inp.q_for(form, scale), form_args(form)
        self.inp, self.form, self.scale = inp, form, scale
        self.o, self.A = ref64(q, inp.k, inp.v, scale, **kw)
        s32 = scores(q, inp.k, scale, dtype=F32, **kw)
        v32 = inp.v.to(F32)
        outs = {kind: emulate(s32, v32, kind) for kind in EMULATIONS}
        self.y = {kind: rel_l2(e, self.o) for kind, e in outs.items()}
        self.Y = max(self.y.values())
        self.emulated = outs if keep else None
        self.s32, self.v32 = (s32, v32) if keep else (None, None)

    def tol(self):
        return ULP * self.o.abs() + P_ROUND * self.A


_EXPECT = {}


def expect(inp, form, scale=0.0):
    """Expect(...) computed once per (case, form, scale) and shared by the tests of a run; a prescaled q at the default scale IS the re-rounded q
    of the plain entry, so 'pre' and 'vt' share one reference there."""
    f = "vt" if (form == "pre" and scale <= 0) else form
    key = (inp.family, inp.Sq, inp.Sk, inp.H, inp.spike, inp.seed, f, float(scale))
    if key not in _EXPECT:
        e = Expect(inp, f, scale)
        if e.o.numel() > (1 << 22):  # large cases are used once
            return e
        _EXPECT[key] = e
    return _EXPECT[key]


# ------------------------------------------------------------------------------------------------------------------- acceptance
class Reject(AssertionError):
    def __init__(self, criterion, msg):
        super().__init__(msg)
        self.criterion = criterion


class Case:
    """Accumulates the measured figures of one kernel form over its inputs; every check asserts both criteria."""

    def __init__(self, name, record=True):
        self.name, self.record, self.rows = name, record, []

    def check(self, got, exp, what=""):
        """got: bf16 [H, Sq, 128] on the CPU; exp: an Expect.  Returns (relL2, Y, worst d/tol)."""
        g = got.to(F64)
        tag = f"{self.name} {exp.inp.name} {what}".strip()
        if g.shape != exp.o.shape:
            raise Reject("shape", f"{tag}: shape {tuple(g.shape)} vs {tuple(exp.o.shape)}")
        if not torch.isfinite(g).all():
            raise Reject("finite", f"{tag}: non-finite output")
        err, tol = (g - exp.o).abs(), exp.tol()
        ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        worst, rel = float(ratio.max()), rel_l2(g, exp.o)
        self.rows.append((exp.inp.name, what, rel, exp.Y, worst))
        if self.record:
            from tests.util import record as rec

            rec(f"attn_fp64 {tag}", relL2=rel, Y=exp.Y, ratio=(rel / exp.Y if exp.Y > 0 else 0.0), worst_d_over_tol=worst)
        over = err > tol
        if over.any():
            i = int(ratio.reshape(-1).argmax())
            raise Reject("element", f"{tag}: {int(over.sum())} of {err.numel()} elements ({float(over.double().mean()):.2%}) outside 2^-7|o| + 1.05*2^-8*A; worst at flat "
                                    f"index {i}: got {g.reshape(-1)[i].item():.9g} ref {exp.o.reshape(-1)[i].item():.9g} tol {tol.reshape(-1)[i].item():.3g}")
        if rel > TRIANGLE * exp.Y:
            raise Reject("aggregate", f"{tag}: relL2 {rel:.4e} > 1.5 * Y, Y = {exp.Y:.4e} (emulations: {', '.join(f'{k} {y:.4e}' for k, y in exp.y.items())})")
        ex = exp.inp.exact()
        if ex is not None and not torch.equal(got, ex):
            raise Reject("exact", f"{tag}: {int((got != ex).sum())} elements differ from the exact answer of family {exp.inp.family}")
        return rel, exp.Y, worst

    @property
    def max_ratio(self):
        return max((r / y for _, _, r, y, _ in self.rows if y > 0), default=0.0)

    def table(self):
        """One line per (shape, what): the family with the largest relL2 / Y, and the largest d/tol over the families."""
        by = {}
        for n, w, r, y, d in self.rows:
            fam, shape = n.split(" ", 1)
            by.setdefault((shape, w), []).append((r / y if y > 0 else 0.0, fam, r, y, d))
        out = []
        for (shape, w), rows in by.items():
            ratio, fam, r, y, _ = max(rows)
            out.append(f"{self.name:<24} {shape:<26} {w:<18} n={len(rows):<2} relL2 {r:.4e}  Y {y:.4e}  ratio {ratio:5.3f} ({fam:<8})  worst d/tol {max(x[4] for x in rows):5.3f}")
        return out


# ------------------------------------------------------------------------------------------------------------------- the GPU module's shapes
SK_SWEEP = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 320, 1031)  # at Sq = 257, H = 2: nt = 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 5, 5, 17
SK_SWEEP_SQ, SK_SWEEP_H = 257, 2
SQ_SWEEP = (1, 15, 17, 31, 33, 255, 256, 257, 515)  # the 16-row group, the 32-row wave, the 256-row block
SQ_SWEEP_SK, SQ_SWEEP_H = (129, 192), 3
SCALE_SHAPE, ODD_SCALE = (257, 193, 2), 0.05
STAGGER_SQ, STAGGER_SK = 2048 + 5, (1024, 1031, 1088, 1150)  # nine query blocks: rot = 0..7 and the wrap; nt = 16, 17, 17, 18
XCD_SHAPES = ((2053, 129, 57), (2053, 193, 64))  # nwg = 513 (nwg % 8 = 1) and 576 (8 | nwg)
XCD_BATCHED = (2, 2112, 129, 29)  # B, rows per sequence (nine blocks), keys, H: nwg = 522, nwg % 8 = 2
BATCHED = (3, 320, 257, 2)  # B, rows per sequence, keys, H
P9_NT = tuple(range(4, 33))
P9_SQ = 257
P9_FAMILIES = (("R", "middle"), ("N", "none"), ("H", "none"))
CHECKED_HEADS = 8


def sweep_families():
    return [("R", s) for s in SPIKES] + [("N", "none"), ("H", "none"), ("U", "none")]


def checked_heads(H, n=CHECKED_HEADS):
    """First, last and n - 2 spread between them."""
    return sorted({round(i * (H - 1) / (n - 1)) for i in range(n)}) if H > n else list(range(H))


def checked_rows(Sq, n=CHECKED_HEADS, block=256):
    """All rows while there are at most n query blocks, else the rows of the first, the last (ragged) and n - 2 blocks spread between them."""
    nqb = (Sq + block - 1) // block
    if nqb <= n:
        return torch.arange(Sq)
    return torch.cat([torch.arange(b * block, min((b + 1) * block, Sq)) for b in checked_heads(nqb, n)])


def p9_walk_cases(cus=256):
    """(label, Sq, Sk, H, prescaled) of the persistent form's item walk on a chip of `cus` CUs: gridDim.x = cus workgroups take items
    blockIdx.x + i * cus of the (head, query block) list, stepping dq = cus % nqb blocks and dh = cus / nqb heads.  Ragged last query blocks."""
    H1 = next(h for h in range((2 * cus + 2) // 3, 4 * cus) if (3 * h) % cus == 1)
    return [("nqb=1", 200, 256, 2 * cus, False), (f"nqb={cus} dq=0 dh=1", 256 * (cus - 1) + 37, 320, 2, True), (f"nqb={cus // 2}", 256 * (cus // 2 - 1) + 37, 256, 4, False),
            (f"nqb={cus + 1} dh=0", 256 * cus + 37, 320, 2, False), ("items % cus = 1", 2 * 256 + 37, 256, H1, True)]


P9_BATCHED = (2, 320, 256, 128)  # B, rows per sequence (two query blocks, the second of 64 rows), keys, H: 512 items


def gpu_shapes(cus=256):
    """Every (Sq, Sk, H, families) the GPU module checks against float64, heads and query blocks cut to the checked ones (heads and 256-row blocks
    are independent problems for the reference side)."""
    out = [(SK_SWEEP_SQ, Sk, SK_SWEEP_H, sweep_families()) for Sk in SK_SWEEP]
    out += [(Sq, Sk, SQ_SWEEP_H, sweep_families()) for Sk in SQ_SWEEP_SK for Sq in SQ_SWEEP]
    out += [(STAGGER_SQ, Sk, 1, list(P9_FAMILIES)) for Sk in STAGGER_SK]
    out += [(Sq, Sk, min(H, CHECKED_HEADS), list(P9_FAMILIES)) for Sq, Sk, H in XCD_SHAPES]
    out += [(XCD_BATCHED[1], XCD_BATCHED[2], CHECKED_HEADS, list(P9_FAMILIES)), (BATCHED[1], BATCHED[2], BATCHED[3], list(P9_FAMILIES))]
    out += [(P9_SQ, nt * TILE, CHECKED_HEADS, list(P9_FAMILIES)) for nt in P9_NT]
    out += [(int(checked_rows(Sq).numel()), Sk, min(H, CHECKED_HEADS), list(P9_FAMILIES)) for _, Sq, Sk, H, _ in p9_walk_cases(cus)]
    out += [(P9_BATCHED[1], P9_BATCHED[2], CHECKED_HEADS, list(P9_FAMILIES))]
    return out
