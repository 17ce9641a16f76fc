"""float64 reference, fp32 emulations, seeded inputs and the acceptance rule for the fused fp16 attention of the HunyuanVideo VAE mid block
(lightx2v_amd/csrc/vae_attn.hip: x2v_vae_attn_prep_f16 + x2v_vae_attn_f16).  Plain PyTorch on the CPU; nothing here imports the library or the
oracle.  Shared by tests/test_vae_attn16_ref_host.py (the yardstick checked without a GPU) and tests/test_gpu_vae_attn16_fp64.py (the kernel
checked against it).

One head of width C over n = frames * hw tokens, qkv fp32 [n, 3 C] = q | k | v.  The contract (include/x2v.h): q, k, v rounded to fp16 once; a score
is the dot product of the fp16 rows times fp32(scale) * 1.4426950408889634f, in base 2; row i sees the keys j < lim_i = (i // hw + 1) * hw; the
softmax runs online over 64-key tiles, a row's reference maximum m following its running maximum only when that has grown by more than 8; p = 2^(s - m)
is rounded to fp16 for P . V only and enters the row sum unrounded; out = accumulator * (1 / row sum) in fp32.

Acceptance (Case.check), no share of elements left out:
  * every element: |got - o| <= 1.05 * 2^-10 * A + 2^-22 * |o|, A = sum_j w_j |v_jc| the softmax-weighted mean of |v|: got - o = sum_j w_j delta_j v_j
    with |delta_j| <= 2 * 2^-11 (the fp16 rounding of p, numerator against the unrounded row sum; attn_ref's P_ROUND moved from bf16 to fp16), and
    2^-22 |o| for the fp32 division and the final multiplication;
  * aggregate: relL2(got - o) <= 1.5 * Y, Y the larger relative L2 error of two emulations of a correct kernel on the same inputs (64-key tiles
    with the per-row lazy maximum; one pass with the global maximum) - computed here, never from the code under test; 1.5 is attn_ref's triangle factor;
  * family U only (read-out): |got - o| <= 2^-21 * max(|o|, 2^-10) - every p is exactly 1, every sum an integer below 2^24, so only the division and
    the multiplication round (2^-24 each, relative); 2^-21 leaves a factor of four for a reciprocal that is good to one ulp.

Input families (Inputs), seeded:
  U  q = 0, k random, v integers in [-8, 8]: out[i] = mean(v[:lim_i]).  Inputs asserts, for every row, that the means over lim_i - 1 and lim_i + 1 keys
     (keys from n on are the zero padding a kernel could read) lie outside the read-out rule in at least one channel: a prefix limit off by one key
     in any row is rejected, however flat the softmax.
  L  rank-one scores s_ij = a_i g_j in base-2 units (q_i = a_i e, k_j = b_j e, e four-hot): g constant inside a 64-key tile plus a jitter of +-0.2,
     stepping from tile to tile by one of LADDERS; a_i cycles through 1, 0.5, -1 inside every 16 rows, so the rows of one block move their reference
     maximum at different tiles and some never do; v random.
  R  N(0, 1) everywhere, the keys of the last frame times a gain of 1 or 6 (the inputs of tests/test_gpu_vae_attn16.py)."""
import math

import torch

F64, F32, F16 = torch.float64, torch.float32, torch.float16
TILE = 64  # keys per tile, and query rows per workgroup (vae_attn.hip VA_KEYS, VA_ROWS)
LAZY = 8.0  # VA_LAZY
P_ROUND = 1.05 * 2.0 ** -10
DIV = 2.0 ** -22
TRIANGLE = 1.5
READOUT, READOUT_FLOOR = 2.0 ** -21, 2.0 ** -10
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=F32)
LADDERS = ("+3", "+7.5", "+8.5", "-3", "flat+40", "flat+160")
GAINS = (1.0, 6.0)
JITTER = 0.2
A_CYCLE = (1.0, 0.5, -1.0)
EMULATIONS = ("lazy8", "global")
MUTATIONS = ("see_one_more", "hide_last_visible", "block_first_row_limit", "pad_keys_leak", "skip_o_rescale", "skip_l_rescale")
# (C, hw, frames): a frame boundary on a tile edge and one key either side of it; pure causal with a last block of 6 rows; one tile only; one frame
# (only the tail from n on is masked); the ladder's 5-tile walk; blocks that span frames with a last block of 4 rows
CASES = ((128, 64, 3), (128, 63, 3), (128, 65, 3), (128, 1, 70), (128, 5, 7), (128, 129, 1), (128, 64, 5), (512, 24, 3), (512, 33, 4), (512, 1, 65), (512, 64, 5))
R_AT_512 = ((512, 24, 3), (512, 33, 4))  # the two C = 512 cases that also run family R


def scale_log2e(scale):
    """The float the launcher hands to the kernel: (float)scale * 1.4426950408889634f."""
    return torch.tensor(scale, dtype=F32) * LOG2E_F32


def limits(n, hw):
    """lim_i = (i // hw + 1) * hw, int64 [n]."""
    return (torch.arange(n) // hw + 1) * hw


def _split16(qkv, n, C, dtype):
    return tuple(t.to(F16).to(dtype) for t in qkv[:n, : 3 * C].split(C, dim=1))


def ref64(qkv, n, C, hw, scale):
    """float64 attention in base 2 on the fp16-rounded operands.  Returns (o, A), both [n, C]: o unrounded, A = sum_j w_j |v_jc|."""
    q, k, v = _split16(qkv, n, C, F64)
    s = (q @ k.t()) * scale_log2e(scale).to(F64)
    s = torch.where(torch.arange(n)[None, :] < limits(n, hw)[:, None], s, torch.tensor(-math.inf, dtype=F64))
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    w = w / w.sum(-1, keepdim=True)
    return w @ v, w @ v.abs()


# ------------------------------------------------------------------------------------------------------------------- emulations
def spans_frames(n, hw):
    """Whether some 64-row block holds rows of two frames."""
    lim = limits(n, hw)
    return any(int(lim[min(r0 + TILE, n) - 1]) != int(lim[r0]) for r0 in range(0, n, TILE))


def mutation_applies(mut, n, hw):
    """A row with a key behind its limit exists when there is a second frame or zero padding inside the last tile; every row has a last visible key
    to hide once n >= 2; the first row's limit differs from a later row's only in a block that spans frames; padding keys exist only in a partly
    filled last tile; a rescale needs a second tile (tile 0 starts from an empty state)."""
    return {"see_one_more": n // hw >= 2 or n % TILE != 0, "hide_last_visible": n >= 2, "block_first_row_limit": spans_frames(n, hw),
            "pad_keys_leak": n % TILE != 0, "skip_o_rescale": n > TILE, "skip_l_rescale": n > TILE}[mut]


def emulate(qkv, n, C, hw, scale, kind="lazy8", mut=None):
    """A correct kernel in fp32 torch: fp32 scores of the fp16 operands; kind 'lazy8' walks 64-key tiles with the online softmax, each ROW's reference
    maximum adopting its running maximum only when that has grown by more than 8 (tile 0 always), the accumulated output and the row sum rescaled by
    2^(m_old - m_new) at each such move; kind 'global' is one pass under the global row maximum.  p is rounded to fp16 for P . V only and unrounded
    in the row sum; out = o * (1 / l) in fp32.  Keys n .. 64 ceil(n / 64) are the zero rows the preparation writes (score 0, v = 0), masked by the
    limit like any other.  mut: one of MUTATIONS - a subtly WRONG kernel, for the host module's rejection tests.  Returns fp32 [n, C]."""
    assert kind in EMULATIONS and (mut is None or mut in MUTATIONS)
    q, k, v = _split16(qkv, n, C, F32)
    nk = (n + TILE - 1) // TILE * TILE
    k, v = torch.nn.functional.pad(k, (0, 0, 0, nk - n)), torch.nn.functional.pad(v, (0, 0, 0, nk - n))
    s = (q @ k.t()) * scale_log2e(scale)
    lim = limits(n, hw)
    if mut == "see_one_more":
        lim = lim + 1
    elif mut == "hide_last_visible":
        lim = lim - 1
    elif mut == "block_first_row_limit":
        lim = lim[torch.arange(n) // TILE * TILE]
    vis = torch.arange(nk)[None, :] < lim[:, None]
    if mut == "pad_keys_leak":
        vis = vis | ((lim == n)[:, None] & (torch.arange(nk) >= n)[None, :])
    s = torch.where(vis, s, torch.tensor(-math.inf, dtype=F32))
    if kind == "global":
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        return (p.to(F16).to(F32) @ v) * (1.0 / p.sum(-1, keepdim=True))
    m, l, o = torch.full((n,), -math.inf), torch.zeros(n), torch.zeros(n, C)
    for t0 in range(0, nk, TILE):
        st = s[:, t0 : t0 + TILE]
        mt = st.amax(-1)
        move = mt > m + LAZY  # tile 0: m = -inf, always (key 0 is visible to every row)
        m_new = torch.where(move, mt, m)
        al = torch.where(move, torch.exp2(m - m_new), torch.ones(n))  # tile 0: 2^-inf = 0
        m = m_new
        p = torch.exp2(st - m[:, None])
        l = (l if mut == "skip_l_rescale" else l * al) + p.sum(-1)
        o = (o if mut == "skip_o_rescale" else o * al[:, None]) + p.to(F16).to(F32) @ v[t0 : t0 + TILE]
    return o * (1.0 / l)[:, None]


def rel_l2(got, o):
    n = o.norm()
    return float((got.to(F64) - o).norm() / n) if n > 0 else float((got.to(F64) - o).norm())


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 41) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ladder(n, variant, g):
    """g_j of family L: the tile's level plus a jitter in [-0.2, 0.2].  A step of 7.5 stays below the threshold of 8 with the jitter and one of 8.5
    above it; 'flat' ladders jump in the last tile of the sequence, which the rows of the last frame see."""
    tile = torch.arange(n) // TILE
    last = (n - 1) // TILE
    level = {"+3": 3.0 * tile, "+7.5": 7.5 * tile, "+8.5": 8.5 * tile, "-3": -3.0 * tile, "flat+40": 40.0 * (tile == last), "flat+160": 160.0 * (tile == last)}[variant]
    return level.to(F32) + JITTER * (2 * torch.rand(n, generator=g) - 1)


class Inputs:
    """One seeded case: qkv fp32 [n, 3 C] on the CPU, scale = 1 / sqrt(C).  variant: None (U), one of LADDERS (L), one of GAINS (R)."""

    def __init__(self, family, C, hw, frames, variant=None):
        assert family in "ULR" and variant in {"U": (None,), "L": LADDERS, "R": GAINS}[family]
        self.family, self.C, self.hw, self.frames, self.variant = family, C, hw, frames, variant
        self.n, self.scale = hw * frames, 1.0 / math.sqrt(C)
        n = self.n
        g = _gen("ULR".index(family), C, hw, frames, 0 if variant is None else 1 + (LADDERS.index(variant) if family == "L" else GAINS.index(variant)))
        qkv = torch.zeros(n, 3 * C)
        if family == "U":
            qkv[:, C : 2 * C] = torch.randn(n, C, generator=g)
            qkv[:, 2 * C :] = torch.randint(-8, 9, (n, C), generator=g).to(F32)
        elif family == "L":
            hot = [3, C // 4 + 5, C // 2 + 17, C - 1]  # one in each quarter of the row: every k-step region of Q K^T carries a quarter of the score
            a = torch.tensor(A_CYCLE)[(torch.arange(n) % 16) % 3]
            b = ladder(n, variant, g) / (len(hot) * float(scale_log2e(self.scale)))
            qkv[:, hot] = a[:, None].expand(n, len(hot))
            qkv[:, [C + h for h in hot]] = b.to(F16).to(F32)[:, None].expand(n, len(hot))
            qkv[:, 2 * C :] = torch.randn(n, C, generator=g)
        else:
            qkv = torch.randn(n, 3 * C, generator=g)
            qkv[n - hw :, C : 2 * C] *= variant  # the keys of the last frame: the running maximum rises late in the walk
        self.qkv = qkv
        if family == "U":
            self.sharpness = self._assert_sharp()

    @property
    def name(self):
        return f"{self.family}{'' if self.variant is None else f'({self.variant:g})' if self.family == 'R' else f'({self.variant})'} C={self.C} hw={self.hw} frames={self.frames}"

    def _assert_sharp(self):
        """Family U's premise, in float64: for every row, the mean over one key fewer (where a key remains) and over one key more (keys from n on are
        zeros) differs from the row's own by more than the read-out rule allows in at least one channel.  Returns the smallest such margin."""
        n, C = self.n, self.C
        v = self.qkv[:, 2 * C :].to(F64)
        csum = torch.cat([torch.zeros(1, C, dtype=F64), v.cumsum(0), v.sum(0, keepdim=True)])  # csum[L] = sum of the first L keys, L = 0 .. n + 1
        lim = limits(n, self.hw)
        o = csum[lim] / lim[:, None]
        tol = READOUT * o.abs().clamp_min(READOUT_FLOOR)
        worst = math.inf
        for d in (-1, 1):
            L = lim + d
            rows = L >= 1
            margin = (((csum[L[rows]] / L[rows, None]) - o[rows]).abs() / tol[rows]).amax(-1)
            assert bool((margin > 1).all()), f"{self.name}: row {int(rows.nonzero()[int(margin.argmin())])} reads the same means from {d:+d} keys"
            worst = min(worst, float(margin.min()))
        return worst


class Expect:
    """Reference side of one Inputs: o, A in float64, the emulations' relative L2 errors y and their maximum Y."""

    def __init__(self, inp, keep=False):
        self.inp = inp
        self.o, self.A = ref64(inp.qkv, inp.n, inp.C, inp.hw, inp.scale)
        outs = {kind: emulate(inp.qkv, inp.n, inp.C, inp.hw, inp.scale, kind) for kind in EMULATIONS}
        self.y = {kind: rel_l2(e, self.o) for kind, e in outs.items()}
        self.Y = max(self.y.values())
        self.emulated = outs if keep else None

    def tol(self):
        return P_ROUND * self.A + DIV * self.o.abs()


_EXPECT = {}


def expect(inp):
    """Expect(inp) computed once per case and shared by the tests of a run."""
    key = (inp.family, inp.C, inp.hw, inp.frames, inp.variant)
    if key not in _EXPECT:
        _EXPECT[key] = Expect(inp)
    return _EXPECT[key]


def case_inputs(C, hw, frames, families="ULR"):
    """The Inputs of one (C, hw, frames): U, the six ladders, R at both gains."""
    out = []
    for f in families:
        out += [Inputs(f, C, hw, frames, v) for v in {"U": (None,), "L": LADDERS, "R": GAINS}[f]]
    return out


def gpu_families(C, hw, frames):
    """U and L everywhere, R on every C = 128 case and on two of the C = 512 ones."""
    return "ULR" if C == 128 or (C, hw, frames) in R_AT_512 else "UL"


# ------------------------------------------------------------------------------------------------------------------- acceptance
class Reject(AssertionError):
    def __init__(self, criterion, msg):
        super().__init__(msg)
        self.criterion = criterion


def _ratio(err, tol):
    return torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


class Case:
    """Accumulates the measured figures of one checked implementation over its inputs; every check asserts every criterion."""

    def __init__(self, name, record=True):
        self.name, self.record, self.rows = name, record, []

    def check(self, got, exp, what=""):
        """got: fp32 [n, C] on the CPU; exp: an Expect.  Returns (relL2, Y, worst d/tol)."""
        g = got.to(F64)
        tag = f"{self.name} {exp.inp.name} {what}".strip()
        if g.shape != exp.o.shape:
            raise Reject("shape", f"{tag}: shape {tuple(g.shape)} vs {tuple(exp.o.shape)}")
        if not torch.isfinite(g).all():
            raise Reject("finite", f"{tag}: {int((~torch.isfinite(g)).any(1).sum())} rows with non-finite output")
        err, tol = (g - exp.o).abs(), exp.tol()
        ratio = _ratio(err, tol)
        worst, rel = float(ratio.max()), rel_l2(g, exp.o)
        self.rows.append((exp.inp.name, what, rel, exp.Y, worst))
        if self.record:
            from tests.util import record as rec

            rec(f"vae_attn16_fp64 {tag}", relL2=rel, Y=exp.Y, ratio=(rel / exp.Y if exp.Y > 0 else 0.0), worst_d_over_tol=worst)
        if exp.inp.family == "U":
            r = _ratio(err, READOUT * exp.o.abs().clamp_min(READOUT_FLOOR))
            if float(r.max()) > 1:
                i = int(r.amax(-1).argmax())
                raise Reject("readout", f"{tag}: {int((r > 1).any(1).sum())} rows outside 2^-21 max(|o|, 2^-10) of the mean over their prefix; worst row {i} "
                                        f"(limit {int(limits(exp.inp.n, exp.inp.hw)[i])}) at {float(r.max()):.3g} times the rule")
        if worst > 1:
            i = int(ratio.reshape(-1).argmax())
            over = ratio > 1
            raise Reject("element", f"{tag}: {int(over.sum())} of {err.numel()} elements ({float(over.double().mean()):.2%}) outside 1.05*2^-10*A + 2^-22|o|; worst d/tol "
                                    f"{worst:.3f} at row {i // g.shape[1]} column {i % g.shape[1]}: got {g.reshape(-1)[i].item():.9g} ref {exp.o.reshape(-1)[i].item():.9g}")
        if rel > TRIANGLE * exp.Y:
            raise Reject("aggregate", f"{tag}: relL2 {rel:.4e} > 1.5 * Y, Y = {exp.Y:.4e} (emulations: {', '.join(f'{k} {y:.4e}' for k, y in exp.y.items())})")
        return rel, exp.Y, worst

    @property
    def max_ratio(self):
        return max((r / y for _, _, r, y, _ in self.rows if y > 0), default=0.0)

    @property
    def max_worst(self):
        return max((r[4] for r in self.rows), default=0.0)

    def table(self):
        return [f"{self.name:<16} {n:<40} {w:<8} relL2 {r:.4e}  Y {y:.4e}  ratio {(r / y if y > 0 else 0.0):5.3f}  worst d/tol {d:5.3f}" for n, w, r, y, d in self.rows]
