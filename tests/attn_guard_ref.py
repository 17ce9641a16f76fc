"""The sum guard of the ping-pong attention kernels' softmax half-step (A9_SOFTMAX in lightx2v_amd/csrc/attn.hip), in plain PyTorch on the CPU:
the lane's tile sums in the kernel's own association, the guard, the lazy-rescale walk with the decision taken guard-then-max, and the inputs
of tests/test_gpu_attn_sum_guard.py, each built to reach one arm of that code.  Nothing here imports the library.  Shared by
tests/test_attn_sum_guard_host.py, tests/test_gpu_attn_sum_guard.py and tools/attn_guard_rate.py.

The kernel: scores leave the MFMA as sc = s - m_run.  Lane (c, qd) owns, for the query row of its column c, the 16 keys 32 j + 8 qd + e of a
64-key tile (j = 0, 1; e = 0..7); it adds their P = exp2(sc) into two chains in key order (chain 0: even e, chain 1: odd e), each started from
its first P.  The guard fires for the wave when some lane's chain 0 + chain 1 >= GUARD_T; only then are the row maxima looked for and the exact
condition `some row's max > 8` evaluated (attn_ref.emulate's 'lazy8' decision)."""
import torch

from tests import attn_ref as A

F64, F32, BF16 = A.F64, A.F32, A.BF16
THR = 8  # RESCALE_THR of every instantiation the launchers use
GUARD_T = float(torch.tensor(2.0 ** THR, dtype=F32) * (torch.tensor(1.0, dtype=F32) - torch.tensor(2.0 ** -10, dtype=F32)))  # A9_GUARD_T
LANES = 4  # the four qd of a query column


def chain_sums(p16):
    """p16 [..., 16]: a lane's P values of one query group in key order -> (chain 0, chain 1), added one by one in the dtype of p16."""
    c0, c1 = p16[..., 0], p16[..., 1]
    for i in range(2, 16, 2):
        c0, c1 = c0 + p16[..., i], c1 + p16[..., i + 1]
    return c0, c1


def guard16(p16):
    """Does a lane holding these 16 values fire the guard?"""
    c0, c1 = chain_sums(p16)
    return (c0 + c1) >= GUARD_T


def lane_values(p):
    """p [..., 64] (one tile's P of a row, key order) -> [..., 4 lanes, 16]: lane qd's keys 32 j + 8 qd + e in (j, e) order."""
    x = p.reshape(*p.shape[:-1], 2, LANES, 8)
    return x.transpose(-3, -2).reshape(*p.shape[:-1], LANES, 16)


def _waves(x, fill):
    """x [H, Sq] -> [H, waves, 32], the last wave padded with `fill`."""
    H, Sq = x.shape
    pad = (-Sq) % A.WAVE_ROWS
    return torch.nn.functional.pad(x, (0, pad), value=fill).reshape(H, -1, A.WAVE_ROWS)


def _per_row(w, Sq):
    """[H, waves] -> [H, Sq]"""
    return w.unsqueeze(-1).expand(-1, -1, A.WAVE_ROWS).reshape(w.shape[0], -1)[:, :Sq]


def emulate_guarded(s, v, dtype=F32, trace=None):
    """attn_ref.emulate(s, v, 'lazy8') with the rescale decision taken the kernel's way: guard first, then the exact condition, both wave-uniform.
    Everything else is emulate's arithmetic line for line, so the outputs are bit-equal exactly when every decision is the same.  trace: a list
    that receives, per tile after the first, a dict of [H, waves] tensors: `guard`, `exact` (would the max-only decision fire), `lane_sum` (the
    largest chain 0 + chain 1 of the wave) and `top` (the largest sc of the wave)."""
    s, v = s.to(dtype), v.to(dtype)
    H, Sq, Sk = s.shape
    m, l, o = None, torch.zeros(H, Sq, dtype=dtype, device=s.device), torch.zeros(H, Sq, A.D, dtype=dtype, device=s.device)
    for t0 in range(0, Sk, A.TILE):
        st = s[..., t0 : t0 + A.TILE]
        mt = st.amax(-1)
        if m is None:
            m = mt
        else:
            pad = torch.nn.functional.pad(st - m.unsqueeze(-1), (0, A.TILE - st.shape[-1]), value=-1e30)  # the kernel's key mask
            c0, c1 = chain_sums(lane_values(torch.exp2(pad)))
            lane_sum = (c0 + c1).amax(-1)
            guard = _waves(lane_sum >= GUARD_T, False).any(-1)
            exact = _waves(mt - m > THR, False).any(-1)
            if trace is not None:
                trace.append(dict(guard=guard, exact=exact, lane_sum=_waves(lane_sum, 0.0).amax(-1), top=_waves(mt - m, -1e30).amax(-1)))
            grow = _per_row(guard & exact, Sq)
            m_new = torch.where(grow, torch.maximum(m, mt), m)
            al = torch.exp2(m - m_new)
            l = l * al
            o = o * al.unsqueeze(-1)
            m = m_new
        p = torch.exp2(st - m.unsqueeze(-1))
        l = l + p.sum(-1)
        o = o + p.to(BF16).to(dtype) @ v[:, t0 : t0 + A.TILE]
    return (o / l.unsqueeze(-1)).to(BF16)


# ------------------------------------------------------------------------------------------------------------------- the GPU module's inputs
CASES = ("a", "b", "c-middle", "c-last", "d", "e")
ARMS = {"a": "hot", "b": "false-positive", "c-middle": "rescale", "c-last": "rescale", "d": "rescale", "e": "rescale"}
ROW, ROW_E = 5, 32  # the query row a case aims at: one of the first wave; the 33rd row, alone in the second wave
QUIET = 2.0 ** (THR - 1)  # a lane sum this far below GUARD_T stays below it in fp32 as well
B_LO, B_HI = 5.2, 5.8  # case (b): sc of the eight keys, inside the 5..6 the construction is specified with
C_LO, C_HI = 9.0, 12.0
D_MIN = 140.0
Q_BOOST = 8.0  # case (d): the aimed row of q is this much longer, so its key can stay short


def _aim(inp, row, keys, above, m_row):
    """Overwrite K rows `keys` with the multiple of the aimed row's (rounded, scaled) q that scores m_row + above for it, per head."""
    qp = A.prescale_q(inp.q)[:, row].to(F64)  # [H, 128]: what both v9 forms multiply (a prescaled q at the default scale is this q)
    alpha = (m_row + above) / (qp * qp).sum(-1)  # [H]
    inp.k[:, keys] = (alpha.unsqueeze(-1) * qp).to(BF16).unsqueeze(1).expand(-1, len(keys), -1)


def build_case(case, Sq, Sk, H):
    """(inputs, tile, wave, arm) of one case: an 'R' family of attn_ref with a few K rows (case d: and one q row) overwritten; `tile` is the key
    tile the case aims at (None: every tile stays quiet) and `wave` the wave that must reach `arm` there."""
    assert case in CASES and Sk > 3 * A.TILE
    inp = A.Inputs("R", Sq, Sk, H)
    inp.q, inp.k = inp.q.clone(), inp.k.clone()
    inp.seed = ("sum-guard", case)  # its own entry in attn_ref.expect's table
    nt = (Sk + A.TILE - 1) // A.TILE
    row = ROW_E if case == "e" else ROW
    if case == "d":
        inp.q[:, row] = inp.q[:, row] * Q_BOOST
    m_row = A.scores(inp.q, inp.k[:, : A.TILE], q_rounded=True)[:, row].amax(-1)  # [H]: the aimed row's reference after tile 0
    if case == "a":  # keys behind the first tile half as long: their scores stay near 0
        inp.k[:, A.TILE :] = inp.k[:, A.TILE :] * 0.5
        tile = None
    elif case == "b":  # tile 2, lane qd = 2, key group j = 1: keys 32 j + 8 qd + e
        tile = 2
        _aim(inp, row, list(range(tile * A.TILE + 48, tile * A.TILE + 56)), 0.5 * (B_LO + B_HI), m_row)
    elif case == "c-last":
        tile = nt - 1
        assert Sk % A.TILE != 0, "case c-last wants a partly filled last tile"
        _aim(inp, row, [Sk - 1], 0.5 * (C_LO + C_HI), m_row)
    elif case == "d":
        tile = 1
        _aim(inp, row, [tile * A.TILE + 21], D_MIN + 10.0, m_row)
    else:  # c-middle, e
        tile = 2
        _aim(inp, row, [tile * A.TILE + 37], 0.5 * (C_LO + C_HI), m_row)
    return inp, tile, row // A.WAVE_ROWS, ARMS[case]


def assert_lands(inp, tile, wave, arm):
    """The construction really reaches its arm: the walk in float64 on the scores the kernels see, with margins that fp32 cannot cross.  Every tile
    other than the aimed one, and every other wave in it, must stay on the hot path."""
    s = A.scores(inp.q, inp.k, q_rounded=True)
    trace = []
    emulate_guarded(s, inp.v, F64, trace)
    name = f"{inp.name} {inp.seed[1]}"
    for t, tr in enumerate(trace, start=1):
        for h in range(inp.H):
            for w in range(tr["guard"].shape[1]):
                top, lane = float(tr["top"][h, w]), float(tr["lane_sum"][h, w])
                if t != tile or w != wave:
                    assert lane <= QUIET and top <= THR - 1, f"{name}: tile {t} head {h} wave {w} is not quiet (lane sum {lane:.1f}, top {top:.2f})"
                elif arm == "false-positive":
                    assert lane >= 8 * 2.0 ** B_LO > 1.1 * GUARD_T and B_LO <= top <= B_HI, f"{name}: tile {t} head {h}: lane sum {lane:.1f}, top {top:.2f}"
                    assert bool(tr["guard"][h, w]) and not bool(tr["exact"][h, w])
                else:
                    lo, hi = (D_MIN, 1e9) if inp.seed[1] == "d" else (C_LO, C_HI)
                    assert lo <= top <= hi, f"{name}: tile {t} head {h}: top {top:.2f} outside [{lo}, {hi}]"
                    assert bool(tr["guard"][h, w]) and bool(tr["exact"][h, w])
    if arm == "hot":
        late = s[..., A.TILE :].amax(-1) - s[..., : A.TILE].amax(-1)
        assert float(late.max()) <= 2.0, f"{name}: a score {float(late.max()):.2f} above the first tile's max"
    if inp.seed[1] == "d":
        assert torch.isfinite(inp.q.float()).all() and torch.isfinite(inp.k.float()).all() and float(inp.k.float().abs().max()) < 64.0
    return trace
