"""A second witness for the guard of the ping-pong attention kernels' softmax half-step (A9_SOFTMAX in lightx2v_amd/csrc/attn.hip), in plain
PyTorch on the CPU, and the planted inputs of tests/test_gpu_attn_softmax_trim.py.  The kernels guard the lazy rescale with the sum of a query
group's two chain sums (tests/attn_guard_ref.py: the lane map, the chain association, GUARD_T).  The LARGEST of a lane's four chain sums (two
query groups x two chains) is a sound witness as well, one instruction shorter and with fewer false positives; it was built and measured slower
on the GPU, so the kernels keep the pair sum.  What is pinned here holds for either: both fire whenever the exact condition
does, the chain-max guard on a subset of the pair-sum guard's tiles, and the m_run / rescale sequence is the same under both — a later change
of witness changes no output bit.  Nothing here imports the library."""
import torch

from tests import attn_guard_ref as G
from tests import attn_ref as A

F64, F32, BF16 = A.F64, A.F32, A.BF16
THR, GUARD_T = G.THR, G.GUARD_T


def chain_max16(p16):
    """p16 [..., 16]: a lane's P of one query row in key order -> the larger of its two chain sums."""
    c0, c1 = G.chain_sums(p16)
    return torch.maximum(c0, c1)


def guard16(p16):
    return chain_max16(p16) >= GUARD_T


def pair_guard16(p16):
    """The guard the kernels use."""
    return G.guard16(p16)


def emulate_guarded(s, v, dtype=F32, trace=None, witness="chain"):
    """attn_guard_ref.emulate_guarded with the witness chosen: 'chain' (max of the chain sums) or 'pair' (chain 0 + chain 1).  trace receives, per
    tile after the first, `guard`, `exact`, `fired` (= guard & exact, the rescale decision), `lane_sum` (the wave's largest witness value),
    `top` (its largest sc) — [H, waves] each — and `m` (the running reference [H, Sq] after the tile)."""
    assert witness in ("chain", "pair")
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
            c0, c1 = G.chain_sums(G.lane_values(torch.exp2(pad)))
            lane_sum = (torch.maximum(c0, c1) if witness == "chain" else c0 + c1).amax(-1)
            guard = G._waves(lane_sum >= GUARD_T, False).any(-1)
            exact = G._waves(mt - m > THR, False).any(-1)
            grow = G._per_row(guard & exact, Sq)
            m_new = torch.where(grow, torch.maximum(m, mt), m)
            al = torch.exp2(m - m_new)
            l = l * al
            o = o * al.unsqueeze(-1)
            if trace is not None:
                trace.append(dict(guard=guard, exact=exact, fired=guard & exact, lane_sum=G._waves(lane_sum, 0.0).amax(-1), top=G._waves(mt - m, -1e30).amax(-1), m=m_new.clone()))
            m = m_new
        p = torch.exp2(st - m.unsqueeze(-1))
        l = l + p.sum(-1)
        o = o + p.to(BF16).to(dtype) @ v[:, t0 : t0 + A.TILE]
    return (o / l.unsqueeze(-1)).to(BF16)


# ------------------------------------------------------------------------------------------------------------------- the GPU module's inputs
# A crossing score in each of the four chains of a lane: query group g = the aimed row's 16-row half of its wave, chain = the key's parity.
ROWS = {0: 5, 1: 21}  # a row of group 0 / group 1 of the first wave
CHAINS = tuple((g, c) for g in (0, 1) for c in (0, 1))
ARMS = ("hot",) + tuple(f"chain{g}{c}-{where}" for where in ("middle", "last") for g, c in CHAINS) + ("eight-at-2^5", "inf", "second-wave")


def build_arm(arm, Sq, Sk, H):
    """(inputs, tile, wave, kind) for one arm: kind is 'hot', 'silent' (the pair-sum guard fires without cause, the chain-max guard does not), or 'rescale'."""
    assert arm in ARMS and Sk > 3 * A.TILE
    nt = (Sk + A.TILE - 1) // A.TILE
    inp = A.Inputs("R", Sq, Sk, H)
    inp.q, inp.k = inp.q.clone(), inp.k.clone()
    inp.seed = ("softmax-trim", arm)
    inp.k[:, A.TILE :] = inp.k[:, A.TILE :] * 0.5  # keys behind the first tile half as long: every tile but the aimed one stays quiet at any Sq
    if arm == "hot":
        return inp, None, 0, "hot"
    row = G.ROW_E if arm == "second-wave" else G.ROW if arm in ("eight-at-2^5", "inf") else ROWS[int(arm[5])]
    if arm == "inf":
        inp.q[:, row] = inp.q[:, row] * G.Q_BOOST
    m_row = A.scores(inp.q, inp.k[:, : A.TILE], q_rounded=True)[:, row].amax(-1)  # [H]: the aimed row's reference after tile 0
    if arm == "eight-at-2^5":  # tile 2, lane qd = 2, key group j = 1: keys 32 j + 8 qd + e
        G._aim(inp, row, list(range(2 * A.TILE + 48, 2 * A.TILE + 56)), 0.5 * (G.B_LO + G.B_HI), m_row)
        return inp, 2, row // A.WAVE_ROWS, "silent"
    if arm == "inf":
        G._aim(inp, row, [A.TILE + 21], G.D_MIN + 10.0, m_row)
        return inp, 1, row // A.WAVE_ROWS, "rescale"
    if arm == "second-wave":
        G._aim(inp, row, [2 * A.TILE + 37], 0.5 * (G.C_LO + G.C_HI), m_row)
        return inp, 2, row // A.WAVE_ROWS, "rescale"
    c, where = int(arm[6]), arm.split("-")[1]
    tile = 2 if where == "middle" else nt - 1
    left = min(A.TILE, Sk - tile * A.TILE)
    key = tile * A.TILE + (left - 1 if (left - 1) % 2 == c else left - 2)  # the last key of the tile with parity c (keys 32 j + 8 qd + e: chain = e & 1)
    assert key % 2 == c and tile * A.TILE <= key < Sk
    G._aim(inp, row, [key], 0.5 * (G.C_LO + G.C_HI), m_row)
    return inp, tile, row // A.WAVE_ROWS, "rescale"


def assert_lands(inp, tile, wave, kind):
    """The walk in float64 on the scores the kernels see: the aimed (tile, wave) reaches its arm under the chain-max guard, every other tile and
    wave stays on the hot path with margins fp32 cannot cross, and the rescale decisions are those of the pair-sum guard."""
    s = A.scores(inp.q, inp.k, q_rounded=True)
    new, old = [], []
    emulate_guarded(s, inp.v, F64, new, "chain")
    emulate_guarded(s, inp.v, F64, old, "pair")
    name = f"{inp.name} {inp.seed[1]}"
    for t, (tr, to) in enumerate(zip(new, old), start=1):
        assert torch.equal(tr["fired"], to["fired"]) and torch.equal(tr["m"], to["m"]), f"{name}: tile {t}: the two guards decide differently"
        assert bool((to["guard"] | ~tr["guard"]).all()), f"{name}: tile {t}: the chain-max guard fires where the pair-sum guard does not"
        for h in range(inp.H):
            for w in range(tr["guard"].shape[1]):
                top, lane = float(tr["top"][h, w]), float(tr["lane_sum"][h, w])
                if t != tile or w != wave:
                    assert lane <= G.QUIET and top <= THR - 1, f"{name}: tile {t} head {h} wave {w} is not quiet (chain sum {lane:.1f}, top {top:.2f})"
                elif kind == "silent":
                    # four of the eight keys per chain, plus the chain's four other keys (quiet: each P <= 2^2)
                    assert 4 * 2.0 ** G.B_LO <= lane <= 4 * 2.0 ** G.B_HI + 16 < 0.95 * GUARD_T and G.B_LO <= top <= G.B_HI, f"{name}: chain sum {lane:.1f}, top {top:.2f}"
                    assert not bool(tr["guard"][h, w]) and bool(to["guard"][h, w]) and not bool(tr["exact"][h, w])
                else:
                    lo, hi = (G.D_MIN, 1e9) if inp.seed[1] == "inf" else (G.C_LO, G.C_HI)
                    assert lo <= top <= hi, f"{name}: tile {t} head {h}: top {top:.2f} outside [{lo}, {hi}]"
                    assert bool(tr["guard"][h, w]) and bool(tr["exact"][h, w])
    return new
