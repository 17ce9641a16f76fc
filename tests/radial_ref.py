"""float64 reference for block-sparse attention (x2v_attn_bsr_fwd_bf16_vt) in tests/attn_ref.py's conventions: head-major bf16 tensors q [H, S, 128],
k / v [H, S, 128], base-2 scores, the q re-rounding of the non-prescaled pre-transposed-V form.  Plain PyTorch on the CPU; nothing here imports the
library.  The mask is bool [ceil(S/128), ceil(S/128)] over 128-row x 128-key blocks: query row i attends key j iff mask[i // 128, j // 128] (and
j < S).  Shared by tests/test_radial_host.py and tests/test_gpu_attn_bsr.py.

pad_keys=True is the reference wrapper's behaviour instead (attentions/common/radial_attn.py:21-31): q / k / v zero-padded to a multiple of 128, so a
row that attends the last key block also attends ceil(S/128) * 128 - S keys of score 0 and value 0.
"""
import numpy as np
import torch

from tests import attn_ref as R

BLOCK = 128
F64, F32, BF16 = R.F64, R.F32, R.BF16


def n_blocks(S):
    return (S + BLOCK - 1) // BLOCK


def as_mask(block_mask, S):
    m = torch.as_tensor(np.asarray(block_mask.cpu() if isinstance(block_mask, torch.Tensor) else block_mask))
    assert m.dtype == torch.bool and tuple(m.shape) == (n_blocks(S), n_blocks(S)), f"mask {tuple(m.shape)} for S={S}"
    return m


def attended_keys(mask_row, S, pad_keys=False):
    """Key indices one block row attends, ascending; with pad_keys the zero keys S .. ceil(S/128)*128 - 1 count as keys of the last block."""
    end = n_blocks(S) * BLOCK if pad_keys else S
    idx = [torch.arange(b * BLOCK, min((b + 1) * BLOCK, end)) for b in torch.nonzero(mask_row).flatten().tolist()]
    return torch.cat(idx) if idx else torch.zeros(0, dtype=torch.int64)


def _rows(r, S):
    return slice(r * BLOCK, min((r + 1) * BLOCK, S))


def _padded(k, v, S, pad_keys):
    if not pad_keys or S % BLOCK == 0:
        return k, v
    z = torch.zeros(k.shape[0], n_blocks(S) * BLOCK - S, k.shape[2], dtype=k.dtype)
    return torch.cat([k, z], 1), torch.cat([v, z], 1)


def masked_ref64(q, k, v, block_mask, scale=0.0, prescaled=False, q_rounded=False, pad_keys=False):
    """Masked softmax attention in float64.  Returns (o, A) as attn_ref.ref64: o [H, S, 128] unrounded, A = sum_j w_j |v_jd| over the attended keys."""
    H, S, _ = q.shape
    m = as_mask(block_mask, S)
    k, v = _padded(k, v, S, pad_keys)
    o, A = torch.zeros(H, S, R.D, dtype=F64), torch.zeros(H, S, R.D, dtype=F64)
    for r in range(m.shape[0]):
        keys = attended_keys(m[r], S, pad_keys)
        assert keys.numel(), f"block row {r} attends nothing"
        o[:, _rows(r, S)], A[:, _rows(r, S)] = R.ref64(q[:, _rows(r, S)], k[:, keys], v[:, keys], scale, prescaled, q_rounded)
    return o, A


class MaskedExpect:
    """attn_ref.Expect for a masked case: o, A from masked_ref64 and Y from attn_ref.emulate run per block row on the attended keys only (gathered in
    ascending order: whole 128-key blocks, so the emulation's 64-key tiles are the kernel's).  Works with attn_ref.Case.check."""

    def __init__(self, inp, form, block_mask, scale=0.0):
        q, kw = inp.q_for(form, scale), R.form_args(form)
        S = inp.Sq
        m = as_mask(block_mask, S)
        self.inp, self.form, self.scale, self.mask = inp, form, scale, m
        self.o, self.A = masked_ref64(q, inp.k, inp.v, m, scale, **kw)
        outs = {kind: torch.zeros(inp.H, S, R.D, dtype=BF16) for kind in R.EMULATIONS}
        v32 = inp.v.to(F32)
        for r in range(m.shape[0]):
            keys = attended_keys(m[r], S)
            s32 = R.scores(q[:, _rows(r, S)], inp.k[:, keys], scale, dtype=F32, **kw)
            for kind in R.EMULATIONS:
                outs[kind][:, _rows(r, S)] = R.emulate(s32, v32[:, keys], kind)
        self.y = {kind: R.rel_l2(e, self.o) for kind, e in outs.items()}
        self.Y = max(self.y.values())

    def tol(self):
        return R.ULP * self.o.abs() + R.P_ROUND * self.A

    def rows(self, rows):
        """The same expectation cut to some query rows (for checks of one block row)."""
        c = object.__new__(MaskedExpect)
        c.__dict__.update(self.__dict__)
        c.o, c.A = self.o[:, rows], self.A[:, rows]
        c.inp = self.inp.take(rows=rows) if isinstance(rows, torch.Tensor) else self.inp
        return c


_EXPECT = {}


def expect(inp, form, block_mask, scale=0.0, tag=None):
    """MaskedExpect computed once per (case, form, mask) in a run."""
    f = "vt" if (form == "pre" and scale <= 0) else form
    m = as_mask(block_mask, inp.Sq)
    key = (inp.family, inp.Sq, inp.H, inp.spike, inp.seed, f, float(scale), tag if tag is not None else m.numpy().tobytes())
    if key not in _EXPECT:
        _EXPECT[key] = MaskedExpect(inp, f, m, scale)
    return _EXPECT[key]


# ------------------------------------------------------------------------------------------------------------------- fixtures
def load_fixtures(path):
    """tests/golden/radial_masks.npz -> [(meta dict, bool [n, n] tensor), ..] (tools/gen_radial_golden.py wrote it from the unmodified reference)."""
    import json

    z = np.load(path)
    meta = json.loads(bytes(z["meta"]).decode())
    out = []
    for i, md in enumerate(meta):
        n = md["n"]
        out.append((md, torch.from_numpy(np.unpackbits(z[f"mask_{i}"])[: n * n].reshape(n, n).astype(bool))))
    return out


def fixture_mask(fixtures, tpf, frames, model_type="wan", decay_factor=1):
    for md, m in fixtures:
        if (md["tokens_per_frame"], md["frames"], md["model_type"], md["decay_factor"]) == (tpf, frames, model_type, decay_factor):
            return m
    raise KeyError((tpf, frames, model_type, decay_factor))


def random_mask(nb, density, seed, diagonal=True):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(nb, nb, generator=g) < density
    if diagonal:
        m |= torch.eye(nb, dtype=torch.bool)
    m[~m.any(1), 0] = True
    return m
