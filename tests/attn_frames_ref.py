"""float64 restatement of x2v_attn_frames_fwd_bf16's arithmetic (include/x2v.h, steps 1-6), seeded inputs and the acceptance rule of
tests/test_gpu_attn_frames.py.  Plain PyTorch on the CPU; nothing here imports the library.

Per frame the kernel IS dense attention of the frame's rows over the frame's Kf keys in the rounding model tests/attn_ref.py documents (fp32 base-2
scores, P rounded to bf16 for the PV product only, fp32 row sum of the unrounded exponentials, one rounding of O), with the global row maximum — its
'global' emulation.  So the reference is attn_ref.ref64 per frame and the bar is attn_ref.Case.check unchanged: per element 2^-7 |o| + 1.05 2^-8 A,
and relL2 <= 1.5 Y with Y from attn_ref's emulations of a correct kernel on the same frame.  Nothing is tuned against the kernel's output.

Inputs: frame t's V rows carry the offset 4 (t + 1) and its K rows the direction 0.5 d_t (d_t a +-1 vector of the frame's own), so an output row
computed from another frame's keys is wrong by ~4 against a bar of ~0.05 (`shift` builds that wrong reference for the host-side check)."""
import torch

from tests import attn_ref as A

D = A.D


class FrameInputs:
    """q [H, n_frames * rpf, 128]; k, v [H, n_frames, Kf, 128]; bf16 on the CPU."""

    def __init__(self, H, Kf, n_frames, rpf):
        g = torch.Generator().manual_seed(7 + 100000 * H + 1000 * Kf + rpf)
        self.H, self.Kf, self.n_frames, self.rpf = H, Kf, n_frames, rpf
        t = torch.arange(n_frames, dtype=torch.float32).view(1, n_frames, 1, 1)
        d = (torch.randint(0, 2, (1, n_frames, 1, D), generator=g) * 2 - 1).float()
        self.q = torch.randn(H, n_frames * rpf, D, generator=g).to(A.BF16)
        self.k = (torch.randn(H, n_frames, Kf, D, generator=g) + 0.5 * d).to(A.BF16)
        self.v = (torch.randn(H, n_frames, Kf, D, generator=g) + 4.0 * (t + 1)).to(A.BF16)
        self.name = f"frames H={H} Kf={Kf} rpf={rpf}"

    def exact(self):
        return None

    def q_for(self, prescaled):
        return A.prescale_q(self.q) if prescaled else self.q


class Expect:
    """Reference side of global rows [row0, row0 + Sq) in attn_ref.Expect's shape (o, A, Y, y, tol()); shift: every row attends frame
    (t + shift) % n_frames instead of its own — a wrong kernel."""

    def __init__(self, inp, row0, Sq, prescaled, shift=0):
        self.inp = inp
        q = inp.q_for(prescaled)[:, row0 : row0 + Sq]
        frame = (row0 + torch.arange(Sq)) // inp.rpf
        kw = dict(prescaled=prescaled, q_rounded=not prescaled)
        self.o, self.A = torch.empty(inp.H, Sq, D, dtype=A.F64), torch.empty(inp.H, Sq, D, dtype=A.F64)
        emu = {kind: torch.empty(inp.H, Sq, D, dtype=A.BF16) for kind in A.EMULATIONS}
        for t in frame.unique().tolist():
            rows, kt, vt = frame == t, inp.k[:, (t + shift) % inp.n_frames], inp.v[:, (t + shift) % inp.n_frames]
            self.o[:, rows], self.A[:, rows] = A.ref64(q[:, rows], kt, vt, **kw)
            s32 = A.scores(q[:, rows], kt, dtype=A.F32, **kw)
            for kind in A.EMULATIONS:
                emu[kind][:, rows] = A.emulate(s32, vt.to(A.F32), kind)
        self.y = {kind: A.rel_l2(e, self.o) for kind, e in emu.items()}
        self.Y = max(self.y.values())
        self.emulated = emu

    def tol(self):
        return A.ULP * self.o.abs() + A.P_ROUND * self.A


def ranges(rpf, n_frames=3):
    """(row0, Sq): whole frames from 0; a start mid-frame with a partial last frame; a range inside one frame; a single row (a frame's last)."""
    return [(0, n_frames * rpf), (rpf // 2 + 3, rpf + rpf // 3), (rpf + 5, min(rpf - 7, 21)), (2 * rpf - 1, 1)]
