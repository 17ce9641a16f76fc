"""The plumbing the packed-sequence encoder towers share (t5.py, llama.py, clip_text.py): one grow-only workspace, a bounded cache of launch plans
and the loop that runs one (clip.py runs its per-batch plans with the same loop).  A tower says which buffers it needs (`_buffers`) and which
launches make up a pass (`_launches`); what `forward_packed` hands back is its own."""
from collections import OrderedDict

import torch

from . import lib

MAX_PLANS = 16  # launch plans kept per model (least recently used first out)


def run_plan(plan):
    """A plan is a list of (C entry, raw arguments)."""
    for fn, args in plan:
        rc = fn(*args)
        if rc != 0:
            lib._check(rc, fn.__name__)


class PackedTower:
    DTYPE = torch.float16  # of every workspace buffer

    def _init_plumbing(self):
        self._bufs, self._rows, self._plans, self._tokenizer = {}, 0, OrderedDict(), None

    def _buffers(self):
        """name → columns, or (columns, rows) for a buffer that does not follow M."""
        raise NotImplementedError

    def _launches(self, p, M, cu_arr, batch, stream):
        """The pass as a list of (C entry, raw arguments); `p` holds the workspace's pointers by buffer name."""
        raise NotImplementedError

    def _workspace(self, M):
        """Row views [M, ...] of ONE set of buffers, sized to the largest M seen so far (growing it drops the launch plans, which hold its pointers):
        a service encoding prompts of many lengths holds one workspace, not one per length."""
        if M > self._rows:

            def buf(spec):
                cols, rows = spec if isinstance(spec, tuple) else (spec, M)
                return torch.empty((rows, cols), dtype=self.DTYPE, device=self.device)

            self._plans.clear()
            self._bufs = {k: buf(spec) for k, spec in self._buffers().items()}
            self._rows = M
        return {k: v[:M] for k, v in self._bufs.items()}

    def _plan(self, lens, stream):
        """The launches of one pass: pointers, strides, the sequence bounds and the stream are fixed per (lengths, stream)."""
        key = (lens, stream)
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        M = sum(lens)
        p = {k: v.data_ptr() for k, v in self._workspace(M).items()}
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        cu_arr = (lib._i32 * len(cu))(*cu)  # a host array, read at launch time: the plan's attention launches keep it alive
        plan = self._plans[key] = self._launches(p, M, cu_arr, len(lens), stream)
        while len(self._plans) > MAX_PLANS:
            self._plans.popitem(last=False)
        return plan

    def _run_packed(self, lens):
        run_plan(self._plan(tuple(lens), lib._stream()))
        return sum(lens)
