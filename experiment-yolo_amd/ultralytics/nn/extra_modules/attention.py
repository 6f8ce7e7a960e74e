"""Attention blocks on the HIP path: SimAM, the parameter-free attention (drop-in for reference
nn/extra_modules/attention.py:53-77)."""
from __future__ import annotations

import torch.nn as nn

from ...hip.runtime import HipModule
from ..rows import same_width_row

__all__ = ("SimAM",)


class SimAM(HipModule):
    """``x * sigmoid(d^2 / (4 (sum(d^2) / n + e_lambda)) + 0.5)`` with ``d = x - mean(x)`` and ``n = H W - 1``, the mean and the sum
    taken per image and channel over the plane (reference :69-77; csrc/simam.hip).  No parameters, no buffers, no ``state_dict``
    keys; constructor signature, attribute names (``activaton`` as the reference spells it, ``e_lambda``), ``__repr__`` and
    ``get_module_name`` are the reference's, so its pickles rebuild.  A 1x1 map has ``n = 0``: the output is NaN (0 / 0), here as
    there."""
    # (concat_dst stays False although ``forward_act`` takes ``out``: that is how the Concat plan was before the attribute, not a decision)

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:969-970; YAML 1.1 reads ``1e-4`` as a string, the reference evals it (:817)
        return same_width_row(row, [float(a) if isinstance(a, str) else a for a in row.args])

    def __init__(self, e_lambda=1e-4):
        super().__init__()
        self.activaton = nn.Sigmoid()
        self.e_lambda = e_lambda

    def __repr__(self):
        s = self.__class__.__name__ + '('
        s += ('lambda=%f)' % self.e_lambda)
        return s

    @staticmethod
    def get_module_name():
        return "simam"

    def forward_act(self, x, out=None):
        return self.rt.eng.simam(x, float(self.e_lambda), out, name=f"SimAM (layer {getattr(self, 'i', '?')})")
