"""One row of a model YAML as the module class it names sees it (``HipModule.yaml_row``), and the helpers the row hooks share.

``parse_model`` (nn/tasks.py) keeps what is true of every row; what a row means for one class -- its constructor arguments, its
output width, its down-sampling -- is that class's ``yaml_row``.  Nothing here imports a module class."""
from __future__ import annotations

import math
from typing import Callable, NamedTuple


def make_divisible(x, divisor=8):
    return int(math.ceil(x / divisor) * divisor)


class Row(NamedTuple):
    """What ``parse_model`` knows when it reaches a row."""
    i: int             # layer index
    name: str          # the YAML's module name
    fl: list           # from-list (``f`` as a list)
    n: int             # repeat count after depth scaling
    args: list         # the row's args, 'nc' and 'None' substituted
    nc: int
    chs: list          # width of every input, in ``fl`` order
    down: list         # down-sampling of every input against the image, in ``fl`` order
    scaled: Callable   # scaled(c, capped=True) = make_divisible(min(c, max_channels) * width, 8); capped=False leaves the min out
    yaml: dict         # the model YAML itself

    @property
    def layer(self):
        return f"layer {self.i} ({self.name})"


def conv_row(cls, row, check=None, stride=1, stride_arg=False):
    """The ``(c1, c2, ...)`` rows (reference tasks.py:825-864): c1 is the input's width, c2 the row's first argument, scaled unless it
    is ``nc``.  ``check(row, c1, c2, args)`` is the class's own refusal, raised with the layer named; ``cls.repeat_is_arg`` inserts the
    repeat count as the third argument (reference :874-875).  The stride is ``args[3]`` where ``stride_arg`` says so and the row has one,
    else ``stride``."""
    c1, c2 = row.chs[0], row.args[0]
    if c2 == row.nc and row.nc % 8 and not cls.ragged_out:
        raise NotImplementedError(f"{row.layer} would be {row.nc} channels wide: only a Conv can produce a width that is not a multiple of 8")
    if c2 != row.nc:
        c2 = row.scaled(c2)
    args = [c1, c2, *row.args[1:]]
    if check is not None:
        check(row, c1, c2, args)
    if cls.repeat_is_arg:
        args.insert(2, row.n)
    s = args[3] if stride_arg and len(args) > 3 else stride
    return args, c2, row.down[0] * s


def same_width_row(row, args, scale=1):
    """The rows whose output is as wide as their input (reference tasks.py:965-970) on a map ``scale`` times as large."""
    return args, row.chs[0], row.down[0] / scale


def hidden_width_check(row, hidden, halved):
    """C2f and SPPF: their hidden widths (C2f: the chunk of cv1's output, SPPF: the pooled slices) are 8-channel granules too."""
    if row.i > 0 and hidden % 8:
        raise NotImplementedError(f"{row.layer} has a hidden width of {hidden} channels ({halved} halved): not a multiple of 8")
