"""float64 restatement of the two entries of csrc/gsconv.hip on the operands the kernels see (NHWC).

forward:  x2 = cat(x1, d) along the channels; y = cat(x2[..., 0::2], x2[..., 1::2]): every even channel, then every odd one.
backward: the inverse interleave: d(x2)[..., 0::2] = dy[..., :c_], d(x2)[..., 1::2] = dy[..., c_:]; dx1 is its first c_ channels, dd the
          rest.
Both are permutations: no arithmetic, so a kernel's stored result EQUALS them.  tests/test_host_slimneck.py ties them to the
reference's reshape / permute form (nn/extra_modules/block.py:902-908) and to autograd."""
import torch


def forward(x1, d):
    """x1, d: (N, H, W, c_) -> y (N, H, W, 2 c_)."""
    x2 = torch.cat([torch.as_tensor(x1), torch.as_tensor(d)], -1)
    return torch.cat([x2[..., 0::2], x2[..., 1::2]], -1)


def backward(dy):
    """dy: (N, H, W, 2 c_) -> (dx1, dd), each (N, H, W, c_)."""
    dy = torch.as_tensor(dy)
    c_ = dy.shape[-1] // 2
    g = torch.empty_like(dy)
    g[..., 0::2], g[..., 1::2] = dy[..., :c_], dy[..., c_:]
    return g[..., :c_].clone(), g[..., c_:].clone()


def reference_form(x2):
    """The reference's own lines (block.py:902-908) on an NCHW tensor."""
    b, n, h, w = x2.size()
    b_n = b * n // 2
    y = x2.reshape(b_n, 2, h * w)
    y = y.permute(1, 0, 2)
    y = y.reshape(2, -1, n // 2, h, w)
    return torch.cat((y[0], y[1]), 1)
