"""Glue between the nn.Module tree (parameter holders with the reference's names) and the HIP engine.

``Runtime.materialize(root)`` moves every parameter of ``root`` into ONE flat fp32 device buffer laid out as
[bias group | decayed weights | norm weights] (the optimizer groups of reference engine/trainer.py:1146-1154), points
``param.data`` / ``param.grad`` at views of it, flattens the floating-point buffers (BN running statistics) likewise,
and builds a ConvSpec per convolution.  Flat storage is what makes the single-launch optimizer/EMA and the single-bucket
RCCL all-reduce possible.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import DY_ACT_NONE, DY_ACT_SILU
from .engine import BN2D_EPS, BN2D_MOM, BN3D_EPS, BN3D_MOM, Act, ConvSpec, Engine, Storage

PAD = 8  # every tensor starts at a multiple of 8 floats inside the flat buffers


def _round(n):
    return (n + PAD - 1) // PAD * PAD


class Runtime:
    def __init__(self, root: nn.Module, device):
        self.root = root
        self.eng = Engine(device)
        self.specs = {}
        # Parameters no forward reads (``HipModule.unused_modules``: VoVGSCSP's ``res``, which the reference constructs and never
        # calls).  The set is static -- it follows from the module classes, not from a flag -- so launch-list keys and
        # StepPlan._check_flags never see it.  Such a module builds no ConvSpec; its parameters keep ``requires_grad`` (as in the
        # reference, where their ``.grad`` simply stays None) but are masked like frozen ones: gradient views at the sink, their
        # slice of the flat gradient exactly zero, no optimizer update, no weight decay, no share in the clip norm (``_flatten`` finds them).
        self._flatten()
        for m in root.modules():
            if isinstance(m, HipModule) and id(m) not in self.unused_mods:
                m._build_specs(self)
        self._pack_sig = None
        self.refresh_frozen()  # parameters already frozen at construction: their gradients go to the sink from the start

    # ---- flat parameter / buffer storage -------------------------------------------------------------------------
    def _flatten(self):
        dev = self.eng.device
        root = self.root
        self.unused_mods = {id(s) for m in root.modules() if isinstance(m, HipModule) for u in m.unused_modules() for s in u.modules()}
        self.unused_params = {id(p) for m in root.modules() if id(m) in self.unused_mods for p in m.parameters(recurse=False)}
        norm_types = tuple(v for k, v in nn.__dict__.items() if "Norm" in k and isinstance(v, type))
        groups = ([], [], [])  # bias, decayed weights, norm weights  (reference build_optimizer order g[2], g[0], g[1])
        seen = set()
        for mname, mod in self.root.named_modules():
            for pname, p in mod.named_parameters(recurse=False):
                if id(p) in seen:
                    continue
                seen.add(id(p))
                full = f"{mname}.{pname}" if mname else pname
                gi = 0 if "bias" in full else (2 if isinstance(mod, norm_types) else 1)
                groups[gi].append((full, p))
        # Six segments [neck + head: bias | decayed | norm][backbone: bias | decayed | norm]: the parameters whose gradients are final
        # FIRST in the backward pass (everything behind the YAML's backbone) sit in front, so each data-parallel gradient bucket is one
        # contiguous slice of the flat gradient buffer that RCCL reduces in place (StepPlan, DY_DP_BUCKETS=2; DDP's reducer works on
        # contiguous buckets too, reference engine/trainer.py:694-695).  A root without a backbone / head split has empty first segments.
        nb = len(self.root.yaml.get("backbone", [])) if isinstance(getattr(self.root, "yaml", None), dict) else None

        def late(name):
            parts = name.split(".")
            return nb is not None and len(parts) > 1 and parts[0] == "model" and parts[1].isdigit() and int(parts[1]) >= nb

        segs = [[(n, p) for n, p in g if late(n)] for g in groups] + [[(n, p) for n, p in g if not late(n)] for g in groups]
        self.param_names = [n for g in segs for n, _ in g]
        self.param_group = {n: k % 3 for k, g in enumerate(segs) for n, _ in g}  # optimizer group of every parameter
        offs, total, bounds = {}, 0, []
        for g in segs:
            for n, p in g:
                offs[n] = total
                total += _round(p.numel())
            bounds.append(total)
        self.n_params_flat, self.seg_bounds = total, bounds[:5]
        self.bucket_split = bounds[2]  # [0, bucket_split): neck + head (the first gradient bucket); the rest: backbone
        groups = segs
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self._n_params_for_gb = total  # flat_g is created with the buffers' staging tail once their size is known (below)
        self.frozen = torch.zeros(total, dtype=torch.uint8, device=dev)
        self.param_off = offs
        # floating-point buffers (running statistics)
        fb = []
        for mname, mod in self.root.named_modules():
            for bname, b in mod.named_buffers(recurse=False):
                if b is not None and b.dtype.is_floating_point:
                    fb.append((mod, bname, b))
        tot = sum(_round(b.numel()) for _, _, b in fb)
        # ONE exchange buffer [gradients | staging copy of the float buffers]: the data-parallel step all-reduces it whole, so the
        # DDP-style "rank 0's BN statistics win" rides on the gradient all-reduce (rank 0 stages its buffers, the others zeros)
        self.flat_gb = torch.zeros(total + max(tot, PAD), dtype=torch.float32, device=dev)
        self.flat_g = self.flat_gb[:total]
        self.gviews = {}
        for g in groups:
            for n, p in g:
                o, k = offs[n], p.numel()
                view = self.flat_p[o:o + k].view(p.shape)
                view.copy_(p.data.to(dev, torch.float32))
                p.data = view
                gv = self.flat_g[o:o + k].view(p.shape)
                p.grad = None if id(p) in self.unused_params else gv  # (None, as in the reference: every torch.optim optimizer skips it)
                self.gviews[id(p)] = gv
                if not self.updates(p):
                    self.frozen[o:o + _round(k)] = 1
                else:
                    self.frozen[o + k:o + _round(k)] = 1  # padding never moves
        self.flat_b = torch.zeros(max(tot, PAD), dtype=torch.float32, device=dev)
        o = 0
        for mod, bname, b in fb:
            k = b.numel()
            view = self.flat_b[o:o + k].view(b.shape)
            view.copy_(b.to(dev, torch.float32))
            mod._buffers[bname] = view
            o += _round(k)
        self.n_buffers_flat = max(tot, PAD)
        names = {id(mod): mname for mname, mod in self.root.named_modules()}
        self.buffer_layout = [(f"{names[id(mod)]}.{bname}" if names[id(mod)] else bname, b.numel()) for mod, bname, b in fb]
        # integer buffers just move
        for mod in self.root.modules():
            for bname, b in list(mod._buffers.items()):
                if b is not None and not b.dtype.is_floating_point:
                    mod._buffers[bname] = b.to(dev)
            if isinstance(mod, HipModule):
                mod.__dict__["rt"] = self

    def layout(self):
        """Where every parameter and float buffer lives in the flat buffers: two runtimes with equal layouts can exchange ``flat_p`` /
        ``flat_b`` wholesale (ModelEMA.eval_model)."""
        return [(n, self.param_off[n]) for n in self.param_names], self.n_params_flat, self.buffer_layout, self.n_buffers_flat

    def refresh_frozen(self):
        """Re-read ``requires_grad`` flags (BaseTrainer freezes '.dfl' and the ``freeze=`` layers after construction, engine/trainer.py:
        662-682).  The optimizer mask follows them, and so does WHERE every ConvSpec's parameter gradients go: a trainable parameter's
        into its view of the flat gradient buffer, a frozen one's into a sink of its own that nothing reads -- the flat gradient of a
        frozen parameter is exactly zero after every backward pass, so it enters neither the clip norm nor an all-reduce.  Launch lists
        record these pointers: a StepPlan traced before a flag changed refuses to run afterwards (StepPlan._check_flags)."""
        flags = tuple(p.requires_grad for _, p in self.root.named_parameters())
        if flags == getattr(self, "_flags", None):
            return
        self._flags = flags
        self.frozen.zero_()
        need, offs = 0, {}
        for n, p in self.root.named_parameters():
            o, k = self.param_off[n], p.numel()
            if not self.updates(p):
                self.frozen[o:o + _round(k)] = 1
                offs[n] = need
                need += _round(k)
            else:
                self.frozen[o + k:o + _round(k)] = 1
        self.flat_g.masked_fill_(self.frozen.bool(), 0.0)
        if need > (self.flat_sink.numel() if self.flat_sink is not None else 0):
            self.flat_sink = torch.zeros(need, dtype=torch.float32, device=self.eng.device)
            self.eng.keep.append(self.flat_sink)  # (launch lists recorded under earlier flags may still name the old one)
        for n, p in self.root.named_parameters():
            o, k = self.param_off[n], p.numel()
            src, o = (self.flat_g, o) if self.updates(p) else (self.flat_sink, offs[n])
            self.gviews[id(p)] = src[o:o + k].view(p.shape)
        for sp in self.specs.values():
            self._bind_grads(sp)

    flat_sink = None

    def updates(self, p):
        """``p`` receives a gradient and an optimizer update: it is trainable and some forward reads it."""
        return p.requires_grad and id(p) not in self.unused_params

    def unused_parameter_names(self):
        """Names (as in ``named_parameters()`` of the root) of the parameters no forward reads, in flat-buffer order."""
        byid = {id(p): n for n, p in self.root.named_parameters()}
        return sorted((byid[i] for i in self.unused_params if i in byid), key=self.param_off.get)

    def _bind_grads(self, sp):
        """Point a ConvSpec's gradient views at where its parameters' gradients go now (``refresh_frozen``); ``sp.trainable``: it owns a
        parameter that has one."""
        prm = sp.params
        g = {k: (None if v is None else self.gviews.get(id(v))) for k, v in prm.items()}
        sp.gweight, sp.gbias = g["weight"], g["bias"]
        if prm.get("bn_w") is not None:
            sp.gbn_w, sp.gbn_b = g["bn_w"], g["bn_b"]
        if prm.get("bn3d_w") is not None:
            sp.gbn3d = (g["bn3d_w"], g["bn3d_b"])
        # (a fused eval model's split convs hand in plain views, not Parameters: they have no gradient and are never trained)
        sp.trainable = any(getattr(v, "requires_grad", False) for v in prm.values())

    # ---- conv specs -----------------------------------------------------------------------------------------------
    def _bn_dict(self, bn):
        return dict(weight=bn.weight.data, bias=bn.bias.data, running_mean=bn.running_mean, running_var=bn.running_var,
                    nbt=bn.num_batches_tracked)

    def make_spec(self, key, conv: nn.Module, bn, act, ks, stride, eps=BN2D_EPS, mom=BN2D_MOM, name="", ld=None):
        sp = self.specs.get(key)
        if sp is not None and sp.weight.data_ptr() == conv.weight.data.data_ptr() and (sp.bn is None) == (bn is None):
            return sp
        w = conv.weight.data
        w2 = w if ld is not None else (w.reshape(w.shape[0], w.shape[1], ks, ks) if w.dim() != 4 or w.shape[2] != ks else w)
        sp = ConvSpec(name, w2, None if conv.bias is None else conv.bias.data, None if bn is None else self._bn_dict(bn), ks,
                      stride, act, eps, mom, groups=int(getattr(conv, "groups", 1)))
        sp.ld = ld
        sp.params = dict(weight=conv.weight, bias=conv.bias, bn_w=None if bn is None else bn.weight, bn_b=None if bn is None else bn.bias)
        self._bind_grads(sp)
        self.eng.prepare_conv(sp)
        self.specs[key] = sp
        sp.packed = False
        return sp

    def spec(self, m):
        """ConvSpec of a ``Conv`` module (fused or not)."""
        return self.specs[id(m)]

    def ldconv(self, m, x, out=None):
        sp_p, sp_c = self.specs[(id(m), "p_conv")], self.specs[(id(m), "conv", x.C)]
        return self.eng.ldconv(sp_p, sp_c, m._pn_i32, m.num_param, m.stride, x, out)

    def pack_all(self, transposed=True):
        """Refresh every MFMA weight pack from the fp32 masters in ONE launch (recorded at the start of each step)."""
        import ctypes as C
        specs = [sp for sp in self.specs.values() if not sp.dw]  # (a depthwise spec has no packs: its kernels read the masters)
        if not specs:
            return
        key = (transposed, tuple(sp.weight.data_ptr() for sp in specs))
        cached = getattr(self, "_pack_tbl", None)
        if cached is None or cached[0] != key:
            L = self.eng.L
            sz = L.dy_pack_desc_bytes()
            n = len(specs) * (2 if transposed else 1)
            host = (C.c_char * (sz * n))()
            blocks, i = 0, 0
            for sp in specs:
                for tr in ((0, 1) if transposed else (0,)):
                    ld = sp.ld or (0, 0, sp.weight.shape[1])
                    nb = L.dy_pack_desc_fill(C.byref(host, i * sz), sp.weight.data_ptr(), 0, (sp.wpack_t if tr else sp.wpack).data_ptr(),
                                             sp.cout, ld[2] if sp.ld else sp.weight.shape[1], sp.ks, sp.stride, tr, ld[0], ld[1], blocks)
                    if nb < 0:
                        raise RuntimeError(f"dy_pack_desc_fill failed for {sp.name}")
                    blocks += nb
                    i += 1
            dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(self.eng.device)
            self.eng.keep.append(dev)
            self._pack_tbl = cached = (key, dev, n, blocks)
        self.eng.call("dy_pack_weights_batched", cached[1].data_ptr(), cached[2], cached[3])

    def ensure_packed(self):
        """Eager (inference) path: re-pack when any master weight changed (torch version counters + explicit marks)."""
        sig = (self._dirty_mark, tuple(sp.weight._version for sp in self.specs.values()))
        if sig != self._pack_sig:
            self.pack_all(transposed=False)
            self._pack_sig = sig

    _dirty_mark = 0

    def mark_dirty(self):
        self._dirty_mark += 1

    # ---- tensor <-> Act ------------------------------------------------------------------------------------------
    def to_act(self, x: torch.Tensor) -> Act:
        """Public-API tensor (N,C,H,W) -> Act.  C not a multiple of 8 (the RGB image) is zero-padded."""
        eng = self.eng
        if x.dim() != 4:
            raise ValueError(f"expected a (N,C,H,W) tensor, got {tuple(x.shape)}")
        x = x.to(eng.device)
        N, Cc, H, W = x.shape
        if Cc % 8:
            return eng.import_image(x.float().contiguous(), (Cc + 7) // 8 * 8)
        st = Storage(eng, N, H, W, Cc)
        st.buf.copy_(x.permute(0, 2, 3, 1))
        return st.act()

    @staticmethod
    def to_tensor(a: Act) -> torch.Tensor:
        """Act -> logical (N,C,H,W) fp16 tensor sharing memory with the NHWC buffer (channels-last strides)."""
        return a.st.buf[..., a.c0:a.c0 + a.C].permute(0, 3, 1, 2)


class HipModule(nn.Module):
    """Base of every hot-path module: ``forward`` accepts public tensors or engine Acts and routes to ``forward_act``."""

    rt: Runtime | None = None
    # what the model graph (nn/tasks.py) asks a module class, instead of keeping lists of classes
    ragged_in = False      # may read a width that is not a multiple of 8 (every other module moves whole 8-channel granules)
    ragged_out = False     # may produce such a width (a ``[nc, ...]`` row: the one width make_divisible does not touch)
    repeat_is_arg = False  # the row's repeat count is a constructor argument: the row builds ONE module
    concat_dst = False     # ``forward_act(x, out)`` can write into a channel slice of a Concat's buffer

    @classmethod
    def yaml_row(cls, row):
        """One model-YAML row (nn/rows.py ``Row``) -> (constructor arguments, output width, down-sampling of the output)."""
        raise NotImplementedError(f"{row.layer}: {cls.__name__} does not say how it reads a model YAML row")

    def _build_specs(self, rt):
        """Register this module's ConvSpecs with the runtime (overridden by modules that own convolutions)."""

    def unused_modules(self):
        """Sub-modules this module constructs and never calls (their parameters are state no forward reads: ``Runtime``)."""
        return ()

    def _runtime(self, device):
        rt = self.__dict__.get("rt")
        if rt is None or rt.eng.device != torch.device(device):
            rt = Runtime(self, device)  # standalone use of a sub-module: it becomes its own root
        return rt

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        for m in self.modules():  # parameters were re-created: flat views are stale
            if isinstance(m, HipModule):
                m.__dict__.pop("rt", None)
        return out

    def forward(self, x, *args, **kwargs):
        first = x[0] if isinstance(x, (list, tuple)) else x
        if isinstance(first, Act):
            return self.forward_act(x, *args, **kwargs)
        dev = first.device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: the HIP hot path runs on the GPU only (got a {dev.type} tensor); "
                               "there is deliberately no CPU fallback")
        rt = self._runtime(dev)
        rt.eng.training = self.training
        xs = [rt.to_act(t) for t in x] if isinstance(x, (list, tuple)) else rt.to_act(x)
        with torch.no_grad():
            rt.ensure_packed()
            y = self.forward_act(xs, *args, **kwargs)
        return self._export(rt, y)

    def _export(self, rt, y):
        from .engine import SegAct, UpAct
        if isinstance(y, (SegAct, UpAct)):
            y = rt.eng.dense(y)
        if isinstance(y, Act):
            return rt.to_tensor(y)
        if isinstance(y, (list, tuple)):
            return type(y)(self._export(rt, t) for t in y)
        return y
