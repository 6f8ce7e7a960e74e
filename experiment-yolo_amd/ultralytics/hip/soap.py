"""SOAP -- "Shampoo with Adam in the preconditioner's eigenbasis" (arXiv 2409.11321) -- as the reference trainer ships it
(engine/trainer.py:54-473) and builds it (``SOAP(g[2], lr=lr, betas=(momentum, 0.95), weight_decay=0.0)`` + the two other
parameter groups, :1156-1165): betas (momentum, 0.95), eps 1e-8, preconditioner refreshed every 10 steps, 1-D tensors (biases,
norm weights) run plain Adam, decoupled weight decay applied after the step, bias correction on, first call only seeds the
preconditioner.  Options the reference never switches on (merge_dims, precondition_1d, normalize_grads, channels_last) are not
carried.

Two implementations live here.  ``Soap`` is the restatement pinned to the reference's class on the CPU (tests/test_host_logic.py):
host-driven torch ops over views of the flat parameter / gradient buffers, about 35 ATen launches per tensor and step.  It is what
``DY_SOAP_HIP=0`` selects.  ``SoapHip`` is the same step, operation for operation, as grouped HIP kernels (csrc/soap.hip): the state
sits in pools, a descriptor table (``SoapTable`` -> ``DySoapDesc``) names every trainable tensor, and one launch serves all tensors of
the model for each kind of work -- about two dozen launches per step whatever the model.  Only the eigendecomposition of the first
call and the QR of every tenth step stay ``torch.linalg`` in float64 (``_basis_eigh`` says why), batched per matrix size.  DESIGN.md
section 18."""
from __future__ import annotations

import torch


class _State:
    __slots__ = ("step", "m", "v", "gg", "q")

    def __init__(self, g):
        self.step = 0
        self.m, self.v = torch.zeros_like(g), torch.zeros_like(g)
        # one Gram accumulator per dimension of a >= 2-D tensor; None = that dimension is left alone
        self.gg = [None] if g.dim() == 1 else [torch.zeros(n, n, device=g.device, dtype=g.dtype) for n in g.shape]
        self.q = None


def _rotate(t, bases, back):
    """Contract every dimension of ``t`` with its basis (or cycle it unchanged when it has none): after len(bases) contractions the
    dimensions are back in their original order.  Forward uses Q, back uses Q^T (reference project / project_back)."""
    for q in bases:
        if q is None:
            t = t.permute(*range(1, t.dim()), 0)
        else:
            t = torch.tensordot(t, q, dims=[[0], [1 if back else 0]])
    return t


def _gram_update(st, g, beta):
    if g.dim() == 1:
        return
    for k, acc in enumerate(st.gg):
        others = [d for d in range(g.dim()) if d != k]
        acc.lerp_(torch.tensordot(g, g, dims=[others, others]), 1 - beta)


def _basis_eigh(st):
    out = []
    for acc in st.gg:
        if acc is None:
            out.append(None)
            continue
        eye = 1e-30 * torch.eye(acc.shape[0], device=acc.device, dtype=acc.dtype)
        q = None
        if not acc.is_cuda:  # the reference's path: float32, float64 only when LAPACK gives up
            try:
                _, q = torch.linalg.eigh(acc + eye)
            except Exception:
                q = None
        if q is None:
            # On the GPU the float32 eigensolver returned bases that were not orthogonal for the rank-deficient Gram matrices of
            # the small detection-head layers (Q^T Q off by O(1)): projecting and projecting back then no longer cancel and the
            # layer's weights grew 10x per step.  float64 there -- these matrices are at most a few hundred wide.
            _, q = torch.linalg.eigh(acc.double() + eye.double())
            q = q.to(acc.dtype)
        out.append(torch.flip(q, [1]))  # descending eigenvalues
    return out


def _basis_qr(st):
    """One power iteration + QR per dimension; the second-moment estimate follows the re-sorted eigen directions."""
    out, v = [], st.v
    for k, (acc, q) in enumerate(zip(st.gg, st.q)):
        if acc is None:
            out.append(None)
            continue
        est = torch.diag(q.T @ acc @ q)
        order = torch.argsort(est, descending=True)
        v = v.index_select(k, order)
        if acc.is_cuda:
            q2, _ = torch.linalg.qr((acc @ q[:, order]).double())
            q2 = q2.to(acc.dtype)
        else:
            q2, _ = torch.linalg.qr(acc @ q[:, order])
        out.append(q2)
    st.v = v
    return out


def _refresh(st, g, beta, every):
    """reference update_preconditioner: momentum leaves the old basis, Gram matrices take the new gradient, the basis is created
    (eigh) or refreshed (QR every ``every`` steps), momentum enters the current basis again."""
    if st.q is not None:
        st.m = _rotate(st.m, st.q, back=True)
    _gram_update(st, g, beta)
    if st.q is None:
        st.q = _basis_eigh(st)
    if st.step > 0 and st.step % every == 0:
        st.q = _basis_qr(st)
    if st.step > 0:
        st.m = _rotate(st.m, st.q, back=False)


class Soap:
    """``params``: list of (tensor view, group index); ``step(grads, lr[3], weight_decay[3])`` updates the views in place."""

    def __init__(self, params, beta1=0.9, beta2=0.95, eps=1e-8, every=10, max_precond_dim=10000):
        self.params, self.beta1, self.beta2, self.eps, self.every = list(params), beta1, beta2, eps, every
        self.max_precond_dim = max_precond_dim
        self.state = {}

    @torch.no_grad()
    def step(self, grads, lr, weight_decay):
        for i, ((p, grp), g) in enumerate(zip(self.params, grads)):
            st = self.state.get(i)
            if st is None:
                st = self.state[i] = _State(g)
                st.gg = [a if (a is None or a.shape[0] <= self.max_precond_dim) else None for a in st.gg]
                _refresh(st, g, self.beta2, self.every)
                continue  # the first call only seeds the preconditioner: the current gradient never meets its own projection
            gp = _rotate(g, st.q, back=False)
            st.step += 1
            st.m.mul_(self.beta1).add_(gp, alpha=1 - self.beta1)
            st.v.mul_(self.beta2).add_(gp.square(), alpha=1 - self.beta2)
            size = lr[grp] * (1 - self.beta2 ** st.step) ** 0.5 / (1 - self.beta1 ** st.step)
            upd = _rotate(st.m / (st.v.sqrt() + self.eps), st.q, back=True)
            p.add_(upd, alpha=-size)
            if weight_decay[grp] > 0.0:
                p.add_(p, alpha=-lr[grp] * weight_decay[grp])
            _refresh(st, g, self.beta2, self.every)


# ---- the same step as grouped HIP kernels (csrc/soap.hip) --------------------------------------------------------------------------
SOAP_MAX_DIMS = 5  # include/dealyolo_hip.h DY_SOAP_MAX_DIMS (the ScalSeq conv3d weight has five dimensions)
_TILE, _EW = 32, 1024  # csrc/soap.hip SOAP_T, SOAP_EW


def _cdiv(a, b):
    return -(-a // b)


class SoapTable:
    """Where every trainable tensor's SOAP state lives, and which workgroups of each launch are its own: pure host arithmetic over
    ``views`` = [(name, flat offset, numel, shape, optimizer group)], the list ``StepPlan._soap_make`` builds.

    ``entries[i]``: dict(off, numel, group, ndim, shape, geom = [(A, n, B) per dimension], has_q, pool_off, ord_off, rot_blk, gram_blk,
    ew_blk).  Gram matrices (and, at the same offsets, eigenbases) are pooled by size: ``sizes`` = [(n, first float, count, first int of
    the order pool)] in ascending n, the count_n matrices of one size being one contiguous (count_n, n, n) tensor."""

    def __init__(self, views, max_precond_dim=10000):
        self.views = list(views)
        self.max_precond_dim = max_precond_dim
        ents, by_n = [], {}
        for name, off, numel, shape, group in self.views:
            shape = tuple(int(s) for s in shape)
            nd = len(shape)
            if not 1 <= nd <= SOAP_MAX_DIMS:
                raise ValueError(f"SOAP: '{name}' has {nd} dimensions, the descriptor table holds 1..{SOAP_MAX_DIMS}")
            k = 1
            for s in shape:
                k *= s
            if k != numel or numel <= 0 or numel >= 2 ** 31:
                raise ValueError(f"SOAP: '{name}': shape {shape} does not hold {numel} elements (or more than 2^31 - 1)")
            geom, a = [], 1
            for d, n in enumerate(shape):
                geom.append((a, n, numel // (a * n)))
                a *= n
            has_q = [int(nd > 1 and n <= max_precond_dim) for n in shape]
            for d, n in enumerate(shape):
                if has_q[d]:
                    by_n.setdefault(n, []).append((len(ents), d))
            ents.append(dict(name=name, off=int(off), numel=int(numel), group=int(group), ndim=nd, shape=shape, geom=geom, has_q=has_q,
                             pool_off=[0] * nd, ord_off=[0] * nd))
        self.sizes, pool, opool = [], 0, 0
        for n in sorted(by_n):
            self.sizes.append((n, pool, len(by_n[n]), opool))
            for i, d in by_n[n]:
                ents[i]["pool_off"][d], ents[i]["ord_off"][d] = pool, opool
                pool += n * n
                opool += n
        self.n_gram, self.gram_floats, self.order_ints = sum(c for _, _, c, _ in self.sizes), pool, opool
        # first workgroup of every entry in each launch
        rot, gram, ew = [0] * SOAP_MAX_DIMS, 0, 0
        for e in ents:
            e["rot_blk"], e["gram_blk"], e["ew_blk"] = list(rot), [], ew
            ew += _cdiv(e["numel"], _EW)
            for d in range(SOAP_MAX_DIMS):
                if d < e["ndim"] and e["has_q"][d]:
                    _a, n, _b = e["geom"][d]
                    rot[d] += _cdiv(n, _TILE) * _cdiv(e["numel"] // n, _TILE)
                    e["gram_blk"].append(gram)
                    gram += 1 if n <= 8 else _cdiv(n, _TILE) ** 2
                else:
                    rot[d] += _cdiv(e["numel"], _EW)
                    e["gram_blk"].append(gram)
        self.entries, self.rot_blocks, self.gram_blocks, self.ew_blocks = ents, rot, gram, ew
        self.passes = max(2, max((e["ndim"] for e in ents), default=1))  # (two at least: a chain that ends where it began needs a stop between)
        if max(rot + [gram, ew]) >= 2 ** 31:
            raise ValueError("SOAP: more workgroups than a launch holds")

    def descriptors(self):
        """The table as the library reads it: a ctypes array of DySoapDesc."""
        from . import DySoapDesc
        arr = (DySoapDesc * len(self.entries))()
        for t, e in zip(arr, self.entries):
            t.off, t.numel, t.group, t.ndim, t.ew_blk = e["off"], e["numel"], e["group"], e["ndim"], e["ew_blk"]
            for d in range(SOAP_MAX_DIMS):
                live = d < e["ndim"]
                t.shape[d] = e["shape"][d] if live else 1
                t.has_q[d] = e["has_q"][d] if live else 0
                t.pool_off[d] = e["pool_off"][d] if live else 0
                t.ord_off[d] = e["ord_off"][d] if live else 0
                t.rot_blk[d], t.gram_blk[d] = e["rot_blk"][d], e["gram_blk"][d]
        return arr


class _PoolState:
    """What ``Soap.state[i]`` is to its readers (``StepPlan.soap_state``, the tests): ``m``, ``v``, ``gg[k]``, ``q[k]`` are views into
    the pools of the ``SoapHip`` that owns them, ``step`` is its Python step count."""
    __slots__ = ("_o", "m", "v", "gg", "_q")

    def __init__(self, owner, e):
        o, k, sh = e["off"], e["numel"], e["shape"]
        self._o = owner
        self.m, self.v = owner.m[o:o + k].view(sh), owner.v[o:o + k].view(sh)
        pick = lambda pool: [pool[p:p + n * n].view(n, n) if h else None for p, n, h in zip(e["pool_off"], sh, e["has_q"])]  # noqa: E731
        self.gg, self._q = pick(owner.gram), pick(owner.basis)

    @property
    def step(self):
        return self._o.t

    @property
    def q(self):
        return self._q if self._o.seeded else None


class SoapHip:
    """``Soap`` on the device: ``step(grads)`` runs one optimizer step over the flat buffers from the FLAT gradient tensor (unscaled and
    clipped inside the kernels), in ``Soap.step``'s order: rotate g -> moments -> rotate the update back -> apply -> rotate m back ->
    Gram -> (refresh) -> rotate m forward; the first call only seeds (Gram from zero, eigh).  One 4-byte read-back per step (found_inf:
    a skipped step must not advance ``t``, which the refresh schedule and the checkpoint need); ``launches`` counts the kernels issued."""

    def __init__(self, views, flat_p, hyper, state, partials, beta1=0.9, beta2=0.95, eps=1e-8, every=10, max_precond_dim=10000, grouped=()):
        from . import lib
        self.L = lib()
        self.beta1, self.beta2, self.eps, self.every = beta1, beta2, eps, every
        self.p, self.hyper, self.dev_state, self.partials = flat_p, hyper, state, partials
        dev, n = flat_p.device, flat_p.numel()
        self.n = n
        self.table = tb = SoapTable(views, max_precond_dim)
        for e in tb.entries:
            sh = e["shape"]
            if e["name"] in grouped:  # ``grouped``: names of the weights of grouped (depthwise) convolutions, (C, 1, k, k)
                raise NotImplementedError(f"SOAP: '{e['name']}' is a depthwise convolution weight {sh} = (C, 1, k, k); the grouped HIP step has not "
                                          f"been verified on such a tensor: train this graph with SGD / Adam* / RMSProp")
            if e["off"] < 0 or e["off"] + e["numel"] > n:
                raise ValueError(f"SOAP: '{e['name']}' lies outside the flat parameter buffer")
        f = lambda k, dt=torch.float32: torch.zeros(max(k, 1), dtype=dt, device=dev)  # noqa: E731
        self.m, self.v, self.sa, self.sb = f(n), f(n), f(n), f(n)
        self.gram, self.basis, self.order = f(tb.gram_floats), f(tb.gram_floats), f(tb.order_ints, torch.int32)
        self.desc = torch.frombuffer(bytearray(bytes(tb.descriptors())), dtype=torch.uint8).to(dev)
        self.nt = len(tb.entries)
        self.t, self.seeded, self.launches = 0, False, 0
        self.state = {}       # filled once there is state to show, as Soap's is

    # ---- launches ----------------------------------------------------------------------------------------------------------------
    def _s(self):
        return torch.cuda.current_stream(self.p.device).cuda_stream

    def _call(self, name, kernels, *args):
        from . import check
        check(getattr(self.L, name)(*args, self._s()), name)
        self.launches += kernels

    def _chain(self, one, src, last=None):
        """``one(dst, src, k)`` for k = 0 .. passes - 1 through the two scratch buffers; the last pass writes ``last`` if given."""
        cur, P = src, self.table.passes
        for k in range(P):
            dst = last if (last is not None and k == P - 1) else (self.sb if cur is self.sa else self.sa)
            one(dst, cur, k)
            cur = dst
        return cur

    def _rotate(self, src, back, scaled=False, last=None):
        tb, st = self.table, self.dev_state.data_ptr()
        return self._chain(lambda d, s, k: self._call("dy_soap_rotate", 1, d.data_ptr(), s.data_ptr(), self.desc.data_ptr(), self.nt, tb.rot_blocks[k],
                                                      self.basis.data_ptr(), k, int(back), int(scaled and k == 0), st), src, last)

    def _gram(self, grads):
        self._call("dy_soap_gram", 1 if self.table.gram_blocks else 0, self.gram.data_ptr(), grads.data_ptr(), self.desc.data_ptr(), self.nt,
                   self.table.gram_blocks, 1.0 - self.beta2, self.dev_state.data_ptr())

    # ---- the refresh: torch.linalg in float64, one call per matrix size ----------------------------------------------------------
    def _pools(self):
        for n, p, c, o in self.table.sizes:
            yield n, self.gram[p:p + c * n * n].view(c, n, n), self.basis[p:p + c * n * n].view(c, n, n), self.order[o:o + c * n].view(c, n)

    def _seed_bases(self):
        for n, gg, q, _ in self._pools():
            eye = 1e-30 * torch.eye(n, device=gg.device, dtype=torch.float64)
            _, vec = torch.linalg.eigh(gg.double() + eye)  # float64: see _basis_eigh
            q.copy_(torch.flip(vec, [2]).to(q.dtype))      # descending eigenvalues

    def _refresh_bases(self):
        for n, gg, q, order in self._pools():
            est = torch.diagonal(q.transpose(1, 2) @ gg @ q, dim1=1, dim2=2)
            # (stable, where Soap._basis_qr takes torch's default sort: tied estimates -- the 1 x 1 matrices, directions that are exactly
            # zero -- may come out in another order there; a permutation among equal estimates changes nothing the step can see)
            idx = torch.argsort(est, dim=1, descending=True, stable=True)
            order.copy_(idx)
            mat = (gg @ torch.gather(q, 2, idx[:, None, :].expand_as(q))).double()
            q2, _ = torch.linalg.qr(mat)  # (84 ms for DEAL-YOLO-N against 121 matrix by matrix, the same bits: profiles/r19_soap.md)
            q.copy_(q2.to(q.dtype))
        tb, st = self.table, self.dev_state.data_ptr()
        self._chain(lambda d, s, k: self._call("dy_soap_permute_v", 1, d.data_ptr(), s.data_ptr(), self.desc.data_ptr(), self.nt, tb.ew_blocks,
                                               self.order.data_ptr(), k, st), self.v, last=self.v)

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, grads, lr, weight_decay):
        """``grads``: the flat fp32 gradient tensor in the parameter layout (loss-scaled, unclipped).  Returns False for a skipped step."""
        import ctypes as C
        if grads.numel() < self.n or grads.dtype != torch.float32 or not grads.is_contiguous():
            raise ValueError("SOAP: the gradient is not a flat fp32 tensor in the parameter layout")
        tb, st, desc = self.table, self.dev_state.data_ptr(), self.desc.data_ptr()
        self._call("dy_grad_norm", 2, grads.data_ptr(), self.n, self.hyper.data_ptr(), st, self.partials.data_ptr())
        if float(self.dev_state[2]) != 0.0:  # the step's one read-back: a skipped step advances nothing
            return False
        if not self.seeded:
            self._gram(grads)
            self._seed_bases()
            self.seeded = True
            self.state = {i: _PoolState(self, e) for i, e in enumerate(tb.entries)}
            return True
        self.t += 1
        t = self.t
        gp = self._rotate(grads, back=False, scaled=True)
        self._call("dy_soap_adam", 1, self.m.data_ptr(), self.v.data_ptr(), gp.data_ptr(), gp.data_ptr(), desc, self.nt, tb.ew_blocks, self.beta1,
                   1.0 - self.beta1, self.beta2, 1.0 - self.beta2, self.eps, st)
        upd = self._rotate(gp, back=True)
        size = (C.c_float * 3)(*[lr[g] * (1 - self.beta2 ** t) ** 0.5 / (1 - self.beta1 ** t) for g in range(3)])
        decay = (C.c_float * 3)(*[lr[g] * weight_decay[g] if weight_decay[g] > 0.0 else 0.0 for g in range(3)])
        self._call("dy_soap_apply", 1, self.p.data_ptr(), upd.data_ptr(), desc, self.nt, tb.ew_blocks, size, decay, st)
        self._rotate(self.m, back=True, last=self.m)
        self._gram(grads)
        if t % self.every == 0:
            self._refresh_bases()
        self._rotate(self.m, back=False, last=self.m)
        return True

    # ---- checkpoints: the per-tensor dictionary Soap's state gives ---------------------------------------------------------------
    def load(self, saved):
        """Take the state of the tensors ``saved`` names, {table index: dict(step, m, v, gg, q)} as ``StepPlan.soap_state`` writes it
        under either implementation, into the pools."""
        if not saved:
            return
        at = {(int(d["step"]), d["q"] is not None) for d in saved.values()}
        if len(at) != 1:
            raise ValueError("SOAP: the saved tensors are at different steps; the grouped step keeps one count for all of them")
        if len(saved) != len(self.table.entries):
            raise ValueError(f"SOAP: the saved state names {len(saved)} of this run's {len(self.table.entries)} trainable tensors; the grouped "
                             "step keeps one step count and one basis pool for all of them (was the run saved under another freeze=?)")
        (self.t, self.seeded), = at
        for i, d in saved.items():
            e = self.table.entries[i]
            s = self.state.setdefault(i, _PoolState(self, e))
            has = [bool(h) for h in e["has_q"]]
            if [t is not None for t in d["gg"]] != has or (d["q"] is not None and [t is not None for t in d["q"]] != has):
                raise ValueError(f"SOAP: the saved state of '{e['name']}' keeps other dimensions preconditioned than this run does")
            s.m.copy_(d["m"])
            s.v.copy_(d["v"])
            for dst, src in zip(s.gg + s._q, list(d["gg"]) + list(d["q"] or [None] * len(has))):
                if dst is not None and src is not None:
                    dst.copy_(src)
