"""Adam on the multi-tensor HIP kernel (torch.optim.Adam semantics of train_gan.py:483-484: eps 1e-8, no weight
decay, parameters whose ``.grad`` is None are skipped and keep their step count)."""
import collections
import ctypes as C

import torch

from . import lib as L
from . import ops


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        # weight_decay / amsgrad are carried (at the only values the path uses) so that state dicts interchange with
        # torch.optim.Adam's: the reference saves and resumes optimizerG.pth / optimizerD.pth (train_gan.py:331-332,492-493)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))
        self._tables = collections.OrderedDict()      # (param ptr, grad ptr)* -> _Table, least recently used first
        self._chunk = None
        self._arenas, self._arena_off = [], 0         # pinned staging; never freed (a captured graph re-reads its slices)
        self._free = {}                               # nbytes -> recycled pinned slices of evicted eager-mode tables

    MAX_TABLES = 8     # eager-mode bound: a new (param, grad) address pattern beyond this evicts the least recently used one

    def _pinned(self, nbytes):
        """slice of a pinned host arena.  Arenas are only ever added (a hipGraph that captured the upload of a table replays
        the copy FROM its pinned slice, so a slice that a capture has seen is never reused or freed), and only outside capture."""
        free = self._free.get(nbytes)
        if free:
            return free.pop()
        if not self._arenas or self._arena_off + nbytes > self._arenas[-1].numel():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HipAdam: pinned staging arena exhausted during graph capture; run a warm-up step first")
            total = sum(p.numel() for g in self.param_groups for p in g["params"])
            nparams = sum(len(g["params"]) for g in self.param_groups)
            per_table = 64 * nparams + 8 * (total // 4096 + nparams) + 256
            self._arenas.append(torch.empty(max(16 * per_table, nbytes), dtype=torch.uint8).pin_memory())
            self._arena_off = 0
        out = self._arenas[-1][self._arena_off: self._arena_off + nbytes]
        self._arena_off += nbytes
        return out

    def _state_for(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros(1, dtype=torch.int32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        return st

    def state_dict(self):
        """torch.optim.Adam's layout: per parameter ``step`` (f32 scalar on the host), ``exp_avg``, ``exp_avg_sq``."""
        sd = super().state_dict()
        sd["state"] = {k: {**st, "step": st["step"].detach().to("cpu", torch.float32).reshape(())} if "step" in st else st
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a ``torch.optim.Adam`` state dict (a reference optimizerG.pth / optimizerD.pth) or our own."""
        for g in state_dict["param_groups"]:
            if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("HipAdam implements Adam without weight decay / amsgrad / maximize (train_gan.py:483-484)")
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = torch.as_tensor(st["step"]).detach().reshape(1).round().to(device=p.device, dtype=torch.int32)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self._tables.clear()          # the tables hold raw pointers into the replaced state tensors

    def _table(self, ps, device):
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for p in ps)
        hit = self._tables.get(key)
        if hit is not None:
            self._tables.move_to_end(key)
            return hit[:4]
        if self._chunk is None:
            self._chunk = L.load().xmc_adam_chunk_elems()
        ents = (L.AdamEntry * len(ps))()
        chunks = []
        for i, p in enumerate(ps):
            st = self._state_for(p)
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous() or not p.is_contiguous():
                raise RuntimeError("HipAdam needs contiguous f32 parameters and gradients")
            ents[i].param, ents[i].grad = p.data_ptr(), g.data_ptr()
            ents[i].m, ents[i].v = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            ents[i].step, ents[i].n = st["step"].data_ptr(), p.numel()
            chunks += [(i, c) for c in range((p.numel() + self._chunk - 1) // self._chunk)]
        # pinned staging (allocated outside capture) + async copies: legal inside hipGraph capture
        raw = bytes(ents)
        chb = torch.tensor(chunks, dtype=torch.int32).numpy().tobytes()
        n0, n1 = (len(raw) + 63) // 64 * 64, (len(chb) + 63) // 64 * 64
        tab_h, ch_h = self._pinned(n0), self._pinned(n1)
        tab_h[: len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        ch_h[: len(chb)].copy_(torch.frombuffer(bytearray(chb), dtype=torch.uint8))
        tab = tab_h.to(device, non_blocking=True)
        ch = ch_h.to(device, non_blocking=True).view(torch.int32)
        capturing = torch.cuda.is_current_stream_capturing()
        self._tables[key] = (tab, ch, len(ps), len(chunks), tab_h, ch_h, capturing)
        # Gradients are re-allocated by every backward; when their addresses move (allocator churn at epoch boundaries,
        # evaluation, checkpointing) a new table is built.  Keep the working set bounded: evict the least recently used table
        # that no graph capture has seen and recycle its pinned slices.
        if len(self._tables) > self.MAX_TABLES and not capturing:
            torch.cuda.current_stream().synchronize()      # rare; the evicted table's upload must be done before its slice is reused
            for k in list(self._tables):
                if len(self._tables) <= self.MAX_TABLES:
                    break
                ent = self._tables[k]
                if k != key and not ent[6]:
                    del self._tables[k]
                    for h in (ent[4], ent[5]):
                        self._free.setdefault(h.numel(), []).append(h)
        return self._tables[key][:4]

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, scaler=None, ema=None):
        """``grad_scale``: factor applied to every gradient element as the kernel reads it; 1.0 is torch.optim.Adam exactly.
        ``scaler`` (an `ops.LossScaler`, the IEEE-half mode): the gradients are those of scale x loss -- they are read times
        1 / scale; if ANY of them (over all parameter groups) is inf / NaN the step is skipped on the device (no parameter,
        moment or step counter changes) and the scale backs off; the scaler's counters say so afterwards.
        ``ema`` (a `ParamEMA`): its shadow weights take one update from the weights this step leaves -- inside the Adam kernel
        for the tensors that have a gradient, in a launch of their own for the shadow tensors that have none -- and its update
        counter advances by one; a step the scaler skips leaves the shadow and the counter alone as well."""
        assert closure is None
        groups, fused = [], set()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                raise RuntimeError("HipAdam runs on the GPU only (no CPU fallback)")
            groups.append((group, self._table(ps, ps[0].device), ema._table(ps, fused=True)[0] if ema is not None else None))
            fused.update(id(p) for p in ps)
        rest = [p for p in ema.params if id(p) not in fused] if ema is not None else []      # shadow tensors without a gradient
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if groups or rest else None
        if scaler is not None:
            assert grad_scale == 1.0

        def launch(group, table, etab, mode, bump):
            """one `xmc_optim_step`: ``etab`` None = no shadow update in this launch"""
            tab, ch, nt, nc = table
            b1, b2 = group["betas"]
            s = L.OptimStep(table=tab.data_ptr(), chunks=ch.data_ptr(), ntensors=nt, nchunks=nc, lr=float(group["lr"]), beta1=float(b1),
                            beta2=float(b2), eps=float(group["eps"]), grad_scale=float(grad_scale), mode=mode)
            if scaler is not None:
                s.scale_dev, s.flags_dev = scaler.sf.data_ptr(), scaler.si.data_ptr()
                s.growth, s.backoff, s.interval = scaler.growth, scaler.backoff, scaler.interval
            if etab is not None:
                s.ema_table, s.num_updates_dev, s.bump = etab.data_ptr(), ema.num_updates.data_ptr(), bump
                s.decay, s.start = ema.decay, ema.start
            L.call("xmc_optim_step", C.byref(s), st)

        one_call = len(groups) == 1 and not rest       # check, update and rescale in one call
        if scaler is not None and not one_call:
            # every group is checked before any tensor (or shadow) is updated; the last update also ends the scaler's step
            for group, table, _ in groups:
                launch(group, table, None, L.ADAM_CHECK, 0)
        if rest:        # (reads the found-inf flag, so before the launch that clears it; bumps the counter only if it is the last launch)
            etab, ech, ent, enc = ema._table(rest)
            L.call("xmc_ema_step", C.c_void_p(etab.data_ptr()), ent, C.c_void_p(ech.data_ptr()), enc, float(ema.decay), int(ema.start),
                   C.c_void_p(ema.num_updates.data_ptr()), C.c_void_p(scaler.si.data_ptr()) if scaler is not None else None,
                   0 if groups else 1, st)
        for gi, (group, table, etab) in enumerate(groups):
            last = gi == len(groups) - 1
            mode = L.ADAM_UPDATE
            if scaler is not None:
                mode |= (L.ADAM_CHECK if one_call else 0) | (L.ADAM_RESCALE if last else 0)
            launch(group, table, etab, mode, 1 if last else 0)
        self._repack()

    def _repack(self):
        # the kernels wrote the parameters behind autograd's back: invalidate their packed copies and re-pack, in one launch,
        # the ones that exist (ops._PackEntry)
        changed = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        for p in changed:
            p._xmc_epoch = getattr(p, "_xmc_epoch", 0) + 1
        ops.repack_params(changed)


class ParamEMA:
    """Exponential moving average of a module's parameters, kept on the device (the weights a GAN is sampled from at evaluation
    time): per applied optimizer step ``e += (1 - d) * (p - e)`` with ``d = 0`` for the first ``start`` updates (the shadow is
    then a bit-exact copy of the weights) and ``d = decay`` afterwards.  The update count is a device counter and the warm-up is
    decided in the kernel, so the update replays inside a captured iteration across ``start`` and is skipped together with an
    optimizer step that the IEEE-half mode's loss scaler skips.

    The shadow tensors are plain f32 device tensors, not the parameters of a module: the kernels write them behind autograd's
    back, and a module running on them would need the packed-weight bookkeeping of a second network.  To USE the average,
    `copy_to` a module of the same class: an ordinary, autograd-visible write that invalidates that module's packed weights by
    the mechanism every ``p.copy_`` uses.  Buffers (BatchNorm running statistics) are not averaged; `copy_to` copies the source
    module's.  Updated by ``HipAdam.step(ema=...)`` (fused into the Adam kernel) or, after any other optimizer, by `update`."""

    def __init__(self, module, decay, start=0):
        decay, start = float(decay), int(start)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ParamEMA: decay must be in [0, 1), got {decay}")
        if start < 0:
            raise ValueError(f"ParamEMA: start must be >= 0, got {start}")
        self.decay, self.start = decay, start
        self.source = module
        self.names, self.params = [], []
        for name, p in module.named_parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"ParamEMA needs contiguous f32 parameters ({name})")
            self.names.append(name)
            self.params.append(p)
        if not self.params:
            raise ValueError("ParamEMA: the module has no parameters")
        self.shadow = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self._shadow_of = {id(p): e for p, e in zip(self.params, self.shadow)}
        device = self.params[0].device
        self.num_updates = torch.zeros(1, dtype=torch.int32, device=device)
        self._tables = {}                  # (param ptrs, with_params) -> (table, chunks, ntensors, nchunks, pinned staging...)
        self._chunk = None
        self._arenas, self._arena_off = [], 0
        if device.type == "cuda":
            self._pinned(0)                # the staging arena exists before anything is captured

    # pinned staging of the device tables, as HipAdam's: only ever added to, and only outside capture
    def _pinned(self, nbytes):
        if not self._arenas or self._arena_off + nbytes > self._arenas[-1].numel():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ParamEMA: pinned staging arena exhausted during graph capture; run a warm-up step first")
            total = sum(p.numel() for p in self.params)
            per_table = 32 * len(self.params) + 8 * (total // 4096 + len(self.params)) + 256
            self._arenas.append(torch.empty(max(8 * per_table, nbytes), dtype=torch.uint8).pin_memory())
            self._arena_off = 0
        out = self._arenas[-1][self._arena_off: self._arena_off + nbytes]
        self._arena_off += nbytes
        return out

    def _table(self, ps, fused=False):
        """device table of XmcEmaEntry for the parameters ``ps`` (in that order; a parameter that is not tracked gets a NULL
        shadow), uploaded from pinned staging.  ``fused``: the table rides beside HipAdam's own (same tensors, same order, its chunk
        list); otherwise it comes with the chunk list of a standalone launch over exactly these tensors, all of them tracked."""
        with_params = not fused
        key = (tuple(p.data_ptr() for p in ps), with_params)
        hit = self._tables.get(key)
        if hit is not None:
            return hit[:4]
        device = ps[0].device
        if device.type != "cuda":
            raise RuntimeError("ParamEMA runs on the GPU only (no CPU fallback)")
        if self._chunk is None:
            self._chunk = L.load().xmc_adam_chunk_elems()
        ents = (L.EmaEntry * len(ps))()
        chunks = []
        for i, p in enumerate(ps):
            e = self._shadow_of.get(id(p))
            if e is None and with_params:
                raise RuntimeError("ParamEMA: not a parameter of the averaged module")
            ents[i].shadow, ents[i].param, ents[i].n = (e.data_ptr() if e is not None else None), p.data_ptr(), p.numel()
            chunks += [(i, c) for c in range((p.numel() + self._chunk - 1) // self._chunk)]
        raw = bytes(ents)
        chb = torch.tensor(chunks, dtype=torch.int32).numpy().tobytes() if with_params else b""
        n0, n1 = (len(raw) + 63) // 64 * 64, (len(chb) + 63) // 64 * 64
        tab_h, ch_h = self._pinned(n0), self._pinned(n1)
        tab_h[: len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        tab = tab_h.to(device, non_blocking=True)
        ch = None
        if with_params:
            ch_h[: len(chb)].copy_(torch.frombuffer(bytearray(chb), dtype=torch.uint8))
            ch = ch_h.to(device, non_blocking=True).view(torch.int32)
        self._tables[key] = (tab, ch, len(ps), len(chunks), tab_h, ch_h)
        return self._tables[key][:4]

    @torch.no_grad()
    def update(self, skip_flag=None):
        """one update of every shadow tensor from the current weights, in one launch, and the counter's bump.  ``skip_flag``: a
        device int32 (a loss scaler's found-inf flag); while it is non-zero the launch changes nothing."""
        tab, ch, nt, nc = self._table(self.params)
        L.call("xmc_ema_step", C.c_void_p(tab.data_ptr()), nt, C.c_void_p(ch.data_ptr()), nc, float(self.decay), int(self.start),
               C.c_void_p(self.num_updates.data_ptr()), C.c_void_p(skip_flag.data_ptr()) if skip_flag is not None else None, 1,
               C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def state_dict(self):
        """``{"shadow": {parameter name: tensor}, "num_updates", "decay", "start"}`` (reads the counter back: synchronises)"""
        return {"shadow": {n: e.detach().clone() for n, e in zip(self.names, self.shadow)},
                "num_updates": int(self.num_updates.item()), "decay": self.decay, "start": self.start}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """``sd["shadow"]`` may be any mapping that holds the parameters' names (a generator's plain ``state_dict`` does)"""
        missing = [n for n in self.names if n not in sd["shadow"]]
        if missing:
            raise KeyError(f"ParamEMA.load_state_dict: no shadow for {missing}")
        for n, e in zip(self.names, self.shadow):
            e.copy_(sd["shadow"][n])             # in place: the device tables hold these addresses
        self.num_updates.fill_(int(sd["num_updates"]))
        if "decay" in sd:
            self.decay = float(sd["decay"])
        if "start" in sd:
            self.start = int(sd["start"])

    @torch.no_grad()
    def copy_to(self, module):
        """write the shadow weights, and the source module's buffers, into ``module`` (same class as the source): ``p.copy_`` on the
        parameters themselves, which autograd sees (``p._version`` moves), so cached packed copies of them are stale by
        construction.  Returns ``module``."""
        targets = dict(module.named_parameters())
        if set(targets) != set(self.names):
            raise KeyError("ParamEMA.copy_to: the module's parameters are not those of the averaged module")
        for n, e in zip(self.names, self.shadow):
            targets[n].copy_(e)
        src = dict(self.source.named_buffers())
        for n, b in module.named_buffers():
            b.copy_(src[n])
        return module
