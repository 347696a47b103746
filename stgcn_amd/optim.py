"""AdamW whose whole step is ONE HIP kernel (``stgcn_adamw_step``) instead of the per-tensor loops /
multi-tensor launches of ``torch.optim.AdamW`` (reference: main.py:147-148, step at main.py:169).

Semantics follow torch.optim.AdamW with amsgrad=False, maximize=False: decoupled weight decay, bias-corrected
moments, and -- like the reference's optimizer -- parameters whose ``.grad`` is None are skipped entirely (no
decay, no state).  It subclasses ``torch.optim.Optimizer`` so LR schedulers (StepLR at main.py:156) work.

``capturable=True`` keeps the step count and the learning rate in device memory so that ``step()`` can be
recorded into a hipGraph; call ``sync_lr()`` after a scheduler changed ``param_groups[i]['lr']``.

``NAdamW`` and ``Lion`` are the reference's two other optimizers (main.py:149-154, ``--opt nadamw | lion``) with the same
surface: one HIP launch per ``step()`` (``stgcn_optim_step``) and the fused step tail (``flush_with`` through
``stgcn_grad_flush_optim``).

``max_grad_norm`` (all three, default None = off: every launch is the one that runs without it) clips the gradient by its global norm
inside the step, with the semantics of ``torch.nn.utils.clip_grad_norm_(params_with_grad, max_norm)`` followed by ``step()``: the norm
over the live parameters of ALL groups is measured once on the device (fp64 sums), ``coef = min(1, max_norm / (norm + 1e-6))`` is formed
in fp32 and the update sees ``coef * g``.  ``step()`` is a norm launch + the update (``stgcn_grad_norm``, ``stgcn_optim_step_clip``);
``flush_with`` is the gradient flush with the norm as its epilogue + the update (``stgcn_grad_flush_clip``).  Both are capturable.  The
value lives in ``param_groups[i]['max_grad_norm']`` (group 0's is used) and so travels in ``state_dict``.  UNLIKE torch, ``.grad`` and
the arena views keep the UNCLIPPED gradient after the step: nothing scales them in place.  ``last_grad_norm`` / ``last_clip_coef`` are
device tensors of one fp32 each (views of the clip state; reading them synchronises).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def _check_max_grad_norm(v):
    if v is not None and not float(v) > 0.0:       # (NaN fails the comparison too; +inf is allowed: the norm is measured, coef = 1)
        raise ValueError(f"max_grad_norm = {v} must be > 0 (or None: no clipping)")


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False, max_grad_norm=None):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0.0:
            raise ValueError("invalid AdamW hyper-parameter")
        _check_max_grad_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self._init_common(capturable)

    def _init_common(self, capturable):
        self.capturable = capturable
        self._dev = {}     # per group: (step tensor, lr tensor) on the device (capturable mode)
        self.trainer_owns_step = False   # a trainer advances the device step count itself (stgcn_prepack counters): step() must not
        self._clip_state = None          # fp64 device words of stgcn_grad_clip (max_grad_norm), created on first use
        self._clip_retired = []          # outgrown states: a captured graph may still hold their address

    # ---- clipping by global norm (max_grad_norm) ----------------------------------------------------------------------------------------
    def _max_grad_norm(self):
        v = self.param_groups[0].get("max_grad_norm")
        return None if v is None else float(v)

    def _clip(self, L, dev, words, max_norm):
        """the stgcn_grad_clip block over a zeroed state of at least ``words`` fp64 words on ``dev``"""
        st = self._clip_state
        if st is None or st.device != dev or st.numel() < words:
            if st is not None:
                self._clip_retired.append(st)
            st = self._clip_state = torch.zeros(int(words), dtype=torch.float64, device=dev)
        c = _lib.GradClip()
        c.state, c.state_words, c.max_norm = st.data_ptr(), st.numel(), max_norm
        return c

    @staticmethod
    def _table_words(L, table, count):
        w = C.c_int64(0)
        L.check(L.dll.stgcn_grad_clip_words(table, count, C.byref(w)), "stgcn_grad_clip_words")
        return int(w.value)

    def _clip_word(self, k):
        return None if self._clip_state is None else self._clip_state.view(torch.float32)[2 * k:2 * k + 1]

    @property
    def last_grad_norm(self):
        """The global gradient norm the last clipping step measured: a device tensor of one fp32 (None before the first such step)."""
        return self._clip_word(_lib.CLIP_TOTAL)

    @property
    def last_clip_coef(self):
        """The factor the last clipping step applied, min(1, max_grad_norm / (norm + 1e-6)): a device tensor of one fp32."""
        return self._clip_word(_lib.CLIP_COEF)

    def _optim_hyper(self, group, step, step_dev, lr_dev, gi):
        """the kind-generic hyper-parameter block (stgcn_optim_step_clip takes every kind through it)"""
        h = _lib.OptimHyper()
        b1, b2 = group["betas"]
        h.kind, h.lr, h.beta1, h.beta2 = _lib.OPT_ADAMW, float(group["lr"]), float(b1), float(b2)
        h.eps, h.weight_decay, h.momentum_decay = float(group["eps"]), float(group["weight_decay"]), 0.0
        h.step, h.step_dev, h.lr_dev, h.mu_product, h.mu_product_dev = step, step_dev, lr_dev, 1.0, None
        return h

    def sync_lr(self):
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev:
                self._dev[gi][1].fill_(float(group["lr"]))

    @torch.no_grad()
    def device_step_counter(self, device) -> torch.Tensor:
        """The device-side step count of group 0 (capturable mode), created on first use.  A trainer that advances it
        itself (e.g. on the weight-pack launch at the start of the step, ``stgcn_prepack`` counters) passes
        ``bump_step=False`` to ``flush_with``."""
        group = self.param_groups[0]
        if 0 not in self._dev:
            self._dev[0] = (torch.zeros(1, dtype=torch.int64, device=device), torch.full((1,), float(group["lr"]), device=device))
        return self._dev[0][0]

    def flush_with(self, sink, grads, bump_step: bool = True):
        """``sink.flush()`` + ``step()`` in ONE launch (stgcn_grad_flush with the optimizer table): every gradient element is
        reduced from the backward partials and consumed by AdamW on the spot.  ``grads``: {parameter: gradient buffer} of the
        sink (all live parameters of the single param group); same arithmetic and state as ``step()``.
        With ``max_grad_norm`` two launches: the flush, whose epilogue leaves the global norm and the clip coefficient on the device,
        then the update on ``coef * g``; the gradient buffers keep the unclipped gradient."""
        from . import ops
        assert len(self.param_groups) == 1, "flush_with handles one parameter group"
        group = self.param_groups[0]
        live = [p for p in group["params"] if p in grads]
        assert len(live) == len(grads), "gradient sink holds parameters this optimizer does not own"
        dev = live[0].device
        table = (_lib.AdamwTensor * len(live))()
        for i, p in enumerate(live):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("stgcn_amd.optim.AdamW handles contiguous float32 parameters only")
            st = self.state[p]
            if not st:
                self._init_state(st, p)
            table[i].param, table[i].grad = p.data_ptr(), grads[p].data_ptr()
            table[i].exp_avg, table[i].exp_avg_sq, table[i].numel = st["exp_avg"].data_ptr(), self._v_ptr(st), p.numel()
        max_norm = self._max_grad_norm()
        make = self._hyper if max_norm is None else self._optim_hyper
        if self.capturable and dev.type == "cuda":
            self.device_step_counter(dev)
            step_t, lr_t = self._dev[0]
            if bump_step:
                step_t.add_(1)
            hyper = make(group, 0, step_t.data_ptr(), lr_t.data_ptr(), 0)
        else:
            group["_step"] = group.get("_step", 0) + 1
            hyper = make(group, group["_step"], None, None, 0)
        stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
        if max_norm is None:
            sink.flush(table, hyper, stream)
        else:
            L = _lib.lib()
            clip = self._clip(L, dev, max(sink.clip_words(), self._table_words(L, table, len(live))), max_norm)
            sink.flush(stream=stream, clip=clip)
            L.check(L.dll.stgcn_optim_step_clip(table, len(live), C.byref(hyper), C.byref(clip), stream), "stgcn_optim_step_clip")
        self._advance_host(group, hyper)

    # ---- what the optimizer kinds differ in (state tensors, hyper-parameter block, launch) ------------------------------------------
    def _init_state(self, st, p):
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _v_ptr(self, st):
        return st["exp_avg_sq"].data_ptr()

    def _hyper(self, group, step, step_dev, lr_dev, gi):
        hyper = _lib.AdamwHyper()
        b1, b2 = group["betas"]
        hyper.lr, hyper.beta1, hyper.beta2, hyper.eps, hyper.weight_decay = float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])
        hyper.step, hyper.step_dev, hyper.lr_dev = step, step_dev, lr_dev
        return hyper

    def _advance_host(self, group, hyper):
        """after a launch: host-side state that eager mode keeps (none for AdamW)"""

    def _launch_step(self, L, table, count, group, step, step_dev, lr_dev, gi, stream):
        b1, b2 = group["betas"]
        L.check(L.dll.stgcn_adamw_step(table, count, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                       float(group["weight_decay"]), step, step_dev, lr_dev, stream), "stgcn_adamw_step")

    def state_dict(self):
        """torch's state_dict plus the step counts, which capturable mode keeps in device tensors outside ``state`` (without them a
        resumed run would restart the bias correction at t = 1: a ~10x too large first update)."""
        sd = super().state_dict()
        for gi, g in enumerate(sd["param_groups"]):
            if gi in self._dev:
                g["_step"] = int(self._dev[gi][0].item())
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            if self.capturable and "_step" in group:
                live = [p for p in group["params"]]
                if live and live[0].is_cuda:
                    dev = live[0].device
                    if gi not in self._dev:
                        self._dev[gi] = (torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), float(group["lr"]), device=dev))
                    self._dev[gi][0].fill_(int(group["_step"]))
                    self._dev[gi][1].fill_(float(group["lr"]))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        max_norm = self._max_grad_norm()
        work = []          # clipping: the norm runs over every group's live gradients before the first update
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            dev = live[0].device
            for p in live:
                if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("stgcn_amd.optim.AdamW handles contiguous float32 parameters only")
                st = self.state[p]
                if not st:
                    self._init_state(st, p)
            step_dev = lr_dev = None
            if self.capturable and dev.type == "cuda":
                if gi not in self._dev:
                    self._dev[gi] = (torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), float(group["lr"]), device=dev))
                step_t, lr_t = self._dev[gi]
                if not self.trainer_owns_step:
                    step_t.add_(1)
                step_dev, lr_dev = step_t.data_ptr(), lr_t.data_ptr()
                step = 0
            else:
                group["_step"] = group.get("_step", 0) + 1
                step = group["_step"]
            table = (_lib.AdamwTensor * len(live))()
            for i, p in enumerate(live):
                st = self.state[p]
                table[i].param, table[i].grad = p.data_ptr(), p.grad.data_ptr()
                table[i].exp_avg, table[i].exp_avg_sq, table[i].numel = st["exp_avg"].data_ptr(), self._v_ptr(st), p.numel()
            stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
            if max_norm is None:
                self._launch_step(L, table, len(live), group, step, step_dev, lr_dev, gi, stream)
            else:
                work.append((table, group, step, step_dev, lr_dev, gi, stream, dev))
        if work:
            self._clipped_updates(L, work, max_norm)
        return loss

    def _clipped_updates(self, L, work, max_norm):
        """ONE norm over the gradients of all groups (stgcn_grad_norm), then each group's update on coef * g (stgcn_optim_step_clip)"""
        stream, dev = work[0][6], work[0][7]
        if any(w[7] != dev for w in work):
            raise RuntimeError("max_grad_norm: the parameters of all groups must live on one device")
        rows = [t for w in work for t in w[0]]
        full = (_lib.AdamwTensor * len(rows))()
        for i, t in enumerate(rows):
            full[i].grad, full[i].numel = t.grad, t.numel
        words = max([self._table_words(L, full, len(rows))] + [self._table_words(L, w[0], len(w[0])) for w in work])
        clip = self._clip(L, dev, words, max_norm)
        L.check(L.dll.stgcn_grad_norm(full, len(rows), C.byref(clip), stream), "stgcn_grad_norm")
        for table, group, step, step_dev, lr_dev, gi, stream, _ in work:
            h = self._optim_hyper(group, step, step_dev, lr_dev, gi)
            L.check(L.dll.stgcn_optim_step_clip(table, len(table), C.byref(h), C.byref(clip), stream), "stgcn_optim_step_clip")
            self._advance_host(group, h)


class _OptimKind(AdamW):
    """NAdamW / Lion: AdamW's surface (capturable step count and lr, ``sync_lr``, ``flush_with``, ``trainer_owns_step``, state_dict with the
    step count) over the kind-generic entry points ``stgcn_optim_step`` / ``stgcn_grad_flush_optim``."""
    KIND = -1

    def __init__(self, params, defaults, capturable):
        lr, (b1, b2), wd = defaults["lr"], defaults["betas"], defaults["weight_decay"]
        if lr < 0.0 or defaults.get("eps", 0.0) < 0.0 or not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0 or wd < 0.0:
            raise ValueError(f"invalid {type(self).__name__} hyper-parameter")
        _check_max_grad_norm(defaults.get("max_grad_norm"))
        torch.optim.Optimizer.__init__(self, params, defaults)
        self._init_common(capturable)
        self._mu = {}      # NAdamW, capturable: per group the two device slots of the running product mu_1 ... mu_t (step parity)

    def _mu_slots(self, gi):
        if gi not in self._mu:
            self._mu[gi] = torch.ones(2, dtype=torch.float32, device=self._dev[gi][0].device)
        return self._mu[gi]

    def _hyper(self, group, step, step_dev, lr_dev, gi):
        h = _lib.OptimHyper()
        b1, b2 = group["betas"]
        h.kind, h.lr, h.beta1, h.beta2 = self.KIND, float(group["lr"]), float(b1), float(b2)
        h.eps, h.weight_decay, h.momentum_decay = float(group.get("eps", 0.0)), float(group["weight_decay"]), float(group.get("momentum_decay", 0.0))
        h.step, h.step_dev, h.lr_dev = step, step_dev, lr_dev
        h.mu_product = float(group.get("_mu_product", 1.0))
        h.mu_product_dev = self._mu_slots(gi).data_ptr() if (self.KIND == _lib.OPT_NADAMW and step_dev) else None
        return h

    _optim_hyper = _hyper

    def _launch_step(self, L, table, count, group, step, step_dev, lr_dev, gi, stream):
        h = self._hyper(group, step, step_dev, lr_dev, gi)
        L.check(L.dll.stgcn_optim_step(table, count, C.byref(h), stream), "stgcn_optim_step")
        self._advance_host(group, h)

    def state_dict(self):
        sd = super().state_dict()
        for gi, g in enumerate(sd["param_groups"]):
            if gi in self._mu and "_step" in g:
                g["_mu_product"] = float(self._mu[gi][int(g["_step"]) & 1].item())
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            if self.capturable and gi in self._dev and "_mu_product" in group:
                self._mu_slots(gi).fill_(float(group["_mu_product"]))


class NAdamW(_OptimKind):
    """torch.optim.NAdam(lr, betas, eps, weight_decay, momentum_decay, decoupled_weight_decay=True) as main.py:150 builds it (amsgrad-free,
    maximize False).  The running product of the momentum schedule mu_t = beta1 (1 - 0.5 * 0.96^(t * momentum_decay)) is an fp32 number on
    the host in eager mode (``param_groups[i]['_mu_product']``, advanced like torch's state tensor) and two device floats in capturable mode,
    read and advanced by the update launch itself (stgcn_hip.h, stgcn_optim_hyper)."""
    KIND = _lib.OPT_NADAMW

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3, capturable=False,
                 max_grad_norm=None):
        if momentum_decay < 0.0:
            raise ValueError("invalid NAdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay,
                                      max_grad_norm=max_grad_norm), capturable)

    def _advance_host(self, group, hyper):
        if hyper.mu_product_dev:
            return
        t, b1, md = float(hyper.step), float(group["betas"][0]), float(group["momentum_decay"])
        mu = b1 * (1.0 - 0.5 * (0.96 ** (t * md)))
        group["_mu_product"] = float(np.float32(group.get("_mu_product", 1.0)) * np.float32(mu))     # torch: fp32 state tensor *= mu


class Lion(_OptimKind):
    """script/opt.py ``Lion(lr, betas=(0.9, 0.99), weight_decay)`` as main.py:152 builds it: p *= 1 - lr wd ; c = beta1 m + (1 - beta1) g ;
    p -= lr sign(c) ; m = beta2 m + (1 - beta2) g.  One state tensor (``exp_avg``), no eps."""
    KIND = _lib.OPT_LION

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-2, capturable=False, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay, max_grad_norm=max_grad_norm), capturable)

    def _init_state(self, st, p):
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _v_ptr(self, st):
        return None
