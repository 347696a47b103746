"""Data-parallel training step of the reference loop body (main.py:164-171) on MI355X.

One process per GPU (torchrun / torch.distributed, backend "nccl" = RCCL over xGMI).  The model is
replicated (245 K parameters + a 171 KB operator), the minibatch is sharded: rank r takes windows
[step*B_global + r*B_local, ... + B_local) of the unshuffled index (the reference iterates with
shuffle=False, main.py:127), so W ranks x bs 32 reproduces one device at bs 32*W.  The only exchange is
ONE all-reduce per step over a flat fp32 gradient buffer (~0.98 MB for METR-LA): latency-bound, not
link-bound on xGMI, so no bucketing.

Parameters that never receive a gradient (10 unused align convs) are excluded from the flat buffer and
from the optimizer's work exactly like torch.optim.AdamW skips ``grad is None`` in the reference.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist


def dist_env():
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, local_rank, world


def init_distributed(backend: Optional[str] = None):
    """One process per GPU.  The device is bound BEFORE the process group is created so that RCCL builds its
    communicator on the right GPU (and the first collective does not have to guess)."""
    rank, local_rank, world = dist_env()
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this driver stack
        if backend == "nccl":
            try:
                dist.init_process_group(backend=backend, rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            except TypeError:      # older signature without device_id
                dist.init_process_group(backend=backend, rank=rank, world_size=world)
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    if world > 1:      # every data-parallel rank draws its own dropout masks (the shards are different windows of one global batch)
        from .layers import DropoutStream
        base = DropoutStream.seed - DropoutStream.rank_offset
        DropoutStream.rank_offset = rank        # survives a later DropoutStream.manual_seed(s) of user code (set-seed-after-init order)
        DropoutStream.manual_seed(base)
    return rank, local_rank, world


def probe_collective_capture(timeout_s: float = 60.0) -> Tuple[bool, str]:
    """Can this machine record an RCCL all-reduce inside a hipGraph and replay it?  Every rank runs the SAME small experiment in a CHILD
    process (its own process group on MASTER_PORT + 17, same GPU, a 1 MB buffer: warm-up collective, capture, three replays, value check)
    under a watchdog: a capture or replay that hangs -- the failure mode that cannot be caught with try / except -- costs ``timeout_s``
    and one killed child, not the run.  The verdicts are combined over the ranks (all must succeed).  Returns (ok, reason)."""
    rank, local_rank, world = dist_env()
    if not (dist.is_available() and dist.is_initialized()) or world <= 1:
        return False, "no process group"
    if dist.get_backend() != "nccl":
        return False, f"backend {dist.get_backend()}: its collectives are host calls, not stream operations"
    ok, why = run_collective_capture_child(dict(os.environ), timeout_s)
    flag = torch.tensor([1 if ok else 0], device=torch.device("cuda", local_rank))
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) == 0 and ok:
        ok, why = False, "another rank's probe failed"
    return ok, why


def capture_child_env(env: dict) -> dict:
    """Environment of the probe's child: the parent's rank variables, the rendezvous port shifted by 17, and WITHOUT the launcher's
    TORCHELASTIC_* variables -- under ``torch.distributed.run`` TORCHELASTIC_USE_AGENT_STORE makes ``env://`` rendezvous attach to the
    agent's store as a client; on the shifted port nobody serves one, so every child would wait for its timeout and the probe would
    always say "hung".  Without them rank 0's child hosts its own store."""
    env = {k: v for k, v in env.items() if not k.startswith("TORCHELASTIC_")}
    env["MASTER_PORT"] = str(int(env.get("MASTER_PORT", "29500")) + 17)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def run_collective_capture_child(env: dict, timeout_s: float = 60.0) -> Tuple[bool, str]:
    """One rank's share of ``probe_collective_capture``: the experiment in a child process (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from
    ``env``, port shifted by 17 so that it cannot meet the parent's group), killed after ``timeout_s``."""
    import subprocess
    import sys
    code = (
        "import os, torch, torch.distributed as dist\n"
        "r, lr, w = int(os.environ['RANK']), int(os.environ['LOCAL_RANK']), int(os.environ['WORLD_SIZE'])\n"
        "torch.cuda.set_device(lr)\n"
        "dist.init_process_group('nccl', rank=r, world_size=w, device_id=torch.device('cuda', lr))\n"
        "t = torch.full((1 << 18,), float(r + 1), device='cuda')\n"
        "dist.all_reduce(t); torch.cuda.synchronize()\n"
        "t.fill_(float(r + 1))\n"
        "s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())\n"
        "g = torch.cuda.CUDAGraph()\n"
        "with torch.cuda.graph(g, capture_error_mode='thread_local'):\n"
        "    dist.all_reduce(t)\n"
        "    t.mul_(1.0 / w)\n"
        "for _ in range(3):\n"
        "    t.fill_(float(r + 1)); g.replay()\n"
        "torch.cuda.synchronize()\n"
        "want = sum(range(1, w + 1)) / w\n"
        "assert abs(float(t[0]) - want) < 1e-6 and abs(float(t[-1]) - want) < 1e-6, (float(t[0]), want)\n"
        "dist.destroy_process_group()\n"
        "print('CAPTURE_OK')\n")
    env = capture_child_env(env)
    ok, why = False, ""
    try:
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout_s)
        ok = p.returncode == 0 and "CAPTURE_OK" in p.stdout
        why = "" if ok else ("probe failed: " + (p.stderr.strip().splitlines() or ["rc %d" % p.returncode])[-1][:200])
    except subprocess.TimeoutExpired:
        why = f"probe hung for {timeout_s:.0f} s (killed)"
    except Exception as e:  # noqa: BLE001
        why = "probe could not run: " + repr(e)[:200]
    return ok, why


def _broadcast_sparse_operator(gso: torch.Tensor, comm_dev, src: int) -> torch.Tensor:
    """Rank ``src``'s sparse operator on every rank: the ranks may hold different numbers of stored entries, so the lengths go first, then
    the index and value arrays (a sparse tensor itself cannot be broadcast).  Returns a ``sparse_csr`` / ``sparse_coo`` tensor on ``comm_dev``."""
    csr = gso.layout == torch.sparse_csr
    if not csr and gso.layout != torch.sparse_coo:
        raise ValueError(f"sync_operators: a strided, sparse_csr or sparse_coo operator expected, got {gso.layout}")
    # int64 indices and float32 values on every rank, whatever each rank built its own operator with: the receive buffers must match the sender's
    mine = (gso.crow_indices(), gso.col_indices(), gso.values()) if csr else (gso._indices(), gso._values())
    mine = tuple(t.detach().to(torch.int64) for t in mine[:-1]) + (mine[-1].detach().to(torch.float32),)
    meta = torch.tensor([1 if csr else 0, gso.shape[0], gso.shape[1]] + [t.numel() for t in mine] + [0] * (3 - len(mine)), dtype=torch.int64,
                        device=comm_dev)
    dist.broadcast(meta, src=src)
    src_csr, rows, cols, *lens = (int(v) for v in meta.tolist())
    if bool(src_csr) != csr:
        raise ValueError("sync_operators: the ranks hold sparse operators of different layouts")
    out = []
    for i, t in enumerate(mine):
        shape = (2, lens[i] // 2) if (not csr and i == 0) else (lens[i],)
        b = t.detach().to(comm_dev, copy=True).contiguous() if dist.get_rank() == src else torch.empty(shape, dtype=t.dtype, device=comm_dev)
        dist.broadcast(b, src=src)
        out.append(b)
    if csr:
        return torch.sparse_csr_tensor(out[0], out[1], out[2], size=(rows, cols))
    return torch.sparse_coo_tensor(out[0], out[1], size=(rows, cols))


def sync_operators(model, src: int = 0) -> None:
    """Data-parallel replicas must train with ONE graph shift operator: ``gso`` is a plain attribute (not a parameter, not a
    buffer, never all-reduced -- layers.py:128/179 of the reference), and the reference's ``calc_chebynet_gso`` depends on numpy's
    global RNG state (script/utility.py:59-76), so differently seeded ranks would silently hold different operators.  Broadcasts
    every fused block's ``gso`` from rank ``src`` (no-op without a process group)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return
    from .layers import STConvBlock
    seen = {}
    for m in model.modules():
        if isinstance(m, STConvBlock) and torch.is_tensor(m.gso):
            g = seen.get(id(m.gso))
            if g is None:
                # the collective runs on the process group's device (RCCL needs a tensor on this rank's GPU; `gso` is a plain attribute
                # that .to(device) never moved, so it is often still a CPU tensor) and the result goes back where the operator lived
                home = m.gso.device
                comm_dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
                if m.gso.layout != torch.strided:
                    g = _broadcast_sparse_operator(m.gso, comm_dev, src).to(home)
                else:
                    t = m.gso.detach().to(comm_dev, copy=True).contiguous()
                    dist.broadcast(t, src=src)
                    g = t.to(home)
                seen[id(m.gso)] = g
            m.gso = g
            m.graph_conv.gso = g
            gc = getattr(m.graph_conv, "cheb_graph_conv", None) or getattr(m.graph_conv, "graph_conv", None)
            if gc is not None:
                gc.gso = g
            m._gso_cache = None


class FlatGradAllReduce:
    """Sum-all-reduce of every live gradient in one collective, then scale by 1/world."""

    def __init__(self, params: List[torch.nn.Parameter], world: int):
        self.params = list(params)
        self.world = world
        self.flat: Optional[torch.Tensor] = None
        self.live: Optional[List[torch.nn.Parameter]] = None

    def __call__(self):
        if self.world <= 1:
            return
        live = [p for p in self.params if p.grad is not None]
        if self.live is None or len(live) != len(self.live):
            self.live = live
            n = sum(p.numel() for p in live)
            self.flat = torch.empty(n, dtype=torch.float32, device=live[0].device)
        grads = [p.grad.reshape(-1) for p in live]
        torch.cat(grads, out=self.flat)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
        self.flat.mul_(1.0 / self.world)
        torch._foreach_copy_([p.grad.reshape(-1) for p in live], list(self.flat.split([p.numel() for p in live])))


def make_optimizer(model: torch.nn.Module, lr: float = 1e-3, weight_decay: float = 1e-3, name: str = "adamw",
                   capturable: bool = False, max_grad_norm: Optional[float] = None):
    """main.py:147-154 (adamw is the default; nadamw is NAdam with decoupled decay; lion is script/opt.py's Lion).  Each is one HIP
    launch per step and rides in the fused step tail (``flush_with``).
    ``capturable``: keep the step counters on the device so that ``step()`` can live inside a hipGraph.
    ``max_grad_norm``: clip the gradient by its global norm inside the step (``clip_grad_norm_(params, max_grad_norm)`` + ``step()``;
    None = off).  Every trainer of this module goes through the optimizer, so it holds for all of them: the fused tail becomes flush with
    the norm epilogue + update, every other path norm + update -- under ``world > 1`` after the all-reduce, i.e. the norm of the mean
    gradient, as one process on the whole batch would clip.  ``.grad`` / the arena views keep the UNCLIPPED gradient (torch scales them)."""
    params = list(model.parameters())
    if name == "adamw":
        from .optim import AdamW        # one HIP kernel per step (stgcn_adamw_step)
        return AdamW(params, lr=lr, weight_decay=weight_decay, capturable=capturable, max_grad_norm=max_grad_norm)
    if name == "nadamw":
        from .optim import NAdamW       # main.py:150 (stgcn_optim_step)
        return NAdamW(params, lr=lr, weight_decay=weight_decay, capturable=capturable, max_grad_norm=max_grad_norm)
    if name == "lion":
        from .optim import Lion         # main.py:152
        return Lion(params, lr=lr, weight_decay=weight_decay, capturable=capturable, max_grad_norm=max_grad_norm)
    raise ValueError(f"ERROR: The {name} optimizer is undefined.")   # main.py:154


LOSSES = ("mse", "mae", "huber")      # nn.MSELoss() (main.py:136), nn.L1Loss(), nn.HuberLoss(huber_delta): ops.LOSS_KINDS


def check_loss(loss: str, huber_delta: float = 1.0) -> None:
    """Refuse a loss name the trainers do not know, or a Huber delta that is not finite and positive (``ValueError``)."""
    import math
    if loss not in LOSSES:
        raise ValueError(f"unknown loss {loss!r}: one of {', '.join(LOSSES)} expected")
    if loss == "huber" and not (math.isfinite(huber_delta) and huber_delta > 0):
        raise ValueError(f"huber_delta = {huber_delta} must be finite and positive")


def fwd_loss_bwd(model, x, y, loss: str = "mse", huber_delta: float = 1.0, valid=None):
    """forward -> loss (MSELoss: main.py:166-168) -> backward with the loss formed inside the fused head's backward (``ops.loss_backward``;
    one loss launch + ``pred.backward(dpred)`` for a model without the fused head).  ``valid`` (bool / uint8 like ``y``, or an
    ``ops.LossMask``): the mean over the observed labels only (``data.observed_mask``).  Returns the loss (shape [])."""
    from . import ops
    check_loss(loss, huber_delta)
    y_pred = model(x).reshape(len(x), -1)
    return ops.loss_backward(y_pred, y, loss, huber_delta, valid=valid)[0]


def check_in_launch_waits(model) -> None:
    """Raise if a fused operator's last forward had an in-launch wait that gave up (the tiles of a LayerNorm slab / window wait for each
    other inside ONE launch; a wait is bounded, and a starved tile writes NaN and sets a sticky word instead of hanging the device).  The
    NaN reaches the loss anyway -- this names the operator and the slab / window.  Synchronises the stream: call it where the loss is read
    (once per epoch, after a timed loop), not inside the step."""
    from .layers import OutputBlock, STConvBlock
    for name, m in model.named_modules():
        if isinstance(m, (STConvBlock, OutputBlock)):
            w = m.chain_status()
            if w:
                what = "(b, t) slab" if isinstance(m, STConvBlock) else "window"
                raise RuntimeError(f"{name or type(m).__name__}: an in-launch wait of the last forward gave up on {what} {w - 1} -- its outputs are NaN "
                                   f"(the device was not this launch's alone for stgcn_set_chain_spin_ticks; the next weight pack re-arms the words)")


def fused_tail_supported(model, live_params) -> bool:
    """The fused step tail (``GradSink`` / ``stgcn_grad_flush``) writes the gradient of every parameter OWNED BY A FUSED OPERATOR
    (``STConvBlock``, a supported ``OutputBlock``) and nothing else.  A live parameter outside of them (the two ``nn.Linear`` of the
    Ko == 0 head, models.py:46-51, or any user module around the model) gets its gradient from autograd, which would ACCUMULATE
    into the never-zeroed arena view installed as ``.grad``: such models take the plain step (zero_grad / backward / step)."""
    from . import ops
    from .layers import OutputBlock, STConvBlock
    owned = set()
    for m in model.modules():
        if isinstance(m, STConvBlock) or (isinstance(m, OutputBlock) and ops.head_supported(m.cfg)):
            owned.update(id(p) for p in m.parameters())
    return all(id(p) in owned for p in live_params)


class GradArena:
    """One flat fp32 buffer holding the gradient of every live parameter (those the model actually uses: the reference
    leaves ``.grad`` None for the 10 idle align convs) in ``model.parameters()`` order, with one view
    per parameter installed as ``param.grad``.  It is at once the destination of ``ops.GradSink.flush`` (no per-step
    gradient allocations, no autograd accumulation) and the data-parallel all-reduce buffer (no flatten / unflatten
    copies around the collective)."""

    def __init__(self, live_params: List[torch.nn.Parameter]):
        from . import ops
        self.params = list(live_params)
        dev = self.params[0].device
        self.flat = torch.zeros(sum(p.numel() for p in self.params), dtype=torch.float32, device=dev)
        self.grads = {}
        off = 0
        for p in self.params:
            self.grads[p] = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.sink = ops.GradSink(self.grads)

    def install(self):
        for p, g in self.grads.items():
            p.grad = g


def fused_train_step(model, optimizer, x, y, arena: GradArena, world: int = 1, all_reduce=None, loss: str = "mse",
                     huber_delta: float = 1.0, valid=None):
    """The loop body of main.py:165-169 with the step tail fused: forward -> backward with the loss (``loss``) formed inside the head and
    deferred reductions -> ONE launch for all gradient reductions + AdamW (world == 1), or reductions into the flat arena ->
    ``all_reduce(arena.flat)`` -> AdamW (world > 1; the 1/world of the gradient mean rides on the loss gradient).
    ``param.grad`` are the arena views (overwritten every step, never accumulated).  ``valid``: as in ``fwd_loss_bwd``; with
    world > 1 each rank takes the mean over its own observed labels and the ranks are averaged, as DDP around a masked mean does."""
    from . import ops
    check_loss(loss, huber_delta)
    if not fused_tail_supported(model, arena.params):
        raise RuntimeError("fused_train_step: the model has live parameters outside the fused operators (see fused_tail_supported); "
                           "use train_step")
    arena.install()
    with ops.grad_sink_scope(arena.sink):
        y_pred = model(x).reshape(len(x), -1)
        value = ops.loss_backward(y_pred, y, loss, huber_delta, grad_scale=1.0 / world, valid=valid)      # (valid after the flush below)
    if world <= 1 and hasattr(optimizer, "flush_with"):
        optimizer.flush_with(arena.sink, arena.grads)
    else:
        arena.sink.flush(stream=torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else None)
        if world > 1 and all_reduce is not None:
            all_reduce(arena.flat)
        optimizer.step()
    return value[0]


def train_step(model, optimizer, x, y, allreduce: Optional[FlatGradAllReduce] = None, loss: str = "mse", huber_delta: float = 1.0,
               valid=None):
    """zero_grad -> forward -> loss (MSELoss) -> backward -> [all-reduce] -> optimizer.step (main.py:165-169).  ``valid``: as in
    ``fwd_loss_bwd``.  Returns the loss tensor (no host sync: the reference's per-step .item() at main.py:170 is deferred)."""
    from .layers import DropoutStream
    check_loss(loss, huber_delta)
    optimizer.zero_grad(set_to_none=True)
    value = fwd_loss_bwd(model, x, y, loss, huber_delta, valid=valid)
    if allreduce is not None:
        allreduce()
    optimizer.step()
    DropoutStream.advance()      # (device-counter mode only: eager mode consumes a fresh host offset per forward)
    return value.detach()


def tail_step(model, optimizer, x, y, world: int = 1, rank: int = 0, loss: str = "mse", huber_delta: float = 1.0, valid=None):
    """The partial last minibatch of an epoch (the reference iterates with ``DataLoader(drop_last=False)``, main.py:126-131, so its
    last step sees n < batch_size windows).  ``x`` / ``y`` are the GLOBAL tail batch (n windows, the same tensors on every rank);
    rank r takes a contiguous share of ceil(n / world) windows -- possibly none -- and weights its loss gradient by n_local / n, so
    the SUM all-reduce of the gradients is exactly the gradient of the mean loss over the n windows (``weight by local count``,
    SURVEY.md section 8e; every loss kind is a mean).  Eager launches: a captured step has a fixed batch shape.  Returns the global mean loss (tensor).
    ``valid`` (bool / uint8 like ``y``): the masked mean, for world == 1 only -- with a mask the weight of a rank's share is its OBSERVED
    count over the batch's, a device value that the host-side n_local / n cannot stand in for (``NotImplementedError`` for world > 1)."""
    from . import ops
    from .layers import DropoutStream
    check_loss(loss, huber_delta)
    if valid is not None and world > 1:
        raise NotImplementedError("tail_step: valid= with world > 1 is not implemented: the weight of a rank's share of a masked mean is its "
                                  "observed count over the batch's, not n_local / n")
    n = len(x)
    per = (n + world - 1) // world
    lo, hi = min(rank * per, n), min(rank * per + per, n)
    optimizer.zero_grad(set_to_none=True)
    dev = x.device
    loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
    # A live GraphedTrainStep may have put its step counters (dropout position, AdamW step count, series window index) on the model's
    # weight-pack launch (``model._step_counters``): this eager step must not let that launch advance the WINDOW index (the tail batch
    # is handed over explicitly; the next replay has to start at the window the index already points to), so the counters are suspended
    # around the forward and the two that a tail step does consume -- dropout position and optimizer step count -- are advanced below.
    # The dropout position: a folded step's sites see the counter AFTER the pack launch's bump, so between two replays the word still holds
    # the position the LAST replay drew at -- this step has to move it on BEFORE its forward (as the suspended pack launch would have), or
    # the tail batch repeats that replay's masks.  Unfolded steps leave the word at the next free position and advance it after the step.
    folded = getattr(model, "_step_counters", None)
    drop_folded = folded is not None and any(c[0] is DropoutStream.counter for c in folded)
    if folded is not None:
        model._step_counters = None
    if drop_folded:
        DropoutStream.advance()
    try:
        if hi > lo:
            pred = model(x[lo:hi]).reshape(hi - lo, -1)
            value = ops.loss_backward(pred, y[lo:hi].contiguous(), loss, huber_delta, grad_scale=(hi - lo) / n,
                                      valid=None if valid is None else valid[lo:hi].contiguous())
            loss_sum = value * ((hi - lo) / n)
    finally:
        if folded is not None:
            model._step_counters = folded
    if world > 1:
        params = [p for p in model.parameters() if p.requires_grad]
        live = torch.tensor([1.0 if p.grad is not None else 0.0 for p in params], device=dev)
        dist.all_reduce(live, op=dist.ReduceOp.MAX)          # a rank with an empty share has no gradients at all
        keep = [p for p, l in zip(params, live.tolist()) if l > 0]
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in keep])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        for p, g in zip(keep, flat.split([p.numel() for p in keep])):
            p.grad = g.view_as(p).clone()
        dist.all_reduce(loss_sum, op=dist.ReduceOp.SUM)
    if getattr(optimizer, "trainer_owns_step", False) and hasattr(optimizer, "device_step_counter"):
        optimizer.device_step_counter(dev).add_(1)       # (the suspended pack launch would have counted this step)
    optimizer.step()
    if not drop_folded:
        DropoutStream.advance()  # device-counter mode: the tail batch and the next replay must not share dropout masks
    return loss_sum[0].detach()


def chained_fwd_bwd(model, x, y, chains: int, streams=None, loss: str = "mse", huber_delta: float = 1.0):
    """zero_grad'ed forward + loss (MSE, or ``loss``) + backward of one minibatch as ``chains`` independent micro-batch chains.

    Every kernel of this path is a 10-40 us launch whose workgroups walk load -> MFMA -> store together, so a single
    in-order chain leaves the memory system idle while the MFMA pipes run and vice versa.  The windows of a minibatch are
    independent (LayerNorm is per (b, t) slab), so the minibatch is cut into ``chains`` slices whose
    complete forward + backward run CONCURRENTLY on separate HIP streams (one fork at the start, one join at the end;
    per-chain workspaces through ``ops.chain_scope``); their parameter gradients are summed in a fixed order after the
    join, which equals the gradient of the mean loss over the whole minibatch.  ``streams[c]`` (c >= 1) are the side
    streams; ``None`` runs the chains back to back on the current stream (CPU emulator / tests).
    Sets ``p.grad`` and returns the detached mean loss."""
    from contextlib import nullcontext
    from . import ops
    check_loss(loss, huber_delta)
    F = torch.nn.functional
    loss_fn = {"mse": F.mse_loss, "mae": F.l1_loss, "huber": lambda p, t: F.huber_loss(p, t, delta=huber_delta)}[loss]
    params = [p for p in model.parameters() if p.requires_grad]
    B = len(x)
    assert chains >= 1 and B % chains == 0, f"batch {B} does not split into {chains} chains"
    Bc = B // chains
    use_streams = streams is not None and x.is_cuda and chains > 1
    main = torch.cuda.current_stream(x.device) if use_streams else None
    losses, grads = [], []
    for c in range(chains):
        s = streams[c] if (use_streams and c > 0) else None
        if s is not None:
            s.wait_stream(main)                       # fork: inputs / parameters are ready on the main stream
        with (torch.cuda.stream(s) if s is not None else nullcontext()), ops.chain_scope(c):
            xc, yc = x[c * Bc:(c + 1) * Bc], y[c * Bc:(c + 1) * Bc]
            pred = model(xc).reshape(Bc, -1)
            value = loss_fn(pred, yc) * (1.0 / chains)
            grads.append(torch.autograd.grad(value, params, allow_unused=True))
            losses.append(value.detach())
    if use_streams:
        for c in range(1, chains):
            main.wait_stream(streams[c])              # join
    live = [i for i, g in enumerate(grads[0]) if g is not None]
    acc = [grads[0][i] for i in live]
    for c in range(1, chains):
        torch._foreach_add_(acc, [grads[c][i] for i in live])
    for i, g in zip(live, acc):
        params[i].grad = g
    total = losses[0]
    for l in losses[1:]:
        total = total + l
    return total


class WindowOrder:
    """The window table of a shuffled epoch: ``order`` is a static int64 device tensor of ``usable`` window starts (the windows in whole
    global minibatches); the step at position ``pos`` reads window ``b`` from series row ``order[pos + b]`` (``ops.bind_input_index(...,
    table=order)``).  The buffer is allocated once and only ever written in place: a captured graph holds its address."""

    def __init__(self, num: int, usable: int, device, seed: int = 0):
        self.num, self.usable = int(num), int(usable)
        assert 0 < self.usable <= self.num
        self.order = torch.arange(self.usable, dtype=torch.int64, device=device)      # identity: the unshuffled epoch
        # a CPU generator: every data-parallel rank with the same seed draws the same table, no collective needed
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(int(seed))

    def set_order(self, starts) -> None:
        """``starts``: ``usable`` int64 window starts (sequence or tensor), each in [0, num - 1].  Checked on the host BEFORE anything
        is uploaded (ValueError); then written into the existing buffer on the current stream."""
        import numpy as np
        if isinstance(starts, torch.Tensor):
            if starts.dtype != torch.int64:
                raise ValueError(f"set_order: int64 window starts expected, got {starts.dtype}")
            host = starts.detach().to("cpu").reshape(-1) if starts.dim() == 1 else None
        else:
            arr = np.asarray(starts)
            if arr.dtype != np.int64:
                raise ValueError(f"set_order: int64 window starts expected, got {arr.dtype}")
            host = torch.from_numpy(np.ascontiguousarray(arr)) if arr.ndim == 1 else None
        if host is None or host.numel() != self.usable:
            raise ValueError(f"set_order: {self.usable} window starts expected (one per window of the whole global minibatches), got "
                             f"{'a non 1-D value' if host is None else host.numel()}")
        lo, hi = int(host.min()), int(host.max())
        if lo < 0 or hi > self.num - 1:
            raise ValueError(f"set_order: window starts must lie in [0, {self.num - 1}], got [{lo}, {hi}]")
        self.order.copy_(host, non_blocking=False)

    def reshuffle(self) -> None:
        """The next epoch's permutation: a draw over ALL ``num`` windows cut to whole minibatches, so that a different remainder is left
        out every epoch (``DataLoader(shuffle=True, drop_last=True)``)."""
        self.set_order(torch.randperm(self.num, generator=self.generator)[:self.usable])


class GraphedTrainStep:
    """The loop body of main.py:165-169 captured once into hipGraph(s) and replayed.

    The eager step is host-bound on MI355X (the GPU needs ~1 ms of kernels, Python + ~100 launches need
    more), so the whole step -- forward, MSE, backward, AdamW, dropout-counter bump -- is recorded with
    ``torch.cuda.graph`` and replayed with one host call.  Kernel arguments are frozen by capture, hence:
      * inputs are copied into static buffers before each replay;
      * the dropout offset comes from a device counter (``DropoutStream.use_device_counter``);
      * the optimizer is built ``capturable`` (device-side step counts).
    With world > 1 the step is split into two graphs around ONE eager RCCL all-reduce of the flat gradient
    buffer (fwd+bwd+reductions into the flat ``GradArena`` | all-reduce | AdamW).
    ``fused`` (default on, ``STGCN_FUSED_STEP=0`` disables): the step tail of ``fused_train_step``.
    """

    def __init__(self, model, optimizer, x_example: torch.Tensor, y_example: torch.Tensor, world: int = 1, warmup: int = 3,
                 chains: int = 1, fused: Optional[bool] = None, series: Optional[torch.Tensor] = None, n_his: int = 12,
                 n_pred: int = 3, rank: int = 0, capture_collective: bool = False, shuffle: bool = False, shuffle_seed: int = 0,
                 loss: str = "mse", huber_delta: float = 1.0, valid: Optional[torch.Tensor] = None):
        """``loss`` / ``huber_delta``: the loss the step trains on ("mse", "mae", "huber": ``LOSSES``), frozen into the capture like every
        other kernel argument.  An unknown name is refused here, not at the first step.

        ``valid`` (with ``series``): a (time, N) bool or uint8 tensor over the rows of ``series``, 1 = observed (``data.observed_mask``).
        The step then trains on the observed labels only: the mask stays resident beside the series and is read through the same index
        word and the same ``WindowOrder`` table as the labels, and the head's fc backward launch forms the batch's observed count from a
        per-row table built here once -- the launches of the step are those of the unmasked step.  Needs ``series=``; refused with
        ``chains > 1`` (the chained path forms its loss with torch).  Both are a ``ValueError`` here.

        ``series``: optional resident (time, N) float32 device tensor (already z-scored).  The step then takes its windows
        straight from it (device-side windowing): window b of the minibatch is rows
        [s + b, s + b + n_his) of the series (read in place through a strided view, no (num, 1, n_his, N) tensor, no per-step
        input copies), its label row s + b + n_his + n_pred - 1 (script/dataloader.py:32-47), and s advances by the global
        batch on the device every replay (unshuffled order like main.py:127, wrapping at the end of the series).  Call the
        step without arguments; ``x_example`` / ``y_example`` only give the batch size.

        ``shuffle`` (with ``series``): shuffled epochs.  The step reads window b from series row ``order[s + b]`` of a device table
        (``step.order``, int64, one entry per window of the whole global minibatches) instead of row ``s + b``; ``s`` still advances by
        the global batch on the device, rank r still reads entries ``s + r B + b``.  The first permutation is drawn before the warm-up
        steps (``torch.randperm`` over ALL windows with a CPU generator seeded ``shuffle_seed``, cut to whole minibatches: every rank
        draws the same table); ``reshuffle()`` draws the next one, ``set_order(starts)`` installs any table.  Both write the existing
        buffer in place: no re-capture, no per-step copies, the same launches.  Without ``shuffle`` no table is bound.

        ``capture_collective`` (world > 1): record the gradient all-reduce INSIDE the graph -- one graph per step (forward, backward,
        reductions, RCCL all-reduce, AdamW), no host round trip around the collective.  Only for a backend whose collectives are stream
        operations (nccl = RCCL); the caller is expected to have probed that such a capture works on this machine
        (``probe_collective_capture``: a capture that hangs instead of raising would otherwise take the run with it)."""
        from .layers import DropoutStream
        check_loss(loss, huber_delta)
        if valid is not None and series is None:
            raise ValueError("valid= needs the resident series (series=...): the mask is read through the labels' index word")
        if valid is not None and int(chains) > 1:
            raise ValueError("valid= with chains > 1 is not supported: the chained path forms its loss outside the fused head")
        assert x_example.is_cuda, "hipGraph capture needs the MI355X path"
        self.model, self.opt, self.world = model, optimizer, world
        self.loss_kind, self.huber_delta = loss, float(huber_delta)
        dev = x_example.device
        self.series, self.index, self._index_bump = series, None, None
        self.mask = None                          # ops.LossMask view over the label rows of the batch (valid=)
        self._order: Optional[WindowOrder] = None
        if shuffle and series is None:
            raise ValueError("shuffle=True needs the resident series (series=...)")
        self.chains = int(chains)                 # micro-batch chains on concurrent streams (chained_fwd_bwd)
        if fused is None:
            fused = os.environ.get("STGCN_FUSED_STEP", "1") != "0"
        # fused step tail (GradArena / GradSink): one-launch loss, one launch for all gradient reductions + AdamW
        # (decided for good after the first plain step has shown which parameters are live: fused_tail_supported)
        self.fused = bool(fused) and self.chains == 1 and hasattr(optimizer, "flush_with")
        self.arena: Optional[GradArena] = None
        self.streams = [None] + [torch.cuda.Stream(device=dev) for _ in range(self.chains - 1)]
        if series is None:
            self.x = torch.empty_like(x_example)
            self.y = torch.empty_like(y_example)
            self.x.copy_(x_example)
            self.y.copy_(y_example)
        else:
            from . import ops
            B, N = len(x_example), series.shape[1]
            assert series.is_cuda and series.dtype == torch.float32 and series.is_contiguous() and B > 1
            num = series.shape[0] - n_his - n_pred                      # windows as the reference counts them (dataloader.py:36)
            # whole global minibatches only: the reference's DataLoader(drop_last=False) also yields the partial tail batch
            # (main.py:126-131); a captured step has a fixed batch shape, so the tail (< B * world windows per epoch) is left to
            # the eager path (``train.tail_step``).  The constructor itself runs `warmup` + 1 REAL optimizer steps (capture needs
            # warmed-up allocator state): the window position after construction is (warmup + 1) * B * world.
            usable = num // (B * world) * (B * world)
            assert usable > 0, "series shorter than one global minibatch of windows"
            # a model with bf16 activations reads its windows from a bf16 copy of the series (made once; the labels stay fp32)
            cd = getattr(model, "compute_dtype", None)
            self.series_x = series if cd in (None, series.dtype) else series.to(cd)
            self.x = torch.as_strided(self.series_x, (B, 1, n_his, N), (N, n_his * N, N, 1))   # window b = rows [b, b + n_his)
            self.y = series[n_his + n_pred - 1:n_his + n_pred - 1 + B]                         # label rows, (B, N) contiguous
            self.index = torch.full((1,), rank * B, dtype=torch.int64, device=dev)             # first window of this rank
            self._index_bump = (self.index, B * world, usable)
            if shuffle:
                self._order = WindowOrder(num, usable, dev, shuffle_seed)
                self._order.reshuffle()
            table = None if self._order is None else self._order.order
            ops.bind_input_index(self.x, self.index, N, table=table)
            ops.bind_input_index(self.y, self.index, N, table=table)
            if valid is not None:
                if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != tuple(series.shape):
                    raise ValueError(f"valid: a bool / uint8 tensor of the series' shape {tuple(series.shape)} expected, got "
                                     f"{getattr(valid, 'dtype', type(valid))} {tuple(getattr(valid, 'shape', ()))}")
                self.mask_series = ops.LossMask(valid.to(dev), N)       # resident; row_valid: one int32 per series row
                self.mask = self.mask_series.rows(n_his + n_pred - 1, B)      # the rows of self.y
                self.mask.bind(self.index, N, table=table)
        if DropoutStream.counter is None or DropoutStream.counter.device != dev:
            DropoutStream.use_device_counter(dev)
        self.counter = DropoutStream.counter     # the captured kernels hold this address: keep it alive with the graph
        self.loss = None
        self.flat = None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        self.fold = False       # step counters advanced by the weight-pack launch instead of two tiny launches of their own
        with torch.cuda.stream(side):
            for i in range(max(warmup, 2 if self.fused else 1)):
                if self.fused and i > 0 and self.arena is None:
                    live = [p for p in model.parameters() if p.grad is not None]      # the first (plain) step showed them
                    if not fused_tail_supported(model, live):
                        self.fused = False
                if self.fused and i > 0:
                    if self.arena is None:
                        self.arena = GradArena([p for p in model.parameters() if p.grad is not None])
                        # the step counters ride on the weight-pack launch for every world size: with world > 1 the second graph is then
                        # exactly ONE launch (AdamW over the all-reduced arena), no add_ / remainder_ launches of the counters
                        self._try_fold_counters(dev)         # (is itself one fused training step)
                        continue
                    self._eager_fused_once()
                else:
                    self._eager_once()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if not self.fused:
            self.opt.zero_grad(set_to_none=True)
        self.capture_collective = bool(capture_collective) and world > 1
        self.g1 = torch.cuda.CUDAGraph()
        # with a process group alive its watchdog thread polls events while this thread captures: "thread_local" keeps such calls of OTHER
        # threads from invalidating the capture (the default "global" mode is for single-threaded programs)
        cap = dict(capture_error_mode="thread_local") if world > 1 else {}
        with torch.cuda.graph(self.g1, **cap):
            if self.fused:
                self.loss = self._fused_fwd_bwd()
                if world > 1:
                    self.flat = self.arena.flat
                    if self.capture_collective:      # the whole step in ONE graph: collective and optimizer follow on the capturing stream
                        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
                        self.opt.step()
                        if not self.fold:
                            DropoutStream.advance()
                            self._advance_series()
                else:
                    self.opt.flush_with(self.arena.sink, self.arena.grads, bump_step=not self.fold)
                    if not self.fold:
                        DropoutStream.advance()
                        self._advance_series()
            else:
                self.loss = self._fwd_bwd()
                if world > 1:
                    self.live = [p for p in model.parameters() if p.grad is not None]
                    self.flat = torch.cat([p.grad.reshape(-1) for p in self.live])
                    if self.capture_collective:
                        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
                        self.flat.mul_(1.0 / world)
                        torch._foreach_copy_([p.grad.reshape(-1) for p in self.live], list(self.flat.split([p.numel() for p in self.live])))
                        self.opt.step()
                        DropoutStream.advance()
                        self._advance_series()
                else:
                    self.opt.step()
                    DropoutStream.advance()
                    self._advance_series()
        self.g2 = None
        if world > 1 and not self.capture_collective:
            self.g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g2, pool=self.g1.pool(), **cap):
                if not self.fused:
                    self.flat.mul_(1.0 / world)
                    torch._foreach_copy_([p.grad.reshape(-1) for p in self.live], list(self.flat.split([p.numel() for p in self.live])))
                self.opt.step()
                if not self.fold:
                    DropoutStream.advance()
                    self._advance_series()
        # one full replay inside the constructor: a capture / replay problem surfaces here (where the caller can
        # still fall back to eager launches of the same kernels), not inside a timed loop
        self(x_example, y_example)
        torch.cuda.synchronize(dev)

    @property
    def order(self) -> Optional[torch.Tensor]:
        """The static device table of window starts (int64, one per window of the whole global minibatches); None without ``shuffle``."""
        return None if self._order is None else self._order.order

    def set_order(self, starts) -> None:
        """Install a table of window starts (``WindowOrder.set_order``: validated on the host, written in place on the current stream)."""
        if self._order is None:
            raise RuntimeError("set_order: this step was built without shuffle=True (no window table is bound)")
        self._order.set_order(starts)

    def reshuffle(self) -> None:
        """Draw the next epoch's permutation (``WindowOrder.reshuffle``); call it between epochs."""
        if self._order is None:
            raise RuntimeError("reshuffle: this step was built without shuffle=True (no window table is bound)")
        self._order.reshuffle()

    def check(self) -> None:
        """``check_in_launch_waits`` on the step's model (synchronises: for the places where the loss is read)."""
        check_in_launch_waits(self.model)

    def close(self):
        """Undo the process-global state a captured step leaves behind (device dropout counter, step counters on the model's pack
        launch, input-index bindings) so that later EAGER steps on the same model behave like clean eager steps."""
        from . import ops
        from .layers import DropoutStream
        if getattr(self.model, "_step_counters", None) is not None:
            self.model._step_counters = None
        if self.series is not None:
            ops.unbind_input_index(self.x)
            ops.unbind_input_index(self.y)
            if self.mask is not None:
                self.mask.unbind()
        if DropoutStream.counter is self.counter:
            DropoutStream.disable_device_counter()
        if hasattr(self.opt, "trainer_owns_step"):
            self.opt.trainer_owns_step = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _fwd_bwd(self):
        if self.chains > 1:
            return chained_fwd_bwd(self.model, self.x, self.y, self.chains, self.streams, self.loss_kind, self.huber_delta)
        return fwd_loss_bwd(self.model, self.x, self.y, self.loss_kind, self.huber_delta, valid=self.mask)

    def _fused_fwd_bwd(self):
        """forward, one-launch loss + gradient (carrying the 1/world of the gradient mean), backward with deferred reductions;
        with world > 1 the reductions are flushed into the flat arena here (the all-reduce follows outside the graph)."""
        from . import ops
        self.arena.install()
        with ops.grad_sink_scope(self.arena.sink):
            y_pred = self.model(self.x).reshape(len(self.x), -1)
            loss = ops.loss_backward(y_pred, self.y, self.loss_kind, self.huber_delta,
                                     grad_scale=1.0 / self.world, valid=self.mask)      # (written by the gradient flush of the step)
        if self.world > 1:
            self.arena.sink.flush(stream=torch.cuda.current_stream(self.x.device).cuda_stream)
        return loss[0]

    def _try_fold_counters(self, dev):
        """Let the model's weight-pack launch advance the dropout position and the optimizer step count; verified by one
        eager step (a model whose forward does not go through stgcn_prepack keeps the explicit bumps)."""
        from .layers import DropoutStream
        step_t = self.opt.device_step_counter(dev)
        self.model._step_counters = [(DropoutStream.counter, DropoutStream.SITE_STRIDE, 0), (step_t, 1, 0)]
        i0 = None
        if self._index_bump is not None:
            # unfolded steps advance the window position AFTER the step, the pack launch advances it BEFORE: step back once
            idx, inc, mod = self._index_bump
            i0 = int(idx.item())
            idx.sub_(inc).remainder_(mod)
            self.model._step_counters.append(self._index_bump)
        c0, s0 = int(DropoutStream.counter.item()), int(step_t.item())
        self.fold = True
        self.opt.trainer_owns_step = True       # the pack launch counts the steps: AdamW.step() must not count them again
        self._eager_fused_once()
        if int(DropoutStream.counter.item()) != c0 + DropoutStream.SITE_STRIDE or int(step_t.item()) != s0 + 1:
            self.model._step_counters = None          # the pack launch did not run: advance them the explicit way
            DropoutStream.counter.fill_(c0 + DropoutStream.SITE_STRIDE)
            step_t.fill_(s0 + 1)
            if i0 is not None:
                self._index_bump[0].fill_((i0 + self._index_bump[1]) % self._index_bump[2])
            self.fold = False
            self.opt.trainer_owns_step = False

    def _eager_fused_once(self):
        from .layers import DropoutStream
        self._fused_fwd_bwd()
        if self.world > 1:
            dist.all_reduce(self.arena.flat)
            self.opt.step()                  # (fold: the pack launch counted the step, trainer_owns_step keeps step() from counting again)
            if not self.fold:
                DropoutStream.advance()
                self._advance_series()
        else:
            self.opt.flush_with(self.arena.sink, self.arena.grads, bump_step=not self.fold)
            if not self.fold:
                DropoutStream.advance()
                self._advance_series()

    def _eager_once(self):
        from .layers import DropoutStream
        self.opt.zero_grad(set_to_none=True)
        self._fwd_bwd()
        if self.world > 1:
            live = [p for p in self.model.parameters() if p.grad is not None]
            flat = torch.cat([p.grad.reshape(-1) for p in live])
            dist.all_reduce(flat)
            flat.mul_(1.0 / self.world)
            torch._foreach_copy_([p.grad.reshape(-1) for p in live], list(flat.split([p.numel() for p in live])))
        self.opt.step()
        DropoutStream.advance()
        self._advance_series()

    def _advance_series(self):
        """the window position when no pack launch carries it (world > 1 or an unfolded step): two tiny launches"""
        if self._index_bump is not None and not self.fold:
            idx, inc, mod = self._index_bump
            idx.add_(inc).remainder_(mod)

    def __call__(self, x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.series is None:
            self.x.copy_(x, non_blocking=True)
            self.y.copy_(y, non_blocking=True)
        self.g1.replay()
        if self.g2 is not None:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.g2.replay()
        return self.loss


def _workspace_owners(model):
    from .layers import OutputBlock, STConvBlock
    return [(name or type(m).__name__, m) for name, m in model.named_modules() if isinstance(m, (STConvBlock, OutputBlock))]


class GraphedEvalPass:
    """The reference's per-epoch scoring (``evaluate_model`` + ``evaluate_metric``, script/utility.py:90-121; main.py:173, :184-203) as
    hipGraph replays over a split that stays on the device: one batch = the model's eval-mode forward on the strided in-place view of the
    series + ONE ``stgcn_eval_accumulate`` launch that adds the batch into a device-resident fp64 state and moves the position words on
    to the next batch.  ``run()`` = arm, ``ceil(num / B)`` replays, one synchronise, one 40-byte copy -- instead of a gather, ~7 launches
    from Python and a host synchronisation per batch.

    ``series``: the z-scored (rows, N) split (numpy or tensor); ``num = rows - n_his - n_pred`` windows as the reference counts them
    (script/dataloader.py:36).  ``scaler``: a fitted ``data.ZScore`` (``scale_`` / ``mean_``) for MAE / RMSE / WMAPE in the data's units,
    None = the identity.  Ragged tail: batch k starts at window ``min(k B, num - B)`` and counts only the windows from ``k B`` on, so
    the last batch overlaps its predecessor instead of reading past the series, with ONE graph (LayerNorm is per (b, t) slab: a
    window's prediction does not depend on the batch that carries it).  ``num < B`` raises ValueError (``data.evaluate_*`` serve such splits).
    ``capture=False`` runs the identical launches eagerly (CPU emulator; also the fallback when capture raises).

    Beside a live ``GraphedTrainStep`` on the same model, in either construction order: the pass touches neither the dropout counter nor the
    optimizer's step counter nor ``model._step_counters`` (an eval-mode forward hands no counters to the pack launch), and its position
    words are its own.  A captured graph holds the addresses of the model's workspaces, which ``ops.WorkspaceCache`` reallocates when a
    plan grows: the constructor refuses (RuntimeError, before anything moved) if its forward would grow an existing workspace, and holds
    on to the buffers its own graph uses.  ``close()`` / the context manager drop the index bindings.

    ``valid``: a (rows, N) bool / uint8 array or tensor over ``series``, 1 = observed.  The pass then scores the observed labels only
    (``stgcn_eval_accumulate_masked``, still one launch per batch) and ``run()`` also returns "mape" and "elements" (observed)."""

    def __init__(self, model, series, n_his: int, n_pred: int, batch_size: int, scaler=None, capture: bool = True, valid=None):
        import numpy as np
        from . import _lib, ops
        self.model, self.B, self.n_his, self.n_pred = model, int(batch_size), int(n_his), int(n_pred)
        emu = _lib.lib().is_emulator
        dev = next(model.parameters()).device
        if not torch.is_tensor(series):
            series = torch.as_tensor(np.asarray(series, dtype=np.float32))
        self.series = series.detach().to(device=dev, dtype=torch.float32).contiguous()
        if self.series.dim() != 2:
            raise ValueError(f"GraphedEvalPass: series must be (rows, N), got {tuple(self.series.shape)}")
        rows, N = self.series.shape
        B = self.B
        self.num = int(rows) - self.n_his - self.n_pred
        if B < 1 or self.num < B:
            raise ValueError(f"GraphedEvalPass: the split has {self.num} windows, fewer than one batch of {B} "
                             f"(use data.evaluate_model / data.evaluate_metric for it)")
        self.batches = (self.num + B - 1) // B
        cd = getattr(model, "compute_dtype", None)
        # a model with bf16 activations reads its windows from a bf16 copy of the series (made once; labels and metrics stay fp32)
        self.series_x = self.series if cd in (None, self.series.dtype) else self.series.to(cd)
        self.x = torch.as_strided(self.series_x, (B, 1, self.n_his, N), (N, self.n_his * N, N, 1))     # window b = rows [b, b + n_his)
        self.y = self.series[self.n_his + self.n_pred - 1:self.n_his + self.n_pred - 1 + B]            # label rows of windows 0 .. B-1
        self.valid = self.valid_y = None
        if valid is not None:
            v = valid if torch.is_tensor(valid) else torch.as_tensor(np.asarray(valid))
            if v.dtype not in (torch.bool, torch.uint8) or tuple(v.shape) != tuple(self.series.shape):
                raise ValueError(f"GraphedEvalPass: valid must be a bool / uint8 mask of the series' shape {tuple(self.series.shape)}, got "
                                 f"{v.dtype} {tuple(v.shape)}")
            self.valid = v.detach().to(dev).contiguous().view(torch.uint8) if v.dtype == torch.bool else v.detach().to(dev).contiguous()
            self.valid_y = self.valid[self.n_his + self.n_pred - 1:self.n_his + self.n_pred - 1 + B]      # beside self.y, moved by pos like it
        self.state, self.pos = ops.eval_state(dev, masked=self.valid is not None)
        self.scale = self.mean = None
        if scaler is not None:
            self.scale = torch.as_tensor(np.asarray(scaler.scale_, dtype=np.float32).reshape(-1)).to(dev).contiguous()
            self.mean = torch.as_tensor(np.asarray(scaler.mean_, dtype=np.float32).reshape(-1)).to(dev).contiguous()
            if self.scale.numel() != N or self.mean.numel() != N:
                raise ValueError(f"GraphedEvalPass: the scaler describes {self.scale.numel()} columns, the series has {N}")
        self._refuse_workspace_growth(ops, B, cd or torch.float32)
        before = {name: {c: b.data_ptr() for c, b in m._ws.bufs.items()} for name, m in _workspace_owners(model)}
        self.index = self.pos[0:1]                   # first window of the batch: the forward's input and the labels move with it
        ops.bind_input_index(self.x, self.index, N)
        self.graph = None
        was_training = model.training
        model.eval()
        try:
            use_graph = bool(capture) and not emu and self.series.is_cuda
            ops.eval_arm(self.state, self.pos)
            if use_graph:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self._batch()                    # warm-up: allocator state, workspaces, operator caches
                    self._batch()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
            else:
                self._batch()
            moved = [f"{name} (chain {c})" for name, m in _workspace_owners(model) for c, p in before[name].items()
                     if m._ws.bufs[c].data_ptr() != p]
            if moved:
                raise RuntimeError(f"GraphedEvalPass: the workspace of {', '.join(moved)} was reallocated by the evaluation forward at batch size "
                                   f"{B}; a captured training step still holds the old address.  Build the evaluation pass before the "
                                   f"training step, or use a batch size no larger than the training step's")
            # the buffers this pass's graph reads and writes stay alive with it, whatever a later, larger plan does to the caches
            self._ws_keep = [b for _, m in _workspace_owners(model) for b in m._ws.bufs.values()]
            if use_graph:
                try:
                    g = torch.cuda.CUDAGraph()
                    cap = dict(capture_error_mode="thread_local") if (dist.is_available() and dist.is_initialized()) else {}
                    with torch.cuda.graph(g, **cap):
                        self._batch()
                    ops.eval_arm(self.state, self.pos)
                    g.replay()                       # a capture / replay problem surfaces here, not inside an epoch
                    torch.cuda.synchronize(dev)
                    self.graph = g
                except Exception as e:  # noqa: BLE001 -- the same launches run eagerly instead
                    import warnings
                    warnings.warn(f"GraphedEvalPass: hipGraph capture failed ({e!r}); running the batches eagerly")
                    torch.cuda.synchronize(dev)
                    self.graph = None
        except BaseException:
            ops.unbind_input_index(self.x)
            raise
        finally:
            model.train(was_training)

    def _refuse_workspace_growth(self, ops, B, dtype):
        """Raise before anything is reallocated if this pass's forward needs more workspace than a module already owns."""
        from .layers import STConvBlock
        T = self.n_his
        for name, m in _workspace_owners(self.model):
            if isinstance(m, STConvBlock):
                need = max(ops.query_plan(ops.make_desc(m.cfg, B, T, tr, tr, dtype=dtype)).ws_floats for tr in (True, False))
                T -= 2 * (m.cfg.Kt - 1)
            elif ops.head_supported(m.cfg):
                need = max(ops.query_head_plan(ops.make_head_desc(m.cfg, B, T, tr, tr, dtype=dtype)).ws_floats for tr in (True, False))
            else:
                continue
            have = m._ws.bufs.get(0)
            if have is not None and have.numel() < need:
                raise RuntimeError(f"GraphedEvalPass: the evaluation forward at batch size {B} needs {need} workspace floats in {name}, which "
                                   f"owns {have.numel()}: its workspace would grow and move under a captured training step.  Build the "
                                   f"evaluation pass before the training step, or use a batch size no larger than the training step's")

    def _batch(self):
        from . import ops
        with torch.no_grad():
            pred = self.model(self.x).reshape(self.B, -1)
            if pred.dtype != torch.float32 or not pred.is_contiguous():
                pred = pred.float().contiguous()
            ops.eval_accumulate(pred, self.y, self.state, self.scale, self.mean, pos=self.pos, num_windows=self.num, valid=self.valid_y)

    def run(self) -> dict:
        """One pass over the split: {"mse", "mae", "rmse", "wmape"} as the reference defines them (floats) and "windows" (int).  With
        ``valid``: the same over the observed labels, plus "mape", "elements" (observed labels) and "windows" (all scored windows)."""
        from . import ops
        model = self.model
        was_training = model.training
        model.eval()
        try:
            ops.eval_arm(self.state, self.pos)
            if self.graph is not None:
                for _ in range(self.batches):
                    self.graph.replay()
            else:
                for _ in range(self.batches):
                    self._batch()
            words = self.state[:5 if self.valid is None else 6].cpu()      # the pass's one synchronisation and one device-to-host copy
        finally:
            model.train(was_training)
        check_in_launch_waits(model)                 # (where the numbers are read)
        m = ops.eval_metrics(words.tolist())
        if self.valid is not None:
            m["windows"] = self.num
            return m
        n = m.pop("elements")
        m["windows"] = n // self.series.shape[1]
        return m

    def close(self):
        """Drop the input-index binding of the pass's window view (its graph must not be replayed afterwards)."""
        from . import ops
        ops.unbind_input_index(self.x)
        self.graph = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
