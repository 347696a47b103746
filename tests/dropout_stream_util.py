"""Shared pieces of the dropout-stream tests (tests/test_emu_dropout_stream.py on the emulator, tests/test_gpu_dropout_stream.py on the
GPU): the generator grid, the positions every dropout site of the tiny_cheb_f32 model draws at, and the training step with dropout on
against the float64 oracle fed with masks from the independent Philox of tests/philox_ref.py.

A block's dropped pattern is read off its output: an element was dropped iff it is -0.0 (drop_encode), fp32 and bf16 alike.  The head's
mask is not visible in its output; the oracle trajectories cover it (and every backward consumer of a mask).

Not covered: element indices above 2^34, where the counter's second word (q hi) is nonzero -- a mask that large does not fit in a test.
"""
import dataclasses

import numpy as np
import torch

from oracle import stgcn_oracle as orc
from tests import philox_ref as ref
from tests.helpers import cfg_from_fixture, fixture_gso, fixture_params, load_fixture, maxabs

# ---- the generator grid (section "generator against the reference") ------------------------------------------------------------
GRID_N = (4, 4 * 255, 4 * 256, 4 * 257, 1 << 16)          # 256 threads x 4 elements per workgroup: the last one full, partial, absent
GRID_P = (0.0, 1e-6, 0.1, 0.3, 0.5, 0.9, 0.999)
GRID_SEEDS = (0, 0x5EED5EED, 0xFEDCBA9876543210)
GRID_OFFSETS = (0, 1, (7 << 32) + (3 << 20) + 5, 2 ** 64 - 1)
# (host offset o, device counter c): the mask equals the one at host offset (o + c) mod 2^64
COUNTER_CASES = ((5, 3 << 20), (0xFFFFFFF0, 0x20), ((1 << 32) - 1, 1), ((7 << 32) + 9, (1 << 40) + (1 << 20)), (2 ** 64 - 1, 2))
BAD_DROPRATES = (1.0, 1.5, -0.25, float("inf"), float("nan"))

# ---- bars of the droprate-0 trajectory (test_training_trajectory_matches_oracle, README) -----------------------------------------
LOSS_RTOL, PARAM_ATOL, GRAD_RTOL = 1e-4, 1e-4, 1e-4
FIXTURE = "tiny_cheb_f32"
SEED = 0x1234_5678_9ABC          # (a seed with its high word set)


def bind(dev):
    from tests.block_util import bind as b
    return b(dev)


def expected_scale(n, p, seed, offset):
    """what ops.dropout_mask must return, bit for bit: 0 or float32(1) / (float32(1) - float32(p))"""
    _, keep = ref.keep_mask(n, p, seed, offset)
    return np.where(keep, ref.keep_scale(p), np.float32(0.0)).astype(np.float32)


def check_generator_grid(dev, n):
    from stgcn_amd import ops
    for p in GRID_P:
        for seed in GRID_SEEDS:
            for off in GRID_OFFSETS:
                got = ops.dropout_mask(n, p, seed, off, torch.device(dev)).cpu().numpy()
                want = expected_scale(n, p, seed, off)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, p, hex(seed), hex(off))


def check_device_counter(dev):
    from stgcn_amd import ops
    n = 4 * 257
    for o, c in COUNTER_CASES:
        cnt = torch.tensor([c], dtype=torch.int64, device=dev)
        for p, seed in ((0.5, 0x5EED5EED), (0.3, 0xFEDCBA9876543210)):
            got = ops.dropout_mask(n, p, seed, o, torch.device(dev), offset_dev=cnt).cpu().numpy()
            assert np.array_equal(got, expected_scale(n, p, seed, (o + c) % 2 ** 64)), (hex(o), hex(c))
            assert np.array_equal(got, ops.dropout_mask(n, p, seed, (o + c) % 2 ** 64, torch.device(dev)).cpu().numpy())
        assert int(cnt.item()) == c       # (read, never written)


def check_refusals(dev):
    """droprate outside [0, 1), NaN included: ValueError (STGCN_ERR_INVALID) from the mask entry point and from the three descriptors."""
    import pytest
    from stgcn_amd import ops
    bcfg = ops.BlockConfig(Kt=3, Ks=3, n_vertex=20, c_in=1, channels=(64, 16, 64), act_func="glu", graph_conv_type="cheb_graph_conv", droprate=0.5)
    hcfg = ops.HeadConfig(Ko=4, n_vertex=20, c_in=64, channels=(128, 128), end_channel=1, act_func="glu", droprate=0.5)
    ops.query_plan(ops.make_desc(bcfg, 2, 12, True, True))
    ops.query_head_plan(ops.make_head_desc(hcfg, 2, 4, True, True))
    for p in BAD_DROPRATES:
        with pytest.raises(ValueError, match="droprate"):
            ops.dropout_mask(8, p, 1, 0, torch.device(dev))
        with pytest.raises(ValueError, match="droprate"):
            ops.query_plan(ops.make_desc(dataclasses.replace(bcfg, droprate=p), 2, 12, True, True))
        with pytest.raises(ValueError, match="droprate"):
            ops.query_head_plan(ops.make_head_desc(dataclasses.replace(hcfg, droprate=p), 2, 4, True, True))
    # the largest float32 below 1 is a droprate like any other
    top = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    got = ops.dropout_mask(1024, top, 1, 0, torch.device(dev)).cpu().numpy()
    assert np.array_equal(got, expected_scale(1024, top, 1, 0))


# ---- the model and where its sites draw ----------------------------------------------------------------------------------------------
def fresh_model(dev, p, dtype=torch.float32, counter=False, seed=SEED):
    """tiny_cheb_f32's model with droprate p and sites 1, 2 (blocks), 3 (head); the stream seeded; device-counter mode on request."""
    from stgcn_amd import DropoutStream
    from tests.optim_kinds_util import tiny_model
    bind(dev)
    DropoutStream._sites = 0
    if counter:
        DropoutStream.use_device_counter(torch.device(dev))
    else:
        DropoutStream.disable_device_counter()
    DropoutStream.manual_seed(seed)
    m, x, y = tiny_model(dev, droprate=p)
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    assert [b._site for b in m.st_blocks] == [1, 2] and m.output._site == 3
    return m, x, y


def batch(dev, B, seed):
    """a batch of the tiny model's shapes with B windows"""
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((B, 1, 12, 20))).float().to(dev), torch.from_numpy(rs.standard_normal((B, 20))).float().to(dev)


class BlockOutputs:
    """forward hooks on the ST blocks: ``calls`` is the list of (block index, output tensor) in call order (detached views of the outputs
    themselves: a captured step's static outputs can be read again after every replay, and no autograd graph outlives its step)"""

    def __init__(self, model):
        self.calls = []
        self.hooks = [b.register_forward_hook(lambda mod, i, o, l=l: self.calls.append((l, o.detach()))) for l, b in enumerate(model.st_blocks)]

    def take(self):
        out, self.calls = self.calls, []
        return out

    def remove(self):
        for h in self.hooks:
            h.remove()


def dropped(out):
    """bool [B][T][N][C]: the elements of a block output (logical (B, C, T, N), fp32 or bf16) that are -0.0"""
    o = out.detach().permute(0, 2, 3, 1).float().cpu().contiguous()
    return ((o == 0) & torch.signbit(o)).numpy()


def expected_dropped(shape_cl, p, seed, position):
    _, keep = ref.keep_mask(int(np.prod(shape_cl)), p, seed, position)
    return ~keep.reshape(shape_cl)


def assert_pattern(out, p, position, what=""):
    from stgcn_amd import DropoutStream
    got = dropped(out)
    want = expected_dropped(got.shape, p, DropoutStream.seed, position)
    assert np.array_equal(got, want), f"{what}: the pattern is not the reference's at position {position} ({(got != want).mean():.3f} of the elements differ)"


def assert_calls(calls, p, positions, what=""):
    """``calls`` of one forward per chain: call j is block j % 2 of chain j // 2; positions[chain][block]"""
    assert len(calls) == 2 * len(positions), (what, len(calls))
    for j, (l, out) in enumerate(calls):
        assert l == j % 2
        assert_pattern(out, p, positions[j // 2][l], f"{what} chain {j // 2} block {l}")


def counter_value():
    from stgcn_amd import DropoutStream
    return int(DropoutStream.counter.item())


# ---- the oracle with the reference's masks ----------------------------------------------------------------------------------------------
SITE_SHAPES = ((8, 20, 64), (4, 20, 64), (1, 20, 128))      # channels-last (T, N, C) of the two block outputs and of the head's fc1 output


def oracle_masks(B, p, seed, positions, chains=1):
    """keep masks of one step for oracle.stgcn_oracle: ``positions`` of (block 0, block 1, head) for chain 0; chain c draws at
    + CHAIN_STRIDE * c with its element index restarting (the whole-batch mask is the concatenation)."""
    from stgcn_amd import DropoutStream
    Bc = B // chains
    masks = []
    for k, shape in enumerate(SITE_SHAPES):
        parts = [ref.keep_mask(Bc * int(np.prod(shape)), p, seed, positions[k] + DropoutStream.CHAIN_STRIDE * c)[1].reshape((Bc,) + shape)
                 for c in range(chains)]
        m = torch.from_numpy(np.concatenate(parts))
        masks.append(m.permute(0, 3, 1, 2) if k < 2 else m)      # blocks: (B, C, T, N); head: (B, 1, N, channels[1])
    return masks


def oracle_trajectory(dtype, p, seed, steps, chains=1):
    """``steps``: [(x, y, positions of block 0, block 1 and the head)].  AdamW at the trainer's defaults.  Returns (losses, gradients of step 1, final parameters)."""
    fx = load_fixture(FIXTURE)
    cfg = dataclasses.replace(cfg_from_fixture(fx), droprate=float(np.float32(p)))
    params = fixture_params(fx, cfg, dtype)
    gso = torch.from_numpy(fixture_gso(FIXTURE, fx)).to(dtype)
    state, losses, first = {}, [], None
    for x, y, positions in steps:
        km = oracle_masks(len(x), p, seed, positions, chains)
        loss, grads = orc.train_step(x.detach().cpu().to(dtype), y.detach().cpu().to(dtype), gso, params, cfg, state, km)
        losses.append(float(loss))
        if first is None:
            first = grads
    return losses, first, params


def figures(losses, grads, params, o_losses, o_grads, o_params):
    """worst relative loss error, worst gradient error relative to its tensor's max abs, worst absolute parameter error"""
    f = {"loss": max(abs(a - b) / abs(b) for a, b in zip(losses, o_losses) if a is not None), "grad": None, "param": 0.0}
    if grads is not None:
        n, f["grad"] = 0, 0.0
        for k, g in o_grads.items():
            assert (g is None) == (grads.get(k) is None), k
            if g is not None:
                f["grad"] = max(f["grad"], maxabs(grads[k], g.numpy()) / float(g.abs().max()))
                n += 1
        assert n == 28
    for k, v in o_params.items():
        f["param"] = max(f["param"], maxabs(params[k], v.numpy()))
    return f


def compare_with_oracle(name, p, seed, steps, losses, grads, params, chains=1, report=None):
    """The bars, against the float64 oracle; the float32 oracle's own distance is measured beside it.  ``grads``: {name: array or None} of
    step 1, or None where a trainer never exposes them; a loss of None: a step whose loss the trainer never hands out."""
    o64 = oracle_trajectory(torch.float64, p, seed, steps, chains)
    o32 = oracle_trajectory(torch.float32, p, seed, steps, chains)
    got = figures(losses, grads, params, *o64)
    own = figures(o32[0], None if grads is None else {k: (None if g is None else g.numpy()) for k, g in o32[1].items()},
                  {k: v.numpy() for k, v in o32[2].items()}, *o64)
    e = lambda v: "not exposed" if v is None else f"{v:.2e}"
    print(f"dropout step errors | {name} | p={p} | loss {e(got['loss'])} (f32 oracle {e(own['loss'])}) | grad {e(got['grad'])} "
          f"({e(own['grad'])}) | param {e(got['param'])} ({e(own['param'])})")
    if report is not None:
        report.append({"case": name, "p": p, "got": got, "f32_oracle": own})
    for key, bar in (("loss", LOSS_RTOL), ("grad", GRAD_RTOL), ("param", PARAM_ATOL)):
        if got[key] is None:
            continue
        # a case is fit to judge the kernels only where the reference's own float32 evaluation sits well inside the bar
        assert own[key] <= bar / 4, ("ill-conditioned case", name, key, own)
        assert got[key] <= bar, (name, key, got, own)
    return got, own


def model_grads(model):
    return {k: (None if q.grad is None else q.grad.detach().cpu().numpy().copy()) for k, q in model.named_parameters()}


def model_params(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


# ---- scenarios both suites run: every one pins the block patterns of each step AND follows the step with the oracle ---------------------
def run_positions_only(dev, p, dtype):
    """Patterns alone (bf16: the arithmetic has its own stage tests): three forwards without a counter -- site k of forward f at
    3 f + k + 1 --, then two train_steps in device-counter mode -- site + counter before the step."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import make_optimizer, train_step
    m, x, y = fresh_model(dev, p, dtype)
    rec = BlockOutputs(m)
    with torch.no_grad():
        for f in range(3):
            m(x)
            assert_calls(rec.take(), p, [[3 * f + 1, 3 * f + 2]], f"forward {f}")
    DropoutStream.use_device_counter(torch.device(dev))
    try:
        DropoutStream.manual_seed(SEED)
        opt = make_optimizer(m)
        for s in range(2):
            c = counter_value()
            assert c == s * DropoutStream.SITE_STRIDE
            train_step(m, opt, x, y)
            assert_calls(rec.take(), p, [[b._site + c for b in m.st_blocks]], f"step {s}")
    finally:
        rec.remove()
        DropoutStream.disable_device_counter()


def run_chains_without_counter(dev, p):
    """chained_fwd_bwd without a device counter: every forward of every chain takes the next host offsets"""
    from stgcn_amd.train import chained_fwd_bwd
    m, x, y = fresh_model(dev, p)
    rec = BlockOutputs(m)
    chained_fwd_bwd(m, x, y, chains=2, streams=None)
    calls = rec.take()
    rec.remove()
    assert all(o.shape[0] == len(x) // 2 for _, o in calls)
    assert_calls(calls, p, [[1, 2], [4, 5]], "no counter")


def run_eager_trajectory(dev, p, n_steps=3, report=None, name="eager"):
    """``n_steps`` train_steps with AdamW, no counter: site k of forward f at 3 f + k + 1"""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import make_optimizer, train_step
    m, x, y = fresh_model(dev, p)
    opt = make_optimizer(m)
    rec = BlockOutputs(m)
    losses, grads = [], None
    for f in range(n_steps):
        losses.append(float(train_step(m, opt, x, y)))
        assert_calls(rec.take(), p, [[3 * f + 1, 3 * f + 2]], f"step {f}")
        if grads is None:
            grads = model_grads(m)
    rec.remove()
    steps = [(x, y, [3 * f + 1, 3 * f + 2, 3 * f + 3]) for f in range(n_steps)]
    return compare_with_oracle(name, p, DropoutStream.seed, steps, losses, grads, model_params(m), report=report)


def run_counter_trajectory(dev, p, chains=1, report=None):
    """Three steps in device-counter mode (train_step; with two chains chained_fwd_bwd + optimizer step + advance): site + counter before
    the step, chain c at + CHAIN_STRIDE c with its element index restarting; the counter grows by SITE_STRIDE per step."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import chained_fwd_bwd, make_optimizer, train_step
    S, CS = DropoutStream.SITE_STRIDE, DropoutStream.CHAIN_STRIDE
    m, x, y = fresh_model(dev, p, counter=True)
    try:
        opt = make_optimizer(m)
        rec = BlockOutputs(m)
        losses, grads = [], None
        for f in range(3):
            c = counter_value()
            assert c == f * S
            if chains == 1:
                losses.append(float(train_step(m, opt, x, y)))
            else:
                opt.zero_grad(set_to_none=True)
                losses.append(float(chained_fwd_bwd(m, x, y, chains=chains, streams=None)))
                opt.step()
                DropoutStream.advance()
            calls = rec.take()
            assert all(o.shape[0] == len(x) // chains for _, o in calls)
            assert_calls(calls, p, [[b._site + CS * ch + c for b in m.st_blocks] for ch in range(chains)], f"step {f}")
            if grads is None:
                grads = model_grads(m)
        rec.remove()
        steps = [(x, y, [1 + f * S, 2 + f * S, 3 + f * S]) for f in range(3)]
        return compare_with_oracle(f"counter, chains={chains}", p, DropoutStream.seed, steps, losses, grads, model_params(m), chains=chains,
                                   report=report)
    finally:
        DropoutStream.disable_device_counter()


def run_folded_trajectory(dev, p, report=None):
    """The counter on the weight-pack launch, as a captured step with ``fold`` has it, in eager launches (``fused_train_step``): a plain
    step (counter 0), two folded steps, a tail batch of one window, one more folded step.  Every site of a folded step sees the counter
    AFTER the bump (forward by the pattern, backward by the oracle); the tail batch draws at the next position, the step after it at the
    one after that: 0, 2 S, 3 S, 4 S (tail), 5 S."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, tail_step, train_step
    S = DropoutStream.SITE_STRIDE
    m, x, y = fresh_model(dev, p, counter=True)
    xt, yt = batch(dev, 1, 11)
    try:
        opt = make_optimizer(m)
        rec = BlockOutputs(m)
        losses = [float(train_step(m, opt, x, y))]
        assert_calls(rec.take(), p, [[b._site for b in m.st_blocks]], "plain step")
        grads = model_grads(m)
        arena = GradArena([q for q in m.parameters() if q.grad is not None])
        m._step_counters = [(DropoutStream.counter, S, 0)]
        seen = [0]
        for what, xb, yb in (("folded step 1", x, y), ("folded step 2", x, y), ("tail batch", xt, yt), ("step after the tail batch", x, y)):
            c = counter_value()
            if what == "tail batch":
                losses.append(float(tail_step(m, opt, xb, yb)))
                assert m._step_counters is not None
            else:
                losses.append(float(fused_train_step(m, opt, xb, yb, arena)))
            assert counter_value() == c + S, what
            assert_calls(rec.take(), p, [[b._site + c + S for b in m.st_blocks]], what)
            seen.append(c + S)
        rec.remove()
        assert seen == [0, 2 * S, 3 * S, 4 * S, 5 * S]
        steps = [(xb, yb, [1 + k, 2 + k, 3 + k]) for (xb, yb), k in zip(((x, y), (x, y), (x, y), (xt, yt), (x, y)), seen)]
        return compare_with_oracle("folded counter + tail batch", p, DropoutStream.seed, steps, losses, grads, model_params(m), report=report)
    finally:
        m._step_counters = None
        DropoutStream.disable_device_counter()


def run_tail_unfolded(dev, p):
    """train_step, train_step, tail_step on 1 window, train_step: the tail draws at the current counter, the next step SITE_STRIDE on"""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import make_optimizer, tail_step, train_step
    S = DropoutStream.SITE_STRIDE
    m, x, y = fresh_model(dev, p, counter=True)
    xt, yt = batch(dev, 1, 11)
    try:
        opt = make_optimizer(m)
        rec = BlockOutputs(m)
        for s, (fn, xb, yb) in enumerate([(train_step, x, y), (tail_step, xt, yt), (train_step, x, y)]):
            assert counter_value() == s * S
            fn(m, opt, xb, yb)
            assert_calls(rec.take(), p, [[b._site + s * S for b in m.st_blocks]], f"step {s}")
        rec.remove()
    finally:
        DropoutStream.disable_device_counter()


def run_captured(dev, shuffle=False, report=None):
    """``GraphedTrainStep`` at p = 0.5, B = 8, warmup = 2: construction, two replays, a tail batch of 3 windows, one more replay.  The block
    patterns of the captured step's static outputs after construction and after every replay, the tail batch's patterns, the counter, and
    the whole trajectory (constructor steps included) against the oracle.

    Positions.  The step is fused and its counter rides on the weight-pack launch (``fold``): the constructor's plain first step draws at
    counter 0, every later step at the counter AFTER the pack launch's bump -- 2 S, 3 S (the verification replay), then 4 S, 5 S, 6 S (the
    tail batch, which advances before its forward in this mode), 7 S.  ``shuffle``: the resident-series form, windows read through
    ``step.order`` at positions 0, B, 2 B | 3 B, 4 B, 0.

    Not here: the captured step with two micro-batch chains.  At these shapes with dropout on its capture ended in a segmentation fault inside
    the runtime's end-of-capture call on the MI355X, before any check of this file ran; the cause is not known, so the case is left out
    (the chain positions are pinned in eager launches, run_counter_trajectory)."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedTrainStep, make_optimizer, tail_step
    p, B, W, n_his, n_pred = 0.5, 8, 2, 12, 3
    S = DropoutStream.SITE_STRIDE
    m, _, _ = fresh_model(dev, p, counter=True)
    batches = [batch(dev, B, 20 + i) for i in range(4)]
    xt, yt = batch(dev, 3, 31)
    # The series' seed: one at which the float32 ORACLE stays within 1e-5 of the float64 one over these seven steps.  At seeds 7, 8 and 11 it
    # is 1.0e-4 .. 1.6e-4 away, all of it in one element of output.fc1.weight whose first-step gradient is of the order of AdamW's eps = 1e-8:
    # its first update is lr g / (|g| + eps) instead of +- lr, which no fp32 evaluation of g pins to the 1e-4 bar (compare_with_oracle
    # refuses such data instead of judging the kernels by it).
    series = torch.from_numpy(np.random.RandomState(10).standard_normal((5 * B + n_his + n_pred, 20))).float().to(dev) if shuffle else None
    opt = make_optimizer(m, capturable=True)
    rec = BlockOutputs(m)
    kw = dict(series=series, n_his=n_his, n_pred=n_pred, shuffle=True, shuffle_seed=5) if shuffle else {}
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=W, **kw)
    try:
        static = rec.take()[-2:]              # the hook calls of the capture itself: the step's static block outputs
        assert gs.fold, "the pack launch should carry the counter"
        pos = lambda c: [[b._site + c for b in m.st_blocks]]
        assert counter_value() == (W + 1) * S
        built = [0, 2 * S, 3 * S]
        assert_calls(static, p, pos(built[-1]), "after construction")
        if shuffle:
            order = gs.order.cpu().tolist()

            def windows(k):
                starts = order[(k * B) % len(order):(k * B) % len(order) + B]
                return (torch.stack([series[s:s + n_his] for s in starts]).unsqueeze(1), torch.stack([series[s + n_his + n_pred - 1] for s in starts]))
            data = [windows(k) for k in range(6)]
        else:
            data = [batches[0]] * 3 + batches[1:]
        steps = [(*data[k], [1 + c, 2 + c, 3 + c]) for k, c in enumerate(built)]
        losses = [None, None, float(gs.loss)]
        k = 3
        for what in ("replay 1", "replay 2", "tail batch", "replay 3"):
            c = counter_value()
            if what == "tail batch":
                losses.append(float(tail_step(m, opt, xt, yt)))
                c += S
                assert_calls(rec.take(), p, pos(c), what)
                steps.append((xt, yt, [1 + c, 2 + c, 3 + c]))
            else:
                losses.append(float(gs() if shuffle else gs(*data[k])))
                torch.cuda.synchronize()
                c += S
                assert_calls(static, p, pos(c), what)
                assert not rec.take()                  # (a replay runs no Python)
                steps.append((*data[k], [1 + c, 2 + c, 3 + c]))
                k += 1
            assert counter_value() == (len(steps)) * S, what       # one position per step, whoever advanced it
        taken = [s[2][0] - 1 for s in steps]
        assert len(set(taken)) == len(taken) and taken == sorted(taken)      # consecutive steps and the tail batch at distinct positions
        rec.remove()
        name = "captured, shuffled series" if shuffle else "captured"
        return compare_with_oracle(name, p, DropoutStream.seed, steps, losses, None, model_params(m), report=report)
    finally:
        gs.close()
        DropoutStream.disable_device_counter()
