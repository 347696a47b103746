"""-m gpu: the masked loss and metrics (train and score on observed readings only) on the MI355X: the stand-alone launch
(stgcn_loss_grad_masked), the fused head backward (stgcn_outblock_backward_loss_masked, fp32 and bf16), the trainers, the captured step
on a resident series with a resident mask, the evaluation launch (stgcn_eval_accumulate_masked) and the captured evaluation pass.  The
cases, inputs and bars: tests/masked_loss_util.py."""
import numpy as np
import pytest
import torch

from tests import loss_kinds_util as LK
from tests import masked_loss_util as U
from tests.masked_loss_util import BIG, DELTA, KINDS, SINGLE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("kind", KINDS)
def test_standalone_masked_loss_matches_torch_float64(kind):
    U.check_standalone_matches_torch(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_mask_is_bitwise_the_unmasked_entry_and_all_zero_gives_zero(kind):
    U.check_all_ones_is_the_unmasked_entry(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_labels_and_mask_from_a_resident_series_equal_the_gather(kind):
    U.check_resident_series_equals_gather(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_masked_loss_equals_the_two_call_path(kind):
    U.check_fused_equals_two_call(DEV, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_bf16_model_fused_masked_loss_equals_the_two_call_path(kind):
    """One step of a bf16 model (the C2-shaped head of tests/test_gpu_graph.py: its bf16 backward is dense, not refused)."""
    from tests.test_gpu_graph import _make
    m = _make(0.0).set_compute_dtype(torch.bfloat16)
    m.train()
    x = torch.randn(4, 1, 12, 207, generator=torch.Generator().manual_seed(8)).to(DEV)
    U.check_fused_equals_two_call(DEV, kind, (m, x, LK.target_from_own_prediction(m, x)))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["mae", "huber"])
def test_masked_training_trajectory_matches_oracle(kind, fused):
    U.check_model_trajectory(DEV, kind, fused)


def test_tail_step_takes_the_mask_for_one_rank_only():
    U.check_tail_step(DEV, "mae")


# ---- the captured step on the resident series: a batch of 4 windows on the tiny fixture graph, the mask resident beside the series ---
B, N_PRED, BATCHES, REPLAYS, WARMUP = 4, 3, 5, 4, 2


def _series_and_mask(N, n_his):
    g = torch.Generator().manual_seed(6)
    series = torch.randn(BATCHES * B + n_his + N_PRED, N, generator=g).to(DEV)
    valid = (torch.rand(series.shape, generator=g) >= 0.3).to(DEV)
    return series, valid


def _captured(kind, shuffle, masked=True, on_step=None):
    """(replay losses, state_dict, (series, valid, window table, n_his)) of GraphedTrainStep(series=, valid=)."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedTrainStep, make_optimizer
    m, x = LK.tiny_model(DEV)
    n_his, N = x.shape[2], x.shape[3]
    series, valid = _series_and_mask(N, n_his)
    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    try:
        o = make_optimizer(m, capturable=True)
        x0 = torch.stack([series[s:s + n_his] for s in range(B)]).unsqueeze(1).contiguous()
        y0 = series[n_his + N_PRED - 1:n_his + N_PRED - 1 + B].contiguous()
        gs = GraphedTrainStep(m, o, x0, y0, warmup=WARMUP, series=series, n_his=n_his, n_pred=N_PRED, shuffle=shuffle, shuffle_seed=5,
                              loss=kind, huber_delta=DELTA, valid=valid if masked else None)
        assert gs.fused and gs.fold
        order = gs.order.cpu().tolist() if shuffle else list(range(BATCHES * B))
        if on_step is not None:      # the launches of one eager step of this very object (what the capture recorded)
            on_step("begin")
            gs._eager_fused_once()
            torch.cuda.synchronize()
            on_step("end")
        losses = [gs().clone() for _ in range(REPLAYS)]
        torch.cuda.synchronize()
        gs.close()
        return torch.stack(losses).cpu(), {k: v.clone() for k, v in m.state_dict().items()}, (series, valid, order, n_his)
    finally:
        DropoutStream.disable_device_counter()


@pytest.mark.parametrize("shuffle", [False, True], ids=["in_order", "shuffled"])
@pytest.mark.parametrize("kind", ["mae", "huber"])
def test_captured_masked_step_equals_eager_fused_steps_bitwise(kind, shuffle):
    """Four replays equal, bit for bit in loss and parameters, the eager fused_train_step on windows and masks gathered by hand from the
    same positions (the constructor's steps included: one plain step, then fused ones)."""
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    losses, sd, (series, valid, order, n_his) = _captured(kind, shuffle)

    def windows(k):
        starts = order[(k * B) % (BATCHES * B):(k * B) % (BATCHES * B) + B]
        x = torch.stack([series[s:s + n_his] for s in starts]).unsqueeze(1).contiguous()
        shift = n_his + N_PRED - 1
        return x, torch.stack([series[s + shift] for s in starts]).contiguous(), torch.stack([valid[s + shift] for s in starts]).contiguous()

    m2, _ = LK.tiny_model(DEV)
    o2 = make_optimizer(m2)
    x, y, v = windows(0)
    train_step(m2, o2, x, y, loss=kind, huber_delta=DELTA, valid=v)
    arena = GradArena([p for p in m2.parameters() if p.grad is not None])
    ref = []
    for k in range(1, WARMUP + 1 + REPLAYS):
        x, y, v = windows(k)
        ref.append(fused_train_step(m2, o2, x, y, arena, loss=kind, huber_delta=DELTA, valid=v).clone())
    torch.cuda.synchronize()
    ref = torch.stack(ref[-REPLAYS:]).cpu()
    worst = max(float((v2 - sd[k]).abs().max()) for k, v2 in m2.state_dict().items())
    print(kind, shuffle, losses.tolist(), ref.tolist(), "largest parameter difference", worst)
    assert torch.equal(losses, ref), (losses, ref)
    for k, v2 in m2.state_dict().items():
        assert torch.equal(v2, sd[k]), k


def test_masked_step_launch_rows():
    """One eager step of a masked and of an unmasked captured-step object; under STGCN_LAUNCH_LOG (the child of the test below) the byte
    ranges of the launch log that each wrote are recorded."""
    from tests.launch_log_util import span_recorder
    for name, masked in (("masked", True), ("unmasked", False)):
        rec = span_recorder(name, "STGCN_MASKED_LOG_SPANS")
        losses, _, _ = _captured("mae", True, masked=masked, on_step=None if rec is None else (lambda edge: rec("step", edge)))
        assert bool(torch.isfinite(losses).all())


def test_masked_step_launches_are_the_unmasked_steps(tmp_path):
    """The per-step launch list (label, kernel, workgroups) of the masked step is the unmasked step's: the same launches in the same
    order with the same grids, the head's fc backward kernel in its masked instance and nothing added."""
    from tests.launch_log_util import read_launches, run_child
    log, spans = str(tmp_path / "launch.log"), str(tmp_path / "spans.jsonl")
    run_child({"STGCN_LAUNCH_LOG": log, "STGCN_MASKED_LOG_SPANS": spans}, ["tests/test_gpu_masked_loss.py"], "test_masked_step_launch_rows",
              timeout=120)
    rows = read_launches(log, spans)
    masked, plain = rows[("masked", "step")], rows[("unmasked", "step")]
    assert len(plain) > 5 and len(masked) == len(plain)
    assert sum("fc_bwd_kernel" in k for _, k, _ in plain) == 1
    assert [(l, k.replace(", true>", ">") if "fc_bwd_kernel" in k else k, w) for l, k, w in masked] == plain
    assert [k for _, k, _ in masked if "fc_bwd_kernel" in k] == [k.replace("ET>", "ET, true>") for _, k, _ in plain if "fc_bwd_kernel" in k]
    assert not any("loss_grad" in k or "masked" in l for l, k, _ in masked)


# ---- evaluation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [SINGLE, BIG], ids=["single_workgroup", "partial_slabs"])
def test_masked_evaluation_matches_the_float64_host_loop(knob, monkeypatch):
    U.check_eval_against_float64(DEV, knob, monkeypatch)
    U.check_eval_pos_walk(DEV, knob, monkeypatch)


@pytest.mark.parametrize("knob", [SINGLE, BIG], ids=["single_workgroup", "partial_slabs"])
def test_all_ones_mask_leaves_the_unmasked_kernels_words(knob, monkeypatch):
    U.check_eval_all_ones_is_the_unmasked_kernel(DEV, knob, monkeypatch)


def test_captured_masked_eval_pass_equals_eager_launches_and_the_host_loop():
    from tests.optim_kinds_util import tiny_model
    U.bind(DEV)
    U.check_eval_pass(DEV, tiny_model(DEV, droprate=0.5)[0], 20, capture=True)


def test_interleaved_masked_pass_leaves_masked_training_bit_identical():
    """tests/test_gpu_eval_pass.py's interleaving check with masks on both sides: 2 S captured masked training steps with a masked
    validation pass after step S against the same run without any pass."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedEvalPass, GraphedTrainStep, make_optimizer
    from tests.test_gpu_eval_pass import _make
    n_his, n_pred, Bt, N, S = 12, 3, 8, 207, 3
    g = torch.Generator().manual_seed(6)
    series = torch.randn(9 * Bt + n_his + n_pred, N, generator=g).to(DEV)
    val = torch.randn(3 * Bt + 5 + n_his + n_pred, N, generator=g)
    ok_train = (torch.rand(series.shape, generator=g) >= 0.2).to(DEV)
    ok_val = torch.rand(val.shape, generator=g) >= 0.2
    x0, y0 = torch.zeros(Bt, 1, n_his, N, device=DEV), torch.zeros(Bt, N, device=DEV)

    def run(with_pass):
        DropoutStream.disable_device_counter()
        DropoutStream.manual_seed(3)
        DropoutStream._sites = 0
        m = _make(0.5)
        o = make_optimizer(m, capturable=True)
        m.train()
        with GraphedTrainStep(m, o, x0, y0, warmup=2, series=series, n_his=n_his, n_pred=n_pred, loss="mae", valid=ok_train) as gs:
            assert gs.fold
            ev = GraphedEvalPass(m, val, n_his, n_pred, Bt, valid=ok_val) if with_pass else None
            losses, metrics = [], None
            for i in range(2 * S):
                losses.append(gs().clone())
                if with_pass and i == S - 1:
                    assert ev.graph is not None
                    metrics = ev.run()
            gs.check()
            torch.cuda.synchronize()
            if ev is not None:
                assert metrics["windows"] == 3 * Bt + 5 and np.isfinite(metrics["mape"]) and 0 < metrics["elements"] < metrics["windows"] * N
                ev.close()
        return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert bool(torch.isfinite(l0).all()) and torch.equal(l0, l1), (l0, l1)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_refusals_and_the_abi():
    U.check_refusals(DEV)
