"""-m gpu: ``train.GraphedEvalPass`` -- the captured evaluation pass with device-side MSE / MAE / RMSE / WMAPE -- against the reference's
recorded metrics, against eager launches of the same kernels, against the host loop it replaces (``data.evaluate_*``), and beside a live
captured training step, which it must leave bit for bit untouched."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import load_fixture, real_gso

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = [[1], [64, 16, 64], [64, 16, 64], [128, 128], [1]]


def _fixture_model():
    """exactly the set-up of test_gpu_model.test_mae_rmse_match_reference_on_metr_la_windows"""
    from oracle import stgcn_oracle as orc
    from stgcn_amd import data, models
    from tests.gpu_util import bind_hip
    bind_hip()
    fx = load_fixture("pipeline_metr_la")
    n_his, n_pred, bs = int(fx["n_his"]), int(fx["n_pred"]), int(fx["batch_size"])
    cfg = orc.OracleConfig(Kt=3, Ks=3, n_his=n_his, droprate=0.5, blocks=BLOCKS)
    params = orc.random_params(cfg, 207, seed=int(fx["param_seed"]))
    gso = torch.from_numpy(real_gso("metr_la.cheb_sym_norm_lap")).to(DEV)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=gso, enable_bias=True,
                                 droprate=0.5, n_his=n_his)
    model = models.STGCNChebGraphConv(args, BLOCKS, 207)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV)
    vel = fx["vel"].astype(np.float64)
    len_train, len_val, _ = data.split_lengths(len(vel))
    z = data.ZScore().fit(vel[:len_train])
    test = z.transform(vel[len_train + len_val:])
    return fx, model, test, z, n_his, n_pred, bs


def _make(droprate):
    from stgcn_amd import models
    from tests.gpu_util import bind_hip
    bind_hip()
    gso = torch.from_numpy(real_gso("metr_la.cheb_sym_norm_lap")).to(DEV)
    args = types.SimpleNamespace(Kt=3, Ks=3, act_func="glu", graph_conv_type="cheb_graph_conv", gso=gso, enable_bias=True,
                                 droprate=droprate, n_his=12)
    torch.manual_seed(1)
    return models.STGCNChebGraphConv(args, BLOCKS, 207).to(DEV)


def _host(model, series, z, n_his, n_pred, bs):
    from stgcn_amd import data
    sampler = data.WindowSampler(series, n_his, n_pred, DEV)
    mse = data.evaluate_model(model, torch.nn.MSELoss(), sampler.batches(bs))
    return (mse,) + tuple(data.evaluate_metric(model, sampler.batches(bs), z)), len(sampler)


def _within_bars(got, ref):
    """the project's north-star bars: 1e-4 absolute, WMAPE 1e-5"""
    mse, mae, rmse, wmape = ref
    print("pass", got, "against", ref)
    assert abs(got["mse"] - mse) <= 1e-4 and abs(got["mae"] - mae) <= 1e-4 and abs(got["rmse"] - rmse) <= 1e-4, (got, ref)
    assert abs(got["wmape"] - wmape) <= 1e-5, (got, ref)


def test_captured_pass_matches_reference_metrics_and_eager_launches():
    """48 test windows at batch size 32 (a ragged last batch): MSE, MAE, RMSE within 1e-4 and WMAPE within 1e-5 of the reference's
    recorded metrics; the replayed graph equals eager launches of the same kernels bit for bit; two passes return identical dicts."""
    from stgcn_amd.train import GraphedEvalPass
    fx, model, test, z, n_his, n_pred, bs = _fixture_model()
    with GraphedEvalPass(model, test, n_his, n_pred, bs, scaler=z) as ev:
        assert ev.graph is not None, "the pass must have been captured"
        assert ev.num == int(fx["n_test_windows"]) and ev.batches == 2
        got = ev.run()
        assert ev.run() == got
        assert ev.pos.tolist()[:3] == [16, 32, 2]      # after the last batch: parked on the last full window block, nothing left to count
    with GraphedEvalPass(model, test, n_his, n_pred, bs, scaler=z, capture=False) as ev:
        assert ev.graph is None
        eager = ev.run()
    assert got == eager, (got, eager)
    assert got["windows"] == 48
    _within_bars(got, tuple(float(v) for v in fx["metrics"]))


def test_bf16_pass_matches_the_host_loop_on_the_same_model():
    """bf16 activations: the pass and the host loop run the same kernels on the same bf16 model; only the batch that carries the 16 tail
    windows differs (windows 16..47 as one overlapped batch against a 16-window batch)."""
    from stgcn_amd.train import GraphedEvalPass
    fx, model, test, z, n_his, n_pred, bs = _fixture_model()
    model.set_compute_dtype(torch.bfloat16)
    with GraphedEvalPass(model, test, n_his, n_pred, bs, scaler=z) as ev:
        assert ev.graph is not None and ev.series_x.dtype == torch.bfloat16
        got = ev.run()
    ref, n = _host(model, test, z, n_his, n_pred, bs)
    ref16, _ = _host(model, test, z, n_his, n_pred, 16)
    print("host path at batch size 32 / 16:", ref, ref16)
    assert got["windows"] == n
    _within_bars(got, ref)


@pytest.mark.parametrize("order", ["eval_first", "train_first"])
def test_interleaved_pass_leaves_training_bit_identical(order):
    """2 S captured training steps (dropout on, folded counters, device-side windows) with a validation pass after step S against the same
    run without any pass: deterministic kernels, separate position words, no shared counters -- losses and parameters are bit-identical."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedEvalPass, GraphedTrainStep, make_optimizer
    n_his, n_pred, B, N, S = 12, 3, 8, 207, 3
    g = torch.Generator().manual_seed(6)
    series = torch.randn(9 * B + n_his + n_pred, N, generator=g).to(DEV)
    val = torch.randn(3 * B + 5 + n_his + n_pred, N, generator=g)
    x0, y0 = torch.zeros(B, 1, n_his, N, device=DEV), torch.zeros(B, N, device=DEV)

    def run(with_pass):
        DropoutStream.disable_device_counter()
        DropoutStream.manual_seed(3)
        DropoutStream._sites = 0          # both runs build "the same" model: its blocks draw the same dropout sites
        m = _make(0.5)
        o = make_optimizer(m, capturable=True)
        m.train()
        ev = GraphedEvalPass(m, val, n_his, n_pred, B) if (with_pass and order == "eval_first") else None
        with GraphedTrainStep(m, o, x0, y0, warmup=2, series=series, n_his=n_his, n_pred=n_pred) as gs:
            assert gs.fold
            if with_pass and order == "train_first":
                ev = GraphedEvalPass(m, val, n_his, n_pred, B)
            losses, metrics = [], None
            for i in range(2 * S):
                losses.append(gs().clone())
                if with_pass and i == S - 1:
                    assert ev.graph is not None
                    c0, s0, i0 = int(DropoutStream.counter.item()), int(o.device_step_counter(torch.device(DEV)).item()), int(gs.index.item())
                    metrics = ev.run()
                    assert m.training
                    assert (c0, s0, i0) == (int(DropoutStream.counter.item()), int(o.device_step_counter(torch.device(DEV)).item()),
                                            int(gs.index.item()))
            gs.check()
            torch.cuda.synchronize()
            if ev is not None:
                assert metrics["windows"] == 3 * B + 5 and np.isfinite(metrics["mse"])
                ev.close()
        return torch.stack(losses).cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert torch.equal(l0, l1), (l0, l1)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_pass_refuses_to_grow_a_workspace_under_a_captured_step():
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedEvalPass, GraphedTrainStep, make_optimizer
    n_his, n_pred, B, N = 12, 3, 8, 207
    g = torch.Generator().manual_seed(2)
    series = torch.randn(4 * B + n_his + n_pred, N, generator=g).to(DEV)
    val = torch.randn(70 + n_his + n_pred, N, generator=g)
    DropoutStream.disable_device_counter()
    m = _make(0.5)
    o = make_optimizer(m, capturable=True)
    m.train()
    with GraphedTrainStep(m, o, torch.zeros(B, 1, n_his, N, device=DEV), torch.zeros(B, N, device=DEV), warmup=2, series=series,
                          n_his=n_his, n_pred=n_pred) as gs:
        ptrs = {n: mod._ws.buf.data_ptr() for n, mod in m.named_modules() if hasattr(mod, "_ws")}
        with pytest.raises(RuntimeError, match=r"st_blocks\.0.*Build the evaluation pass before the training step"):
            GraphedEvalPass(m, val, n_his, n_pred, 4 * B)
        assert ptrs == {n: mod._ws.buf.data_ptr() for n, mod in m.named_modules() if hasattr(mod, "_ws")}, "nothing moved"
        l = float(gs())                                     # the captured step still runs on its own buffers
        assert np.isfinite(l)
        with GraphedEvalPass(m, val, n_his, n_pred, B) as ev:   # the step's own batch size fits
            assert ev.run()["windows"] == 70


def test_hundred_replays_at_the_c2_shape_match_the_host_loop():
    """207 nodes, batch size 32, 3 205 windows (= 5 mod 32, like the demo's validation split): 101 replays against the host loop."""
    from stgcn_amd import data
    from stgcn_amd.train import GraphedEvalPass
    n_his, n_pred, bs, N = 12, 3, 32, 207
    rs = np.random.RandomState(0)
    rows = 100 * bs + 5 + n_his + n_pred
    raw = np.clip(55 + 10 * np.sin(2 * np.pi * np.arange(rows)[:, None] / 288 + rs.uniform(0, 2 * np.pi, N)[None, :])
                  + rs.normal(0, 3, (rows, N)), 0, 80)
    z = data.ZScore().fit(raw)
    zs = z.transform(raw)
    model = _make(0.5)
    with GraphedEvalPass(model, zs, n_his, n_pred, bs, scaler=z) as ev:
        assert ev.graph is not None and ev.batches == 101
        got = ev.run()
        assert ev.run() == got
    ref, n = _host(model, zs, z, n_his, n_pred, bs)
    assert got["windows"] == n == 100 * bs + 5
    _within_bars(got, ref)
