"""-m gpu: shuffled epochs of the resident-series training step -- the captured step reads window b of a minibatch from series row
``order[pos + b]`` of a device table (``GraphedTrainStep(shuffle=True)``) and trains exactly like the same windows gathered on the
host and fed one batch per step, with the same launches as the unshuffled step."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests.test_gpu_graph import DEV, _make

pytestmark = pytest.mark.gpu
N_HIS, N_PRED, B, N = 12, 3, 8, 207
BATCHES = 5          # minibatches of windows in the series (the shapes of test_resident_series_step_equals_explicit_batches)


def _series(extra=0):
    g = torch.Generator().manual_seed(6)
    return torch.randn(BATCHES * B + extra + N_HIS + N_PRED, N, generator=g).to(DEV)


def _windows(series, series_x, starts):
    x = torch.stack([series_x[s:s + N_HIS] for s in starts]).unsqueeze(1).contiguous()
    y = torch.stack([series[s + N_HIS + N_PRED - 1] for s in starts]).contiguous()
    return x, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_captured_shuffled_step_equals_explicit_gathered_batches(dtype):
    """Replays across a wrap of the position, ``reshuffle()``, replays again; against ``train_step`` on the windows of ``step.order``
    gathered on the host.  The bars are those of the unshuffled comparison (it is the same comparison): losses rtol 1e-5, every
    state_dict entry within 2e-5.  bf16: both sides round the same fp32 series to bf16 once.  The series holds 3 windows more than whole
    minibatches, so the permutation leaves a remainder out."""
    from stgcn_amd import DropoutStream
    from stgcn_amd.train import GraphedTrainStep, make_optimizer, train_step
    series = _series(extra=3)
    series_x = series.to(dtype)
    num, usable = BATCHES * B + 3, BATCHES * B
    x0, y0 = _windows(series, series, range(B))

    DropoutStream.use_device_counter(torch.device(DEV))
    DropoutStream.manual_seed(3)
    m = _make(0.0).set_compute_dtype(dtype)
    o = make_optimizer(m, capturable=True)
    gs = GraphedTrainStep(m, o, x0, y0, warmup=2, series=series, n_his=N_HIS, n_pred=N_PRED, shuffle=True, shuffle_seed=5)
    assert gs.fold, "the pack launch should carry the batch position"
    assert gs.order.dtype == torch.int64 and gs.order.numel() == usable and gs.order.is_cuda
    ptr = gs.order.data_ptr()
    first = gs.order.cpu().tolist()
    ref_perm = torch.randperm(num, generator=torch.Generator().manual_seed(5))[:usable].tolist()
    assert first == ref_perm and first != sorted(first)
    # the constructor ran positions 0, B, 2B; two more replays finish the epoch, the third wraps to position 0
    losses = [float(gs().item()) for _ in range(2)]
    torch.cuda.synchronize()
    assert int(gs.index.item()) == 4 * B
    gs.reshuffle()
    second = gs.order.cpu().tolist()
    assert second != first and gs.order.data_ptr() == ptr and len(set(second)) == usable and max(second) <= num - 1
    losses += [float(gs().item()) for _ in range(3)]          # positions 0, B, 2B of the second table
    torch.cuda.synchronize()
    assert int(gs.index.item()) == 2 * B
    gs.close()
    DropoutStream.disable_device_counter()

    m2 = _make(0.0).set_compute_dtype(dtype)
    o2 = make_optimizer(m2)
    seq = [first[k * B:(k + 1) * B] for k in range(5)] + [second[k * B:(k + 1) * B] for k in range(3)]
    ref_losses = [float(train_step(m2, o2, *_windows(series, series_x, s)).item()) for s in seq]
    torch.cuda.synchronize()
    print("shuffled step losses", losses, "explicit", ref_losses[-5:])
    worst = max(float((v.float() - m.state_dict()[k].float()).abs().max()) for k, v in m2.state_dict().items())
    print("largest state_dict difference", worst)
    assert np.allclose(losses, ref_losses[-5:], rtol=1e-5, atol=0), (losses, ref_losses)
    for k, v in m2.state_dict().items():
        assert float((v - m.state_dict()[k]).abs().max()) <= 2e-5, k


def test_table_mode_issues_the_same_launches():
    """Three eager fused steps with and without a table under the library's kernel timer: the same kernel labels, the same call counts."""
    from stgcn_amd import _lib, ops
    from stgcn_amd.train import GradArena, fused_train_step, make_optimizer, train_step
    series = _series()
    table = torch.randperm(BATCHES * B, generator=torch.Generator().manual_seed(2)).to(DEV)
    xv = torch.as_strided(series, (B, 1, N_HIS, N), (N, N_HIS * N, N, 1))
    yv = series[N_HIS + N_PRED - 1:N_HIS + N_PRED - 1 + B]
    profiles = []
    for tab in (None, table):
        m = _make(0.0)
        L = _lib.lib()
        o = make_optimizer(m)
        idx = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.bind_input_index(xv, idx, N, table=tab)
        ops.bind_input_index(yv, idx, N, table=tab)
        try:
            train_step(m, o, xv, yv)                                  # plain step: shows which parameters are live
            arena = GradArena([p for p in m.parameters() if p.grad is not None])
            m._step_counters = [(idx, B, BATCHES * B)]                # the position rides on the pack launch, as in the captured step
            fused_train_step(m, o, xv, yv, arena)                     # warm-up outside the timer
            torch.cuda.synchronize()
            L.dll.stgcn_profile_enable(1)
            for _ in range(3):
                fused_train_step(m, o, xv, yv, arena)
            torch.cuda.synchronize()
            buf = C.create_string_buffer(1 << 15)
            L.check(L.dll.stgcn_profile_collect(buf, len(buf)), "stgcn_profile_collect")
            L.dll.stgcn_profile_enable(0)
            assert int(idx.item()) == 4 * B
        finally:
            ops.unbind_input_index(xv)
            ops.unbind_input_index(yv)
            m._step_counters = None
        profiles.append({k: v["calls"] for k, v in json.loads(buf.value.decode()).items()})
    assert profiles[0] and profiles[0] == profiles[1], profiles
